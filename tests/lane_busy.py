"""A filler that keeps one stream busy for a chosen time, with a result known in advance (tests/test_lane_order.py,
scripts/lane_order_time.py).

Matrix products of preallocated tensors written with out=: nothing is allocated on the stream while it runs, so the
caching allocator never synchronises behind the test's back.  The operands hold -1, 0 and 1 only, so every sum is an
integer below 2^24 and the float32 product is exact whatever the order of the additions: the expected product comes from
a float64 product made once at setup, and a filler that was cut short, or run on memory somebody else wrote, does not
equal it."""
import math

N = 2048          # 2 * N^3 = 17 GFLOP a product: a fraction of a millisecond on an MI355X
CEILING_S = 0.2   # no filler runs longer than this


class Busy:
    def __init__(self, device="cuda:0", n=N, seed=0):
        import torch
        g = torch.Generator(device="cpu").manual_seed(seed)
        self.a = torch.randint(-1, 2, (n, n), generator=g).to(torch.float32).to(device)
        self.b = torch.randint(-1, 2, (n, n), generator=g).to(torch.float32).to(device)
        self.out = torch.zeros((n, n), dtype=torch.float32, device=device)
        self.expected = (self.a.double() @ self.b.double()).to(torch.float32)
        assert float(self.expected.abs().max()) <= n
        self.tick = torch.zeros(64, dtype=torch.int32, device=device)   # concurrent_stream's small kernel works on this
        for _ in range(3):   # warm up: the library picks and loads its kernel here, not inside a measurement
            torch.mm(self.a, self.b, out=self.out)
            self.tick.add_(1)
        torch.cuda.synchronize()
        assert torch.equal(self.out, self.expected)
        # one product, timed with events on the current stream (the median of five runs of ten)
        times = []
        for _ in range(5):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(10):
                torch.mm(self.a, self.b, out=self.out)
            t1.record()
            t1.synchronize()
            times.append(t0.elapsed_time(t1) * 1e-3 / 10)
        self.seconds_per_product = sorted(times)[2]

    def concurrent_stream(self, other, tries=8, probe_seconds=0.005):
        """A new torch stream whose work the device runs side by side with `other`'s, or None.  A process has only a few
        hardware queues, and streams that share one run in the order they were fed: behind a filler on such a stream a
        writer on `other` waits whether the library orders it or not, and the case would prove nothing.  The probe: a short
        filler on the candidate, one small kernel on `other`; the pair is concurrent if that kernel is done while the
        candidate is still busy.  torch hands its pooled streams out in turn, so the next candidate sits on another queue."""
        import torch
        for _ in range(tries):
            s = torch.cuda.Stream(device=self.a.device)
            torch.cuda.synchronize()
            with torch.cuda.stream(s):
                for _ in range(self.repeats(probe_seconds)):
                    torch.mm(self.a, self.b, out=self.out)
            done = torch.cuda.Event()
            with torch.cuda.stream(other):
                self.tick.add_(1)
                done.record()
            done.synchronize()
            side_by_side = not s.query()
            torch.cuda.synchronize()
            if side_by_side:
                return s
        return None

    def repeats(self, seconds):
        """Products that keep a stream busy for `seconds` (at most CEILING_S)."""
        return max(1, math.ceil(min(seconds, CEILING_S) / self.seconds_per_product))

    def queue(self, stream, seconds):
        """Queue the filler on `stream`; returns the number of products queued."""
        import torch
        reps = self.repeats(seconds)
        with torch.cuda.stream(stream):   # the BLAS library's per-stream workspace comes into being here, not in the run
            torch.mm(self.a, self.b, out=self.out)
        self.out.zero_()
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            for _ in range(reps):
                torch.mm(self.a, self.b, out=self.out)
        return reps

    def result_is_expected(self):
        """After the run: the product the filler left behind is the one known in advance."""
        import torch
        return torch.equal(self.out, self.expected)
