"""Timing of the reachability maps (artp_reachability_map_dev) on the C2 map (400x400 @ 0.04 m) at n_yaw 8 / 16 / 32, on
an 800x800 @ 0.04 m map at n_yaw 16 and 32, and of the incremental form: a 40x40 rectangle grown by the halo on 400^2.
Device events around each call into a device buffer, 10 repetitions after two warm-ups, median and min..max.  The same run
times the fused sample + validate step of 2^22 states on the same map (the headline's work) for the cost per state.
Output: one text table (profiles/reach_time.txt).
Usage: python scripts/reach_time.py [--out FILE] [--reps N] [--only 400x16]  (the last form is the
rocprofv3 --kernel-trace --stats run)"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from art_planner_amd.context import Context  # noqa: E402
from synthetic import map_from_device, raw_map  # noqa: E402


def timed(fn, reps):
    import torch
    for _ in range(2):
        fn()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), min(ms), max(ms)


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reach_time.txt"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", default="", help="one case, e.g. 400x16 (for a kernel trace)")
    a = ap.parse_args()
    ctx = Context(0, "yaml")
    ctx.use_torch_stream()
    lines = [f"device {ctx.arch}", "",
             f"== reachability maps: ms per artp_reachability_map_dev call (device events), median [min..max] of {a.reps}"]
    cases = [(400, 8), (400, 16), (400, 32), (800, 16), (800, 32)]
    if a.only:
        cases = [tuple(int(v) for v in a.only.split("x"))]
    for n in sorted({c[0] for c in cases}):
        gm = map_from_device(ctx, raw_map(n, 0.04, seed=1234), "yaml")
        S = 1 << 22
        se3 = torch.empty((S, 7), dtype=torch.float64, device="cuda:0")
        valid = torch.empty(S, dtype=torch.uint8, device="cuda:0")
        ref = timed(lambda: ctx.sample_and_validate_dev(42, 0, S, se3, valid), a.reps) if not a.only else None
        if ref:
            ns_state = ref[0] * 1e6 / S
            lines.append(f"{n}x{n}: fused sample + validate of 2^22 states {ref[0]:.3f} ms = {ns_state:.3f} ns per state")
        del se3, valid
        mask = torch.zeros(gm.rows * gm.cols, dtype=torch.int32, device="cuda:0")
        for nn, n_yaw in cases:
            if nn != n:
                continue
            t = timed(lambda: ctx.reachability_map_dev(mask, n_yaw), a.reps)
            poses = gm.rows * gm.cols * n_yaw
            m = mask.cpu().numpy().view(np.uint32)
            frac = float(np.unpackbits(m.view(np.uint8)).sum()) / poses
            row = (f"  {n}x{n} n_yaw {n_yaw:2d}: {poses:9d} poses  {t[0]:8.3f} ms [{t[1]:.3f}..{t[2]:.3f}]  "
                   f"{t[0] * 1e6 / poses:.3f} ns per pose")
            if ref:
                row += f" ({t[0] * 1e6 / poses / ns_state:.2f}x the sampled state)"
            row += f"  valid {frac:.3f}"
            lines.append(row)
            print(row, flush=True)
        if n == 400 and not a.only:
            halo = ctx.reachability_halo()
            r0, c0, side = 180, 180, 40
            g0, g1 = max(0, r0 - halo), min(gm.rows, r0 + side + halo)
            h0, h1 = max(0, c0 - halo), min(gm.cols, c0 + side + halo)
            rect = (g0, h0, g1 - g0, h1 - h0)
            part = torch.zeros(rect[2] * rect[3], dtype=torch.int32, device="cuda:0")
            t = timed(lambda: ctx.reachability_map_dev(part, 16, rect), a.reps)
            row = (f"  {n}x{n} n_yaw 16, a {side}x{side} rectangle grown by the halo ({halo} cells) = {rect[2]}x{rect[3]} "
                   f"cells: {t[0]:.3f} ms [{t[1]:.3f}..{t[2]:.3f}]")
            lines.append(row)
            print(row, flush=True)
    ctx.close()
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out and not a.only:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
