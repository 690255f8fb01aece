"""Timing of the cost-to-go fields (artp_field_compute): the tiled form against the plain form, in one run on one machine,
on the C2 map (400x400 @ 0.04 m) at n_yaw 8 / 16 / 32 and on an 800x800 @ 0.04 m map at n_yaw 16.  The mask is the map's
own reachability mask, on the device; objective 1; one source, the valid node nearest the centre.  Device events around
each call (it includes the allocation of the field and the hop-count search), 10 repetitions after two warm-ups, median
and min..max, the two forms alternating.  Also recorded: the outer rounds, tile runs and plain sweeps from
artp_field_stats, and the reachability_map_dev time of the same lattice.
Output: one text table (profiles/field_time.txt).
Usage: python scripts/field_time.py [--out FILE] [--reps N] [--only 400x16] [--form tiled|plain]  (the last two: the
rocprofv3 --kernel-trace --stats run)"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from art_planner_amd.context import Context  # noqa: E402
from synthetic import map_from_device, raw_map  # noqa: E402


def event_ms(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "field_time.txt"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", default="", help="one case, e.g. 400x16 (for a kernel trace)")
    ap.add_argument("--form", default="", help="with --only: tiled or plain alone")
    a = ap.parse_args()
    ctx = Context(0, "yaml")
    ctx.use_torch_stream()
    lines = [f"device {ctx.arch}", "",
             "== cost-to-go fields: ms per artp_field_compute call (device events), objective 1, one source at the centre,",
             f"   median [min..max] of {a.reps}, tiled and plain alternating; reach = reachability_map_dev of the same lattice"]
    cases = [(400, 8), (400, 16), (400, 32), (800, 16)]
    if a.only:
        cases = [tuple(int(v) for v in a.only.split("x"))]
    for n in sorted({c[0] for c in cases}):
        gm = map_from_device(ctx, raw_map(n, 0.04, seed=1234 if n == 400 else 99), "yaml")
        mask = torch.zeros(gm.rows * gm.cols, dtype=torch.int32, device="cuda:0")
        for nn, n_yaw in cases:
            if nn != n:
                continue
            reach = [event_ms(lambda: ctx.reachability_map_dev(mask, n_yaw)) for _ in range(a.reps + 2)][2:]
            m = mask.cpu().numpy().view(np.uint32).reshape(gm.cols, gm.rows).T
            bits = ((m[..., None] >> np.arange(n_yaw, dtype=np.uint32)) & 1).astype(bool)
            nodes = np.argwhere(bits)
            src = [tuple(int(v) for v in nodes[np.argmin((nodes[:, 0] - n // 2) ** 2 + (nodes[:, 1] - n // 2) ** 2)])]
            forms = [f for f in ("tiled", "plain") if not a.form or f == a.form]
            ms = {f: [] for f in forms}
            stats, dist = {}, {}
            for rep in range(a.reps + 2):
                for form in forms:
                    box = {}

                    def run():
                        box["f"] = ctx.cost_field(mask, n_yaw, src, objective=1, plain_sweeps=(form == "plain"))
                    t = event_ms(run)
                    if rep >= 2:
                        ms[form].append(t)
                    stats[form] = box["f"].stats()
                    if rep == 0:
                        dist[form] = box["f"].dist()
                    box["f"].close()
            if len(forms) == 2:
                assert np.array_equal(dist["tiled"].view(np.uint64), dist["plain"].view(np.uint64))
            st = stats[forms[0]]
            row = (f"  {n}x{n} n_yaw {n_yaw:2d}: {st['nodes']:9d} nodes, {st['reached_nodes']:9d} reached  "
                   f"reach {np.median(reach):7.3f} ms")
            lines.append(row)
            print(row, flush=True)
            for form in forms:
                s, t = stats[form], ms[form]
                row = f"      {form:5s} {np.median(t):9.3f} ms [{min(t):.3f}..{max(t):.3f}]  "
                if form == "tiled":
                    row += (f"{s['outer_rounds']} outer rounds, {s['tile_launches']} tile runs of {s['tiles']} tiles; "
                            f"hop counts: {s['hop_rounds']} rounds, {s['hop_tile_launches']} tile runs")
                else:
                    row += f"{s['plain_sweeps']} sweeps; hop counts: {s['hop_rounds']} sweeps"
                lines.append(row)
                print(row, flush=True)
            if len(forms) == 2:
                row = f"      plain / tiled = {np.median(ms['plain']) / np.median(ms['tiled']):.2f}x, same bits"
                lines.append(row)
                print(row, flush=True)
        del mask
    ctx.close()
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out and not a.only:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
