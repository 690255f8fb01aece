"""Timing of the clearance maps and the clearance-weighted fields, in one run on one machine.
1. The C2 map (400x400 @ 0.04 m), its own reachability mask on the device, 16 headings, radius 12 and 32, device events,
   median of --reps: clearance_map alone (device mask, device output); the two steps of the table build inside a
   clearance_cost_field (the field's own events: the clearance map, the table kernel); the whole clearance_cost_field next to
   cost_field on the same mask and source (the valid node nearest the centre).
2. Plan statistics on the 120x120 Perlin maps at 8 headings that tests/test_cost_field_plan.py uses (amplitudes 0.25 and
   0.5, objective 1, forward, 16 targets): the raw paths that hold a move checkMotion rejects, and rounds, moves checked and
   moves blocked of one plan(), for gain 0 against the default gain (2.0, margin 0.2 m, radius 12), yaw_spread 0 and 1.
Output: one text table (profiles/field_clearance_time.txt).
Usage: python scripts/field_clearance_time.py [--out FILE] [--reps N]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from art_planner_amd.context import Context  # noqa: E402
from synthetic import map_from_device, raw_map  # noqa: E402

N = 400


def event_ms(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def med(v):
    return f"{np.median(v):9.3f} ms [{min(v):.3f}..{max(v):.3f}]"


def timing(ctx, reps, lines):
    import torch
    n_yaw = 16
    map_from_device(ctx, raw_map(N, 0.04, seed=1234), "yaml")
    mask = ctx.reachability_map(n_yaw)
    mask_t = torch.from_numpy(np.asfortranarray(mask).T.copy().view(np.int32)).to(f"cuda:{ctx.device}").T
    d2_t = torch.zeros(N * N * n_yaw, dtype=torch.int16, device=f"cuda:{ctx.device}")
    bits = ((mask[..., None] >> np.arange(n_yaw, dtype=np.uint32)) & 1).astype(bool)
    nodes = np.argwhere(bits)
    src = tuple(int(v) for v in nodes[np.argmin((nodes[:, 0] - N // 2) ** 2 + (nodes[:, 1] - N // 2) ** 2)])
    lines += [f"== {N}x{N} @ 0.04 m, {n_yaw} headings, {int(bits.sum())} nodes, objective 1, source {src}; median of {reps} "
              "[min..max], device events"]
    plain = []
    for rep in range(reps + 1):
        box = {}

        def run():
            box["f"] = ctx.cost_field(mask_t, n_yaw, [src], objective=1)
        t = event_ms(run)
        box["f"].close()
        if rep:
            plain.append(t)
    lines += [f"  cost_field (unchanged code)                   {med(plain)}"]
    for R in (12, 32):
        for s in (0, 1):
            ms = [event_ms(lambda: ctx.clearance_map_dev(mask_t, n_yaw, d2_t, R, yaw_spread=s)) for _ in range(reps + 1)][1:]
            d2 = d2_t.cpu().numpy().view(np.uint16)
            lines += [f"  clearance_map R {R:2d} yaw_spread {s}               {med(ms)}   "
                      f"{int(((d2 != 0) & (d2 != 0xffff)).sum())} nodes within R of an obstacle"]
        whole, cmap, table, search = [], [], [], []
        for rep in range(reps + 1):
            box = {}

            def run():
                box["f"] = ctx.clearance_cost_field(mask_t, n_yaw, [src], objective=1, radius_cells=R, margin=0.2, gain=2.0)
            t = event_ms(run)
            st = box["f"].learned_stats()
            box["f"].close()
            if rep:
                whole.append(t)
                cmap.append(st["rows_ms"])
                table.append(st["combine_ms"])
                search.append(st["dist_ms"] + st["hop_ms"])
        lines += [f"  clearance_cost_field R {R:2d}: whole call         {med(whole)}   = {np.median(whole) / np.median(plain):.2f} x cost_field",
                  f"      its clearance map                         {med(cmap)}",
                  f"      its table build ({st['table_bytes'] >> 20} MB)                  {med(table)}",
                  f"      its two searches (host time)              {med(search)}"]


def plans(ctx, lines):
    from test_cost_field_plan import world
    n_yaw = 8
    lines += ["", "== plan() on the 120x120 Perlin maps at 8 headings, objective 1, forward, 16 targets, margin 0.2 m, radius 12:",
              "   raw = paths of the new field that hold a move check_motions rejects"]
    for amplitude in (0.25, 0.5):
        gm, mask, src, targets = world(ctx, amplitude, n_yaw)
        for s in (0, 1):
            for gain in (0.0, 2.0):
                with ctx.clearance_cost_field(mask, n_yaw, [src], objective=1, gain=gain, yaw_spread=s) as f:
                    paths = [f.path(t) for t in targets]
                    raw = sum(not ctx.check_motions(p[1][:-1], p[1][1:]).all() for p in paths if p and len(p[0]) > 1)
                    hops = sum(len(p[0]) - 1 for p in paths if p)
                    res = f.plan(targets)
                    st = f.plan_stats()
                    d2 = f.clearance()
                    low = [min(int(d2[tuple(v)]) for v in r[1][3:-3]) for r in res if r[0] == 0 and len(r[1]) > 6]
                lines += [f"  amplitude {amplitude:4.2f} yaw_spread {s} gain {gain:3.1f}: raw {raw:2d} of 16 ({hops} moves); plan: "
                          f"{st['rounds']} rounds, {st['moves_checked']} moves checked, {st['moves_blocked']} blocked, statuses "
                          f"{[r[0] for r in res].count(0)} x 0 / {[r[0] for r in res].count(1)} x 1 / {[r[0] for r in res].count(2)} x 2, "
                          f"median least d2 on a checked path (three states at each end left out) {int(np.median(low)) if low else -1}"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "field_clearance_time.txt"))
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    ctx = Context(0, "yaml")
    ctx.use_torch_stream()
    lines = [f"device {ctx.arch}", ""]
    timing(ctx, a.reps, lines)
    plans(ctx, lines)
    ctx.close()
    for row in lines:
        print(row, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
