"""Timing of artp_field_simplify_paths, in one run on one machine: the C2 map (400x400 @ 0.04 m),
objective 1, at 16 and at 8 headings, a goal-rooted (reverse) field from the valid node nearest the centre and the 16
targets of scripts/field_plan_time.py; plan() gives the checked lattice paths.  Per window (16, 64, 256): the host time of
one simplify() of all 16 paths, the library's stats (candidates, usable ones, batches, stream time of the evaluation and of
the search), the states kept against the states in, and the summed cost against the lattice chains' cost under the same
pricing (the call at window 1, which keeps every state).
Next to it what the library offered before: Roadmap.simplify (all pairs of one path, pairs listed and searched on the host)
on the same 16 paths one after the other, with a roadmap of the same objective and velocities.  The two do NOT compute the
same thing unless the window covers the path: the roadmap's routine may join any two states of a path, the windowed call
only states at most `window` apart.  Medians of --reps runs after one warm-up.
Output: one text table (profiles/field_simplify_time.txt).
Usage: python scripts/field_simplify_time.py [--out FILE] [--reps N]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from art_planner_amd.context import Context  # noqa: E402
from art_planner_amd.roadmap import Roadmap  # noqa: E402
from synthetic import map_from_device, raw_map  # noqa: E402

N = 400
WINDOWS = (16, 64, 256)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "field_simplify_time.txt"))
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    ctx = Context(0, "yaml")
    map_from_device(ctx, raw_map(N, 0.04, seed=1234), "yaml")
    lines = [f"device {ctx.arch}", "",
             f"== artp_field_simplify_paths: {N}x{N} @ 0.04 m, objective 1, goal-rooted field, the 16 checked paths of plan() to",
             f"   the targets of scripts/field_plan_time.py, all in one call; median of {a.reps} calls after a warm-up.",
             "   call = host time of CostField.simplify; eval and search = stream time (library stats); cost = sum over the 16",
             "   paths, lattice = the same paths at window 1 (every state kept, same pricing).",
             "   Roadmap.simplify = the host routine over ALL pairs of one path, 16 calls one after the other: it is not",
             "   limited to a window, so it computes the same thing only where the window covers the path."]
    for n_yaw in (16, 8):
        mask = ctx.reachability_map(n_yaw)
        bits = ((mask[..., None] >> np.arange(n_yaw, dtype=np.uint32)) & 1).astype(bool)
        nodes = np.argwhere(bits)
        src = tuple(int(v) for v in nodes[np.argmin((nodes[:, 0] - N // 2) ** 2 + (nodes[:, 1] - N // 2) ** 2)])
        with ctx.cost_field(mask, n_yaw, [src], objective=1, reverse=True) as f:
            d = f.dist()
            order = np.argsort(d, axis=None, kind="stable")
            order = order[:int(np.isfinite(d).sum())]
            ranks = np.linspace(len(order) // 2, len(order) - 1, 16).astype(int)
            targets = [tuple(int(v) for v in np.unravel_index(order[r], d.shape)) for r in ranks]
            paths = [r[2] for r in f.plan(targets) if r[0] == 0]
            n_in = sum(len(p) for p in paths)
            lattice = f.simplify(paths, window=1)
            assert all(r[0] == 0 and len(r[1]) == len(p) for r, p in zip(lattice, paths))
            lattice_cost = sum(r[3] for r in lattice)
            rows = [f"  n_yaw {n_yaw}, source {src}: {len(paths)} paths of {min(map(len, paths))}..{max(map(len, paths))} states, "
                    f"{n_in} in all; lattice cost {lattice_cost:.3f}"]
            for w in WINDOWS:
                ms, stats, res = [], [], None
                for rep in range(a.reps + 1):
                    t0 = time.perf_counter()
                    res = f.simplify(paths, window=w)
                    t1 = time.perf_counter()
                    if rep:
                        ms.append((t1 - t0) * 1e3)
                        stats.append(f.simplify_stats())
                st = stats[-1]
                med = lambda k: float(np.median([s[k] for s in stats]))
                cost = sum(r[3] for r in res)
                rows.append(f"      window {w:3d}: call {np.median(ms):9.3f} ms [{min(ms):.3f}..{max(ms):.3f}]  eval {med('eval_ms'):8.3f} ms, "
                            f"search {med('search_ms'):6.3f} ms, library host time {med('host_ms'):8.3f} ms; {st['candidates']} candidates, "
                            f"{st['usable_candidates']} usable, {st['batches']} batches; kept {st['states_kept']} of {n_in} states; "
                            f"cost {cost:.3f} = {cost / lattice_cost:.4f} of the lattice's")
            # what there was before: one path at a time, all pairs, through the host
            ms, kept, cost = [], 0, 0.0
            rms = [Roadmap(ctx, p[0], p[-1], n_milestones=8, objective=1, max_lon_vel=0.5, max_lat_vel=0.1, max_ang_vel=0.5)
                   for p in paths]
            for rep in range(a.reps + 1):
                t0 = time.perf_counter()
                out = [rm.simplify(p) for rm, p in zip(rms, paths)]
                t1 = time.perf_counter()
                if rep:
                    ms.append((t1 - t0) * 1e3)
                kept, cost = sum(len(o[0]) for o in out), sum(o[1] for o in out)
            for rm in rms:
                rm.close()
            pairs = sum(len(p) * (len(p) - 1) // 2 for p in paths)
            rows.append(f"      Roadmap.simplify x {len(paths)}: {np.median(ms):9.3f} ms [{min(ms):.3f}..{max(ms):.3f}]  {pairs} pairs; "
                        f"kept {kept} of {n_in} states; cost {cost:.3f} = {cost / lattice_cost:.4f} of the lattice's")
        for row in rows:
            print(row, flush=True)
        lines += rows
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
