"""Timing of artp_roadmap_solve_many against the sequential set_query + solve loop on the C2 map (400x400 @ 0.04 m),
10 000 milestones, constructions 0 and 1.  N = 1, 16, 256, 1024 goals spread over the map; per N five repetitions after a
warm-up, wall clock around the call (the call returns host results: it ends synchronised), median and min..max; the
sequential loop alternates with it for N <= 256.  Before every repetition the roadmap's own query is set again, which
clears the verdict cache: each call checks its motions from scratch, as each sequential query does.  Lazy removals
persist in both (as they do for the reference's kept roadmap).
Output: one text table (profiles/roadmap_many_time.txt).
Usage: python scripts/roadmap_many_time.py [--out FILE] [--only-n N --constructions 0 --reps 1]  (the last form is the
rocprofv3 --kernel-trace --stats run)"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from art_planner_amd import _capi  # noqa: E402
from art_planner_amd.context import Context  # noqa: E402
from art_planner_amd.roadmap import Roadmap  # noqa: E402
from synthetic import make_map  # noqa: E402


def sequential(rm, start, goals):
    for g in goals:
        try:
            rm.set_query(start, g)
            rm.solve()
        except _capi.ArtpError:
            pass


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "roadmap_many_time.txt"))
    ap.add_argument("--only-n", type=int, default=0)
    ap.add_argument("--constructions", default="0,1")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    ctx = Context(0, "yaml")
    gm = make_map(400, 0.04, seed=1234)
    ctx.upload_map(gm)
    se3 = ctx.sample_states(99, 0, 1 << 16)
    ok = se3[ctx.validate_states(se3) != 0]
    pick = lambda x, y: ok[np.argmin(np.hypot(ok[:, 0] - x, ok[:, 1] - y))]  # noqa: E731
    start, goal = pick(gm.pos_x - 6.4, gm.pos_y - 6.4), pick(gm.pos_x + 6.4, gm.pos_y + 6.4)
    s7 = ctx.sample_states(7, 0, 1 << 16)
    pool = s7[ctx.validate_states(s7) != 0]
    ns = [a.only_n] if a.only_n else [1, 16, 256, 1024]
    lines = [f"device {ctx.arch}", "",
             f"== C2 400x400@0.04 Perlin, 10 000 milestones: start {np.round(start[:3], 2).tolist()}, goals spread over "
             f"the map; wall ms per call, median [min..max] of {a.reps}"]
    for cons in [int(c) for c in a.constructions.split(",")]:
        t0 = time.perf_counter()
        rm = Roadmap(ctx, start, goal, n_milestones=10000, seed=1, construction=cons)
        st = rm.stats()
        lines.append(f"construction {cons}: {st['vertices']} vertices, {st['candidate_edges']} edges, k {st['k']} "
                     f"(build {time.perf_counter() - t0:.1f} s)")
        rm.solve_many(start, pool[:16])  # warm-up: code objects, scratch
        sequential(rm, start, pool[:4])
        for n in ns:
            goals = pool[:: max(1, len(pool) // n)][:n]
            tm, ts, info = [], [], None
            for _ in range(a.reps):
                rm.set_query(start, goal)  # a fresh verdict cache for every call
                t0 = time.perf_counter()
                r = rm.solve_many(start, goals)
                tm.append((time.perf_counter() - t0) * 1e3)
                info = r
                if n <= 256 and a.reps > 1:
                    t0 = time.perf_counter()
                    sequential(rm, start, goals)
                    ts.append((time.perf_counter() - t0) * 1e3)
            s = info["stats"]
            solved = int((info["status"] == 0).sum())
            row = (f"  N {n:5d}  solve_many {np.median(tm):9.2f} ms [{min(tm):.2f}..{max(tm):.2f}]  rounds {s['rounds']:3d}  "
                   f"motions {s['motions']:7d}  removed {s['removed']:5d}  fallback {s['fallback']:2d}  solved {solved}")
            if ts:
                row += (f"  | sequential {np.median(ts):9.2f} ms [{min(ts):.2f}..{max(ts):.2f}]  "
                        f"speedup {np.median(ts) / np.median(tm):6.1f}x")
            lines.append(row)
            print(row, flush=True)
        rm.close()
    ctx.close()
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
