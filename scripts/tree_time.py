"""Timing of the tree planners (artp_tree_*): device microseconds per stage and batch (hipEvents, Tree(profile=True)) at
B = 1024 and 4096 on the C2 map, and what a 10 ms plan_time (the reference's params.yaml value) reaches on C1 and C2 for
every variant: batches, vertices, best cost, the first solution's batch.  Output: one text table (profiles/tree_time.txt).
Usage: python scripts/tree_time.py [--batches N]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from art_planner_amd.context import Context  # noqa: E402
from art_planner_amd.tree import Tree  # noqa: E402
from synthetic import make_map  # noqa: E402

STAGES = ["sample", "nearest", "steer+count", "first motion+count", "near set", "near motions", "parent",
          "rewire", "rrt# sssp", "cost fold+prune"]
VARIANTS = ["rrt_star", "inf_rrt_star", "rrt_sharp"]


def c1(ctx):
    gm = make_map(100, 0.1, flat=True)
    ctx.upload_map(gm)
    probe = ctx.sample_states(1, 0, 64)
    z0 = float(probe[ctx.validate_states(probe) != 0][0, 2])
    return np.array([-4.0, -4.0, z0, 0, 0, 0, 1.0]), np.array([4.0, 4.0, z0, 0, 0, 0, 1.0])


def c2(ctx):
    gm = make_map(400, 0.04, seed=1234)
    ctx.upload_map(gm)
    se3 = ctx.sample_states(99, 0, 1 << 16)
    ok = se3[ctx.validate_states(se3) != 0]
    pick = lambda x, y: ok[np.argmin(np.hypot(ok[:, 0] - x, ok[:, 1] - y))]  # noqa: E731
    return pick(gm.pos_x - 6.4, gm.pos_y - 6.4), pick(gm.pos_x + 6.4, gm.pos_y + 6.4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=10)
    args = ap.parse_args()
    ctx = Context(0, "yaml")
    print(f"device {ctx.arch}")
    for name, setup in (("C2 400x400@0.04 Perlin", c2), ("C1 flat 100x100@0.1", c1)):
        s, g = setup(ctx)
        print(f"\n== {name}: start {np.round(s[:3], 2).tolist()} goal {np.round(g[:3], 2).tolist()}")
        for variant in VARIANTS:
            for B in (1024, 4096):
                t = Tree(ctx, s, g, variant, batch=B, profile=True)
                t.grow(1)  # warm-up batch (first launches), not counted
                base = t.stage_times()
                t0 = time.perf_counter()
                t.grow(args.batches)
                wall = (time.perf_counter() - t0) / args.batches * 1e6
                us = (t.stage_times() - base) / args.batches
                st = t.stats()
                print(f"{variant:13s} B={B:5d}  per batch (us): " + "  ".join(f"{n} {u:.0f}" for n, u in zip(STAGES, us))
                      + f"  | sum {us.sum():.0f}, wall {wall:.0f} | vertices {st['vertices']} cost {t.solve()[1]:.4f}")
                t.close()
        for variant in VARIANTS:
            for rep in range(3):
                t = Tree(ctx, s, g, variant, batch=1024, plan_time=0.01)
                t0 = time.perf_counter()
                out = t.grow(0)
                ms = (time.perf_counter() - t0) * 1e3
                st = t.stats()
                _, cost = t.solve()
                print(f"{variant:13s} plan_time 10 ms (run {rep}): grow {ms:.2f} ms, batches {out['batches']}, vertices "
                      f"{out['vertices']}, best cost {cost:.4f}, first solution batch {st['first_solution_batch']}, "
                      f"{'SOLVED' if np.isfinite(cost) else 'NOT SOLVED'}")
                t.close()
        # convergence curve at B = 1024 (the budget of tests/test_tree.py::test_convergence_on_flat_c1)
        opt = np.linalg.norm(g[:3] - s[:3]) / 0.5
        for variant in VARIANTS:
            t = Tree(ctx, s, g, variant, batch=1024)
            curve = []
            for _ in range(30):
                t.grow(1)
                curve.append(t.solve()[1] / opt)
            print(f"{variant:13s} best cost / straight line per batch: " + " ".join(f"{c:.4f}" for c in curve))
            t.close()
    ctx.close()


if __name__ == "__main__":
    main()
