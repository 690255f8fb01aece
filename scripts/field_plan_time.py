"""Timing of artp_field_plan, in one run on one machine: the C2 map (400x400 @ 0.04 m), objective 1,
at 16 and at 8 headings, a goal-rooted (reverse) and a forward field from the valid node nearest the centre, 16 targets
taken at even ranks over the farther half of the field's finite distances.  Per case: one plan() on a new field -- rounds,
moves checked and blocked, ms per round split into descent, check (poses, checkMotion, block kernel) and the repair passes
-- and, in the same run, the time of a new artp_field_compute on the same mask: without blocked moves that is the only way
to a field at all, and it cannot take a move out.  The plan is run --reps times, each on a new field (the blocks of one
run would leave the next nothing to do); medians.
Output: one text table (profiles/field_plan_time.txt).
Usage: python scripts/field_plan_time.py [--out FILE] [--reps N]"""
import argparse
import os
import sys
import time

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "field_plan_time.txt"))
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    ctx = Context(0, "yaml")
    ctx.use_torch_stream()
    map_from_device(ctx, raw_map(N, 0.04, seed=1234), "yaml")
    lines = [f"device {ctx.arch}", "",
             f"== artp_field_plan: {N}x{N} @ 0.04 m, objective 1, 16 targets at even ranks over the farther half of the finite",
             f"   distances, source = the valid node nearest the centre; median of {a.reps} runs, each on a new field;",
             "   ms per round: descent and check are stream time, passes host time (every round of a pass is read)"]
    for n_yaw in (16, 8):
        mask = ctx.reachability_map(n_yaw)
        bits = ((mask[..., None] >> np.arange(n_yaw, dtype=np.uint32)) & 1).astype(bool)
        nodes = np.argwhere(bits)
        src = tuple(int(v) for v in nodes[np.argmin((nodes[:, 0] - N // 2) ** 2 + (nodes[:, 1] - N // 2) ** 2)])
        for reverse in (True, False):
            kw = dict(objective=1, reverse=reverse)
            fresh_ms, plan_ms, stats, res, raw_bad = [], [], [], None, 0
            for rep in range(a.reps + 1):
                box = {}

                def run():
                    box["f"] = ctx.cost_field(mask, n_yaw, [src], **kw)
                t = event_ms(run)
                f = box["f"]
                if rep == 0:                  # warm-up, and the targets
                    d = f.dist()
                    order = np.argsort(d, axis=None, kind="stable")
                    order = order[:int(np.isfinite(d).sum())]
                    ranks = np.linspace(len(order) // 2, len(order) - 1, 16).astype(int)
                    targets = [tuple(int(v) for v in np.unravel_index(order[r], d.shape)) for r in ranks]
                    paths = [f.path(t_) for t_ in targets]
                    raw_bad = sum(not ctx.check_motions(p[1][:-1], p[1][1:]).all() for p in paths if p and len(p[0]) > 1)
                else:
                    fresh_ms.append(t)
                t0 = time.perf_counter()
                res = f.plan(targets)
                t1 = time.perf_counter()
                if rep > 0:
                    plan_ms.append((t1 - t0) * 1e3)
                    stats.append(f.plan_stats())
                hops = [len(r[1]) - 1 for r in res if r[0] == 0]
                f.close()
            st = stats[-1]
            med = lambda k: float(np.median([s[k] for s in stats]))
            rounds, upd = max(st["rounds"], 1), max(st["updates"], 1)
            rows = [f"  n_yaw {n_yaw}, {'goal-rooted (reverse)' if reverse else 'forward'}, source {src}:",
                    f"      {raw_bad} of 16 raw paths held a failing move; statuses {[r[0] for r in res]}; "
                    f"paths of {min(hops) if hops else 0}..{max(hops) if hops else 0} moves",
                    f"      plan      {np.median(plan_ms):9.3f} ms [{min(plan_ms):.3f}..{max(plan_ms):.3f}]  {st['rounds']} rounds, "
                    f"{st['moves_checked']} moves checked, {st['moves_blocked']} blocked, {st['updates']} repairs of "
                    f"{st['update_tile_runs'] / upd:.0f} tile runs each",
                    f"      per round: descent {med('descent_ms') / rounds:.3f} ms, check {med('check_ms') / rounds:.3f} ms "
                    f"(host time of both {med('round_ms') / rounds:.3f} ms); passes {med('passes_ms') / upd:.3f} ms per repair",
                    f"      new field {np.median(fresh_ms):9.3f} ms [{min(fresh_ms):.3f}..{max(fresh_ms):.3f}] on the same mask; "
                    f"a repair / a new field = {med('passes_ms') / upd / np.median(fresh_ms):.3f}"]
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
