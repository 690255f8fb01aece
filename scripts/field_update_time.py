"""Timing of artp_field_update against a new artp_field_compute on the same final mask, in one run on one machine: the C2
map (400x400 @ 0.04 m), n_yaw 16, objective 1, a reverse field from one goal (the valid node nearest the centre).
The change is what a replanning cycle produces: a 40 x 40 rectangle of both validity layers is rewritten (a block of
+0.6 m on its inner 24 x 24 cells) with update_layer_rects, reachability_map recomputes that rectangle grown by
reachability_halo() and the result is pasted into the old mask.  Three placements of the rectangle: far from the goal,
midway, and around the goal (the goal's own bit kept set).  Masks live on the device for both calls.  Device events around
each whole call, median and min..max of 10 after two warm-ups; every timed update starts from the field of the old mask
(an untimed update back restores it) and its result is compared bit for bit with the new field's.
Output: one text table (profiles/field_update_time.txt).
Usage: python scripts/field_update_time.py [--out FILE] [--reps N] [--only far|midway|goal] [--call update|fresh]
(the last two: the rocprofv3 --kernel-trace --stats run)"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from art_planner_amd.context import Context  # noqa: E402
from synthetic import map_from_device, raw_map  # noqa: E402

N, N_YAW, EDGE = 400, 16, 40


def event_ms(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def to_dev(mask):
    import torch
    return torch.from_numpy(np.ascontiguousarray(mask.T).view(np.int32).reshape(-1)).to("cuda:0")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "field_update_time.txt"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", default="", help="one placement (for a kernel trace)")
    ap.add_argument("--call", default="", help="with --only: update or fresh alone")
    a = ap.parse_args()
    ctx = Context(0, "yaml")
    ctx.use_torch_stream()
    gm = map_from_device(ctx, raw_map(N, 0.04, seed=1234), "yaml")
    layers = [gm["elevation"], gm["elevation_masked"]]          # validity slots 0 (body) and 1 (feet)
    old = ctx.reachability_map(N_YAW)
    bits = ((old[..., None] >> np.arange(N_YAW, dtype=np.uint32)) & 1).astype(bool)
    nodes = np.argwhere(bits)
    goal = tuple(int(v) for v in nodes[np.argmin((nodes[:, 0] - N // 2) ** 2 + (nodes[:, 1] - N // 2) ** 2)])
    halo = ctx.reachability_halo()
    corners = {"far": (330, 330), "midway": (goal[0] + 60, goal[1] + 60),
               "goal": (goal[0] - EDGE // 2, goal[1] - EDGE // 2)}
    lines = [f"device {ctx.arch}", "",
             f"== artp_field_update against a new artp_field_compute on the same mask: {N}x{N} @ 0.04 m, n_yaw {N_YAW},",
             f"   objective 1, reverse field from the goal {goal}; a {EDGE} x {EDGE} rectangle of both validity layers",
             f"   rewritten, its mask recomputed with a halo of {halo} cells; ms per call (device events), median",
             f"   [min..max] of {a.reps}"]
    old_t = to_dev(old)
    for name, (r0, c0) in corners.items():
        if a.only and name != a.only:
            continue
        patches = []
        for lay in layers:
            p = np.array(lay[r0:r0 + EDGE, c0:c0 + EDGE], np.float32)
            p[8:32, 8:32] += np.float32(0.6)
            patches.append(p)
        for slot, p in enumerate(patches):
            ctx.update_layer_rects(slot, [p], [(r0, c0)])
        g0, g1 = max(r0 - halo, 0), max(c0 - halo, 0)
        sub = (g0, g1, min(r0 + EDGE + halo, N) - g0, min(c0 + EDGE + halo, N) - g1)
        new = old.copy()
        new[g0:g0 + sub[2], g1:g1 + sub[3]] = ctx.reachability_map(N_YAW, sub)
        new[goal[0], goal[1]] |= np.uint32(1 << goal[2])
        for slot, lay in enumerate(layers):                      # the next placement starts from the same map
            ctx.update_layer_rects(slot, [np.array(lay[r0:r0 + EDGE, c0:c0 + EDGE], np.float32)], [(r0, c0)])
        new_t = to_dev(new)
        fresh_ms, upd_ms, st, fst, want = [], [], None, None, None
        kw = dict(objective=1, reverse=True)
        if a.call != "update":
            for rep in range(a.reps + 2):
                box = {}

                def run():
                    box["f"] = ctx.cost_field(new_t, N_YAW, [goal], **kw)
                t = event_ms(run)
                if rep >= 2:
                    fresh_ms.append(t)
                fst = box["f"].stats()
                if rep == 0:
                    want = box["f"].dist()
                box["f"].close()
        if a.call != "fresh":
            with ctx.cost_field(old_t, N_YAW, [goal], **kw) as f:
                for rep in range(a.reps + 2):
                    box = {}

                    def run():
                        box["s"] = f.update(new_t, sub)
                    t = event_ms(run)
                    if rep >= 2:
                        upd_ms.append(t)
                    st = box["s"]
                    if rep == 0 and want is not None:
                        assert np.array_equal(f.dist().view(np.uint64), want.view(np.uint64))
                    f.update(old_t, sub)
        rows = [f"  {name}: rectangle at ({r0}, {c0}), sub_rect {sub}"]
        if fst:
            rows.append(f"      new field {np.median(fresh_ms):9.3f} ms [{min(fresh_ms):.3f}..{max(fresh_ms):.3f}]  "
                        f"{fst['outer_rounds']} + {fst['hop_rounds']} rounds, "
                        f"{fst['tile_launches']} + {fst['hop_tile_launches']} tile runs of {fst['tiles']} tiles, "
                        f"{fst['reached_nodes']} of {fst['nodes']} nodes reached")
        if st:
            rows.append(f"      update    {np.median(upd_ms):9.3f} ms [{min(upd_ms):.3f}..{max(upd_ms):.3f}]  "
                        f"{st['changed_words']} words changed (-{st['removed_nodes']} +{st['added_nodes']} nodes), "
                        f"dead {st['dead_nodes']}, hop-dead {st['hop_dead_nodes']}; rounds: unsupport "
                        f"{st['unsupport_rounds']}, dist {st['dist_rounds']}, hops {st['hop_rounds']}; "
                        f"{st['tile_launches']} tile runs")
        if fst and st:
            rows.append(f"      update / new field = {np.median(upd_ms) / np.median(fresh_ms):.3f}, same bits")
        for row in rows:
            print(row, flush=True)
        lines += rows
    ctx.close()
    text = "\n".join(lines) + "\n"
    if a.out and not a.only:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
