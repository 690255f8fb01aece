"""Timing of artp_field_shift_clearance against its two alternatives on the same state, in one run on one machine: a new
artp_field_compute_clearance on the new map, and artp_field_shift of a plain field across the same move.
The world, the windows and the moves of scripts/field_shift_time.py: a Perlin world of 440 x 440 cells at 0.04 m, the map a
400 x 400 window of it, n_yaw 16, objective 1, a reverse field from one goal, every window through the device's
preprocessing and with its own reachability mask; shifts of (4, 0), (16, -8) and (40, 40) cells, one goal AHEAD of the
motion and one BEHIND it.  Clearance: radius 12, margin 0.2 m, gain 2.  Masks live on the device for every call.  Device
events around each whole call, median and min..max of 5 after a warm-up; every timed call starts from a field computed on
the old window, and its result is compared bit for bit with the new field's.  The call's own split (move_ms, clearance_ms,
table_ms, passes_ms) is the last repetition's.
Output: one text table (profiles/field_shift_clearance_time.txt).
Usage: python scripts/field_shift_clearance_time.py [--out FILE] [--reps N]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from art_planner_amd.context import Context  # noqa: E402
from synthetic import GridMap, map_from_device, raw_map  # noqa: E402

N, N_YAW, RES, PAD = 400, 16, 0.04, 40
CLEAR = dict(radius_cells=12, margin=0.2, gain=2.0)


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "field_shift_clearance_time.txt"))
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    ctx = Context(0, "yaml")
    ctx.use_torch_stream()
    world = raw_map(N + PAD, RES, seed=1234)

    def install(corner):
        """The window whose cell (0, 0) is world cell `corner` as the context's map; a window further up the rows lies
        further along +x."""
        top, left = corner
        raw = GridMap(N, N, RES, 1.0 - top * RES, -0.5 - left * RES)
        for name in ("elevation", "traversability"):
            raw.add(name, np.ascontiguousarray(world[name][top:top + N, left:left + N]))
        map_from_device(ctx, raw, "yaml")

    lines = [f"device {ctx.arch}", "",
             f"== artp_field_shift_clearance against a new artp_field_compute_clearance on the same new map and against",
             f"   artp_field_shift of a plain field across the same move: {N}x{N} @ {RES} m windows of a {N + PAD}x{N + PAD} Perlin",
             f"   world, n_yaw {N_YAW}, objective 1, reverse field from one goal, radius {CLEAR['radius_cells']}, margin {CLEAR['margin']}, "
             f"gain {CLEAR['gain']}; each window's",
             f"   own reachability mask; ms per call (device events), median [min..max] of {a.reps}"]
    kw = dict(objective=1, reverse=True)
    for si, sj in ((4, 0), (16, -8), (40, 40)):
        old_c = (max(si, 0), max(sj, 0))                         # old node (r, c) is new node (r + si, c + sj):
        new_c = (old_c[0] - si, old_c[1] - sj)                   # the new window's corner is the old one's minus the shift
        install(old_c)
        old = ctx.reachability_map(N_YAW)
        install(new_c)
        new = ctx.reachability_map(N_YAW)
        both = (old[max(0, -si):N - max(0, si), max(0, -sj):N - max(0, sj), None] >> np.arange(N_YAW, dtype=np.uint32)) & \
               (new[max(0, si):N - max(0, -si), max(0, sj):N - max(0, -sj), None] >> np.arange(N_YAW, dtype=np.uint32)) & 1
        nodes = np.argwhere(both) + (max(0, -si), max(0, -sj), 0)   # old triples that are nodes of both masks
        old_t, new_t = to_dev(old), to_dev(new)
        # cells enter where the new index is low (si > 0) or high (si < 0): that side is ahead of the motion
        side = lambda s, ahead: N // 2 if s == 0 else (N // 4 if (s > 0) == ahead else 3 * N // 4 - abs(s))
        for where in ("ahead", "behind"):
            want_rc = (side(si, where == "ahead"), side(sj, where == "ahead"))
            goal = tuple(int(v) for v in nodes[np.argmin((nodes[:, 0] - want_rc[0]) ** 2 + (nodes[:, 1] - want_rc[1]) ** 2)])
            goal_new = (goal[0] + si, goal[1] + sj, goal[2])
            fresh_ms, shift_ms, plain_ms, st, fst, want = [], [], [], None, None, None
            for rep in range(a.reps + 1):
                box = {}

                def run():
                    box["f"] = ctx.clearance_cost_field(new_t, N_YAW, [goal_new], **kw, **CLEAR)
                t = event_ms(run)
                if rep >= 1:
                    fresh_ms.append(t)
                fst = box["f"].stats()
                if rep == 0:
                    want = box["f"].dist()
                box["f"].close()
            for rep in range(a.reps + 1):
                install(old_c)
                with ctx.clearance_cost_field(old_t, N_YAW, [goal], **kw, **CLEAR) as f:
                    install(new_c)
                    if rep == 0:
                        f.shift_clearance(old_t if (si, sj) == (0, 0) else new_t)   # (the second table is allocated once a field)
                        assert np.array_equal(f.dist().view(np.uint64), want.view(np.uint64))
                        continue
                    box = {}

                    def run():
                        box["s"] = f.shift_clearance(new_t)
                    shift_ms.append(event_ms(run))
                    st = box["s"]
                    assert np.array_equal(f.dist().view(np.uint64), want.view(np.uint64))
            for rep in range(a.reps + 1):
                install(old_c)
                with ctx.cost_field(old_t, N_YAW, [goal], **kw) as f:
                    install(new_c)
                    box = {}

                    def run():
                        box["s"] = f.shift(new_t)
                    t = event_ms(run)
                    if rep >= 1:
                        plain_ms.append(t)
                    sp = box["s"]
            med = np.median(shift_ms)
            rows = [f"  shift ({si}, {sj}), goal {where} at {goal} -> {goal_new}",
                    f"      new clearance field {np.median(fresh_ms):9.3f} ms [{min(fresh_ms):.3f}..{max(fresh_ms):.3f}]  "
                    f"{fst['outer_rounds']} + {fst['hop_rounds']} rounds, "
                    f"{fst['tile_launches']} + {fst['hop_tile_launches']} tile runs of {fst['tiles']} tiles, "
                    f"{fst['reached_nodes']} of {fst['nodes']} nodes reached",
                    f"      plain shift         {np.median(plain_ms):9.3f} ms [{min(plain_ms):.3f}..{max(plain_ms):.3f}]  "
                    f"passes {sp['passes_ms']:.3f} ms; dead_nodes {sp['dead_nodes']}; tile_launches {sp['tile_launches']}",
                    f"      shift_clearance     {med:9.3f} ms [{min(shift_ms):.3f}..{max(shift_ms):.3f}]  "
                    f"move {st['move_ms']:.3f} ms, clearance {st['clearance_ms']:.3f} ms, table {st['table_ms']:.3f} ms, "
                    f"passes {st['passes_ms']:.3f} ms; {st['changed_words']} words changed "
                    f"(-{st['removed_nodes']} +{st['added_nodes']} nodes), {st['left_nodes']} nodes left, "
                    f"{st['changed_slots']} slots changed in {st['weight_tiles']} tiles, "
                    f"dead_nodes {st['dead_nodes']}, hop-dead {st['hop_dead_nodes']}; rounds: unsupport "
                    f"{st['unsupport_rounds']}, dist {st['dist_rounds']}, hops {st['hop_rounds']}; "
                    f"tile_launches {st['tile_launches']}",
                    f"      shift_clearance / new clearance field = {med / np.median(fresh_ms):.3f}, "
                    f"/ plain shift = {med / np.median(plain_ms):.3f}, same bits"]
            for row in rows:
                print(row, flush=True)
            lines += rows
    ctx.close()
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
