"""Timing of artp_field_update_clearance against a new artp_field_compute_clearance on the same
mask, in one run on one machine: the C2 map (400x400 @ 0.04 m), n_yaw 16, a reverse field from one goal (the valid node
nearest the centre), base objective 1, radius_cells 12 and the default margin and gain.
The change is what a replanning cycle produces: a 40 x 40 rectangle of both validity layers is rewritten (a block of
+0.6 m on its inner 24 x 24 cells) with update_layer_rects, reachability_map recomputes that rectangle grown by
reachability_halo() and the result is pasted into the old mask.  Three placements of the rectangle: far from the goal,
midway, and around the goal (the goal's own bit kept set).  For the far placement also the call without a rectangle, which
computes the clearance map and the table of the whole map again.
Masks live on the device for both calls.  Device events around each whole call, median and min..max of 10 after two
warm-ups; every timed update starts from the field of the old mask (an untimed update back restores it) and its dist and
clearance map are compared bit for bit with the new field's.  From
artp_field_clearance_update_stats: the two windows with their device time (events inside the call) and the passes (host
time).
Output: one text table (profiles/field_clearance_update_time.txt).
Usage: python scripts/field_clearance_update_time.py [--out FILE] [--reps N] [--only far|midway|goal]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from art_planner_amd.context import Context  # noqa: E402
from field_update_time import event_ms, to_dev  # noqa: E402
from synthetic import map_from_device, raw_map  # noqa: E402

N, N_YAW, EDGE, RES, RADIUS = 400, 16, 40, 0.04, 12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "field_clearance_update_time.txt"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", default="", help="one placement")
    a = ap.parse_args()
    ctx = Context(0, "yaml")
    ctx.use_torch_stream()
    gm = map_from_device(ctx, raw_map(N, RES, seed=1234), "yaml")
    layers = [gm["elevation"], gm["elevation_masked"]]          # validity slots 0 (body) and 1 (feet)
    old = ctx.reachability_map(N_YAW)
    bits = ((old[..., None] >> np.arange(N_YAW, dtype=np.uint32)) & 1).astype(bool)
    nodes = np.argwhere(bits)
    goal = tuple(int(v) for v in nodes[np.argmin((nodes[:, 0] - N // 2) ** 2 + (nodes[:, 1] - N // 2) ** 2)])
    halo = ctx.reachability_halo()
    corners = {"far": (330, 330), "midway": (goal[0] + 60, goal[1] + 60),
               "goal": (goal[0] - EDGE // 2, goal[1] - EDGE // 2)}
    kw = dict(reverse=True, radius_cells=RADIUS)
    lines = [f"device {ctx.arch}", "",
             f"== artp_field_update_clearance against a new artp_field_compute_clearance on the same mask: {N}x{N} @ {RES} m,",
             f"   n_yaw {N_YAW}, reverse field from the goal {goal}, base objective 1, radius_cells {RADIUS}, default margin",
             f"   and gain; a {EDGE} x {EDGE} rectangle of both validity layers rewritten, its mask recomputed with a halo of",
             f"   {halo} cells; ms per call (device events), median [min..max] of {a.reps}"]
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
        fresh_ms, fst, fls, want = [], None, None, None
        for rep in range(a.reps + 2):
            box = {}

            def run():
                box["f"] = ctx.clearance_cost_field(new_t, N_YAW, [goal], **kw)
            t = event_ms(run)
            if rep >= 2:
                fresh_ms.append(t)
            fst, fls = box["f"].stats(), box["f"].learned_stats()
            if rep == 0:
                want = (box["f"].dist(), box["f"].clearance())
            box["f"].close()
        rows = [f"  {name}: rectangle at ({r0}, {c0}), sub_rect {sub}",
                f"      new field    {np.median(fresh_ms):9.3f} ms [{min(fresh_ms):.3f}..{max(fresh_ms):.3f}]  "
                f"clearance {fls['rows_ms']:.3f} + table {fls['combine_ms']:.3f} ms, searches "
                f"{fls['dist_ms']:.3f} + {fls['hop_ms']:.3f} ms; {fst['outer_rounds']} + {fst['hop_rounds']} rounds, "
                f"{fst['tile_launches']} + {fst['hop_tile_launches']} tile runs of {fst['tiles']} tiles"]
        for label, rect in (("update", sub),) + ((("update, no rect", None),) if name == "far" else ()):
            upd_ms, parts, st = [], [], None
            with ctx.clearance_cost_field(old_t, N_YAW, [goal], **kw) as f:
                for rep in range(a.reps + 2):
                    box = {}

                    def run():
                        box["s"] = f.update_clearance(new_t, rect)
                    t = event_ms(run)
                    st = box["s"]
                    if rep >= 2:
                        upd_ms.append(t)
                        parts.append(st)
                    if rep == 0:
                        assert np.array_equal(f.dist().view(np.uint64), want[0].view(np.uint64))
                        assert np.array_equal(f.clearance(), want[1])
                    f.update_clearance(old_t, rect)
            med = {k: float(np.median([p[k] for p in parts])) for k in ("clearance_ms", "reprice_ms", "passes_ms")}
            rows += [f"      {label:<16s} {np.median(upd_ms):9.3f} ms [{min(upd_ms):.3f}..{max(upd_ms):.3f}]  "
                     f"{st['clearance_tiles']} clearance tiles, changed_d2 {st['changed_d2']}; changed_slots / repriced_slots = "
                     f"{st['changed_slots']} / {st['repriced_slots']} ({st['changed_slots'] / st['repriced_slots']:.5f}), "
                     f"{st['weight_tiles']} weight tiles, {st['changed_words']} words changed "
                     f"(-{st['removed_nodes']} +{st['added_nodes']} nodes)",
                     f"                clearance {med['clearance_ms']:.3f} ms, reprice {med['reprice_ms']:.3f} ms, passes "
                     f"{med['passes_ms']:.3f} ms; dead {st['dead_nodes']}, hop-dead {st['hop_dead_nodes']}; rounds: unsupport "
                     f"{st['unsupport_rounds']}, dist {st['dist_rounds']}, hops {st['hop_rounds']}; {st['tile_launches']} tile runs",
                     f"      {label} / new field = {np.median(upd_ms) / np.median(fresh_ms):.3f}, same bits"]
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
