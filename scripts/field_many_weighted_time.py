"""Timing of the batched learned and clearance-weighted cost fields (artp_field_compute_many_learned / _clearance, DESIGN.md
section 24) against what a caller had before them, in one run on one machine: the C2 map (400x400 @ 0.04 m) at n_yaw 16,
the mask the map's own reachability mask on the device, the light network with the seeded random parameters of the cost
tests on the map's own heights (risk_threshold 1: every edge feasible), clearance at radius 12 (margin 0.2, gain 2,
objective 1).  B = 1, 2, 4, 8, 16 single-source sets, the sources of scripts/field_many_time.py.
Per kind and B, alternating in every repetition:
  batch   one learned_cost_fields / clearance_cost_fields call of B sets
  serial  B successive learned_cost_field / clearance_cost_field calls on the same sources
Device events around each whole call (allocations, table build, copies and hop-count search included); two warm-ups, then
the median of --reps, and that --repeats times: a case's line shows every repeat's median and "spread" is max - min of
those medians.  Rounds and tile runs per case from artp_field_stats, the table build's own time from
artp_field_learned_stats (device events inside the call).  Last, the learned cost matrix of the 16 sources.
--plain measures the plain batch instead (cost_fields, objective 1, B = 8, the same repeats) and prints one line: run in
this checkout and in the parent commit's (there with the same loop on its own package: the parent's library lacks this
commit's symbols and does not load here), alternating in one session, it is the plain-batch comparison of section 24.
Output: one text table (profiles/field_many_weighted_time.txt by default).  What the output file holds from its first
line that starts with "== added by hand" on is kept: the committed file's registers of the tile kernels, the two grid
placements (a development build that is not in the tree) and the plain-batch comparison were added that way.
Usage: python scripts/field_many_weighted_time.py [--out FILE] [--reps N] [--repeats N] [--bs 1,2,4,8,16]
       [--kinds learned,clearance] [--plain]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools")]

import convert_weights as cw  # noqa: E402
import cost_exact_ref as R  # noqa: E402
import motion_cost_oracle as mo  # noqa: E402
from art_planner_amd.context import Context  # noqa: E402
from field_many_time import ORDER, timed  # noqa: E402
from synthetic import map_from_device, raw_map  # noqa: E402


def show(meds):
    return " ".join(f"{v:9.3f}" for v in meds) + f"  spread {max(meds) - min(meds):.3f}"


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "field_many_weighted_time.txt"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--bs", default="1,2,4,8,16")
    ap.add_argument("--kinds", default="learned,clearance")
    ap.add_argument("--plain", action="store_true", help="cost_fields at B = 8 alone, one line on stdout")
    a = ap.parse_args()
    n, n_yaw, res = 400, 16, 0.04
    ctx = Context(0, "yaml")
    ctx.use_torch_stream()
    raw = raw_map(n, res, seed=1234)
    gm = map_from_device(ctx, raw, "yaml")
    ctx.cost_load_weights(cw.to_blob(mo.random_params(0, R.shapes_of(1))))
    elev = np.nan_to_num(np.asarray(raw["elevation"], np.float32))
    ctx.cost_update_map(np.ascontiguousarray(elev[::-1, ::-1]), res, n * res, n * res, gm.pos_x, gm.pos_y)
    mask = torch.zeros(gm.rows * gm.cols, dtype=torch.int32, device="cuda:0")
    ctx.reachability_map_dev(mask, n_yaw)
    torch.cuda.synchronize()
    m = mask.cpu().numpy().view(np.uint32).reshape(gm.cols, gm.rows).T
    nodes = np.argwhere(((m[..., None] >> np.arange(n_yaw, dtype=np.uint32)) & 1).astype(bool))
    pts = [((2 * (g % 4) + 1) * n // 8, (2 * (g // 4) + 1) * n // 8) for g in ORDER]
    srcs = [tuple(int(v) for v in nodes[np.argmin((nodes[:, 0] - r) ** 2 + (nodes[:, 1] - c) ** 2)]) for r, c in pts]
    assert len(set(srcs)) == 16
    if a.plain:
        sets, meds = [[s] for s in srcs[:8]], []
        for repeat in range(a.repeats):
            ms = []
            for rep in range(a.reps + (2 if repeat == 0 else 0)):
                box = {}

                def plain():
                    box["f"] = ctx.cost_fields(mask, n_yaw, sets, objective=1)
                dev, _ = timed(plain)
                if repeat or rep >= 2:
                    ms.append(dev)
                for f in box["f"]:
                    f.close()
            meds.append(float(np.median(ms)))
        print(f"cost_fields B = 8: {show(meds)}", flush=True)
        del mask
        ctx.close()
        return
    calls = {"learned": (lambda s: ctx.learned_cost_fields(mask, n_yaw, s, risk_threshold=1.0),
                         lambda s: ctx.learned_cost_field(mask, n_yaw, s, risk_threshold=1.0)),
             "clearance": (lambda s: ctx.clearance_cost_fields(mask, n_yaw, s, radius_cells=12, objective=1),
                           lambda s: ctx.clearance_cost_field(mask, n_yaw, s, radius_cells=12, objective=1))}
    lines = [f"device {ctx.arch}", "",
             f"== batched weighted cost fields: device ms per case, 400x400, n_yaw 16, {len(nodes)} nodes in the mask,",
             f"   single-source sets spread over the map; per line the medians of {a.reps} of {a.repeats} repeats"]
    for kind in a.kinds.split(","):
        many, single = calls[kind]
        lines += ["", f"  {kind}"]
        print(lines[-1], flush=True)
        for B in [int(v) for v in a.bs.split(",")]:
            sets = [[s] for s in srcs[:B]]
            meds = {"batch": [], "serial": []}
            build = {"batch": [], "serial": []}
            stats = {}
            for repeat in range(a.repeats):
                ms = {"batch": [], "serial": []}
                for rep in range(a.reps + (2 if repeat == 0 else 0)):
                    box = {}

                    def batch():
                        box["batch"] = many(sets)

                    def serial():
                        box["serial"] = [single(s) for s in sets]

                    for name, fn in (("batch", batch), ("serial", serial)):
                        dev, _ = timed(fn)
                        if repeat or rep >= 2:
                            ms[name].append(dev)
                            ls = [f.learned_stats() for f in box[name]]
                            per = [x["rows_ms"] + x["query_ms"] + x["combine_ms"] for x in ls]
                            build[name].append(per[0] if name == "batch" else sum(per))
                    if repeat == 0 and rep == 0:
                        for f, g in zip(box["batch"], box["serial"]):
                            assert np.array_equal(f.dist().view(np.uint64), g.dist().view(np.uint64))
                    stats = {k: [f.stats() for f in box[k]] for k in ("batch", "serial")}
                    for k in ("batch", "serial"):
                        for f in box[k]:
                            f.close()
                for k in ms:
                    meds[k].append(float(np.median(ms[k])))
            sm, ss = stats["batch"], stats["serial"]
            mb, msr = float(np.median(meds["batch"])), float(np.median(meds["serial"]))
            spread = max(max(v) - min(v) for v in meds.values())
            rounds = max(s["outer_rounds"] for s in sm) + max(s["hop_rounds"] for s in sm)
            bb, bs = float(np.median(build["batch"])), float(np.median(build["serial"]))
            rows = [f"    B = {B:2d}",
                    f"      batch   {show(meds['batch'])}   {max(s['outer_rounds'] for s in sm)} + "
                    f"{max(s['hop_rounds'] for s in sm)} rounds, {sum(s['tile_launches'] for s in sm)} + "
                    f"{sum(s['hop_tile_launches'] for s in sm)} tile runs; table build {bb:.3f} ms (once)",
                    f"      serial  {show(meds['serial'])}   {sum(s['outer_rounds'] for s in ss)} + "
                    f"{sum(s['hop_rounds'] for s in ss)} rounds, {sum(s['tile_launches'] for s in ss)} + "
                    f"{sum(s['hop_tile_launches'] for s in ss)} tile runs; table builds {bs:.3f} ms ({B} times)",
                    f"      serial - batch = {msr - mb:.3f} ms against a spread of {spread:.3f} ms; serial / batch = "
                    f"{msr / mb:.2f}x; batch per field {mb / B:.3f} ms; batch search (call - build) per round "
                    f"{(mb - bb) / rounds:.3f} ms"]
            lines += rows
            print("\n".join(rows), flush=True)
    if "learned" in a.kinds.split(","):
        meds = []
        for repeat in range(a.repeats):
            mat = []
            for rep in range(a.reps + (2 if repeat == 0 else 0)):
                box = {}

                def matrix():
                    box["m"] = ctx.learned_cost_matrix(mask, n_yaw, srcs, risk_threshold=1.0, return_stats=True)
                dev, _ = timed(matrix)
                if repeat or rep >= 2:
                    mat.append(dev)
            meds.append(float(np.median(mat)))
        st = box["m"][1]
        row = (f"    learned_cost_matrix of 16 poses: {show(meds)}   {st['groups']} group(s), {st['dist_rounds']} + "
               f"{st['hop_rounds']} rounds, {st['tile_runs']} + {st['hop_tile_runs']} tile runs, table built "
               f"{st['table_builds']} time(s) in {st['build_ms']:.3f} ms, {st['table_copies']} copies, "
               f"{int(np.isfinite(box['m'][0]).sum())} of 256 entries finite")
        lines += ["", row]
        print(row, flush=True)
    del mask
    ctx.close()
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        if os.path.exists(a.out):   # the sections added by hand stay
            old = open(a.out).read()
            at = old.find("\n== added by hand")
            if at >= 0:
                text += old[at:]
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
