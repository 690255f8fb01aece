"""Timing of the learned-cost fields (artp_field_compute_learned) against the objective-1 field of
the same run: the C2 map (400x400 @ 0.04 m), its own reachability mask on the device, 16 headings, one source (the valid
node nearest the centre), the light network with the seeded random parameters of the cost tests on the map's own
heights.  Device events around each whole call (allocations, table build and hop-count search included), 10 repetitions
after two warm-ups, the two objectives alternating.  From artp_field_learned_stats: the three steps of the table build
(device events inside the call) and the two searches (host time: every round is read by the host); from
artp_field_stats: rounds and tile runs; ms per live round = search time / rounds.
Output: one text table (profiles/field_learned_time.txt).
Usage: python scripts/field_learned_time.py [--out FILE] [--reps N] [--n 400] [--only learned|objective1]  (--only: the
rocprofv3 --kernel-trace --stats run)"""
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
from field_time import event_ms  # noqa: E402
from synthetic import map_from_device, raw_map  # noqa: E402


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "field_learned_time.txt"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--n", type=int, default=400)
    ap.add_argument("--only", default="", help="learned or objective1 alone (for a kernel trace)")
    a = ap.parse_args()
    n, n_yaw, res = a.n, 16, 0.04
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
    bits = ((m[..., None] >> np.arange(n_yaw, dtype=np.uint32)) & 1).astype(bool)
    nodes = np.argwhere(bits)
    src = [tuple(int(v) for v in nodes[np.argmin((nodes[:, 0] - n // 2) ** 2 + (nodes[:, 1] - n // 2) ** 2)])]
    # every edge feasible (the risk is at most 1): the learned field reaches what the objective-1 field reaches
    make = {"objective1": lambda: ctx.cost_field(mask, n_yaw, src, objective=1),
            "learned": lambda: ctx.learned_cost_field(mask, n_yaw, src, risk_threshold=1.0)}
    kinds = [k for k in ("objective1", "learned") if not a.only or k == a.only]
    ms = {k: [] for k in kinds}
    parts = {k: [] for k in kinds}
    stats = {}
    for rep in range(a.reps + 2):
        for k in kinds:
            box = {}

            def run():
                box["f"] = make[k]()
            t = event_ms(run)
            if rep >= 2:
                ms[k].append(t)
                parts[k].append(box["f"].learned_stats())
            stats[k] = box["f"].stats()
            box["f"].close()
    lines = [f"device {ctx.arch}", "",
             f"== fields on the {n}x{n} map @ {res} m, n_yaw {n_yaw}, one source at the centre: ms per call (device events),",
             f"   median [min..max] of {a.reps}, the objectives alternating; parts: medians of the same calls"]
    for k in kinds:
        s, t = stats[k], ms[k]
        med = {name: float(np.median([p[name] for p in parts[k]])) for name in parts[k][0]}
        lines.append(f"  {k:10s} {np.median(t):9.3f} ms [{min(t):.3f}..{max(t):.3f}]  {s['nodes']} nodes, {s['reached_nodes']} reached")
        if k == "learned":
            rows = int(med["table_rows"])
            lines.append(f"      table: {rows} rows ({med['table_bytes'] / 1e6:.0f} MB) in {int(med['chunks'])} chunks: rows "
                         f"{med['rows_ms']:.3f} ms, query {med['query_ms']:.3f} ms ({rows / max(med['query_ms'], 1e-9) * 1e3:.3e} "
                         f"rows/s), combine {med['combine_ms']:.3f} ms")
        lines.append(f"      distances: {med['dist_ms']:.3f} ms, {s['outer_rounds']} rounds, {s['tile_launches']} tile runs of "
                     f"{s['tiles']} tiles: {med['dist_ms'] / max(s['outer_rounds'], 1):.4f} ms per round")
        lines.append(f"      hop counts: {med['hop_ms']:.3f} ms, {s['hop_rounds']} rounds, {s['hop_tile_launches']} tile runs: "
                     f"{med['hop_ms'] / max(s['hop_rounds'], 1):.4f} ms per round")
    ctx.close()
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out and not a.only:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
