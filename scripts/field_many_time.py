"""Timing of the batched cost-to-go fields (artp_field_compute_many) against what a caller had before
them, in one run on one machine: on the C2 map (400x400 @ 0.04 m) and on an 800x800 @ 0.04 m map, both at n_yaw 16,
objective 1, the mask the map's own reachability mask on the device.  B = 1, 2, 4, 8, 16 single-source sets, the sources
the valid nodes nearest 16 points spread over the map (the first B of a fixed order that keeps small B spread out too).
Per B, alternating in every repetition:
  batch   one cost_fields call of B sets
  serial  B successive cost_field calls on the same sources
  lanes   the same B calls issued round-robin on the context's four lanes (one host thread: a lane is state of the
          context, and cost_field returns when its field is done)
Device events (on lane 0's stream) around batch and serial, the host's clock around all three (every call is synchronous,
so the host's time is the device's plus the launches and reads); two warm-ups, then the median of --reps.  Rounds and
tile runs per case from artp_field_stats.  Last, a 16-pose cost_matrix on the same sources.
Output: one text table (profiles/field_many_time.txt by default; the two sections at the end of the committed file, the
registers of the tile kernels and scripts/field_time.py on both commits, were added by hand).
Usage: python scripts/field_many_time.py [--out FILE] [--reps N] [--maps 400,800]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from art_planner_amd.context import Context  # noqa: E402
from synthetic import map_from_device, raw_map  # noqa: E402

ORDER = [5, 10, 0, 15, 3, 12, 6, 9, 1, 14, 2, 13, 4, 11, 7, 8]      # cells of a 4 x 4 grid of points over the map


def timed(fn):
    """(device ms between two events on the current torch stream, host ms) of fn()"""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3


def med(v):
    return f"{np.median(v):9.3f} [{min(v):.3f}..{max(v):.3f}]"


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "field_many_time.txt"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--maps", default="400,800")
    a = ap.parse_args()
    n_yaw = 16
    ctx = Context(0, "yaml")
    ctx.use_torch_stream()
    lines = [f"device {ctx.arch}", "",
             "== batched cost-to-go fields: ms per case, n_yaw 16, objective 1, single-source sets spread over the map,",
             f"   median [min..max] of {a.reps}; dev = device events on lane 0's stream, host = the host's clock"]
    for n in [int(v) for v in a.maps.split(",")]:
        gm = map_from_device(ctx, raw_map(n, 0.04, seed=1234 if n == 400 else 99), "yaml")
        mask = torch.zeros(gm.rows * gm.cols, dtype=torch.int32, device="cuda:0")
        ctx.reachability_map_dev(mask, n_yaw)
        torch.cuda.synchronize()
        m = mask.cpu().numpy().view(np.uint32).reshape(gm.cols, gm.rows).T
        nodes = np.argwhere(((m[..., None] >> np.arange(n_yaw, dtype=np.uint32)) & 1).astype(bool))
        pts = [((2 * (g % 4) + 1) * n // 8, (2 * (g // 4) + 1) * n // 8) for g in ORDER]
        srcs = [tuple(int(v) for v in nodes[np.argmin((nodes[:, 0] - r) ** 2 + (nodes[:, 1] - c) ** 2)]) for r, c in pts]
        assert len(set(srcs)) == 16
        lines += ["", f"  {n}x{n}, {len(nodes)} nodes in the mask"]
        print(lines[-1], flush=True)
        for B in (1, 2, 4, 8, 16):
            sets = [[s] for s in srcs[:B]]
            ms = {k: [] for k in ("batch dev", "batch host", "serial dev", "serial host", "lanes host")}
            stats = {}
            for rep in range(a.reps + 2):
                box = {}

                def batch():
                    box["many"] = ctx.cost_fields(mask, n_yaw, sets, objective=1)

                def serial():
                    box["serial"] = [ctx.cost_field(mask, n_yaw, s, objective=1) for s in sets]

                def lanes():
                    out = []
                    for b, s in enumerate(sets):
                        ctx.set_lane(b % 4)
                        out.append(ctx.cost_field(mask, n_yaw, s, objective=1))
                    ctx.set_lane(0)
                    box["lanes"] = out

                for name, fn in (("batch", batch), ("serial", serial), ("lanes", lanes)):
                    dev, host = timed(fn)
                    if rep >= 2:
                        ms[name + " host"].append(host)
                        if name != "lanes":
                            ms[name + " dev"].append(dev)
                if rep == 0:
                    for f, g in zip(box["many"], box["serial"]):
                        assert np.array_equal(f.dist().view(np.uint64), g.dist().view(np.uint64))
                stats = {k: [f.stats() for f in box[k]] for k in ("many", "serial")}
                for k in ("many", "serial", "lanes"):
                    for f in box[k]:
                        f.close()
            sm, ss = stats["many"], stats["serial"]
            rows = [f"    B = {B:2d}",
                    f"      batch   dev {med(ms['batch dev'])}  host {med(ms['batch host'])}   "
                    f"{max(s['outer_rounds'] for s in sm)} + {max(s['hop_rounds'] for s in sm)} rounds, "
                    f"{sum(s['tile_launches'] for s in sm)} + {sum(s['hop_tile_launches'] for s in sm)} tile runs",
                    f"      serial  dev {med(ms['serial dev'])}  host {med(ms['serial host'])}   "
                    f"{sum(s['outer_rounds'] for s in ss)} + {sum(s['hop_rounds'] for s in ss)} rounds, "
                    f"{sum(s['tile_launches'] for s in ss)} + {sum(s['hop_tile_launches'] for s in ss)} tile runs",
                    f"      lanes   {'':33s}  host {med(ms['lanes host'])}",
                    f"      serial / batch = {np.median(ms['serial dev']) / np.median(ms['batch dev']):.2f}x (dev), "
                    f"lanes / batch = {np.median(ms['lanes host']) / np.median(ms['batch host']):.2f}x (host); "
                    f"batch per field {np.median(ms['batch dev']) / B:.3f} ms"]
            lines += rows
            print("\n".join(rows), flush=True)
        mat = {"dev": [], "host": []}
        for rep in range(a.reps + 2):
            box = {}

            def matrix():
                box["m"] = ctx.cost_matrix(mask, n_yaw, srcs, objective=1, return_stats=True)
            dev, host = timed(matrix)
            if rep >= 2:
                mat["dev"].append(dev)
                mat["host"].append(host)
        st = box["m"][1]
        row = (f"    cost_matrix of 16 poses: dev {med(mat['dev'])}  host {med(mat['host'])}   {st['groups']} group(s), "
               f"{st['dist_rounds']} + {st['hop_rounds']} rounds, {st['tile_runs']} + {st['hop_tile_runs']} tile runs, "
               f"{int(np.isfinite(box['m'][0]).sum())} of 256 entries finite")
        lines.append(row)
        print(row, flush=True)
        del mask
    ctx.close()
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
