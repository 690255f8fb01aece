#!/usr/bin/env python3
"""Learned motion cost, the full-width network (network.py, blob version 2) against the light one (network_light.py, version 1),
measured in the same run: feature-extractor time per map at C3 (400^2) and C4 (800^2) -- the two launches of
artp_cost_update_map_dev, timed with events on the context's stream -- with the network's dense f16 FLOPs as a fraction of the
MI355X's 2.5 PFLOP/s peak, and the per-edge MLP's queries per second (artp_cost_query_dev on 2^20 edges).  Seeded weights
(convert_weights.random_params); the timing does not depend on their values.
usage: python scripts/cost_full_time.py [out.txt]     (default profiles/cost_full_time.txt)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import convert_weights as cw  # noqa: E402
from art_planner_amd.context import Context  # noqa: E402
from synthetic import make_map  # noqa: E402

PEAK = 2.5e15   # MI355X dense f16 matrix peak, FLOP/s
REPS, WARM, B = 50, 5, 1 << 20


def cnn_flops(shapes, n):
    """2 x MACs of network.CNNpart on an n x n map, every layer as the network defines it (conv1 and conv2 separately)."""
    h = n
    total = 0
    for name, pool in (("init_conv1", 0), ("init_conv2", 2), ("init_conv3", 0), ("init_conv4", 3), ("init_conv5", 0),
                       ("init_flatten", 0)):
        co, ci, kh, kw = shapes[name]
        h = h - kh + 1
        total += 2 * co * ci * kh * kw * h * h
        if pool == 2:
            h //= 2
        elif pool == 3:
            h -= 2
    return total


def time_stream(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / reps   # us


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "cost_full_time.txt")
    ctx = Context(0, "yaml")
    ctx.use_torch_stream()
    lines = [f"# scripts/cost_full_time.py on {torch.cuda.get_device_name(0)} ({ctx.arch}); {REPS} timed updates after {WARM} "
             f"warm-up ones per case, events on the stream; FC: artp_cost_query_dev on {B} edges",
             f"{'network':8s} {'map':>5s} {'features':>9s} {'CNN us':>9s} {'GFLOP':>8s} {'of 2.5 PF':>9s} {'FC Mq/s':>9s} {'fc path':>8s}"]
    rng = np.random.default_rng(0)
    for tag, shapes in (("light", cw.SHAPES), ("full", cw.SHAPES_FULL)):
        ctx.cost_load_weights(cw.to_blob(cw.random_params(0, shapes)))
        for n, seed in ((400, 1234), (800, 77)):
            gm = make_map(n, 0.04, seed=seed)
            elv = torch.from_numpy(np.ascontiguousarray(gm["elevation"][::-1, ::-1]).astype(np.float32)).cuda()
            us = time_stream(lambda: ctx.cost_update_map_dev(elv, gm.res, gm.len_x, gm.len_y), REPS)
            F = ctx.cost_features().shape[0]
            fl = cnn_flops(shapes, n)
            s = rng.uniform(-0.5 * gm.len_x, 0.5 * gm.len_x, (B, 2))
            d = rng.uniform(-0.6, 0.6, (B, 2))
            e = np.stack([s[:, 0] + d[:, 0], s[:, 1] + d[:, 1], rng.uniform(-np.pi, np.pi, B), s[:, 0], s[:, 1],
                          rng.uniform(-np.pi, np.pi, B)], 1).astype(np.float32)
            et = torch.from_numpy(e).cuda()
            ct = torch.empty((B, 3), dtype=torch.float32, device="cuda")
            fc_us = time_stream(lambda: ctx.cost_query_dev(et, ct), 20)
            path = "mfma" if ctx.cost_fc_path()["mfma"] else "fp32"
            lines.append(f"{tag:8s} {n:5d} {F:4d}^2    {us:9.1f} {fl / 1e9:8.1f} {fl / (us * 1e-6) / PEAK:9.3f} "
                         f"{B / (fc_us * 1e-6) / 1e6:9.1f} {path:>8s}")
            print(lines[-1], flush=True)
    ctx.close()
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    open(out_path, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
