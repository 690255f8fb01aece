#!/usr/bin/env python3
"""Golden vectors and the fp16 anchor for the FULL-WIDTH motion-cost network (network.py, n9convNetwork3LR: the class
of grid-1563-blind.pt, grid-1975-blind.pt and grid-1992-perceptive.pt), produced by the REFERENCE network class.

Needs the reference checkout: imports art_planner_motion_cost/src/art_planner_motion_cost/predictor/network.py where it
lies (nothing is copied).  usage: make_golden_cost_full.py <that predictor directory>
The same inputs and the same procedure as make_golden_cost.py / make_golden_cost_anchor.py, with the seeded parameters
random_params(0, SHAPES_FULL):
  motion_cost_full.npz      the 112 x 112 crop -> [64, 32, 32] features (CNNpart, float32 on CPU) + FCpart outputs of
                            4096 seeded edges
  motion_cost_full_120.npz  the 120 x 120 crop -> [64, 36, 36] (partial tiles in the HIP kernels) + 4096 edges' costs
  motion_cost_full_fp16_anchor.json  the reference's own torch.half-vs-float32 error on those crops and on the maps and
                            edges of tests/test_motion_cost_full.py (statistics only)
"""
import copy
import json
import os
import sys

sys.dont_write_bytecode = True  # the reference tree is read-only: no __pycache__ next to its sources

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
if __name__ == "__main__":
    sys.path.insert(0, os.path.abspath(sys.argv[1]))   # the reference's predictor/ directory
import motion_cost_oracle as mo  # noqa: E402
import convert_weights as cw  # noqa: E402
import network  # noqa: E402  (the reference's full-width class)
from make_golden_cost_anchor import fc, stats  # noqa: E402  (FCpart with torch.ones' cuda device patched out, network.py:162)
from synthetic import make_map  # noqa: E402


def seeded_edges(seed, B, L):
    rng = np.random.default_rng(seed)
    s = rng.uniform(-L / 2, L / 2, (B, 2))
    d = rng.uniform(-0.6, 0.6, (B, 2))
    syaw = rng.uniform(-np.pi, np.pi, B)
    tyaw = rng.uniform(-np.pi, np.pi, B)
    return np.stack([s[:, 0] + d[:, 0], s[:, 1] + d[:, 1], tyaw, s[:, 0], s[:, 1], syaw], 1).astype(np.float32)


def map_edges(gm, n):
    """the edges of test_gpu_full_features_and_costs_match_oracle_at_c3_c4_and_odd_sizes"""
    rng = np.random.default_rng(n)
    B = 20000
    s = rng.uniform(-0.55 * gm.len_x, 0.55 * gm.len_x, (B, 2))
    d = rng.uniform(-0.6, 0.6, (B, 2))
    return np.stack([s[:, 0] + d[:, 0], s[:, 1] + d[:, 1], rng.uniform(-np.pi, np.pi, B), s[:, 0], s[:, 1],
                     rng.uniform(-np.pi, np.pi, B)], 1).astype(np.float32)


def main():
    params = mo.random_params(0, cw.SHAPES_FULL)
    net = network.network().eval()
    sd = net.state_dict()
    for k in sd:
        if not k.endswith("num_batches_tracked"):
            assert tuple(sd[k].shape) == params[k].shape, (k, tuple(sd[k].shape), params[k].shape)
            sd[k] = torch.from_numpy(params[k].copy())
    net.load_state_dict(sd)
    net16 = copy.deepcopy(net).half()

    gm = make_map(400, 0.04, seed=1234)
    elv = np.ascontiguousarray(gm["elevation"][::-1, ::-1]).astype(np.float32)   # server convention, as make_golden_cost.py
    res = 0.04
    anchor = {"what": "reference network.network (full width) on CPU: torch.half evaluation (predictor.py:22,34,44) vs its "
                      "own float32 evaluation, same weights (convert_weights.random_params(0, SHAPES_FULL)), same inputs as "
                      "tests/test_motion_cost_full.py",
              "torch": torch.__version__, "cases": {}}
    for name, n, y0, x0, seed, C_F in (("motion_cost_full.npz", 112, 140, 60, 5, 32),
                                       ("motion_cost_full_120.npz", 120, 30, 250, 6, 36)):
        crop = elv[y0:y0 + n, x0:x0 + n].astype(np.float16).astype(np.float32)   # exactly representable in fp16
        with torch.no_grad():
            feats = net.CNNpart(torch.from_numpy(crop).view(1, 1, n, n))
        assert tuple(feats.shape) == (1, 64, C_F, C_F), feats.shape
        edges = seeded_edges(seed, 4096, n * res)
        costs = fc(net, feats, edges, res, n * res, False)
        f_np = feats.numpy()[0]
        f_o = mo.cnn_features(params, crop)
        c_o = mo.fc_costs(params, f_np, edges, res, n * res, n * res)
        print(name, "max |oracle-ref| features", np.abs(f_o - f_np).max(), "costs", np.abs(c_o - costs).max())
        assert np.abs(f_o - f_np).max() < 2e-3 * max(1.0, np.abs(f_np).max())
        assert np.abs(c_o - costs).max() < 1e-3
        np.savez_compressed(os.path.join(HERE, name), crop=crop.astype(np.float16), res=res, features=f_np.astype(np.float32),
                            edges=edges, costs=costs.astype(np.float32))
        anchor["cases"][f"golden_{n}"] = stats(net, net16, crop, res, edges)
        print(f"golden_{n}", json.dumps(anchor["cases"][f"golden_{n}"]))
    for n in (400, 800, 141, 97):
        gmn = make_map(n, 0.04, seed=1234 if n == 400 else 77)
        e = np.ascontiguousarray(gmn["elevation"][::-1, ::-1]).astype(np.float16).astype(np.float32)
        anchor["cases"][f"map_{n}"] = stats(net, net16, e, gmn.res, map_edges(gmn, n))
        print(n, json.dumps(anchor["cases"][f"map_{n}"]))
    json.dump(anchor, open(os.path.join(HERE, "motion_cost_full_fp16_anchor.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
