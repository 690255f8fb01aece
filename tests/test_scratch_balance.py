"""Temporary device memory of the planner front ends is given back: cycles of roadmap and tree work leave the device's
free memory where it was (csrc/device_scratch.h: temporaries by scope, members by their object's owner).

One cycle = for a batched roadmap under the learned objective (construction 0) and a predecessor-only one of direct edges
(construction 2, the d_k_of table): build, set_query, solve, solve_many with 4 goals, revalidate, grow by 50, destroy;
then a tree of batch 64 grown by 3 batches and destroyed.  The tree's motion log starts at 2^16 entries and three batches
of 64 log a few thousand, so these cycles allocate the log once and do not regrow it (tree_log_reserve's regrow and
its failure paths are exercised on the CPU, tests/test_device_scratch.py)."""
import os
import sys

import numpy as np
import pytest
import torch

import common

pytestmark = pytest.mark.gpu


def _cycle(ctx, start, goal, others):
    from art_planner_amd.roadmap import Roadmap
    from art_planner_amd.tree import Tree
    for kw in (dict(construction=0, objective=2, cost_weights=(0.25, 1.0, 5.0), risk_threshold=0.55),
               dict(construction=2, objective=0)):
        rm = Roadmap(ctx, start, goal, n_milestones=200, seed=5, **kw)
        rm.set_query(others[0], others[1])
        rm.solve()
        out = rm.solve_many(start, others[2:6])
        assert out["status"].shape == (4,)
        rm.revalidate()
        rm.grow(50)
        assert rm.stats()["vertices"] > 200
        rm.close()
    t = Tree(ctx, start, goal, "rrt_star", seed=3, batch=64)
    assert t.grow(3)["batches"] == 3
    t.close()


def test_roadmap_and_tree_cycles_leave_free_device_memory_unchanged():
    sys.path.insert(0, os.path.join(common.ROOT, "oracle"))
    sys.path.insert(0, os.path.join(common.ROOT, "tools"))
    import motion_cost_oracle as mo
    import convert_weights
    from art_planner_amd.context import Context
    from synthetic import make_map
    gm = make_map(100, 0.1, seed=5)
    ctx = Context(0, "yaml")
    try:
        ctx.upload_map(gm)
        ctx.cost_load_weights(convert_weights.to_blob(mo.random_params(0)))
        elv = np.ascontiguousarray(gm["elevation"][::-1, ::-1]).astype(np.float32)
        ctx.cost_update_map(elv, gm.res, gm.len_x, gm.len_y, gm.pos_x, gm.pos_y)
        se3 = ctx.sample_states(99, 0, 1 << 14)
        cand = se3[ctx.validate_states(se3) != 0]
        assert len(cand) >= 8

        def near(x, y):
            return cand[np.argmin(np.hypot(cand[:, 0] - x, cand[:, 1] - y))]

        start, goal = near(gm.pos_x - 3.5, gm.pos_y - 3.5), near(gm.pos_x + 3.5, gm.pos_y + 3.5)
        others = cand[np.linspace(0, len(cand) - 1, 6).astype(int)]
        _cycle(ctx, start, goal, others)  # warm-up: the context's own scratch slots grow to what a cycle needs
        torch.cuda.synchronize()
        free = [torch.cuda.mem_get_info()[0]]
        for _ in range(5):
            _cycle(ctx, start, goal, others)
            torch.cuda.synchronize()
            free.append(torch.cuda.mem_get_info()[0])
        print("free device bytes after the warm-up cycle and after each of five cycles:", free)
        assert free[5] == free[0], free
    finally:
        ctx.close()
