"""ctypes wrapper of the batch-synchronous tree planners (include/artp_c.h: artp_tree_*).

The reference selects them by name (art_planner/src/planner.cpp:92-105): "rrt_star" (OMPL RRTstar), "inf_rrt_star"
(InformedRRTstar) and "rrt_sharp" (RRTsharp).  create = setup with start / goal, grow = solve's sampling loop as
batches, solve = the root -> goal chain of the tree."""
import ctypes as C
from typing import Optional, Tuple

import numpy as np

from . import _capi

VARIANTS = {"rrt_star": 0, "inf_rrt_star": 1, "rrt_sharp": 2}


class Tree:
    def __init__(self, ctx, start, goal, variant="rrt_star", seed=42, first_index=0, objective=0, max_lon_vel=0.5,
                 max_lat_vel=0.1, max_ang_vel=0.5, batch=1024, max_vertices=100000, max_batches=0, plan_time=0.0,
                 range=0.0, rewire_factor=1.1, profile=False):
        """variant: a planner name of VARIANTS or its number.  range 0 = OMPL's default (0.2 x the space's extent)."""
        self.ctx = ctx
        self.L = ctx.L   # the library that made the context
        p = _capi.TreeParams()
        self.L.artp_tree_params_defaults(C.byref(p))
        p.seed, p.first_index = seed, first_index
        p.variant = VARIANTS[variant] if isinstance(variant, str) else int(variant)
        p.objective = objective
        p.max_lon_vel, p.max_lat_vel, p.max_ang_vel = max_lon_vel, max_lat_vel, max_ang_vel
        p.batch, p.max_vertices, p.max_batches = batch, max_vertices, max_batches
        p.plan_time, p.range, p.rewire_factor = plan_time, range, rewire_factor
        p.profile = 1 if profile else 0
        self.params = p
        s = np.ascontiguousarray(start, np.float64).reshape(7)
        g = np.ascontiguousarray(goal, np.float64).reshape(7)
        h = C.c_void_p()
        ctx._chk(self.L.artp_tree_create(ctx.h, C.byref(p), s.ctypes.data, g.ctypes.data, C.byref(h)), "artp_tree_create")
        self.h = h

    def close(self):
        if self.h:
            self.L.artp_tree_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def grow(self, n_batches: int = 0) -> dict:
        """Grow by n_batches batches (0 = until max_vertices / max_batches / plan_time)."""
        out = (C.c_uint64 * 2)()
        self.ctx._chk(self.L.artp_tree_grow(self.h, int(n_batches), C.byref(out)), "artp_tree_grow")
        return {"batches": out[0], "vertices": out[1]}

    def stats(self) -> dict:
        out = (C.c_uint64 * 8)()
        self.ctx._chk(self.L.artp_tree_stats(self.h, C.byref(out)), "artp_tree_stats")
        none = (1 << 64) - 1
        return {"vertices": out[0], "batches": out[1], "samples_drawn": out[2], "motions_checked": out[3],
                "rewires": out[4], "pruned": out[5], "goal": None if out[6] == none else out[6],
                "first_solution_batch": None if out[7] == none else out[7]}

    def export(self) -> dict:
        n = self.stats()["vertices"]
        d = {"verts": np.empty((n, 7), np.float64), "parent": np.empty(n, np.uint32), "cost": np.empty(n, np.float64),
             "edge_cost": np.empty(n, np.float64), "born": np.empty(n, np.uint32), "pruned": np.empty(n, np.uint8)}
        self.ctx._chk(self.L.artp_tree_export(self.h, *(d[k].ctypes.data for k in
                                                        ("verts", "parent", "cost", "edge_cost", "born", "pruned"))),
                      "artp_tree_export")
        return d

    def export_checked(self) -> dict:
        """Every motion checked so far: u, v (0xffffffff = the state did not become a vertex), valid, batch."""
        n = C.c_size_t(0)
        self.ctx._chk(self.L.artp_tree_export_checked(self.h, None, None, None, None, 0, C.byref(n)),
                      "artp_tree_export_checked")
        m = n.value
        d = {"u": np.empty(m, np.uint32), "v": np.empty(m, np.uint32), "valid": np.empty(m, np.uint8),
             "batch": np.empty(m, np.uint32)}
        self.ctx._chk(self.L.artp_tree_export_checked(self.h, d["u"].ctypes.data, d["v"].ctypes.data,
                                                      d["valid"].ctypes.data, d["batch"].ctypes.data, m, C.byref(n)),
                      "artp_tree_export_checked")
        return d

    def solve(self, cap_states=4096) -> Tuple[Optional[np.ndarray], float]:
        """(root -> goal path n x 7, cost), or (None, inf) while the goal is not in the tree."""
        path = np.empty((cap_states, 7), np.float64)
        n, cost = C.c_size_t(0), C.c_double(0.0)
        self.ctx._chk(self.L.artp_tree_solve(self.h, path.ctypes.data, cap_states, C.byref(n), C.byref(cost)),
                      "artp_tree_solve")
        if n.value == 0:
            return None, float("inf")
        return path[:n.value].copy(), cost.value

    def simplify(self, path):
        """Cheapest chain of valid shortcuts through the states of `path` (the roadmap's simplifier)."""
        p = np.ascontiguousarray(path, np.float64).reshape(-1, 7)
        out = np.empty_like(p)
        n, cost = C.c_size_t(0), C.c_double(0.0)
        self.ctx._chk(self.L.artp_tree_simplify_path(self.h, p.ctypes.data, p.shape[0], out.ctypes.data, C.byref(n),
                                                     C.byref(cost)), "artp_tree_simplify_path")
        return out[:n.value].copy(), cost.value

    def stage_times(self) -> np.ndarray:
        """Device microseconds per stage summed over the batches grown (profile=True), include/artp_c.h."""
        out = (C.c_double * 10)()
        self.ctx._chk(self.L.artp_tree_stage_times(self.h, C.byref(out)), "artp_tree_stage_times")
        return np.array(out[:], np.float64)
