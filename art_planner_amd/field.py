"""ctypes wrapper of the cost-to-go fields (include/artp_c.h: artp_field_*): shortest lattice costs
from a set of source poses to every (cell, heading) of a reachability mask."""
import ctypes as C
from typing import Optional, Tuple

import numpy as np

from . import _capi


def _field_params(ctx, objective, plain_sweeps, inner_sweeps, max_lon_vel, max_lat_vel, max_ang_vel):
    """artp_field_params from the keywords cost_field, cost_fields and cost_matrix share."""
    p = _capi.FieldParams()
    ctx.L.artp_field_params_defaults(C.byref(p))
    p.objective, p.plain_sweeps, p.inner_sweeps = int(objective), int(bool(plain_sweeps)), int(inner_sweeps)
    p.max_lon_vel, p.max_lat_vel, p.max_ang_vel = max_lon_vel, max_lat_vel, max_ang_vel
    return p


def _learned_params(ctx, w_energy, w_time, w_risk, risk_threshold, plain_sweeps, inner_sweeps):
    """artp_field_learned_params from the keywords the learned fields share; None keeps a default of the library."""
    p = _capi.FieldLearnedParams()
    ctx.L.artp_field_learned_params_defaults(C.byref(p))
    for name, v in (("w_energy", w_energy), ("w_time", w_time), ("w_risk", w_risk), ("risk_threshold", risk_threshold)):
        if v is not None:
            setattr(p, name, v)
    p.plain_sweeps, p.inner_sweeps = int(bool(plain_sweeps)), int(inner_sweeps)
    return p


def _clearance_params(ctx, margin, gain, radius_cells, yaw_spread, outside_is_obstacle, objective, max_lon_vel, max_lat_vel,
                      max_ang_vel, plain_sweeps, inner_sweeps):
    """artp_field_clearance_params from the keywords the clearance-weighted fields share."""
    p = _capi.FieldClearanceParams()
    ctx.L.artp_field_clearance_params_defaults(C.byref(p))
    b = p.base
    b.objective, b.plain_sweeps, b.inner_sweeps = int(objective), int(bool(plain_sweeps)), int(inner_sweeps)
    b.max_lon_vel, b.max_lat_vel, b.max_ang_vel = max_lon_vel, max_lat_vel, max_ang_vel
    p.clearance.radius_cells, p.clearance.yaw_spread = int(radius_cells), int(yaw_spread)
    p.clearance.outside_is_obstacle = int(bool(outside_is_obstacle))
    p.margin, p.gain = float(margin), float(gain)
    return p


# the Context method behind each batched entry point: what a refused mask is reported under
_METHOD = {"artp_field_compute_many": "cost_fields", "artp_field_compute_many_learned": "learned_cost_fields",
           "artp_field_compute_many_clearance": "clearance_cost_fields", "artp_field_cost_matrix": "cost_matrix",
           "artp_field_cost_matrix_learned": "learned_cost_matrix",
           "artp_field_cost_matrix_clearance": "clearance_cost_matrix"}


def _mask_arg(mask, nr, nc, what):
    """(pointer, on_device, the object that owns the memory) of a mask of an nr x nc rectangle."""
    if hasattr(mask, "data_ptr"):   # a device tensor of nrows * ncols 32-bit words, column-major
        if mask.numel() * mask.element_size() < nr * nc * 4:
            raise _capi.ArtpError(f"{what}: the mask tensor holds fewer than nrows * ncols words")
        return mask.data_ptr(), 1, mask
    m = np.asarray(mask)
    if m.shape != (nr, nc):
        raise _capi.ArtpError(f"{what}: the mask is {m.shape}, the rectangle ({nr}, {nc})")
    keep = np.asfortranarray(m, dtype=np.uint32)
    return keep.ctypes.data, 0, keep


class CostField:
    """One computed field.  Nodes are (r, c, k) triples, r and c local to the rectangle."""

    def __init__(self, ctx, mask, n_yaw, sources, rect=None, reverse=False, objective=1, max_lon_vel=0.5,
                 max_lat_vel=0.1, max_ang_vel=0.5, plain_sweeps=False, inner_sweeps=64):
        p = _field_params(ctx, objective, plain_sweeps, inner_sweeps, max_lon_vel, max_lat_vel, max_ang_vel)
        self._compute(ctx, ctx.L.artp_field_compute, "artp_field_compute", p, mask, n_yaw, sources, rect, reverse)

    @classmethod
    def learned(cls, ctx, mask, n_yaw, sources, rect=None, reverse=False, w_energy=None, w_time=None, w_risk=None,
                risk_threshold=None, plain_sweeps=False, inner_sweeps=64):
        """The field under the motion-cost network (artp_field_compute_learned); None keeps a default of the library."""
        self = cls.__new__(cls)
        p = _learned_params(ctx, w_energy, w_time, w_risk, risk_threshold, plain_sweeps, inner_sweeps)
        self._compute(ctx, ctx.L.artp_field_compute_learned, "artp_field_compute_learned", p, mask, n_yaw, sources, rect,
                      reverse)
        return self

    @classmethod
    def clearance_weighted(cls, ctx, mask, n_yaw, sources, margin=0.2, gain=2.0, radius_cells=12, yaw_spread=0,
                           outside_is_obstacle=False, rect=None, reverse=False, objective=1, max_lon_vel=0.5,
                           max_lat_vel=0.1, max_ang_vel=0.5, plain_sweeps=False, inner_sweeps=64):
        """The field whose move costs are the objective's, inflated near obstacles (artp_field_compute_clearance,
        DESIGN.md section 17)."""
        self = cls.__new__(cls)
        p = _clearance_params(ctx, margin, gain, radius_cells, yaw_spread, outside_is_obstacle, objective, max_lon_vel,
                              max_lat_vel, max_ang_vel, plain_sweeps, inner_sweeps)
        self._compute(ctx, ctx.L.artp_field_compute_clearance, "artp_field_compute_clearance", p, mask, n_yaw, sources, rect,
                      reverse)
        return self

    @classmethod
    def adopt(cls, ctx, handle, nrows, ncols, n_yaw, reverse=False):
        """The CostField of a handle the library gave out already (a field of artp_field_compute_many): the object owns
        it from here on and closes it like any other."""
        self = cls.__new__(cls)
        self.ctx, self.L = ctx, ctx.L
        self.nrows, self.ncols, self.n_yaw, self.reverse = int(nrows), int(ncols), int(n_yaw), bool(reverse)
        self.h = handle if isinstance(handle, C.c_void_p) else C.c_void_p(handle)
        return self

    @classmethod
    def many(cls, ctx, mask, n_yaw, sources_list, rect=None, reverse=False, objective=1, max_lon_vel=0.5,
             max_lat_vel=0.1, max_ang_vel=0.5, plain_sweeps=False, inner_sweeps=64) -> list:
        """One CostField per source set, computed in one batched search (artp_field_compute_many)."""
        p = _field_params(ctx, objective, plain_sweeps, inner_sweeps, max_lon_vel, max_lat_vel, max_ang_vel)
        return cls._many(ctx, "artp_field_compute_many", p, mask, n_yaw, sources_list, rect, reverse)

    @classmethod
    def many_learned(cls, ctx, mask, n_yaw, sources_list, rect=None, reverse=False, w_energy=None, w_time=None, w_risk=None,
                     risk_threshold=None, plain_sweeps=False, inner_sweeps=64) -> list:
        """One learned CostField per source set on one shared build of the weight table
        (artp_field_compute_many_learned)."""
        p = _learned_params(ctx, w_energy, w_time, w_risk, risk_threshold, plain_sweeps, inner_sweeps)
        return cls._many(ctx, "artp_field_compute_many_learned", p, mask, n_yaw, sources_list, rect, reverse)

    @classmethod
    def many_clearance_weighted(cls, ctx, mask, n_yaw, sources_list, margin=0.2, gain=2.0, radius_cells=12, yaw_spread=0,
                                outside_is_obstacle=False, rect=None, reverse=False, objective=1, max_lon_vel=0.5,
                                max_lat_vel=0.1, max_ang_vel=0.5, plain_sweeps=False, inner_sweeps=64) -> list:
        """One clearance-weighted CostField per source set on one clearance map and one weight table
        (artp_field_compute_many_clearance)."""
        p = _clearance_params(ctx, margin, gain, radius_cells, yaw_spread, outside_is_obstacle, objective, max_lon_vel,
                              max_lat_vel, max_ang_vel, plain_sweeps, inner_sweeps)
        return cls._many(ctx, "artp_field_compute_many_clearance", p, mask, n_yaw, sources_list, rect, reverse)

    @classmethod
    def _many(cls, ctx, name, p, mask, n_yaw, sources_list, rect, reverse) -> list:
        """The mask and set handling of the three batched constructors; name = the C entry point, p = its params."""
        r, nr, nc = ctx._reach_rect(rect)
        mask_ptr, on_device, keep = _mask_arg(mask, nr, nc, _METHOD[name])
        sets = [np.ascontiguousarray(s, np.int32).reshape(-1, 3) for s in sources_list]
        off = np.zeros(len(sets) + 1, np.uint64)
        off[1:] = np.cumsum([len(s) for s in sets])
        src = np.concatenate(sets) if sets and int(off[-1]) else np.zeros((1, 3), np.int32)
        handles = (C.c_void_p * max(len(sets), 1))()
        ctx._chk(getattr(ctx.L, name)(ctx.h, C.byref(p), int(n_yaw), r.ctypes.data if r is not None else None, mask_ptr,
                                      on_device, src.ctypes.data, off.ctypes.data, len(sets), int(bool(reverse)), handles),
                 name)
        del keep
        return [cls.adopt(ctx, handles[b], nr, nc, n_yaw, reverse) for b in range(len(sets))]

    @staticmethod
    def matrix(ctx, mask, n_yaw, poses, batch=None, rect=None, objective=1, max_lon_vel=0.5, max_lat_vel=0.1,
               max_ang_vel=0.5, inner_sweeps=64):
        """((n, n) float64 costs from pose i to pose j, the call's stats) of artp_field_cost_matrix."""
        p = _field_params(ctx, objective, False, inner_sweeps, max_lon_vel, max_lat_vel, max_ang_vel)
        return CostField._matrix(ctx, "artp_field_cost_matrix", p, mask, n_yaw, poses, batch, rect, False)

    @staticmethod
    def matrix_learned(ctx, mask, n_yaw, poses, batch=None, rect=None, w_energy=None, w_time=None, w_risk=None,
                       risk_threshold=None, inner_sweeps=64):
        """The same under the learned cost (artp_field_cost_matrix_learned): the stats carry the table's as well."""
        p = _learned_params(ctx, w_energy, w_time, w_risk, risk_threshold, False, inner_sweeps)
        return CostField._matrix(ctx, "artp_field_cost_matrix_learned", p, mask, n_yaw, poses, batch, rect, True)

    @staticmethod
    def matrix_clearance_weighted(ctx, mask, n_yaw, poses, batch=None, margin=0.2, gain=2.0, radius_cells=12, yaw_spread=0,
                                  outside_is_obstacle=False, rect=None, objective=1, max_lon_vel=0.5, max_lat_vel=0.1,
                                  max_ang_vel=0.5, inner_sweeps=64):
        """The same under the clearance-weighted cost (artp_field_cost_matrix_clearance)."""
        p = _clearance_params(ctx, margin, gain, radius_cells, yaw_spread, outside_is_obstacle, objective, max_lon_vel,
                              max_lat_vel, max_ang_vel, False, inner_sweeps)
        return CostField._matrix(ctx, "artp_field_cost_matrix_clearance", p, mask, n_yaw, poses, batch, rect, True)

    @staticmethod
    def _matrix(ctx, name, p, mask, n_yaw, poses, batch, rect, table):
        """The mask and pose handling of the three matrices; table: the entry point also fills the table's stats."""
        r, nr, nc = ctx._reach_rect(rect)
        mask_ptr, on_device, keep = _mask_arg(mask, nr, nc, _METHOD[name])
        t = np.ascontiguousarray(poses, np.int32).reshape(-1, 3)
        out = np.empty((len(t), len(t)), np.float64)
        st, ts = _capi.FieldManyStats(), _capi.FieldManyTableStats()
        args = [ctx.h, C.byref(p), int(n_yaw), r.ctypes.data if r is not None else None, mask_ptr, on_device, t.ctypes.data,
                len(t), int(batch or 0), out.ctypes.data, C.byref(st)] + ([C.byref(ts)] if table else [])
        ctx._chk(getattr(ctx.L, name)(*args), name)
        del keep
        stats = {n: int(getattr(st, n)) for n, _ in _capi.FieldManyStats._fields_}
        if table:
            stats.update({n: (float if t_ is C.c_double else int)(getattr(ts, n)) for n, t_ in _capi.FieldManyTableStats._fields_})
        return out, stats

    def _compute(self, ctx, call, name, params, mask, n_yaw, sources, rect, reverse):
        """The mask and source handling both constructors share; call = the C entry point, params = its struct."""
        self.ctx = ctx
        self.L = ctx.L
        self.h = None
        r, nr, nc = ctx._reach_rect(rect)
        self.nrows, self.ncols, self.n_yaw, self.reverse = nr, nc, int(n_yaw), bool(reverse)
        mask_ptr, on_device, keep = self._mask_arg(mask, "cost_field")
        src = np.ascontiguousarray(sources, np.int32).reshape(-1, 3)
        h = C.c_void_p()
        ctx._chk(call(ctx.h, C.byref(params), int(n_yaw), r.ctypes.data if r is not None else None, mask_ptr, on_device,
                      src.ctypes.data, len(src), int(bool(reverse)), C.byref(h)), name)
        del keep
        self.h = h

    def _mask_arg(self, mask, what):
        """(pointer, on_device, the object that owns the memory) of a mask of the field's rectangle."""
        return _mask_arg(mask, self.nrows, self.ncols, what)

    def close(self):
        if self.h:
            self.L.artp_field_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def dist(self) -> np.ndarray:
        """(nrows, ncols, n_yaw) float64; +inf where the node does not exist or cannot be reached."""
        out = np.empty((self.ncols, self.nrows, self.n_yaw), np.float64)
        self.ctx._chk(self.L.artp_field_dist(self.h, out.ctypes.data), "artp_field_dist")
        return out.transpose(1, 0, 2)

    def clearance(self) -> np.ndarray:
        """(nrows, ncols, n_yaw) uint16: the clearance map d2 of a clearance-weighted field (artp_field_clearance); any
        other field is refused."""
        out = np.empty((self.ncols, self.nrows, self.n_yaw), np.uint16)
        self.ctx._chk(self.L.artp_field_clearance(self.h, out.ctypes.data), "artp_field_clearance")
        return out.transpose(1, 0, 2)

    def dist_dev(self):
        """The field's own device buffer as a torch tensor of nrows * ncols * n_yaw doubles, index
        (r + c nrows) n_yaw + k; valid until close()."""
        import torch
        p = C.c_void_p()
        self.ctx._chk(self.L.artp_field_dist_dev(self.h, C.byref(p)), "artp_field_dist_dev")
        n = self.nrows * self.ncols * self.n_yaw

        class _View:   # __cuda_array_interface__ of the buffer: torch wraps it without a copy
            __cuda_array_interface__ = {"shape": (n,), "typestr": "<f8", "data": (p.value, False), "version": 2}
            owner = self
        return torch.as_tensor(_View(), device=f"cuda:{self.ctx.device}")

    def path(self, target) -> Optional[Tuple[np.ndarray, np.ndarray, float]]:
        """(nodes (n, 3) int32, se3 (n, 7) float64, cost) in travel order -- source -> target, or target -> source for a
        reverse field -- or None when the target cannot be reached."""
        t = np.ascontiguousarray(target, np.int32).reshape(3)
        n, cost = C.c_size_t(0), C.c_double(0.0)
        cap = 1024
        while True:
            nodes = np.empty((cap, 3), np.int32)
            se3 = np.empty((cap, 7), np.float64)
            rc = self.L.artp_field_path(self.h, t.ctypes.data, nodes.ctypes.data, se3.ctypes.data, cap, C.byref(n),
                                        C.byref(cost))
            if rc == -5 and n.value > cap:   # ARTP_ERR_CAPACITY: *n = the states needed
                cap = n.value
                continue
            self.ctx._chk(rc, "artp_field_path")
            break
        if n.value == 0:
            return None
        return nodes[:n.value].copy(), se3[:n.value].copy(), cost.value

    def edge_costs(self, a, b) -> np.ndarray:
        """The device's own cost of each move a[i] -> b[i] ((n, 3) node triples); NaN where it is not a lattice move."""
        a = np.ascontiguousarray(a, np.int32).reshape(-1, 3)
        b = np.ascontiguousarray(b, np.int32).reshape(-1, 3)
        assert len(a) == len(b)
        out = np.empty(len(a), np.float64)
        self.ctx._chk(self.L.artp_field_edge_costs(self.h, a.ctypes.data, b.ctypes.data, len(a), out.ctypes.data),
                      "artp_field_edge_costs")
        return out

    def update(self, mask, rect=None, refresh_heights=False) -> dict:
        """Bring the field to the fixed point of an edited mask in place (artp_field_update): the
        same bits as a new cost_field on it.  mask as in the constructor, over the field's whole rectangle; rect =
        (row0, col0, nrows, ncols) local to the field: only the words inside it are read (None = all).
        refresh_heights re-reads the sampler layer's heights inside rect.  Returns the update's stats."""
        self._update(self.L.artp_field_update, "update", mask, rect, int(bool(refresh_heights)))
        return self._stats(_capi.FieldUpdateStats, self.L.artp_field_update_stats, "artp_field_update_stats", int)

    def update_learned(self, mask=None, rect=None) -> dict:
        """Bring a learned field to the fixed point of the context's current state in place (artp_field_update_learned,
        DESIGN.md section 15): every move priced again by the loaded network on the installed cost map, the mask edited
        as in update() (None: the mask did not change, rect is ignored).  The same bits as a new learned_cost_field with
        the field's own weights, sources and direction.  Returns the update's stats."""
        self._update(self.L.artp_field_update_learned, "update_learned", mask, rect)
        return self.learned_update_stats()

    def learned_update_stats(self) -> dict:
        """The numbers of the last update_learned that succeeded (zeros before the first)."""
        return self._stats(_capi.FieldLearnedUpdateStats, self.L.artp_field_learned_update_stats,
                           "artp_field_learned_update_stats")

    def update_clearance(self, mask, rect=None, refresh_heights=False) -> dict:
        """Bring a clearance-weighted field to the fixed point of an edited mask in place (artp_field_update_clearance,
        DESIGN.md section 18): the clearance map and the weight table computed again around rect, then the passes of
        update().  mask, rect and refresh_heights as in update().  The same bits -- dist, paths, clearance(), edge_costs --
        as a new clearance_cost_field with the field's own parameters on the merged mask.  Returns the update's stats."""
        self._update(self.L.artp_field_update_clearance, "update_clearance", mask, rect, int(bool(refresh_heights)))
        return self.clearance_update_stats()

    def clearance_update_stats(self) -> dict:
        """The numbers of the last update_clearance that succeeded (zeros before the first)."""
        return self._stats(_capi.FieldClearanceUpdateStats, self.L.artp_field_clearance_update_stats,
                           "artp_field_clearance_update_stats")

    def shift(self, mask, refresh_heights=True) -> dict:
        """Carry the field across a move of the map by whole cells (artp_field_shift).  The
        context's installed map is the new one; node (r, c, k) becomes (r + shift_rows, c + shift_cols, k), with the
        shift taken from the two map positions as artp_preprocessed_change takes it.  mask: the field's whole rectangle
        on the new map, as in the constructor.  The same bits as a new cost_field on the new map with that mask, the
        moved sources and the blocked moves that stayed inside.  refresh_heights re-reads every height; without it the
        kept cells keep theirs.  A learned or clearance-weighted field is refused.  Returns the shift's stats: add
        shift_rows and shift_cols to your own node coordinates."""
        mask_ptr, on_device, keep = self._mask_arg(mask, "CostField.shift")
        self.ctx._chk(self.L.artp_field_shift(self.h, mask_ptr, on_device, int(bool(refresh_heights))), "artp_field_shift")
        del keep
        return self.shift_stats()

    def shift_stats(self) -> dict:
        """The numbers of the last shift that succeeded (zeros before the first)."""
        return self._stats(_capi.FieldShiftStats, self.L.artp_field_shift_stats, "artp_field_shift_stats")

    def shift_clearance(self, mask, refresh_heights=True) -> dict:
        """shift() for a clearance-weighted field (artp_field_shift_clearance): the move of shift(),
        the clearance map computed again over the whole rectangle, every weight priced again against the one its node
        carried across the move, then the passes from the tiles where a weight or the mask changed.  mask and
        refresh_heights as in shift().  The same bits -- dist, paths, clearance(), edge_costs -- as a new
        clearance_cost_field on the new map with the field's own parameters, the moved sources and the blocked moves that
        stayed inside.  The first call that moves allocates a second weight table and keeps it.  Any other field is
        refused.  Returns the shift's stats."""
        mask_ptr, on_device, keep = self._mask_arg(mask, "CostField.shift_clearance")
        self.ctx._chk(self.L.artp_field_shift_clearance(self.h, mask_ptr, on_device, int(bool(refresh_heights))),
                      "artp_field_shift_clearance")
        del keep
        return self.clearance_shift_stats()

    def clearance_shift_stats(self) -> dict:
        """The numbers of the last shift_clearance that succeeded (zeros before the first)."""
        return self._stats(_capi.FieldClearanceShiftStats, self.L.artp_field_clearance_shift_stats,
                           "artp_field_clearance_shift_stats")

    def _update(self, call, name, mask, rect, *extra):
        """The mask and rect handling the three updates share; call = the C entry point artp_field_<name>.  mask None
        (update_learned only): no mask and no rect go down."""
        mask_ptr, on_device, keep = (None, 0, None) if mask is None else self._mask_arg(mask, "CostField." + name)
        r = None if rect is None or mask is None else np.ascontiguousarray(rect, np.int32).reshape(4)
        self.ctx._chk(call(self.h, mask_ptr, on_device, r.ctypes.data if r is not None else None, *extra), "artp_field_" + name)
        del keep

    def _stats(self, struct, call, name, conv=lambda v: v) -> dict:
        """One of the library's stats structs of this field as a dict of its members."""
        s = struct()
        self.ctx._chk(call(self.h, C.byref(s)), name)
        return {n: conv(getattr(s, n)) for n, _ in struct._fields_}

    def block_moves(self, a, b) -> int:
        """Block the moves a[i] -> b[i] ((n, 3) node triples, travel direction) and repair the field in place
        (artp_field_block_moves): the same bits as a new field with the same set blocked.  Only the
        stated direction is blocked.  Returns the number of moves that were not blocked before."""
        a = np.ascontiguousarray(a, np.int32).reshape(-1, 3)
        b = np.ascontiguousarray(b, np.int32).reshape(-1, 3)
        assert len(a) == len(b)
        n = C.c_uint64(0)
        self.ctx._chk(self.L.artp_field_block_moves(self.h, a.ctypes.data, b.ctypes.data, len(a), C.byref(n)),
                      "artp_field_block_moves")
        return int(n.value)

    def unblock(self, rect=None) -> int:
        """Clear the blocked moves of the nodes whose cell lies in rect = (row0, col0, nrows, ncols) local to the field
        (None = all) and repair the field (artp_field_unblock).  Returns the number of moves unblocked."""
        r = None if rect is None else np.ascontiguousarray(rect, np.int32).reshape(4)
        n = C.c_uint64(0)
        self.ctx._chk(self.L.artp_field_unblock(self.h, r.ctypes.data if r is not None else None, C.byref(n)),
                      "artp_field_unblock")
        return int(n.value)

    def blocked(self) -> np.ndarray:
        """(nrows, ncols, n_yaw) uint16: bit j of node v = pull slot (v, j) is blocked (forward field: the move onto v from
        its neighbour by offset j; reverse field: the move from v to it).  Zeros when nothing was ever blocked."""
        out = np.empty((self.ncols, self.nrows, self.n_yaw), np.uint16)
        self.ctx._chk(self.L.artp_field_blocked(self.h, out.ctypes.data), "artp_field_blocked")
        return out.transpose(1, 0, 2)

    def blocked_count(self) -> int:
        n = C.c_uint64(0)
        self.ctx._chk(self.L.artp_field_blocked_count(self.h, C.byref(n)), "artp_field_blocked_count")
        return int(n.value)

    def plan(self, targets, max_rounds=64, simplify=False, window=64) -> list:
        """Lazily checked paths to (n, 3) target triples (artp_field_plan): per round the field's path of every pending
        target, one batched check_motions of all their moves, the failing moves blocked and the field repaired.
        Returns one (status, nodes, se3, cost) per target: status 0 = every move passed (nodes (n, 3) int32 and se3
        (n, 7) in travel order, cost = dist[target]), 1 = unreachable, 2 = max_rounds exhausted (nodes and se3 None,
        cost +inf).  The blocks stay on the field: a second call continues.
        simplify=True: the status-0 paths go through simplify(window=window) in one call, and their tuples gain two
        members: the simplified states (k, 7) and their cost under simplify()'s pricing."""
        out = self._plan(targets, max_rounds)
        if simplify and out:
            simple = self.simplify(out, window=window)
            out = [r if s is None else r + (s[2], s[3]) for r, s in zip(out, simple)]
        return out

    def _plan(self, targets, max_rounds) -> list:
        t = np.ascontiguousarray(targets, np.int32).reshape(-1, 3)
        nt = len(t)
        self._plan_stats = None
        if nt == 0:
            return []
        st = np.empty(nt, np.int32)
        cost = np.empty(nt, np.float64)
        off = np.zeros(nt + 1, np.uint64)
        cap = nt * min(self.nrows * self.ncols * self.n_yaw, 1024)
        total, rounds_left = None, int(max_rounds)
        while True:
            nodes = np.empty((cap, 3), np.int32)
            se3 = np.empty((cap, 7), np.float64)
            rc = self.L.artp_field_plan(self.h, t.ctypes.data, nt, max(rounds_left, 1), st.ctypes.data, cost.ctypes.data,
                                        off.ctypes.data, nodes.ctypes.data, se3.ctypes.data, cap)
            if rc in (0, -5):
                total = self._add_plan_stats(total, self._read_plan_stats())
            if rc == -5 and int(off[nt]) > cap:
                # the paths hold more states than the buffers: the work is done and stays on the field; one more
                # round hands the checked paths out, and plan_stats() keeps describing both calls together
                cap = int(off[nt])
                rounds_left = int(max_rounds) - int(total["rounds"])
                continue
            self.ctx._chk(rc, "artp_field_plan")
            break
        self._plan_stats = total
        out = []
        for i in range(nt):
            lo, hi = int(off[i]), int(off[i + 1])
            if st[i] == 0:
                out.append((0, nodes[lo:hi].copy(), se3[lo:hi].copy(), float(cost[i])))
            else:
                out.append((int(st[i]), None, None, float(cost[i])))
        return out

    def simplify(self, paths, window=64, max_batch_pairs=0) -> list:
        """Windowed shortcut simplification of many paths in one call (artp_field_simplify_paths).
        paths: a list of (n, 7) arrays, or the list plan() returns (entries whose status is not 0 pass through as None,
        and so does a None).  A candidate joins states at most `window` apart along the path (0 = all pairs); it must pass
        check_edges_interp and check_motions, and is priced by the field's objective and velocities (a clearance-weighted
        field: unweighted).  Returns one (status, kept_indices, se3, cost) per path: status 0 = simplified, 1 = the input
        itself does not pass (returned unchanged, cost +inf), 2 = empty.  With a window that covers the path the result
        is Roadmap.simplify's bit for bit."""
        idx, arrs = [], []
        for i, p in enumerate(paths):
            if p is None:
                continue
            if isinstance(p, tuple):            # an entry of plan(): (status, nodes, se3, cost, ...)
                if p[0] != 0:
                    continue
                p = p[2]
            idx.append(i)
            arrs.append(np.ascontiguousarray(p, np.float64).reshape(-1, 7))
        out = [None] * len(paths)
        if not idx:
            return out
        n = len(arrs)
        off = np.zeros(n + 1, np.uint64)
        off[1:] = np.cumsum([len(a) for a in arrs])
        total = int(off[n])
        se3_in = np.concatenate(arrs) if total else np.zeros((0, 7))
        prm = _capi.FieldSimplifyParams(int(window), 0, int(max_batch_pairs))
        st, cost, ooff = np.empty(n, np.int32), np.empty(n, np.float64), np.zeros(n + 1, np.uint64)
        kept, se3 = np.empty(max(total, 1), np.uint32), np.empty((max(total, 1), 7), np.float64)   # never more than came in
        self.ctx._chk(self.L.artp_field_simplify_paths(self.h, C.byref(prm), se3_in.ctypes.data, off.ctypes.data, n,
                                                       st.ctypes.data, cost.ctypes.data, ooff.ctypes.data,
                                                       kept.ctypes.data, se3.ctypes.data, max(total, 1)),
                      "artp_field_simplify_paths")
        for j, i in enumerate(idx):
            lo, hi = int(ooff[j]), int(ooff[j + 1])
            out[i] = (int(st[j]), kept[lo:hi].copy(), se3[lo:hi].copy(), float(cost[j]))
        return out

    def simplify_stats(self) -> dict:
        """The numbers of the last simplify() (artp_field_simplify_stats)."""
        return self._stats(_capi.FieldSimplifyStats, self.L.artp_field_simplify_stats, "artp_field_simplify_stats")

    def _read_plan_stats(self) -> dict:
        d = self._stats(_capi.FieldPlanStats, self.L.artp_field_plan_stats, "artp_field_plan_stats")
        n = C.c_size_t(0)
        self.ctx._chk(self.L.artp_field_plan_round_tile_runs(self.h, None, 0, C.byref(n)), "artp_field_plan_round_tile_runs")
        runs = np.zeros(max(n.value, 1), np.uint64)
        self.ctx._chk(self.L.artp_field_plan_round_tile_runs(self.h, runs.ctypes.data, n.value, C.byref(n)),
                      "artp_field_plan_round_tile_runs")
        d["round_tile_runs"] = [int(v) for v in runs[:n.value]]
        return d

    @staticmethod
    def _add_plan_stats(total, d):
        if total is None:
            return d
        out = {k: total[k] + d[k] for k in d}          # counts and times add up, the rounds' lists follow one another
        out["last_update_tile_runs"] = d["last_update_tile_runs"] if d["updates"] else total["last_update_tile_runs"]
        return out

    def plan_stats(self) -> dict:
        """The numbers of the last plan() (artp_field_plan_stats, and round_tile_runs: the tiles that ran in the repair of
        every round, artp_field_plan_round_tile_runs); where plan() had to ask twice because the paths outgrew its
        buffers, the two calls together.  Before the first plan(): the library's own record."""
        if getattr(self, "_plan_stats", None) is not None:
            return dict(self._plan_stats)
        return self._read_plan_stats()

    def learned_stats(self) -> dict:
        """The weight table of a learned field and the time its steps took (artp_field_learned_stats)."""
        return self._stats(_capi.FieldLearnedStats, self.L.artp_field_learned_stats, "artp_field_learned_stats")

    def stats(self) -> dict:
        return self._stats(_capi.FieldStats, self.L.artp_field_stats, "artp_field_stats", int)
