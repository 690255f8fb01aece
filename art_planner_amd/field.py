"""ctypes wrapper of the cost-to-go fields (include/artp_c.h: artp_field_*): shortest lattice costs
from a set of source poses to every (cell, heading) of a reachability mask."""
import ctypes as C
from typing import Optional, Tuple

import numpy as np

from . import _capi


class CostField:
    """One computed field.  Nodes are (r, c, k) triples, r and c local to the rectangle."""

    def __init__(self, ctx, mask, n_yaw, sources, rect=None, reverse=False, objective=1, max_lon_vel=0.5,
                 max_lat_vel=0.1, max_ang_vel=0.5, plain_sweeps=False, inner_sweeps=64):
        p = _capi.FieldParams()
        ctx.L.artp_field_params_defaults(C.byref(p))
        p.objective, p.plain_sweeps, p.inner_sweeps = int(objective), int(bool(plain_sweeps)), int(inner_sweeps)
        p.max_lon_vel, p.max_lat_vel, p.max_ang_vel = max_lon_vel, max_lat_vel, max_ang_vel
        self._compute(ctx, ctx.L.artp_field_compute, "artp_field_compute", p, mask, n_yaw, sources, rect, reverse)

    @classmethod
    def learned(cls, ctx, mask, n_yaw, sources, rect=None, reverse=False, w_energy=None, w_time=None, w_risk=None,
                risk_threshold=None, plain_sweeps=False, inner_sweeps=64):
        """The field under the motion-cost network (artp_field_compute_learned); None keeps a default of the library."""
        self = cls.__new__(cls)
        p = _capi.FieldLearnedParams()
        ctx.L.artp_field_learned_params_defaults(C.byref(p))
        for name, v in (("w_energy", w_energy), ("w_time", w_time), ("w_risk", w_risk), ("risk_threshold", risk_threshold)):
            if v is not None:
                setattr(p, name, v)
        p.plain_sweeps, p.inner_sweeps = int(bool(plain_sweeps)), int(inner_sweeps)
        self._compute(ctx, ctx.L.artp_field_compute_learned, "artp_field_compute_learned", p, mask, n_yaw, sources, rect,
                      reverse)
        return self

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
        nr, nc = self.nrows, self.ncols
        if hasattr(mask, "data_ptr"):   # a device tensor of nrows * ncols 32-bit words, column-major
            if mask.numel() * mask.element_size() < nr * nc * 4:
                raise _capi.ArtpError(f"{what}: the mask tensor holds fewer than nrows * ncols words")
            return mask.data_ptr(), 1, mask
        m = np.asarray(mask)
        if m.shape != (nr, nc):
            raise _capi.ArtpError(f"{what}: the mask is {m.shape}, the rectangle ({nr}, {nc})")
        keep = np.asfortranarray(m, dtype=np.uint32)
        return keep.ctypes.data, 0, keep

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
        mask_ptr, on_device, keep = self._mask_arg(mask, "CostField.update")
        r = None if rect is None else np.ascontiguousarray(rect, np.int32).reshape(4)
        self.ctx._chk(self.L.artp_field_update(self.h, mask_ptr, on_device, r.ctypes.data if r is not None else None,
                                               int(bool(refresh_heights))), "artp_field_update")
        del keep
        s = _capi.FieldUpdateStats()
        self.ctx._chk(self.L.artp_field_update_stats(self.h, C.byref(s)), "artp_field_update_stats")
        return {n: int(getattr(s, n)) for n, _ in _capi.FieldUpdateStats._fields_}

    def update_learned(self, mask=None, rect=None) -> dict:
        """Bring a learned field to the fixed point of the context's current state in place (artp_field_update_learned,
        DESIGN.md section 15): every move priced again by the loaded network on the installed cost map, the mask edited
        as in update() (None: the mask did not change, rect is ignored).  The same bits as a new learned_cost_field with
        the field's own weights, sources and direction.  Returns the update's stats."""
        mask_ptr, on_device, keep = (None, 0, None) if mask is None else self._mask_arg(mask, "CostField.update_learned")
        r = None if rect is None or mask is None else np.ascontiguousarray(rect, np.int32).reshape(4)
        self.ctx._chk(self.L.artp_field_update_learned(self.h, mask_ptr, on_device, r.ctypes.data if r is not None else None),
                      "artp_field_update_learned")
        del keep
        return self.learned_update_stats()

    def learned_update_stats(self) -> dict:
        """The numbers of the last update_learned that succeeded (zeros before the first)."""
        s = _capi.FieldLearnedUpdateStats()
        self.ctx._chk(self.L.artp_field_learned_update_stats(self.h, C.byref(s)), "artp_field_learned_update_stats")
        return {n: getattr(s, n) for n, _ in _capi.FieldLearnedUpdateStats._fields_}

    def learned_stats(self) -> dict:
        """The weight table of a learned field and the time its steps took (artp_field_learned_stats)."""
        s = _capi.FieldLearnedStats()
        self.ctx._chk(self.L.artp_field_learned_stats(self.h, C.byref(s)), "artp_field_learned_stats")
        return {n: getattr(s, n) for n, _ in _capi.FieldLearnedStats._fields_}

    def stats(self) -> dict:
        s = _capi.FieldStats()
        self.ctx._chk(self.L.artp_field_stats(self.h, C.byref(s)), "artp_field_stats")
        return {n: int(getattr(s, n)) for n, _ in _capi.FieldStats._fields_}
