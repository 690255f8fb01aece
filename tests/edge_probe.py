"""Probe edges for checkMotion and the 0.5 m rule (TEST INFRASTRUCTURE; tests/test_edge_probe.py proves on the CPU that
they probe, tests/test_edge_sweep.py runs them on the GPU).

Part 1 is a float64 numpy restatement of the edge rules, outside the library and outside the C oracle's edge loop:
validSegmentCount (R^3 bounds "map centre -/+ full length", the z extent, the frozen extent, the SO(3) count), OMPL's
SE(3) interpolation with its three branches, the state list of checkMotion (interior 1 .. nd-1, then s2), the state
list of the 0.5 m rule and the lastValid rule (nd == 0: -inf).  Validity of a state comes from OracleMap.states_valid;
an edge is valid iff all its restated states are.  The two-pass split of checkMotion is restated too (pass_tasks), so
that the CPU tests can count which probes only one of the passes can see.

Part 2 builds the probe families on one flat 200 x 200 map at 0.05 m with a 0.4 m block raised by 1 m (and one
non-square map with another origin).  For the YAML robot at heading 0 each foot box has a square of about 0.35 m around
the block where the state is invalid; all geometry below is MEASURED on the oracle (zone_on_line), not derived from
the boxes."""
from __future__ import annotations

import functools
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import numpy as np

import common
import oracle_py as O
from synthetic import GridMap

SEG_SO3 = (0.5 * 3.14159265358979323846) * 0.01
DBL_EPS = 2.220446049250313e-16
STRIDES = (2, 3, 8, 16)
FEW_EDGES = 64


# ---- part 1: the rules, restated ------------------------------------------------------------------------------------------
def z_extent(gm: GridMap, rob) -> float:
    e = np.asarray(gm["elevation"], np.float64)
    fin = e[np.isfinite(e)]
    lo, hi = (float(fin.min()), float(fin.max())) if fin.size else (0.0, 0.0)
    return (hi + rob.reach_z / 2) - (lo - rob.reach_z / 2)


def seg_r3(gm: GridMap, zext: float, frozen: float = 0.0) -> float:
    ex = (gm.pos_x + gm.len_x) - (gm.pos_x - gm.len_x)
    ey = (gm.pos_y + gm.len_y) - (gm.pos_y - gm.len_y)
    ext = ((0.0 + ex * ex) + ey * ey) + zext * zext
    return (frozen if frozen > 0.0 else float(np.sqrt(ext))) * 0.01


def quat_dot(a, b):
    return ((a[:, 3] * b[:, 3] + a[:, 4] * b[:, 4]) + a[:, 5] * b[:, 5]) + a[:, 6] * b[:, 6]


def so3_arc(a, b):
    dq = np.abs(quat_dot(a, b))
    return np.where(dq > 1.0 - 1e-9, 0.0, np.arccos(np.minimum(dq, 1.0)))


def segment_counts(gm, zext, frozen, s1, s2, mutate=None):
    """(nd, n_r3, n_so3) of CompoundStateSpace::validSegmentCount.  mutate: 'f' ceil(x) -> floor(x) + 1 in the R^3
    count, 'g' n_so3 left out of the max (the CPU half of the mutation check)."""
    d = s1[:, :3] - s2[:, :3]
    d2 = ((0.0 + d[:, 0] * d[:, 0]) + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    x = np.sqrt(d2) / seg_r3(gm, zext, frozen)
    n_r3 = (np.floor(x) + 1 if mutate == "f" else np.ceil(x)).astype(np.int64)
    n_so3 = np.ceil(so3_arc(s1, s2) / SEG_SO3).astype(np.int64)
    return (n_r3 if mutate == "g" else np.maximum(n_r3, n_so3)), n_r3, n_so3


def interpolate(a, b, t, mutate=None):
    """SE3StateSpace::interpolate on rows: R^3 lerp, SO(3) slerp (theta <= eps: q1; negative dot: sin(t theta) negated).
    mutate 'e': the sign of the dot product ignored."""
    a, b = np.atleast_2d(a), np.atleast_2d(b)
    t = np.broadcast_to(np.asarray(t, np.float64), (a.shape[0],))
    out = np.empty_like(a)
    with np.errstate(invalid="ignore", divide="ignore"):
        out[:, :3] = a[:, :3] + (b[:, :3] - a[:, :3]) * t[:, None]
        theta = so3_arc(a, b)
        d = 1.0 / np.sin(theta)
        s0 = np.sin((1.0 - t) * theta)
        s1 = np.where((quat_dot(a, b) < 0) & (mutate != "e"), -np.sin(t * theta), np.sin(t * theta))
        q = (a[:, 3:] * s0[:, None] + b[:, 3:] * s1[:, None]) * d[:, None]
    out[:, 3:] = np.where((theta > DBL_EPS)[:, None], q, a[:, 3:])
    return out


def interp_counts(s1, s2):
    dx, dy = s2[:, 0] - s1[:, 0], s2[:, 1] - s1[:, 1]
    return np.floor(np.sqrt(dx * dx + dy * dy) / 0.5).astype(np.int64)


def _ragged(counts):
    """(edge index, index within the edge) of sum(counts) items."""
    e = np.repeat(np.arange(len(counts)), counts)
    first = np.cumsum(counts) - counts
    return e, np.arange(len(e)) - first[e]


def motion_states(s1, s2, nd, mutate=None):
    """checkMotion's states: per edge the interior states j = 1 .. nd-1 (t = j / nd), then s2 (reported as j = nd)."""
    e, i = _ragged(np.maximum(nd - 1, 0) + 1)
    j = i + 1
    is_s2 = j == np.maximum(nd, 1)[e]
    j = np.where(is_s2, nd[e], j)
    st = interpolate(s1[e], s2[e], j / np.maximum(nd[e], 1).astype(np.float64), mutate)
    st[is_s2] = s2[e[is_s2]]
    return st, e, j, is_s2


def interp_states(s1, s2, ni, mutate=None):
    """The 0.5 m rule's states: t = (k + 1) / (n_interp + 1), k < n_interp.  mutate 'h': (k + 1) -> k."""
    e, k = _ragged(ni)
    div = 1.0 / (ni[e] + 1)
    return interpolate(s1[e], s2[e], (k if mutate == "h" else k + 1) * div), e, k


def pass_tasks(nd: int, S: int, mutate=None):
    """The two-pass split restated: (tasks of pass 1, tasks of pass 2) as lists of k; k = 0 is s2, k >= 1 interior state
    k.  Pass 1: s2 and every S-th interior state; pass 2: the rest.  mutate 'a': pass 2's + j / (S - 1) dropped;
    'b': coarse = (interior + 1) / S."""
    interior = nd - 1 if nd >= 2 else 0
    coarse = (interior + 1) // S if mutate == "b" else interior // S
    p1 = [j * S for j in range(1 + coarse)]
    p2 = [j + (0 if mutate == "a" else j // (S - 1)) + 1 for j in range(interior - coarse)]
    return p1, p2


@dataclass
class Ref:
    mode: int
    valid: np.ndarray                      # verdict per edge
    count: np.ndarray                      # nd (mode 0) / n_interp (mode 1)
    n_r3: Optional[np.ndarray] = None
    n_so3: Optional[np.ndarray] = None
    t: Optional[np.ndarray] = None         # lastValid.second (1 where valid)
    st: Optional[np.ndarray] = None        # *lastValid.first (s2 where valid)
    states: Optional[np.ndarray] = None
    e: Optional[np.ndarray] = None         # edge of every state
    j: Optional[np.ndarray] = None         # mode 0: interior index, nd for s2; mode 1: k
    ok: Optional[np.ndarray] = None        # validity of every state
    first_bad: Optional[np.ndarray] = None  # mode 0: first failing interior j, nd when only s2 fails, -1 when valid

    def bad_interior(self, i):
        """Sorted interior indices j of edge i that are invalid (mode 0)."""
        lo, hi = np.searchsorted(self.e, [i, i + 1])
        j, ok = self.j[lo:hi], self.ok[lo:hi]
        return np.sort(j[(ok == 0) & (j < max(int(self.count[i]), 1))])

    def ok_of_task(self, i):
        """mode 0: {k: validity} of edge i, k = 0 for s2."""
        lo, hi = np.searchsorted(self.e, [i, i + 1])
        nd = int(self.count[i])
        return {(0 if j == nd or nd == 0 else int(j)): bool(o) for j, o in zip(self.j[lo:hi], self.ok[lo:hi])}


def reference(gm, rob, mode, s1, s2, frozen=0.0, mutate=None) -> Ref:
    """Verdicts, counts and the lastValid pair from the restated rules and OracleMap.states_valid.
    mutate 'd': s2's order nd - 1 -> nd; 'i': s2 never looked at; 'e', 'f', 'g', 'h' see above."""
    s1 = np.ascontiguousarray(s1, np.float64).reshape(-1, 7)
    s2 = np.ascontiguousarray(s2, np.float64).reshape(-1, 7)
    n = len(s1)
    if mode == 1:
        ni = interp_counts(s1, s2)
        st, e, k = interp_states(s1, s2, ni, mutate)
        ok = common.oracle_states_valid_threaded(gm, rob, st) if len(st) else np.empty(0, np.uint8)
        valid = np.ones(n, np.uint8)
        valid[e[ok == 0]] = 0
        return Ref(1, valid, ni, states=st, e=e, j=k, ok=ok)
    nd, n_r3, n_so3 = segment_counts(gm, z_extent(gm, rob), frozen, s1, s2, mutate)
    st, e, j, is_s2 = motion_states(s1, s2, nd, mutate)
    ok = common.oracle_states_valid_threaded(gm, rob, st)
    if mutate == "i":           # the few-edge loop started at chunk + 1: task 0 (s2) is never looked at
        ok = np.where(is_s2, 1, ok).astype(np.uint8)
    valid = np.ones(n, np.uint8)
    valid[e[ok == 0]] = 0
    # the first failure in OMPL's order: interior states in order, then s2 (j = nd sorts last; nd == 0: j = 0 is s2)
    first_bad = np.full(n, np.iinfo(np.int64).max)
    np.minimum.at(first_bad, e[ok == 0], np.where(is_s2, np.maximum(nd[e], 1), j)[ok == 0])
    s2_only = first_bad == np.maximum(nd, 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        order = np.where(s2_only, nd if mutate == "d" else nd - 1, first_bad - 1).astype(np.float64)
        t = np.where(valid != 0, 1.0, order / nd.astype(np.float64))
        last = interpolate(s1, s2, t, mutate)
    last[valid != 0] = s2[valid != 0]
    fb = np.where(valid != 0, -1, np.where(s2_only, nd, first_bad))
    return Ref(0, valid, nd, n_r3, n_so3, t, last, st, e, j, ok, fb)


def two_pass_verdict(ref: Ref, i: int, S: int, mutate=None) -> bool:
    """Edge i's verdict when its states are looked at in the two passes of stride S (pass 2 only if pass 1 passes)."""
    ok = ref.ok_of_task(i)
    nd = int(ref.count[i])
    p1, p2 = pass_tasks(nd, S, mutate)
    look = lambda k: ok[0] if k == nd else ok[k]      # t = nd / nd is s2
    return all(look(k) for k in p1) and all(look(k) for k in p2)


def lane_edges(counts, mutate=None):
    """expand_edges_recs_kernel's edge search restated: the edge of every task w of a batch with these task counts.  A
    wavefront holds 64 consecutive tasks from w0 on: e0 = the last edge with offsets[e0] <= w0, cnt = how many of the next
    64 offsets (offsets[n] = total past the end) lie at or below w, and with cnt == 64 the search goes on from e0 + 64.
    mutate 'c': that follow-on search removed."""
    counts = np.asarray(counts, np.int64)
    n = len(counts)
    off = np.concatenate([[0], np.cumsum(counts)])
    w = np.arange(off[n])
    e0 = np.searchsorted(off[:n], (w // 64) * 64, side="right") - 1
    nxt = off[np.minimum(e0[:, None] + 1 + np.arange(64)[None, :], n)]
    cnt = (nxt <= w[:, None]).sum(axis=1)
    e = e0 + cnt
    if mutate != "c":
        more = cnt == 64
        e[more] = np.searchsorted(off[:n], w[more], side="right") - 1
    return e


# ---- the chunk rule of the few-edge launch, read from few_edges_task_estimate and run_edges_few --------------------------
def few_estimate(gm, zext, frozen, mode, s1, s2):
    """(total, max per edge) of the host's task estimate."""
    ex, ey = 2.0 * gm.len_x, 2.0 * gm.len_y
    seg = (frozen if frozen > 0.0 else np.sqrt(ex * ex + ey * ey + zext * zext)) * 0.01
    d = s1[:, :3] - s2[:, :3]
    if mode == 0:
        r3 = np.sqrt((d * d).sum(axis=1)) / seg
        dq = np.abs(quat_dot(s1, s2))
        so3 = np.where(dq < 1.0, np.arccos(np.minimum(dq, 1.0)), 0.0) / (0.005 * np.pi)
        t = np.maximum(r3, so3) + 2.0
    else:
        t = np.sqrt(d[:, 0] ** 2 + d[:, 1] ** 2) / 0.5 + 1.0
    return float(t.sum()), float(max(1.0, t.max()))


def few_chunks(n: int, max_per_edge: float) -> int:
    chunks = 2048 // n
    want = int(min(max_per_edge, 128.0)) + 1
    chunks = 128 if chunks > 128 else (16 if chunks < 16 else chunks)
    return min(chunks, want)


# ---- part 2: maps and measured geometry -------------------------------------------------------------------------------------
def se3(x, y, yaw, z=0.0):
    x, y, yaw = np.broadcast_arrays(np.asarray(x, np.float64), np.asarray(y, np.float64), np.asarray(yaw, np.float64))
    s = np.zeros((x.size, 7))
    s[:, 0], s[:, 1], s[:, 2] = x.ravel(), y.ravel(), z
    s[:, 5], s[:, 6] = np.sin(yaw.ravel() / 2), np.cos(yaw.ravel() / 2)
    return s


def _flat_with_block(rows, cols, r0, c0, pos=(0.0, 0.0)) -> GridMap:
    gm = GridMap(rows, cols, 0.05, pos[0], pos[1])
    h = np.zeros((rows, cols), np.float32)
    h[r0:r0 + 8, c0:c0 + 8] = 1.0              # 0.4 m square, 1 m high
    gm.add("elevation", h)
    gm.add("elevation_masked", h)
    return gm


@functools.lru_cache(maxsize=None)
def shared_map() -> GridMap:
    """10 m x 10 m, block centred at (0.8, 0): the first foot zone of the line y = 0.3 at heading 0 begins just below x = 0."""
    return _flat_with_block(200, 200, 80, 96)


@functools.lru_cache(maxsize=None)
def rect_map() -> GridMap:
    """12 m x 8 m around (3, -2), block centred at (3.8, -2): ex != ey in the extent."""
    return _flat_with_block(240, 160, 100, 76, pos=(3.0, -2.0))


MAPS = {"shared": shared_map, "rect": rect_map}


def robot():
    return O.robot("yaml")


def zone_on_line(gm, p0, u, yaw, s_lo, s_hi, step=0.005) -> List[Tuple[float, float]]:
    """Invalid stretches (s_in, s_out) of the states p0 + s u at heading yaw, s in [s_lo, s_hi]: a scan at `step`, each
    end then bisected to 1e-7 on the oracle."""
    om = O.OracleMap(gm)
    rob = robot()
    s = np.arange(s_lo, s_hi + step / 2, step)
    v = om.states_valid(rob, se3(p0[0] + s * u[0], p0[1] + s * u[1], yaw))
    assert v[0] and v[-1], "the line must begin and end on valid states"

    def bisect(a, b):      # a, b: validity differs
        va = om.states_valid(rob, se3(p0[0] + a * u[0], p0[1] + a * u[1], yaw))[0]
        while b - a > 1e-7:
            m = 0.5 * (a + b)
            if om.states_valid(rob, se3(p0[0] + m * u[0], p0[1] + m * u[1], yaw))[0] == va:
                a = m
            else:
                b = m
        return a, b

    out = []
    edges = np.flatnonzero(v[1:] != v[:-1])
    for a, b in zip(edges[0::2], edges[1::2]):
        out.append((bisect(s[a], s[a + 1])[1], bisect(s[b], s[b + 1])[0]))      # first and last invalid parameter
    return out


@functools.lru_cache(maxsize=None)
def geometry(which="shared") -> Dict[str, object]:
    """What the families need, measured: the zones of the line y = y0 + 0.3 (heading 0, along +x) and the single short
    zone of the diagonal that clips the outer corner of one foot square."""
    gm = MAPS[which]()
    cx, cy = gm.pos_x + 0.8, gm.pos_y
    g: Dict[str, object] = {"cx": cx, "cy": cy, "y_line": cy + 0.3}
    g["x_zones"] = [(cx - 0.8 + a, cx - 0.8 + b) for a, b in
                    zone_on_line(gm, (cx - 0.8, cy + 0.3), (1.0, 0.0), 0.0, -2.5, 3.0)]
    # rotation in place at ROT_POINT: valid from yaw -0.9 up to a heading near 0.4, invalid beyond (bisected)
    om, rob = O.OracleMap(gm), robot()
    px, py = cx + ROT_POINT[0], cy + ROT_POINT[1]
    lo, hi = 0.3, 0.45
    assert om.states_valid(rob, se3(px, py, lo))[0] and not om.states_valid(rob, se3(px, py, hi))[0]
    while hi - lo > 1e-7:
        mid = 0.5 * (lo + hi)
        if om.states_valid(rob, se3(px, py, mid))[0]:
            lo = mid
        else:
            hi = mid
    g["rot"] = (px, py, hi + 0.004)
    if which == "shared":
        # The foot squares of heading 0 reach out to about (cx - 0.86, cy - 0.51).  A diagonal through a point 0.035 m
        # inside that outer corner clips it in one stretch of about 0.13 m (measured below): short enough for runs of 1-3
        # states at 0.0625 m and 0.125 m segments, and nothing else lies on the line.  s in [-5.6, 5.1] keeps the states
        # 0.6 m and more inside the map's border, beyond which the oracle rejects every state.
        u = (np.sqrt(0.5), -np.sqrt(0.5))
        p0 = (cx - 0.825, cy - 0.475)
        z = zone_on_line(gm, p0, u, 0.0, -5.6, 5.1)
        assert len(z) == 1, z
        g["diag"] = {"p0": p0, "u": u, "s_in": z[0][0], "w": z[0][1] - z[0][0], "s_lo": -5.6, "s_hi": 5.1}
    return g


@dataclass
class Batch:
    """Edges that go through the library in ONE call (or, for the few-edge and pool families, cut into small calls)."""
    name: str
    mode: int
    s1: np.ndarray
    s2: np.ndarray
    frozen: float = 0.0
    map: str = "shared"
    meta: Dict[str, object] = field(default_factory=dict)

    @property
    def n(self):
        return len(self.s1)


@functools.lru_cache(maxsize=None)
def _ref_cached(family: str, index: int) -> Ref:
    b = FAMILIES[family]()[index]
    return reference(MAPS[b.map](), robot(), b.mode, b.s1, b.s2, b.frozen)


def ref_of(family: str, index: int) -> Ref:
    """The restated reference of one batch: computed once, shared, never written to."""
    return _ref_cached(family, index)


def _cat(parts):
    return np.concatenate([np.atleast_2d(p) for p in parts], axis=0) if parts else np.empty((0, 7))


def _line_edge(g, x1, x2, yaw1=0.0, yaw2=0.0):
    return se3(x1, g["y_line"], yaw1), se3(x2, g["y_line"], yaw2)


def filler_edges(m: int, nd: int, seg: float):
    """m valid edges of nd segments each on the line y = -3 (far from the block; asserted valid by the CPU tests)."""
    L = (nd - 0.5) * seg
    x1 = -3.6 + 0.001 * (np.arange(m) % 400)
    return se3(x1, -3.0, 0.0), se3(x1 + L, -3.0, 0.0)


# ---- failure position ------------------------------------------------------------------------------------------------------
ND_LIST = (2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 17, 31, 32, 33, 40)
PHASES = (0.08, 0.5, 0.92)
POS_SEGS = ((12.5, 0.125, 33), (6.25, 0.0625, 40))        # (frozen extent, its segment, largest nd used with it)


@functools.lru_cache(maxsize=None)
def failure_position() -> Tuple[Batch, ...]:
    """Straight edges at heading 0 along the diagonal: interior state j lands just inside the one short zone, for every
    j = 1 .. nd-1, every nd of ND_LIST and three phases; the segment (frozen extent) is long enough that one to three
    consecutive states are invalid.  Each batch is padded with valid edges to more than 4096 edges of 24 tasks or more
    on average, so that run_edges_dev takes two passes."""
    d = geometry()["diag"]
    p0, u = np.array(d["p0"]), np.array(d["u"])
    out = []
    for frozen, seg, nd_max in POS_SEGS:
        assert frozen * 0.01 == seg
        a, b, tag = [], [], []
        for nd in (q for q in ND_LIST if q <= nd_max):
            L = (nd - 0.5) * seg
            h = L / nd
            for j in range(1, nd):
                for f in PHASES:
                    start = d["s_in"] + f * min(h, d["w"]) - j * h
                    assert d["s_lo"] < start and start + L < d["s_hi"]
                    pa, pb = p0 + start * u, p0 + (start + L) * u
                    a.append(se3(pa[0], pa[1], 0.0))
                    b.append(se3(pb[0], pb[1], 0.0))
                    tag.append((nd, j))
        a, b = _cat(a), _cat(b)
        n_probe = len(a)
        fa, fb = filler_edges(4200 - n_probe, 48, seg)
        perm = np.random.default_rng(int(frozen * 100)).permutation(4200)
        s1, s2 = np.concatenate([a, fa])[perm], np.concatenate([b, fb])[perm]
        where = np.empty(4200, np.int64)
        where[perm] = np.arange(4200)
        out.append(Batch(f"position_seg{seg}", 0, s1, s2, frozen,
                         meta={"probe": where[:n_probe], "tag": np.array(tag), "seg": seg}))
    return tuple(out)


# ---- s2 only ------------------------------------------------------------------------------------------------------------------
# Relative to the block's centre.  Found by a scan of the oracle over positions around the block and headings in
# [-0.9, 0.9]: turning in place there is valid from -0.9 up to a heading near 0.4 and invalid beyond (geometry() bisects
# that heading), so rotation-only edges of up to 20 segments end on the first invalid heading with a valid interior.
ROT_POINT = (-0.3, -0.6)


@functools.lru_cache(maxsize=None)
def s2_only() -> Tuple[Batch, ...]:
    """Every interior state valid, s2 invalid, nd = 0 .. 20: straight edges that end 0.02 m inside the first zone of the
    line (frozen extent 12.5: 0.125 m segments), and rotation-only edges that end at the first invalid heading of ROT_POINT."""
    g = geometry()
    x_end = g["x_zones"][0][0] + 0.02
    a, b = [], []
    for nd in range(21):
        L = 0.0 if nd == 0 else (nd - 0.5) * 0.125
        e = _line_edge(g, x_end - L, x_end)
        a.append(e[0]), b.append(e[1])
    px, py, yaw_bad = g["rot"]
    for nd in range(1, 21):
        dyaw = 2.0 * (nd - 0.5) * SEG_SO3
        a.append(se3(px, py, yaw_bad - dyaw)), b.append(se3(px, py, yaw_bad))
    return (Batch("s2_only", 0, _cat(a), _cat(b), 12.5, meta={"nd": list(range(21)) + list(range(1, 21))}),)


# ---- segment-count boundaries ---------------------------------------------------------------------------------------------------
KS = (1, 2, 3, 17)


def _count_edges(g, seg, x_end):
    """Edges along +x that END on x_end (invalid: inside the first zone), so that lastValid.second shows nd."""
    a, b, want = [], [], []
    for k in KS:                                   # planar length k seg exactly, one ulp below, one ulp above
        for side in (0, -1, 1):
            x1 = x_end - k * seg
            if side:
                x1 = np.nextafter(x1, -np.inf if side > 0 else np.inf)
            e = _line_edge(g, x1, x_end)
            a.append(e[0]), b.append(e[1]), want.append(k + (side > 0))
    for k in KS:                                   # pure rotations next to k seg_so3 (1e-9 rad to either side)
        for side in (-1, 1):
            dyaw = 2.0 * (k * SEG_SO3 + side * 1e-9)
            px, py, yaw_bad = g["rot"]
            a.append(se3(px, py, yaw_bad - dyaw)), b.append(se3(px, py, yaw_bad)), want.append(k + (side > 0))
    for m in (2, 5, 11):                           # SO(3) count one above the R^3 count, and the reverse
        for dr, ds in ((0, 1), (1, 0)):
            e = _line_edge(g, x_end - (m + dr - 0.5) * seg, x_end, yaw1=2.0 * (m + ds - 0.5) * SEG_SO3)
            a.append(e[0]), b.append(e[1]), want.append(m + 1)
    return _cat(a), _cat(b), np.array(want)


@functools.lru_cache(maxsize=None)
def count_boundaries() -> Tuple[Batch, ...]:
    """[0] mode 0 on the shared map, frozen extent 12.5 (segment 2^-3 exactly; the edges end at x = 0, inside the first
    zone, so that k seg and its neighbours are exact); [1] the same edges on the non-square map with its own extent
    (no exact multiples there: it pins ex != ey); [2] the 0.5 m rule at planar lengths 0.5 k and one ulp to either side."""
    g = geometry()
    assert g["x_zones"][0][0] < 0.0 < g["x_zones"][0][1] and 12.5 * 0.01 == 0.125
    a, b, want = _count_edges(g, 0.125, 0.0)
    out = [Batch("counts_frozen", 0, a, b, 12.5, meta={"want": want})]
    gr = geometry("rect")
    zr = z_extent(rect_map(), robot())
    seg = seg_r3(rect_map(), zr, 0.0)
    ar, br, wr = _count_edges(gr, seg, gr["x_zones"][0][0] + 0.02)
    out.append(Batch("counts_rect", 0, ar, br, 0.0, map="rect", meta={"want": wr, "seg": seg}))
    a1, b1, w1 = [], [], []
    for k in KS:
        for side in (0, -1, 1):
            L = 0.5 * k
            x2 = L if side == 0 else np.nextafter(L, np.inf if side > 0 else -np.inf)
            for y in (g["y_line"], -3.0):          # through the zones, and clear of the block
                a1.append(se3(0.0, y, 0.0)), b1.append(se3(x2, y, 0.0))
                w1.append(k - (side < 0))
    out.append(Batch("counts_half_metre", 1, _cat(a1), _cat(b1), meta={"want": np.array(w1)}))
    return tuple(out)


# ---- quaternion edges ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def quaternion_edges() -> Tuple[Batch, ...]:
    """Edges along the line through both zones (they fail at an interior state, so the lastValid state shows which way
    the slerp went), rotation-only edges at ROT_POINT and s1 == s2 pairs; every pair also with -q2."""
    g = geometry()
    x_in = g["x_zones"][0][0]
    cut = float(np.sqrt(2e-9))                     # arc at which the dot product is 1 - 1e-9
    a, b = [], []

    def both(e):
        a.append(e[0]), b.append(e[1])
        neg = e[1].copy()
        neg[:, 3:] = -neg[:, 3:]
        a.append(e[0]), b.append(neg)

    for x1, x2 in ((-1.0, 2.0), (x_in - 0.4, x_in + 0.1), (x_in + 0.02, x_in + 0.02), (-2.0, -2.0), (-2.0, -1.0)):
        both(_line_edge(g, x1, x2))                                         # b = -a: theta = 0 with a negative dot
        for dyaw in (np.pi - 1e-5, np.pi + 1e-5, np.pi - 1e-7, np.pi + 1e-7):   # next to a half turn
            both(_line_edge(g, x1, x2, 0.3, 0.3 + dyaw))
        for f in (0.999, 1.001, 0.5, 2.0):                                      # next to the 1 - 1e-9 cut-off
            both(_line_edge(g, x1, x2, 0.0, 2.0 * cut * f))
    px, py, yaw_bad = g["rot"]
    for dyaw in (np.pi - 1e-5, np.pi + 1e-5, 2.0 * cut * 0.999, 2.0 * cut * 1.001):
        both((se3(px, py, yaw_bad - dyaw), se3(px, py, yaw_bad)))
    return (Batch("quaternions", 0, _cat(a), _cat(b), 12.5),)


# ---- empty runs and lane alignment -----------------------------------------------------------------------------------------------
RUNS = (1, 63, 64, 65, 130, 1000)


def _interp_edge(g, c: int, bad_k: Optional[int]):
    """A mode-1 edge of c >= 1 tasks along +x: on the line through the zones with exactly state bad_k inside the first
    zone, or (bad_k None) clear of the block on y = -3."""
    L = 0.5 * c + 0.25
    step = L / (c + 1)
    if bad_k is None:
        return se3(-3.5, -3.0, 0.0), se3(-3.5 + L, -3.0, 0.0)
    x1 = g["x_zones"][0][0] + 0.1 - (bad_k + 1) * step
    return _line_edge(g, x1, x1 + L)


@functools.lru_cache(maxsize=None)
def empty_runs_interp() -> Tuple[Batch, ...]:
    """0.5 m rule: runs of RUNS edges with n_interp = 0 between edges with tasks; for every run length the first edge of
    a run lands on each of the 64 lanes of a wavefront's tasks (meta 'lanes': (run length, lane) of every run).  The edge
    BEHIND a run is invalid in one state, the one in front of it valid: a lane that takes the wrong edge is seen.
    Batches of at most ~5000 edges; the first begins with a run, the last ends with one; [-2] is all empty, [-1] has
    tasks in its last edge only."""
    g = geometry()
    empty = _line_edge(g, g["x_zones"][0][0] + 0.05, g["x_zones"][0][0] + 0.3)      # 0.25 m, both ends invalid: no state is looked at
    batches, a, b, lanes, off = [], [], [], [], 0

    def flush():
        nonlocal a, b, lanes, off
        if a:
            batches.append(Batch(f"empty_interp_{len(batches)}", 1, _cat(a), _cat(b), meta={"lanes": lanes}))
        a, b, lanes, off = [], [], [], 0

    def add(e, c):
        nonlocal off
        a.append(e[0]), b.append(e[1])
        off += c

    for R in RUNS:
        for lane in range(64):
            if len(a) + R + 8 > 5000:
                flush()
            need = (lane - off) % 64
            first = not a and lane == 0 and R == RUNS[0]
            while need:                            # valid edges of at most 12 tasks up to the lane
                c = min(need, 12)
                add(_interp_edge(g, c, None), c)
                need -= c
            if not a and not first:
                add(_interp_edge(g, 12, None), 12), add(_interp_edge(g, 12, None), 12)
                need = (lane - off) % 64
                while need:
                    c = min(need, 12)
                    add(_interp_edge(g, c, None), c)
                    need -= c
            lanes.append((R, off % 64))
            for _ in range(R):
                add(empty, 0)
            if not (R == RUNS[-1] and lane == 63):
                c = 2 + (lane % 5)
                add(_interp_edge(g, c, lane % c), c)
    flush()
    e0, e1 = np.repeat(empty[0], 300, axis=0), np.repeat(empty[1], 300, axis=0)
    batches.append(Batch("empty_interp_all_empty", 1, e0, e1, meta={"lanes": []}))
    last = _interp_edge(g, 3, 2)
    batches.append(Batch("empty_interp_last_only", 1, np.concatenate([e0, last[0]]), np.concatenate([e1, last[1]]),
                         meta={"lanes": []}))
    return tuple(batches)


LANE_SHIFTS = (0, 1, 31, 32, 33, 63)


@functools.lru_cache(maxsize=None)
def empty_runs_two_pass() -> Tuple[Batch, ...]:
    """checkMotion in two passes (frozen extent 12.5): runs of RUNS edges that are EMPTY IN PASS 2 -- they die in pass 1
    on an invalid s2, or have nd <= 1 -- between failure-position probes (alive after pass 1 for most strides, invalid in
    pass 2) and valid edges; one batch per lane shift of the first run.  More than 4096 edges and 24 tasks per edge on
    average.  [-2]: every edge empty in pass 2 (total2 == 0); [-1]: only the last edge has pass-2 tasks."""
    g = geometry()
    pos = failure_position()[0]
    pa, pb = pos.s1[pos.meta["probe"]], pos.s2[pos.meta["probe"]]
    x_end = g["x_zones"][0][0] + 0.02
    dead = _line_edge(g, x_end - 7.5 * 0.125, x_end)           # nd = 8, only s2 invalid
    short_ok = _line_edge(g, -2.0, -2.0 + 0.03)                # nd = 1, valid
    short_bad = _line_edge(g, x_end, x_end)                    # nd = 0, invalid
    fill = filler_edges(1, 60, 0.125)
    out = []
    for bi, shift in enumerate(LANE_SHIFTS):
        rng = np.random.default_rng(100 + bi)
        a, b, runs = [], [], []
        for q in range(shift):                                 # `shift` valid edges of nd = 2: one pass-2 task each (S > 2)
            e = _line_edge(g, -3.0, -3.0 + 1.5 * 0.125)
            a.append(e[0]), b.append(e[1])
        for ri, R in enumerate(RUNS):
            runs.append((R, len(a)))
            for q in range(R):
                e = (dead, short_ok, short_bad)[(q + ri) % 3] if R > 1 else dead
                a.append(e[0]), b.append(e[1])
            pick = rng.choice(len(pa), 60, replace=False)      # probes and long valid edges behind the run
            for i in pick:
                a.append(pa[i:i + 1]), b.append(pb[i:i + 1])
                a.append(fill[0]), b.append(fill[1])
        m = max(0, 4100 - len(a))
        fa, fb = filler_edges(m, 56, 0.125)
        a.append(fa), b.append(fb)
        out.append(Batch(f"empty_two_pass_shift{shift}", 0, _cat(a), _cat(b), 12.5, meta={"runs": runs}))
    n = 4100
    out.append(Batch("two_pass_all_empty", 0, np.repeat(dead[0], n, axis=0), np.repeat(dead[1], n, axis=0), 0.3125,
                     meta={"runs": []}))                        # seg 1/320: nd = 300 (s2 and the last interior states invalid), every edge dies in pass 1
    a = np.concatenate([np.repeat(dead[0], n, axis=0), filler_edges(1, 40, 1 / 320)[0]])
    b = np.concatenate([np.repeat(dead[1], n, axis=0), filler_edges(1, 40, 1 / 320)[1]])
    out.append(Batch("two_pass_last_only", 0, a, b, 0.3125, meta={"runs": []}))
    return tuple(out)


# ---- form thresholds -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def thresholds() -> Tuple[Batch, ...]:
    """n = 4095, 4096, 4097 at a total of exactly 24 n tasks, and n = 4096 one task short of it: the failure-position
    probes of the 0.0625 m segment, filled up with valid edges whose nd makes the total exact (meta 'total')."""
    pos = failure_position()[1]
    pa, pb = pos.s1[pos.meta["probe"]], pos.s2[pos.meta["probe"]]
    tags = pos.meta["tag"]
    out = []
    for n, short in ((4095, 0), (4096, 0), (4097, 0), (4096, 1)):
        tasks = int(tags[:, 0].sum())                            # tasks of a mode-0 edge = nd (nd >= 1)
        m = n - len(pa)
        want = 24 * n - short - tasks
        base = want // m
        nds = np.full(m, base)
        nds[:want - base * m] += 1
        assert 2 <= nds.min() and nds.max() <= 60 and nds.sum() == want
        x1 = -3.6 + 0.001 * (np.arange(m) % 400)
        fa, fb = se3(x1, -3.0, 0.0), se3(x1 + (nds - 0.5) * 0.0625, -3.0, 0.0)
        perm = np.random.default_rng(n + short).permutation(n)
        out.append(Batch(f"threshold_n{n}_short{short}", 0, np.concatenate([pa, fa])[perm], np.concatenate([pb, fb])[perm],
                         6.25, meta={"total": 24 * n - short}))
    return tuple(out)


# ---- few-edge team sizes -----------------------------------------------------------------------------------------------------------
FEW_SEG = 1.0 / 64                      # frozen extent 1.5625: an edge of 200 tasks is 3.1 m long
FEW_CALLS = (1, 2, 63, 64)


def _few_edge(g, tasks: int, kind: str):
    """A mode-0 edge of `tasks` tasks (nd = tasks) along +x.  kind 'ok': clear of the block; 's2': only s2 invalid;
    'last': the last interior state is the first failure (s2 fails too); 'early': fails from state 1 or 2 on."""
    nd = tasks
    L = (nd - 0.5) * FEW_SEG if nd > 1 else 0.4 * FEW_SEG
    h = L / nd
    x_in = g["x_zones"][0][0]
    if kind == "ok":
        return se3(-3.5, -3.0, 0.0), se3(-3.5 + L, -3.0, 0.0)
    x2 = {"s2": x_in + 0.3 * h, "last": x_in + 1.3 * h, "early": x_in + 0.3 * h + max(nd - 2, 0) * h}[kind]
    return _line_edge(g, x2 - L, x2)


@functools.lru_cache(maxsize=None)
def few_edges() -> Tuple[Batch, ...]:
    """One batch per call size: the call holds edges of 1 task, fewer tasks than the grid has chunks, as many, more, and
    (mode 1, second half of the tuple) none.  For call sizes 1 and 2 the chunk count follows the longest edge up to
    128, so calls of one edge are given edges of 127, 128, 129 and 200 tasks in turn (meta 'calls': slices)."""
    g = geometry()
    out = []
    for n in FEW_CALLS:
        cap = min(128, max(16, 2048 // n))
        sizes = [1, 2, 5, cap - 1, cap, cap + 1, 200]
        kinds = ("ok", "s2", "last", "early")
        a, b, calls = [], [], []
        if n == 1:
            for t in sizes:
                for k in kinds:
                    e = _few_edge(g, t, k)
                    calls.append((len(a), len(a) + 1))
                    a.append(e[0]), b.append(e[1])
        elif n == 2:
            for q, t in enumerate(sizes):
                for e in (_few_edge(g, t, kinds[q % 4]), _few_edge(g, sizes[(q + 3) % 7], kinds[(q + 1) % 4])):
                    a.append(e[0]), b.append(e[1])
                calls.append((len(a) - 2, len(a)))
        else:
            lo = len(a)
            for q in range(n):
                e = _few_edge(g, sizes[q % len(sizes)] if q else 200, kinds[(q // len(sizes) + q) % 4])
                a.append(e[0]), b.append(e[1])
            calls.append((lo, len(a)))
        out.append(Batch(f"few_n{n}", 0, _cat(a), _cat(b), 100 * FEW_SEG, meta={"calls": calls, "cap": cap}))
    for n in FEW_CALLS:                                         # the 0.5 m rule: 0, 1 and up to 16 tasks
        a, b = [], []
        for q in range(max(n, 4)):
            c = (0, 1, 15, 16, 7)[q % 5]
            e = (_line_edge(g, -2.0, -1.7) if c == 0 else _interp_edge(g, c, None if q % 2 else (q // 2) % c))
            a.append(e[0]), b.append(e[1])
        calls = [(i, i + 1) for i in range(len(a))] if n == 1 else [(0, 2), (2, 4)] if n == 2 else [(0, n)]
        out.append(Batch(f"few_interp_n{n}", 1, _cat(a), _cat(b), meta={"calls": calls}))
    return tuple(out)


# ---- pool ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pool_subset() -> Tuple[Batch, ...]:
    """At most 200 edges of the failure-position (0.125 m segment) and s2-only probes, for calls of one and two edges."""
    pos = failure_position()[0]
    idx = pos.meta["probe"][::4][:151]
    s = s2_only()[0]
    fa, fb = filler_edges(8, 20, 0.125)
    return (Batch("pool", 0, np.concatenate([pos.s1[idx], s.s1, fa])[:200], np.concatenate([pos.s2[idx], s.s2, fb])[:200], 12.5),)


FAMILIES = {"failure_position": failure_position, "s2_only": s2_only, "count_boundaries": count_boundaries,
            "quaternion_edges": quaternion_edges, "empty_runs_interp": empty_runs_interp,
            "empty_runs_two_pass": empty_runs_two_pass, "thresholds": thresholds, "few_edges": few_edges,
            "pool_subset": pool_subset}


# number of batches of every family (static, so that test collection builds nothing; pinned by test_edge_probe.py)
BATCH_COUNTS = {"failure_position": 2, "s2_only": 1, "count_boundaries": 3, "quaternion_edges": 1, "empty_runs_interp": 23,
                "empty_runs_two_pass": 8, "thresholds": 4, "few_edges": 8, "pool_subset": 1}
BATCH_IDS = [(f, i) for f, c in BATCH_COUNTS.items() for i in range(c)]


def batch(family: str, index: int) -> Batch:
    return FAMILIES[family]()[index]


def same(a, b, tol=0.0) -> bool:
    """Equal within tol; two NaNs and two equal infinities count as equal."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    with np.errstate(invalid="ignore"):
        return a.shape == b.shape and bool(((np.isnan(a) & np.isnan(b)) | (a == b) | (np.abs(a - b) <= tol)).all())


def all_batches():
    return [(f, i, b) for f, fn in FAMILIES.items() for i, b in enumerate(fn())]


def plan_total(ref: Ref) -> int:
    """Sum of the task counts of a mode-0 batch, as motion_plan_kernel forms it: 1 (s2) + max(nd - 1, 0) per edge."""
    return int((1 + np.maximum(ref.count - 1, 0)).sum())
