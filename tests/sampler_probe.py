"""Probe maps for the state sampler (TEST INFRASTRUCTURE; tests/test_sampler_probe.py proves on the CPU that they
probe, tests/test_sampler_sweep.py runs them on the GPU).

The reference sampler (sampler.cpp:56-78) makes two linear scans, "first index whose cumulative value exceeds u, else
the last index".  sample_one answers the same question with a binary search over the row CDF (LDS, or global memory
above 2048 rows), a pivot per 16 columns (counted for cols <= 512, binary-searched above) and a 16-value group
compared against u rounded DOWN to float.  Every map here is small, carries only what the sampler reads (the validity
layers are the sampler's elevation) and is built so that the C oracle's own cells fall, at least CLASS_MIN times, into
every class the map is meant to reach:

  first_col       column 0
  col_last_value  column cols - 2, the last one a value can select (the scan stops there)
  col_else        column cols - 1, reached through the else-clause only
  col_mod0/15     the first / last column of a 16-column group
  cut_group       a column of the last group where cols is not a multiple of 16
  first_row       row 0
  last_row_else   row rows - 1 (else-clause of the row scan)
  nan_row         a row whose column CDF is NaN throughout (0 / 0 of an all-zero row)
  tie_upper       tie probes: sample k lands on the SECOND entry of its own pair (rd(u_k), next float up)
  tie_lower       tie probes: a sample lands on the FIRST entry of a pair (its u lies below every entry of the pair)

CDFs end at 0.9 unless a probe says otherwise, so a tenth of all samples takes either else-clause."""
from __future__ import annotations

import functools
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import numpy as np

import oracle_py as O
from synthetic import GridMap

CLASS_MIN = 100
N_DEFAULT = 1 << 16

COLS = [1, 2, 15, 16, 17, 31, 32, 33, 127, 128, 129, 511, 512, 513, 528, 529, 800, 1100]
ROWS = [1, 2, 3, 2047, 2048, 2049, 2100]
ORIGINS = {"zero": (0.0, 0.0), "near": (0.3, -0.2), "utm": (4.6e5, 5.2e6)}
SPACINGS = [0.04, 0.07, 0.1]
FIRST_INDICES = [0, (1 << 32) - 100, (1 << 32) + 7, (1 << 61) - 50, (1 << 63) + 11]
SEEDS = [0, 42, 0xFFFF_FFFF_0000_0001]
PLATEAUS = [1, 15, 16, 17, 40]
NAN_FROM = [3, 16, 40]


# ---- the counter-based uniforms, restated on arrays ----------------------------------------------------------------------
def uniform01_np(seed: int, index, k: int) -> np.ndarray:
    """artp_oracle_uniform01 on an array of 64-bit indices (unsigned arithmetic that wraps, as in C)."""
    idx = np.atleast_1d(np.asarray(index, np.uint64))
    s = np.full(1, seed, np.uint64)
    m1, m2 = np.full(1, 0xBF58476D1CE4E5B9, np.uint64), np.full(1, 0x94D049BB133111EB, np.uint64)
    x = s + np.full(1, 0x9E3779B97F4A7C15, np.uint64) * (idx * np.uint64(8) + np.full(1, k + 1, np.uint64))
    for rnd in range(2):
        if rnd:
            x = x + s
        x = x ^ (x >> np.uint64(30))
        x = x * m1
        x = x ^ (x >> np.uint64(27))
        x = x * m2
        x = x ^ (x >> np.uint64(31))
    return (x >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def indices(first: int, n: int) -> np.ndarray:
    """first + 0 .. first + n - 1 modulo 2^64."""
    return np.full(1, first, np.uint64) + np.arange(n, dtype=np.uint64)


def rd_f32(u) -> np.ndarray:
    """u rounded DOWN to float32 (the kernel's __double2float_rd)."""
    u = np.asarray(u, np.float64)
    f = u.astype(np.float32)
    up = f.astype(np.float64) > u
    return np.where(up, np.nextafter(f, np.float32(-np.inf)), f).astype(np.float32)


# ---- maps ----------------------------------------------------------------------------------------------------------------
@dataclass
class Probe:
    name: str
    gm: GridMap
    classes: Tuple[str, ...]
    seed: int = 42
    first: int = 12345
    n: int = N_DEFAULT
    gpu: bool = True                      # False: pinned on the CPU only (rows whose CDF turns NaN part-way)
    tie: Optional[dict] = None            # tie probes: {"axis": 0 col / 1 row, "k": K, "rank": sorted rank of each of the K samples, ...}
    extra: Dict[str, object] = field(default_factory=dict)


def sampler_layers(gm: GridMap, rng: np.random.Generator) -> None:
    """Elevation (also both validity layers), unit normals with a random tilt, a spread that straddles min(std, 0.5)."""
    i = np.arange(gm.rows)[:, None]
    j = np.arange(gm.cols)[None, :]
    h = (0.3 * np.sin(0.37 * i) * np.cos(0.23 * j)).astype(np.float32)
    gm.add("elevation", h)
    gm.add("elevation_masked", h)
    nx = rng.uniform(-0.3, 0.3, (gm.rows, gm.cols))
    ny = rng.uniform(-0.3, 0.3, (gm.rows, gm.cols))
    gm.add("normal_x", nx)
    gm.add("normal_y", ny)
    gm.add("normal_z", np.sqrt(1.0 - nx * nx - ny * ny))
    gm.add("plane_fit_std_dev", rng.uniform(0.0, 0.9, (gm.rows, gm.cols)))


def cdf_from_prob(prob: np.ndarray, col_top: float = 0.9, row_top: float = 0.9):
    """computeCumulativeProbabilityDistribution (probability_distribution.cpp:20-46) in float32, each CDF then scaled
    to end at *_top.  An all-zero row divides 0 by 0: its column CDF is NaN throughout."""
    p = np.asarray(prob, np.float32)
    rs = p.sum(axis=1, dtype=np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        cp = np.cumsum(p / rs[:, None], axis=1, dtype=np.float32) * np.float32(col_top)
    cr = np.cumsum(rs / rs.sum(dtype=np.float32), dtype=np.float32) * np.float32(row_top)
    return cp.astype(np.float32), cr.astype(np.float32)


def set_cdf(gm: GridMap, cp: np.ndarray, cr: np.ndarray) -> None:
    assert cp.shape == (gm.rows, gm.cols) and cr.shape == (gm.rows,)
    gm.layers["cum_prob"] = np.asfortranarray(cp, dtype=np.float32)
    gm.layers["cum_prob_rowwise"] = np.ascontiguousarray(cr, np.float32)


_EDGE_COLS = [0, 15, 16, 17, 31, 32, 127, 128, 511, 512, 513, 527, 528]
_EDGE_ROWS = [0, 2046, 2047, 2048]


def shaped_prob(rows: int, cols: int, rng: np.random.Generator) -> np.ndarray:
    """Random cell weights in [0.5, 1.5], heavier at the columns and rows next to a group, pivot or LDS edge and in the
    last group, so that every class collects samples whatever the size of the map."""
    p = rng.uniform(0.5, 1.5, (rows, cols))
    cb, rb = max(1.0, cols / 16.0), max(1.0, rows / 16.0)
    last_group = list(range(((cols - 1) // 16) * 16, cols))
    for c in set(_EDGE_COLS + [cols - 2] + last_group):
        if 0 <= c < cols:
            p[:, c] *= cb
    for r in set(_EDGE_ROWS + [rows - 2]):
        if 0 <= r < rows:
            p[r, :] *= rb
    return p


def default_classes(rows: int, cols: int) -> Tuple[str, ...]:
    c = ["first_col", "col_else", "first_row"]
    if cols >= 2:
        c.append("col_last_value")
    if cols >= 16:
        c.append("col_mod15")
    if cols >= 17:
        c.append("col_mod0")
    if cols > 16 and cols % 16:
        c.append("cut_group")
    if rows >= 2:
        c.append("last_row_else")
    return tuple(c)


def shape_probe(name, rows, cols, res=0.04, pos=(0.3, -0.2), seed=1, **kw) -> Probe:
    rng = np.random.default_rng(seed)
    gm = GridMap(rows, cols, res, pos[0], pos[1])
    sampler_layers(gm, rng)
    set_cdf(gm, *cdf_from_prob(shaped_prob(rows, cols, rng)))
    return Probe(name, gm, default_classes(rows, cols), **kw)


def plateau_probe() -> Probe:
    """Row (L, o): L zero-probability columns from column 16 + o on, for L in PLATEAUS and every o modulo 16."""
    rows, cols = len(PLATEAUS) * 16, 112
    rng = np.random.default_rng(11)
    p = shaped_prob(rows, cols, rng)
    runs = []
    for a, L in enumerate(PLATEAUS):
        for o in range(16):
            p[a * 16 + o, 16 + o:16 + o + L] = 0.0
            p[a * 16 + o, [16 + o - 1, 16 + o + L]] *= 30.0     # the columns on either side of the plateau
            runs.append((a * 16 + o, 16 + o, L))
    gm = GridMap(rows, cols, 0.04, 0.3, -0.2)
    sampler_layers(gm, rng)
    set_cdf(gm, *cdf_from_prob(p))
    return Probe("plateaus", gm, default_classes(rows, cols), n=1 << 17, extra={"runs": runs})


ZERO_ROWS = [0, 1, 7, 20, 21, 22, 23, 47]


def zero_rows_probe() -> Probe:
    """All-zero rows (row 0, the LAST row and some between): plateaus of the row CDF, NaN column CDFs.  A zero row is
    reached through the row scan's else-clause only, i.e. the last row; there both scans end at cols - 1."""
    rows, cols = 48, 40
    rng = np.random.default_rng(12)
    p = shaped_prob(rows, cols, rng)
    p[ZERO_ROWS, :] = 0.0
    gm = GridMap(rows, cols, 0.04, 0.3, -0.2)
    sampler_layers(gm, rng)
    cp, cr = cdf_from_prob(p)
    assert np.isnan(cp[ZERO_ROWS]).all() and np.isfinite(np.delete(cp, ZERO_ROWS, axis=0)).all()
    set_cdf(gm, cp, cr)
    return Probe("zero_rows", gm, ("first_col", "col_else", "col_last_value", "col_mod15", "col_mod0", "cut_group",
                                   "last_row_else", "nan_row"))


def nan_partway_probe() -> Probe:
    """Row i turns NaN at column NAN_FROM[i] and stays NaN (CPU only: the reference's processors cannot produce such a
    row, see include/artp_c.h; the oracle's answer is pinned all the same)."""
    rows, cols = len(NAN_FROM), 64
    rng = np.random.default_rng(13)
    gm = GridMap(rows, cols, 0.04, 0.3, -0.2)
    sampler_layers(gm, rng)
    cp, cr = cdf_from_prob(rng.uniform(0.5, 1.5, (rows, cols)), 1.0, 1.0)
    for i, c in enumerate(NAN_FROM):
        cp[i, c:] = np.nan
    set_cdf(gm, cp, cr)
    return Probe("nan_partway", gm, ("first_col", "col_else", "first_row"), gpu=False)


def tops_at_one_probe() -> Probe:
    """The float32 cumulative sums as they come, ending at 1 up to rounding: no macroscopic else-clause."""
    rows, cols = 40, 72
    rng = np.random.default_rng(14)
    gm = GridMap(rows, cols, 0.04, 0.3, -0.2)
    sampler_layers(gm, rng)
    set_cdf(gm, *cdf_from_prob(shaped_prob(rows, cols, rng), 1.0, 1.0))
    return Probe("tops_at_one", gm, ("first_col", "col_last_value", "col_mod15", "col_mod0", "first_row"))


def tie_probe(name, axis: int, K: int, lanes: int, seed=42, first=12345, n=N_DEFAULT) -> Probe:
    """axis 0: every row of the map is rd(u_0), next(rd(u_0)), rd(u_1), next(rd(u_1)), ..., 1 for the sorted column
    draws u_k (k = 0) of the batch's first K samples: the scan answers sample k at the second entry of its pair (the
    first does not exceed u_k, the second does).  axis 1: the same transposed, for the row draws (k = 1).
    lanes: identical rows (axis 0) / identical columns (axis 1)."""
    u = uniform01_np(seed, indices(first, K), axis)
    order = np.argsort(u, kind="stable")
    us = u[order]
    lo = rd_f32(us)
    hi = np.nextafter(lo, np.float32(np.inf)).astype(np.float32)
    assert (lo[1:] > hi[:-1]).all() and hi[-1] < np.float32(1.0), "the K draws are too close for distinct pairs"
    line = np.empty(2 * K + 1, np.float32)
    line[0:2 * K:2], line[1:2 * K:2], line[2 * K] = lo, hi, 1.0
    rng = np.random.default_rng(15 + axis)
    flat = (np.arange(lanes, dtype=np.float64) + 1.0) / lanes
    if axis == 0:
        gm = GridMap(lanes, 2 * K + 1, 0.04, 0.3, -0.2)
        set_cdf(gm, np.repeat(line[None, :], lanes, axis=0), flat.astype(np.float32))
    else:
        gm = GridMap(2 * K + 1, lanes, 0.04, 0.3, -0.2)
        set_cdf(gm, np.repeat(flat.astype(np.float32)[None, :], 2 * K + 1, axis=0), line)
    sampler_layers(gm, rng)
    rank = np.empty(K, np.int64)
    rank[order] = np.arange(K)
    exact = int((lo.astype(np.float64) == us).sum())          # draws that ARE float32 values: entry == u
    rounds_up = int((us.astype(np.float32).astype(np.float64) > us).sum())
    return Probe(name, gm, ("tie_upper", "tie_lower"), seed=seed, first=first, n=n,
                 tie={"axis": axis, "k": K, "rank": rank, "exact": exact, "rounds_up": rounds_up})


@functools.lru_cache(maxsize=None)
def all_probes() -> Tuple[Probe, ...]:
    ps: List[Probe] = []
    for c in COLS:
        ps.append(shape_probe(f"cols_{c}", 5, c, seed=100 + c, n=(1 << 17) if c > 512 else N_DEFAULT))
    for r in ROWS:
        ps.append(shape_probe(f"rows_{r}", r, 6, seed=200 + r, n=(1 << 17) if r > 512 else N_DEFAULT))
    ps += [plateau_probe(), zero_rows_probe(), nan_partway_probe(), tops_at_one_probe()]
    for oname, pos in ORIGINS.items():
        for res in SPACINGS:
            ps.append(shape_probe(f"origin_{oname}_{res}", 48, 40, res=res, pos=pos, seed=300))
    idx_map = shape_probe("idx", 33, 49, seed=400).gm
    for s in SEEDS:
        for f in FIRST_INDICES:
            ps.append(Probe(f"idx_seed{s:#x}_first{f:#x}", idx_map, default_classes(33, 49), seed=s, first=f))
    # the four maps of the full cross: one per search form, and a tie probe that the validity layers accept
    ps.append(shape_probe("cross_cols_le_512", 64, 129, seed=500, n=1 << 18))
    ps.append(shape_probe("cross_cols_gt_512", 64, 800, seed=501, n=1 << 18))
    ps.append(shape_probe("cross_rows_gt_2048", 2100, 64, seed=502, n=1 << 18))
    ps.append(tie_probe("cross_tie_cols_501", 0, 250, 64, n=1 << 18))
    # tie probes: single-row (cols <= 512, > 512) and single-column (rows <= 2048, > 2048) maps
    ps.append(tie_probe("tie_cols_501", 0, 250, 1))
    ps.append(tie_probe("tie_cols_601", 0, 300, 1))
    ps.append(tie_probe("tie_rows_1001", 1, 500, 1))
    ps.append(tie_probe("tie_rows_2201", 1, 1100, 1))
    names = [p.name for p in ps]
    assert len(set(names)) == len(names)
    return tuple(ps)


CROSS = ("cross_cols_le_512", "cross_cols_gt_512", "cross_rows_gt_2048", "cross_tie_cols_501")


def probe(name: str) -> Probe:
    return next(p for p in all_probes() if p.name == name)


def gpu_probes() -> List[Probe]:
    return [p for p in all_probes() if p.gpu]


# ---- references ----------------------------------------------------------------------------------------------------------
def oracle_samples(p: Probe, kind: str = "yaml", n: Optional[int] = None, first: Optional[int] = None,
                   sample_uniform: bool = False):
    """(states [n, 7], rowcol [n, 2]) of the C oracle's linear-scan sampler."""
    return O.OracleSampler(p.gm, sample_uniform=sample_uniform).sample(
        O.robot(kind), p.seed, p.first if first is None else first, p.n if n is None else n)


def scan_cells_np(gm: GridMap, seed: int, first: int, n: int, chunk: int = 8192) -> np.ndarray:
    """"First index whose cumulative value exceeds u, else the last index" for both scans, in float64 numpy."""
    cp = np.asarray(gm["cum_prob"], np.float64)
    cr = np.asarray(gm["cum_prob_rowwise"], np.float64)
    out = np.empty((n, 2), np.int32)
    idx = indices(first, n)
    for a in range(0, n, chunk):
        u_col = uniform01_np(seed, idx[a:a + chunk], 0)
        u_row = uniform01_np(seed, idx[a:a + chunk], 1)
        row = _first_exceeding(cr[None, :-1], u_row)
        col = _first_exceeding(cp[row, :-1], u_col)
        out[a:a + chunk, 0], out[a:a + chunk, 1] = row, col
    return out


def _first_exceeding(values: np.ndarray, u: np.ndarray) -> np.ndarray:
    """Per sample: the first index of values[..., :] (all but the last entry of a CDF) that exceeds u, else their number."""
    if values.shape[1] == 0:
        return np.zeros(len(u), np.int64)
    hit = values > u[:, None]
    return np.where(hit.any(axis=1), hit.argmax(axis=1), values.shape[1])


def class_masks(p: Probe, rc: np.ndarray) -> Dict[str, np.ndarray]:
    """Which samples (cells rc of the oracle) fall into every class the probe is meant to reach."""
    rows, cols = p.gm.rows, p.gm.cols
    r, c = rc[:, 0], rc[:, 1]
    m = {"first_col": c == 0, "col_last_value": c == cols - 2, "col_else": c == cols - 1, "col_mod0": c % 16 == 0,
         "col_mod15": c % 16 == 15, "cut_group": c >= ((cols - 1) // 16) * 16, "first_row": r == 0,
         "last_row_else": r == rows - 1,
         "nan_row": np.isnan(np.asarray(p.gm["cum_prob"]))[r].all(axis=1) if "nan_row" in p.classes else None}
    if p.tie:
        k, ax = p.tie["k"], 1 - p.tie["axis"]   # rc column that the tie decides: col for axis 0, row for axis 1
        upper = np.zeros(len(rc), bool)
        upper[:k] = rc[:k, ax] == 2 * p.tie["rank"] + 1
        m["tie_upper"] = upper
        lower = rc[:, ax] % 2 == 0
        lower[:k] = False
        m["tie_lower"] = lower
    return {name: m[name] for name in p.classes}
