"""CPU checks of the kernel-order float32 restatement of the device map preprocessing (tests/preprocess_restated.py):
against its float64 reference, against the oracle's own restatement (oracle/map_processors.add_derived_layers), and the
shape of getCircularKernel's footprint at every size the morphology may meet.  The device side of the same chain is
swept in tests/test_preprocess_sweep.py (-m gpu)."""
import numpy as np
import pytest

import preprocess_restated as P
from synthetic import make_map

F32 = np.float32
U = P.U

# (rows, cols, res, robot, params overrides)
MAPS = [
    (61, 97, 0.05, "yaml", {}),
    (97, 61, 0.04, "defaults", {}),
    (41, 37, 0.3, "yaml", {}),
    (70, 53, 0.008, "yaml", {}),
    (5, 3, 0.04, "yaml", {}),
]


@pytest.mark.parametrize("size", range(-1, 201))
def test_disk_rows_are_centred_spans_and_symmetric(size):
    """getCircularKernel(size): every row of the footprint is ONE contiguous span that holds the centre column (what the
    device's one-span-per-row footprint stores), and the disk is symmetric about its anchor (size/2, size/2) -- under
    y -> 2r - y, x -> 2r - x wherever both lie inside, and under transposition; size <= 0: the 3 x 3 rectangle."""
    k = P.disk(size)
    if size <= 0:
        assert k.shape == (3, 3) and k.all()
        return
    assert k.shape == (size, size)
    r = size // 2
    for y in range(size):
        xs = np.flatnonzero(k[y])
        assert xs.size > 0 and xs[-1] - xs[0] + 1 == xs.size and xs[0] <= r <= xs[-1], (size, y, xs)
    assert np.array_equal(k, k.T)
    m = 2 * r - size + 1          # 1 for even sizes: the mirrored row / column `size` lies outside
    inner = k[m:, m:]
    assert np.array_equal(inner, inner[::-1, ::-1])
    assert k[r].all() and k[:, r].all()


@pytest.mark.parametrize("size", [-1, 0, 1, 2, 3, 4, 7, 15, 63, 64, 65, 75, 129])
def test_span_morphology_equals_the_oracle_morphology(size):
    """The restatement's span / sparse-table morphology is the oracle's offset-by-offset one (_erode / _dilate), exactly,
    on a non-square odd map with ties, at sizes on both sides of 64 and wider than the map."""
    rng = np.random.default_rng(size + 7)
    a = (np.round(rng.random((37, 23)) * 8) / 8).astype(F32)
    assert np.array_equal(P.erode(a, size), P.map_processors._erode(a, size))
    assert np.array_equal(P.dilate(a, size), P.map_processors._dilate(a, size))


def test_restatement_agrees_with_the_oracle_chain():
    """On one yaml map the new restatement and oracle/map_processors.add_derived_layers describe the same chain: every
    morphology and mask layer the oracle produces is identical, and so is plane_fit_std_dev (exact differences and a
    max).  The oracle's normals and CDF use np.cross / np.linalg.norm / pairwise sums and differ in the last bits."""
    gm = make_map(200, 0.04, seed=5)
    L = P.preprocess(gm["elevation"], gm.len_x, gm.len_y, gm.pos_x, gm.pos_y, traversability=gm["traversability"])
    assert L["traversability_sample_filter"].sum() > 0          # the oracle's all-zero fallback is not in play
    for name in ("traversability_thresholded", "elevation_masked", "sample_probability", "plane_fit_std_dev"):
        assert np.array_equal(L[name], gm[name]), name
    for name in ("normal_x", "normal_y", "normal_z"):
        assert np.abs(L[name] - gm[name]).max() < 2e-6
    assert L["_hole"].any() and L["_wall"].any() and not L["_hole"].all() and not L["_wall"].all()


@pytest.mark.parametrize("rows,cols,res,rob,over", MAPS, ids=lambda v: str(v))
def test_float32_restatement_within_the_float64_bounds(rows, cols, res, rob, over):
    """The float32 restatement against the float64 reference on the same float32 inputs.  Bounds (u = 2^-24):

    * plane_fit_std_dev: the difference of two floats is exact in float64, the float32 difference is its correct
      rounding, and rounding is monotone: float32(max |dz|64) EXACTLY.
    * normals, N terms, mean unit vector of length m (float64): every unit term carries at most ~6u per component
      (inexact coordinate differences, two products and a difference per component, sum of squares, sqrt, division;
      the cross product's cancellation is bounded by the norm it is divided by); the sequential float32 sum of N unit
      vectors adds at most N u per step relative to a partial sum of length <= N, so the mean is off by <= (6 + N) u;
      the division by the float count is exact in the bound; renormalising a vector of length m amplifies an absolute
      error by 1/m and adds 2u:  (12 + 2N) u / m + 2u -- and never more than 1e-5.
    * blur (k taps, two passes, non-negative terms): each pass has relative error <= (k + 1) u, the second pass carries
      the first's through relatively: (2k + 3) u relative.
    * row CDF over C columns: the row sum has relative error <= C u, every quotient one more u, the running sum of
      non-negative terms <= C u relative: (2C + 3) u relative.
    * row-wise CDF over R rows of C columns: row sums C u, total R u more, quotient u, running sum R u:
      (2R + 2C + 4) u relative."""
    elev, trav = P.sweep_map(rows, cols, res, seed=rows)
    len_x, len_y, pos_x, pos_y = rows * res, cols * res, 0.7, -0.3
    verts = P.sweep_vertices(rows, cols, res, pos_x, pos_y, seed=cols)
    prm, robo = P.params("yaml", **over), P.robot(rob)
    L = P.preprocess(elev, len_x, len_y, pos_x, pos_y, traversability=trav, vertices=verts, prm=prm, rob=robo)
    R = P.reference64(L, elev, (len_x, len_y, pos_x, pos_y), prm, robo)
    assert np.array_equal(L["plane_fit_std_dev"], R["plane_fit_std_dev"].astype(F32))
    assert (R["normal_tol"] <= 1e-5).all()
    for name in ("normal_x", "normal_y", "normal_z"):
        assert (np.abs(L[name] - R[name]) <= R["normal_tol"]).all(), name
    assert P.within(L["n_samples"], R["n_samples"], R["n_samples_tol"])
    assert P.within(L["cum_prob"], R["cum_prob"], R["cum_prob_tol"])
    assert P.within(L["cum_prob_rowwise"], R["cum_prob_rowwise"], R["cum_prob_rowwise_tol"])
    if L["_total"] > 0:
        assert L["cum_prob_rowwise"][-1] == pytest.approx(1.0, abs=rows * 4 * U)
    else:                                       # nothing to sample on this map: the CDFs are NaN, like the device's
        assert rows * cols < 32 and np.isnan(L["cum_prob_rowwise"]).all()


@pytest.mark.parametrize("rows,cols", [(61, 97), (4100, 3), (97, 91)])
def test_unknown_mass_order_and_cap(rows, cols):
    """The cap's masses in known_unknown_mass_kernel's order (one workgroup below 8192 cells, 64 above) are within
    n * 2^-53 of the exact sums, and the capped distribution gives the unobserved cells max_prob of the mass."""
    rng = np.random.default_rng(rows)
    prob = rng.random((rows, cols)).astype(F32)
    obs = np.ones((rows, cols), F32)
    obs[: rows // 3] = 0.0
    known, unknown = P.unknown_mass(prob, obs)
    p64 = prob.astype(np.float64)
    ek, eu = p64[obs > 0].sum(), p64[obs <= 0].sum()
    n = rows * cols
    assert abs(known - ek) <= n * 2.0 ** -53 * ek and abs(unknown - eu) <= n * 2.0 ** -53 * eu
    capped, _ = P.cap_unknown(prob, obs, 0.05)
    c64 = capped.astype(np.float64)
    assert abs(c64[obs <= 0].sum() / c64.sum() - 0.05) < 1e-6


def test_sweep_maps_cover_every_branch():
    """The sweep's maps have cells in both branches of every select (hole mask, wall mask, keep-unsafe, the masked
    elevation) for the yaml and the all-zero parameter sets, at the coarsest and the finest spacing."""
    for rows, cols, res in ((41, 37, 0.3), (100, 80, 0.008)):
        elev, trav = P.sweep_map(rows, cols, res)
        for kind in ("yaml", "defaults"):
            L = P.preprocess(elev, rows * res, cols * res, traversability=trav, prm=P.params(kind))
            for m in (L["_hole"], L["_wall"], L["_keep"], L["traversability_thresholded"] > 0.5):
                assert m.any() and not m.all(), (rows, res, kind)


@pytest.mark.parametrize("n", [1, 2, 3, 5, 8])
def test_reflect101_matches_numpy_reflect_padding(n):
    """gauss_pass_kernel's BORDER_REFLECT_101 index, applied as often as a blur wider than the axis needs, is numpy's
    'reflect' padding (gfedcb|abcdefgh|gfedcba) of any width; an axis of one cell always reads that cell."""
    w = 4 * n + 3
    padded = np.pad(np.arange(n), w, mode="reflect")
    for p in range(-w, n + w):
        assert P.reflect101(p, n) == padded[p + w], (n, p)
