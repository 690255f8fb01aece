"""The device map preprocessing (artp_preprocess_map_ex and what hangs off a preprocessed map) across spacings, shapes,
parameter sets and map contents (-m gpu), against the kernel-order float32 restatement of tests/preprocess_restated.py.

The library is built with -ffp-contract=off and its division and sqrt are correctly rounded, so the restatement is
exact: every layer artp_preprocessed_get_layer returns must be BIT-EQUAL (np.array_equal; NaN cells of cum_prob
compare equal).  On top, the device's floating-point layers must lie within the float64 reference's derived bounds
(the derivations are in tests/test_preprocess_restated.py), so that the restatement and the kernels cannot share a
mistake.

The points reach what the square yaml maps of test_preprocess.py do not: spacings from 0.3 m (footprint sizes <= 0 ->
the 3 x 3 rectangle, one normal term) to 0.008 m (a 75-wide margin disk), disks 63, 64, 65 and 129 wide, rows != cols,
sizes that are no multiple of 8 or 64, tiny maps, a 4100 x 3 map (serial row CDF, the 64-workgroup mass sum), both
parameter sets and robots, observed strips with and without the unknown cap, vertices inside, outside and on the edges
of the map with and without the density term, a blur wider than the map."""
import math

import numpy as np
import pytest

import oracle_py as O
import preprocess_restated as P
from synthetic import GridMap

pytestmark = pytest.mark.gpu

F32 = np.float32
LAYERS = ("elevation", "traversability", "normal_x", "normal_y", "normal_z", "plane_fit_std_dev",
          "traversability_thresholded_no_safety", "traversability_thresholded", "elevation_masked",
          "sample_probability", "cum_prob", "observed", "n_samples", "traversability_sample_filter", "cum_prob_rowwise")
POS = (0.7, -0.3)


def _pt(shape, res=0.04, kind="yaml", robot="yaml", untrav=1, trav=True, observed=False, verts=True, over=None,
        disks=None, cap_acts=False):
    return dict(shape=shape, res=res, kind=kind, robot=robot, untrav=untrav, trav=trav, observed=observed, verts=verts,
                over=over or {}, disks=disks or {}, cap_acts=cap_acts)


POINTS = {
    # spacings
    "res0.3": _pt((41, 37), 0.3, disks=dict(search=2, hole=1, margin=2, fh=1)),
    "res0.2": _pt((53, 47), 0.2),
    "res0.1": _pt((97, 61), 0.1),
    "res0.05": _pt((61, 97), 0.05),
    "res0.04": _pt((130, 121), 0.04),
    "res0.02": _pt((150, 131), 0.02),
    "res0.008-margin75": _pt((100, 80), 0.008, disks=dict(margin=75)),
    # one disk 63, 64, 65 and 129 wide
    "margin63": _pt((100, 80), over=dict(foothold_margin=62.5 * 0.04 / 2), disks=dict(margin=63)),
    "hole64": _pt((100, 80), over=dict(foothold_margin_max_hole_size=64.5 * 0.04), disks=dict(hole=64)),
    "hole65": _pt((80, 100), over=dict(foothold_margin_max_hole_size=65.5 * 0.04), disks=dict(hole=65)),
    "margin65": _pt((100, 80), over=dict(foothold_margin=64.5 * 0.04 / 2), disks=dict(margin=65)),
    "search129": _pt((100, 80), over=dict(foothold_margin_max_drop_search_radius=128.5 * 0.04 / 2),
                     disks=dict(search=129)),
    # shapes
    "odd97x61": _pt((97, 61)),
    "odd61x97": _pt((61, 97)),
    "tiny2x2": _pt((2, 2)),
    "tiny2x7": _pt((2, 7)),
    "tiny5x3-blur-wider-than-map": _pt((5, 3)),
    "tall4100x3-cap": _pt((4100, 3), untrav=0, observed=True, over=dict(max_prob_unknown_samples=0.05), cap_acts=True),
    # parameters
    "defaults-params": _pt((97, 61), kind="defaults"),
    "defaults-robot": _pt((61, 97), robot="defaults"),
    "defaults-both-0.3": _pt((41, 37), 0.3, kind="defaults", robot="defaults"),
    "no-traversability": _pt((97, 61), trav=False),
    "observed-untraversable": _pt((97, 61), observed=True),
    "observed-cap-small": _pt((61, 97), untrav=0, observed=True, over=dict(max_prob_unknown_samples=0.05),
                              cap_acts=True),
    "observed-cap-large": _pt((130, 121), untrav=0, observed=True, over=dict(max_prob_unknown_samples=0.05),
                              cap_acts=True),
    "observed-no-cap": _pt((97, 61), untrav=0, observed=True, over=dict(use_max_prob_unknown_samples=0)),
    "vertices-no-density": _pt((97, 61), over=dict(use_inverse_vertex_density=0)),
    "no-vertices": _pt((61, 97), verts=False),
}


@pytest.fixture(scope="module")
def contexts():
    from art_planner_amd.context import Context, make_params
    made = {}

    def get(robot="yaml", untrav=1):
        if (robot, untrav) not in made:
            made[(robot, untrav)] = Context(0, make_params(robot, unknown_space_untraversable=untrav))
        return made[(robot, untrav)]

    yield get
    for c in made.values():
        c.close()


def _inputs(pt, seed=0, pos=POS):
    rows, cols = pt["shape"]
    res = pt["res"]
    elev, trav = P.sweep_map(rows, cols, res, seed=seed + rows + cols)
    obs = None
    if pt["observed"]:
        obs = np.ones((rows, cols), F32)
        obs[:, : max(cols // 4, 1)] = 0.0                      # unobserved strips
        obs[rows // 2: rows // 2 + max(rows // 8, 1), :] = 0.0
    verts = P.sweep_vertices(rows, cols, res, *pos, seed=seed) if pt["verts"] else None
    return elev, (trav if pt["trav"] else None), obs, verts


def _device(ctx, pt, elev, trav, obs, verts, pos=POS):
    rows, cols = elev.shape
    return ctx.preprocess_map(elev, rows * pt["res"], cols * pt["res"], *pos, traversability=trav, kind=pt["kind"],
                              observed=obs, vertices=verts, **pt["over"])


def _compare(pp, L, tag):
    """Layer-by-layer bit equality; returns the list of mismatching layers (with a short description)."""
    bad = []
    got = {name: pp.layer(name) for name in LAYERS}
    for name in LAYERS:
        a, b = got[name], L[name]
        if not np.array_equal(a, b, equal_nan=True):
            with np.errstate(invalid="ignore"):
                d = a != b
                d &= ~(np.isnan(a) & np.isnan(b))
            bad.append(f"{tag}:{name} ({int(d.sum())} cells)")
    return got, bad


def _expected(name, pos=POS):
    """The restated layers of one point at map position pos, after checking that the point reaches what it is there
    for."""
    pt = POINTS[name]
    rows, cols = pt["shape"]
    res = pt["res"]
    prm = P.params(pt["kind"], **pt["over"])
    rob = P.robot(pt["robot"], unknown_space_untraversable=pt["untrav"])
    geom = (rows * res, cols * res) + tuple(pos)
    # the point reaches the footprint sizes it is there for
    sz = P.sizes(prm, P.cell_size(rows, geom[0]))
    for k, v in pt["disks"].items():
        assert sz[k] == v, (k, sz)
    elev, trav, obs, verts = _inputs(pt, pos=pos)
    L = P.preprocess(elev, *geom, traversability=trav, observed=obs, vertices=verts, prm=prm, rob=rob)
    if min(rows, cols) >= 32:    # the comparison cannot pass on an all-pass map
        for what in ("_hole", "_wall", "_keep"):
            assert L[what].any() and not L[what].all(), what
        if trav is not None:     # without a traversability layer nothing is below the threshold
            assert (L["traversability_thresholded"] > 0.5).any() and (L["traversability_thresholded"] <= 0.5).any()
    if pt["cap_acts"]:
        known, unknown = L["_mass"]
        assert unknown / (known + unknown) > prm.max_prob_unknown_samples
    if pt["verts"] and prm.use_inverse_vertex_density:
        assert 0 < L["_counts"].sum() < len(verts)                 # some vertices in, some out
    if name.startswith("tiny5x3"):
        assert len(L["_taps"]) > 2 * max(rows, cols)               # the blur reflects more than once
    return pt, prm, rob, geom, (elev, trav, obs, verts), L


def _float64_violations(got, L, elev, geom, prm, rob):
    """The device's floating-point layers against the float64 reference's derived bounds: the layers outside them."""
    bad = []
    Ld = dict(L)
    Ld["sample_probability"] = got["sample_probability"]
    R = P.reference64(Ld, elev, geom, prm, rob)
    assert (R["normal_tol"] <= 1e-5).all()
    for k in ("normal_x", "normal_y", "normal_z"):
        if not (np.abs(got[k] - R[k]) <= R["normal_tol"]).all():
            bad.append(f"float64:{k}")
    if not np.array_equal(got["plane_fit_std_dev"], R["plane_fit_std_dev"].astype(F32)):
        bad.append("float64:plane_fit_std_dev")
    if "n_samples" in R and not P.within(got["n_samples"], R["n_samples"], R["n_samples_tol"]):
        bad.append("float64:n_samples")
    if not P.within(got["cum_prob"], R["cum_prob"], R["cum_prob_tol"]):
        bad.append("float64:cum_prob")
    if not P.within(got["cum_prob_rowwise"], R["cum_prob_rowwise"], R["cum_prob_rowwise_tol"]):
        bad.append("float64:cum_prob_rowwise")
    return bad


def _check_point(contexts, name, pos=POS, float64=True, expected=None):
    """One point at map position pos: every layer bit-equal to the restatement (expected: what _expected(name, pos)
    returned, if the caller has it) and, where float64 is set, the device within the float64 bounds.  Returns the number
    of compared cells."""
    pt, prm, rob, geom, (elev, trav, obs, verts), L = expected or _expected(name, pos)
    pp = _device(contexts(pt["robot"], pt["untrav"]), pt, elev, trav, obs, verts, pos)
    got, bad = _compare(pp, L, name)
    if float64:
        bad += _float64_violations(got, L, elev, geom, prm, rob)
    pp.close()
    assert not bad, bad
    return sum(got[k].size for k in LAYERS)


@pytest.mark.parametrize("name", list(POINTS))
def test_preprocessing_is_bit_equal_to_the_restatement(contexts, name):
    _check_point(contexts, name)


def _check_change_from(contexts, shape, pos=POS, shifts=((0, 0), (3, -2), (-4, 5), (None, -1), (2, None))):
    """computeChange between maps whose origins differ by (+-k, -+m) cells and by more than the map: the updated layer,
    its rectangle and its count are exact; the partial last wavefront of change_kernel's reduction is in play
    (rows * cols is no multiple of 64)."""
    rows, cols = shape
    res = 0.05
    ctx = contexts()
    elev, trav = P.sweep_map(rows, cols, res, seed=3)
    len_x, len_y = rows * res, cols * res
    shifts = [(rows + 3 if si is None else si, -(cols + 1) if sj is None else sj) for si, sj in shifts]
    old = ctx.preprocess_map(elev, len_x, len_y, *pos, traversability=trav)
    e2 = elev.copy()
    e2[10:20, 5:17] += F32(0.2)
    t2 = trav.copy()
    t2[40:50, 30:40] = 0.0
    upd, rect, cnt = old.change_from(old, 0.05)
    assert cnt == 0 and rect == (0, 0, 0, 0) and not upd.any()
    for si, sj in shifts:
        new = ctx.preprocess_map(e2, len_x, len_y, pos[0] + si * res, pos[1] + sj * res, traversability=t2)
        upd, rect, cnt = new.change_from(old, 0.05)
        eu, erect, ecnt = P.change(new.layer("elevation"), new.layer("traversability_thresholded"),
                                   old.layer("elevation"), old.layer("traversability_thresholded"), si, sj, 0.05)
        assert np.array_equal(upd, eu), (si, sj, int((upd != eu).sum()))
        assert rect == erect and cnt == ecnt, (si, sj, rect, erect, cnt, ecnt)
        assert np.array_equal(new.layer("updated"), upd)
        if si == 0 and sj == 0:
            assert 0 < cnt < rows * cols
        if abs(si) >= rows or abs(sj) >= cols:
            assert cnt == rows * cols and rect == (0, 0, rows, cols)
        new.close()
    old.close()


@pytest.mark.parametrize("shape", [(97, 61), (61, 97)])
def test_change_from_on_shifted_non_square_maps(contexts, shape):
    _check_change_from(contexts, shape)


def test_reweight_equals_a_fresh_preprocessing(contexts):
    """reweight_dev(vertices) re-runs the sampling distribution on a preprocessed map: every layer bit-equal to a fresh
    preprocess_map with the same vertices; reweight_dev(None) goes back to the map without the density term."""
    import torch
    rows, cols, res = 97, 61, 0.04
    ctx = contexts()
    elev, trav = P.sweep_map(rows, cols, res, seed=11)
    verts = P.sweep_vertices(rows, cols, res, *POS, seed=5)
    geom = (rows * res, cols * res) + POS
    pp = ctx.preprocess_map(elev, *geom, traversability=trav)
    fresh = ctx.preprocess_map(elev, *geom, traversability=trav, vertices=verts)
    vt = torch.tensor(verts, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    pp.reweight_dev(vt, install_sampler=False)
    ctx.synchronize()
    L = P.preprocess(elev, *geom, traversability=trav, vertices=verts)
    assert L["n_samples"].any()
    for name in LAYERS:
        a = pp.layer(name)
        assert np.array_equal(a, fresh.layer(name), equal_nan=True), name
        assert np.array_equal(a, L[name], equal_nan=True), name
    pp.reweight_dev(None, install_sampler=False)
    ctx.synchronize()
    plain = ctx.preprocess_map(elev, *geom, traversability=trav)
    for name in LAYERS:
        assert np.array_equal(pp.layer(name), plain.layer(name), equal_nan=True), name
    for m in (pp, fresh, plain):
        m.close()


def _gridmap(L, rows, cols, res):
    gm = GridMap(rows, cols, res, *POS)
    for name in ("elevation", "elevation_masked", "normal_x", "normal_y", "normal_z", "plane_fit_std_dev", "cum_prob"):
        gm.add(name, L[name])
    gm.layers["cum_prob_rowwise"] = np.ascontiguousarray(L["cum_prob_rowwise"], np.float32)
    return gm


def test_install_of_a_non_square_odd_map_equals_the_host_upload():
    """install() of a 97 x 61 map == upload_map of the restated layers: the same sampled states (the CDFs are
    bit-equal, so every draw lands in the same cell) and labels, which the C oracle confirms; a second install with a
    changed patch (the rectangle path) == a fresh install of the changed map."""
    from art_planner_amd.context import Context
    rows, cols, res = 97, 61, 0.04
    elev, trav = P.sweep_map(rows, cols, res, seed=21)
    geom = (rows * res, cols * res) + POS
    L = P.preprocess(elev, *geom, traversability=trav)
    gm = _gridmap(L, rows, cols, res)
    a, b = Context(0, "yaml"), Context(0, "yaml")
    a.upload_map(gm)
    pp = b.preprocess_map(elev, *geom, traversability=trav)
    pp.install()
    sa, sb = a.sample_states(3, 0, 1 << 15), b.sample_states(3, 0, 1 << 15)
    assert np.array_equal(sa, sb, equal_nan=True)
    la = a.validate_states(sa)
    assert np.array_equal(la, b.validate_states(sa))
    assert np.array_equal(la[:8000], O.OracleMap(gm).states_valid(O.robot("yaml"), sa[:8000]))
    assert 0 < la.sum() < la.size

    e2 = elev.copy()
    e2[30:45, 20:33] += F32(0.15)
    pp2 = b.preprocess_map(e2, *geom, traversability=trav)
    pp2.install()                                   # same geometry: the rectangle path
    c = Context(0, "yaml")
    pp3 = c.preprocess_map(e2, *geom, traversability=trav)
    pp3.install()
    for slot in (0, 1):
        tb, rb = b.partner_table(slot, (rows, cols))
        tc, rc = c.partner_table(slot, (rows, cols))
        assert rb == rc > 0 and np.array_equal(tb, tc), slot
    s2 = c.sample_states(5, 0, 1 << 15)
    assert np.array_equal(b.sample_states(5, 0, 1 << 15), s2, equal_nan=True)
    assert np.array_equal(b.validate_states(s2), c.validate_states(s2))
    L2 = P.preprocess(e2, *geom, traversability=trav)
    gm2 = _gridmap(L2, rows, cols, res)
    assert np.array_equal(b.validate_states(s2[:8000]), O.OracleMap(gm2).states_valid(O.robot("yaml"), s2[:8000]))
    for m in (pp, pp2, pp3):
        m.close()
    for ctx in (a, b, c):
        ctx.close()


def _quantised(elev, mode):
    """inpaintMatrix (mode 0) / _elvMapProcess (mode 1) quantisation and scaling back, as
    test_hole_filling_quantisation_matches_the_reference_arithmetic restates them."""
    lo, hi = F32(np.nanmin(elev)), F32(np.nanmax(elev))
    with np.errstate(invalid="ignore"):
        if mode == 0:
            a, b = F32(255) / (hi - lo), -lo * F32(255) / (hi - lo)
            q = np.clip(np.rint(elev * a + b), 0, 255)
            return q.astype(F32) * ((hi - lo) / F32(255)) + lo
        q = np.clip(np.trunc((elev - lo) * F32(255) / (hi - lo)), 0, 255)
        return q.astype(F32) * (hi - lo) / F32(255) + lo


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("shape", [(97, 61), (61, 97)])
def test_inpaint_on_non_square_maps_with_border_holes(contexts, shape, mode):
    """artp_inpaint_layer on non-square odd maps whose holes touch the borders and all four corners: every cell that is
    not a hole is bit-equal to the quantisation arithmetic (mode 0 with its column-0 / row-0 copy), the holes are
    filled with finite values within the range of the valid cells."""
    rows, cols = shape
    elev, _ = P.sweep_map(rows, cols, 0.05, seed=2)
    elev = np.array(elev)
    holes = np.zeros(shape, bool)
    holes[:3, :4] = True                       # corners
    holes[-2:, -5:] = True
    holes[:4, -1] = True
    holes[-1, :2] = True
    holes[0, 20:30] = True                     # along the borders
    holes[rows // 2: rows // 2 + 6, 0] = True
    holes[-3:, cols // 2] = True
    holes[rows // 3: rows // 3 + 9, cols // 3: cols // 3 + 7] = True    # an interior blob wider than the fill radius
    elev[holes] = np.nan
    out, n = contexts().inpaint_layer(elev, mode)
    assert n == holes.sum() and np.isfinite(out).all()
    ref = _quantised(elev, mode)
    keep = ~holes
    if mode == 0:                              # mat_inpainted.col(0) = col(1); row(0) = row(1)
        ref[:, 0] = ref[:, 1]
        keep[:, 0] = keep[:, 1]
        ref[0, :] = ref[1, :]
        keep[0, :] = keep[1, :]
    assert np.array_equal(out[keep], ref[keep])
    assert out.min() >= np.nanmin(elev) - 1e-6 and out.max() <= np.nanmax(elev) + 1e-6
