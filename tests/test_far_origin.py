"""Validity, edges, reachability, preprocessing, fields and the roadmap's neighbour search on maps far from the origin
(-m gpu): hundreds of metres, kilometres, tens of kilometres and a UTM-sized position (tests/far_origin.py).

The reference works in world-frame float at these points, the oracle does the same arithmetic, and the rounding of a
coordinate decides labels there (tests/test_far_origin_ref.py pins that on the CPU).  So the requirement is the one of
tests/test_gpu_parity.py, unchanged: the same labels, exit codes, counts and layer bits -- every comparison EXACT and made
at the origin in question, against the oracle or a restatement fed that origin."""
import numpy as np
import pytest

import common
import far_origin as FO
import oracle_py as O
from edge_probe import same
from synthetic import map_from_device, raw_map
from test_graph_sweep import _check_roadmap_knn
from test_preprocess_sweep import LAYERS, _check_change_from, _check_point, _expected
from test_reachability import check_every_label, mask_bits

pytestmark = pytest.mark.gpu

ORIGINS = list(FO.ORIGINS)
MAPS = list(FO.MAPS)
PRE_POINTS = ("odd97x61", "res0.1", "defaults-robot")


@pytest.fixture(scope="module")
def contexts():
    """One context per robot (and unknown-space setting), made on first use."""
    from art_planner_amd.context import Context, make_params
    made = {}

    def get(robot="yaml", untrav=1):
        if (robot, untrav) not in made:
            made[(robot, untrav)] = Context(0, make_params(robot, unknown_space_untraversable=untrav))
        return made[(robot, untrav)]

    yield get
    for c in made.values():
        c.close()


def _in_calls(fn, n, sizes):
    """fn(lo, hi) over [0, n) in calls whose sizes cycle through `sizes`; (list of results, number of calls)."""
    out, i, k = [], 0, 0
    while i < n:
        j = min(i + sizes[k % len(sizes)], n)
        out.append(fn(i, j))
        i, k = j, k + 1
    return out, k


def _bad(got, ref):
    return f"{int((np.asarray(got) != np.asarray(ref)).sum())} of {len(ref)} differ"


# ---- 1. states and boxes -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("origin", ORIGINS)
@pytest.mark.parametrize("name", MAPS)
def test_states(contexts, name, origin):
    import torch
    pos = FO.ORIGINS[origin]
    gm = FO.map_at(name, pos)
    se3 = FO.states(name, pos)
    ref, ref_detail = FO.oracle_labels(name, pos), FO.oracle_details(name, pos)
    ctx = contexts()
    ctx.upload_map(gm)
    valid, detail = ctx.validate_states(se3, want_detail=True)
    print(f"states {name}/{origin}: {len(se3)} states, {int((valid != ref).sum())} labels and "
          f"{int((detail[:, :5] != ref_detail[:, :5]).any(axis=1).sum())} details differ from the oracle")
    assert np.array_equal(valid, ref), _bad(valid, ref)
    assert np.array_equal(detail[:, :5], ref_detail[:, :5])
    batch = ctx.validate_states(se3)
    assert np.array_equal(batch, ref), _bad(batch, ref)
    t = torch.from_numpy(se3).cuda()
    v = torch.full((len(se3),), 7, dtype=torch.uint8, device="cuda")
    ctx.validate_states_dev(t, v)
    ctx.synchronize()
    assert np.array_equal(v.cpu().numpy(), ref)

    # the first 32 states, and up to 32 whose label is not the one of origin zero, through the three small-call paths
    knife = np.flatnonzero(ref != FO.oracle_labels(name, FO.ZERO))[:32]
    sel = np.concatenate([np.arange(32), knife])
    s, r = se3[sel], ref[sel]
    got, _ = _in_calls(lambda lo, hi: ctx.validate_states(s[lo:hi]), len(s), (1, 2, 16))
    assert np.array_equal(np.concatenate(got), r), "latency path"
    ctx.set_persistent_latency(True)
    try:
        before = ctx.persistent_latency_stats()["requests"]
        got, calls = _in_calls(lambda lo, hi: ctx.validate_states(s[lo:hi]), len(s), (1, 2))
        used = ctx.persistent_latency_stats()["requests"] - before
    finally:
        ctx.set_persistent_latency(False)
    assert np.array_equal(np.concatenate(got), r), "persistent service"
    assert used == calls, f"the service answered {used} of {calls} calls"
    for n in (16, len(s)):
        v = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
        ctx.validate_states_dev(torch.from_numpy(np.ascontiguousarray(s[:n])).cuda(), v)
        ctx.synchronize()
        assert np.array_equal(v.cpu().numpy(), r[:n]), f"validate_states_dev, {n} states"


@pytest.mark.parametrize("origin", ORIGINS)
@pytest.mark.parametrize("name", MAPS)
def test_boxes(contexts, name, origin):
    import torch
    pos = FO.ORIGINS[origin]
    gm = FO.map_at(name, pos)
    rob = O.robot(FO.ROBOT)
    ctx = contexts()
    ctx.upload_map(gm, sampler=False)
    compared = 0
    for slot, layer in ((0, "elevation"), (1, "elevation_masked")):
        of = O.OracleField(gm[layer], gm.len_x, gm.len_y, gm.pos_x, gm.pos_y)
        for kind, side in (("torso", rob.torso), ("foot", rob.foot)):
            P = FO.box_poses(gm, slot, kind, seed=31)
            ho, eo, _ = of.check_boxes(side, P, want_detail=True)
            assert 0.05 < ho.mean() < 0.95 and len(np.unique(eo)) >= 5
            hg, eg = ctx.check_boxes(slot, side, P, want_exit_codes=True)
            assert np.array_equal(hg, ho), f"slot {slot} {kind}: {_bad(hg, ho)}"
            assert np.array_equal(eg, eo), f"slot {slot} {kind}: exit codes, {_bad(eg, eo)}"
            pt = torch.from_numpy(P).cuda()
            ht = torch.full((len(P),), 7, dtype=torch.uint8, device="cuda")
            et = torch.full((len(P),), 77, dtype=torch.uint8, device="cuda")
            ctx.check_boxes_dev(slot, side, pt, ht, et)
            ctx.synchronize()
            assert np.array_equal(ht.cpu().numpy(), ho) and np.array_equal(et.cpu().numpy(), eo), f"slot {slot} {kind}: _dev"
            compared += len(P)
    print(f"boxes {name}/{origin}: {compared} boxes")


# ---- 2. edges ----------------------------------------------------------------------------------------------------------------
STATE_TOL = 1e-12     # tests/test_edge_sweep.py: lastValid states to 1e-12 of the oracle's; the positions come out bit-equal here


def _assert_edges(ref, idx, what, tol, cm=None, lv=None, interp=None):
    if cm is not None:
        assert np.array_equal(cm, ref["ok"][idx]), f"{what} check_motions: {_bad(cm, ref['ok'][idx])}"
    if lv is not None:
        ok, t, st = lv
        assert np.array_equal(ok, ref["lv_ok"][idx]), f"{what} lastValid verdicts: {_bad(ok, ref['lv_ok'][idx])}"
        assert same(t, ref["lv_t"][idx]), f"{what}: lastValid.second"
        assert same(st, ref["lv_st"][idx], tol), f"{what}: lastValid states beyond {tol:.1e}"
    if interp is not None:
        ei, ni = interp
        assert np.array_equal(ni, ref["nint"][idx]), f"{what}: interpolation counts"
        assert np.array_equal(ei, ref["ei"][idx]), f"{what} 0.5 m rule: {_bad(ei, ref['ei'][idx])}"


def _small_calls(ctx, a, b, sizes):
    """All three entry points on [0, len(a)) in calls of the given sizes: (cm, (ok, t, st), (ei, ni), number of calls)."""
    cm, calls = _in_calls(lambda lo, hi: ctx.check_motions(a[lo:hi], b[lo:hi]), len(a), sizes)
    lv, _ = _in_calls(lambda lo, hi: ctx.check_motions_last_valid(a[lo:hi], b[lo:hi]), len(a), sizes)
    it, _ = _in_calls(lambda lo, hi: ctx.check_edges_interp(a[lo:hi], b[lo:hi]), len(a), sizes)
    return (np.concatenate(cm), tuple(np.concatenate([x[k] for x in lv]) for k in range(3)),
            tuple(np.concatenate([x[k] for x in it]) for k in range(2)), calls)


@pytest.mark.parametrize("origin", ORIGINS)
@pytest.mark.parametrize("name", MAPS)
def test_edges(contexts, name, origin):
    pos = FO.ORIGINS[origin]
    a, b = FO.edge_pairs(name, pos)
    ref = FO.oracle_edges(name, pos)
    ctx = contexts()
    ctx.upload_map(FO.map_at(name, pos), sampler=False)
    every = np.arange(len(a))
    tol = STATE_TOL
    try:
        lv = ctx.check_motions_last_valid(a, b)
        with np.errstate(invalid="ignore"):
            worst = float(np.nanmax(np.abs(lv[2] - ref["lv_st"])))
        print(f"edges {name}/{origin}: {len(a)} pairs, lastValid states within {worst:.2e} of the oracle's (bound {tol:.2e})")
        _assert_edges(ref, every, "two passes", tol, cm=ctx.check_motions(a, b), lv=lv, interp=ctx.check_edges_interp(a, b))
        ctx.set_edge_passes(False, 0)
        _assert_edges(ref, every, "single pass", tol, cm=ctx.check_motions(a, b), lv=ctx.check_motions_last_valid(a, b),
                      interp=ctx.check_edges_interp(a, b))
        ctx.set_edge_passes(True, 0)
        # calls of one and two edges: the few-edges kernel, then the resident pool
        m = 60
        few = np.arange(m)
        cm, lv, it, _ = _small_calls(ctx, a[:m], b[:m], (1, 2))
        _assert_edges(ref, few, "few edges", tol, cm=cm, lv=lv, interp=it)
        ctx.set_persistent_latency(True)
        before = ctx.persistent_latency_stats()["requests"]
        cm, lv, it, calls = _small_calls(ctx, a[:m], b[:m], (1, 2))
        used = ctx.persistent_latency_stats()["requests"] - before
        ctx.set_persistent_latency(False)
        _assert_edges(ref, few, "resident pool", tol, cm=cm, lv=lv, interp=it)
        assert used == 3 * calls, f"the pool answered {used} of {3 * calls} calls"
    finally:
        ctx.set_edge_passes(True, 0)
        ctx.set_few_edges(True)
        ctx.set_persistent_latency(False)


# ---- 3. reachability on a map preprocessed on the device at that origin ------------------------------------------------------
@pytest.mark.parametrize("origin", ORIGINS)
def test_reachability(contexts, origin):
    n, res, seed = FO.MAPS["p120"]
    ctx = contexts()
    gm = map_from_device(ctx, FO.moved(raw_map(n, res, seed=seed), FO.ORIGINS[origin]), FO.ROBOT)
    for n_yaw in (8, 5):
        mask = check_every_label(ctx, gm, n_yaw)           # poses (assert_poses), every bit against oracle and validate_states
        bits = int(mask_bits(mask, n_yaw).sum())
        assert 0 < bits < mask.size * n_yaw
        print(f"reachability p120/{origin}: n_yaw {n_yaw}, {mask.size * n_yaw} bits, {bits} set")
    gm.preprocessed.close()


def test_install_follows_a_map_that_moves():
    """A robot-centred map keeps its size and moves: install() of the same terrain at one position after another, on ONE
    context.  Both height fields must stand at the new position (the labels are the oracle's there) -- the body slot's
    install moves the context's shared geometry, and the feet slot once took that for its own frame and stayed behind."""
    from art_planner_amd.context import Context
    n, res, seed = FO.MAPS["p120"]
    rob = O.robot(FO.ROBOT)
    ctx = Context(0, FO.ROBOT)
    try:
        for oname, pos in [("zero", FO.ZERO), ("near", (0.3, 0.7))] + list(FO.ORIGINS.items()):
            gm = map_from_device(ctx, FO.moved(raw_map(n, res, seed=seed), pos), FO.ROBOT)
            se3 = O.OracleSampler(gm).sample(rob, 11, 5000, 8000)[0]
            ref = common.oracle_states_valid_threaded(gm, rob, se3)
            assert min(int(ref.sum()), int((ref == 0).sum())) >= 100      # both labels occur (sampler_probe.CLASS_MIN)
            got = ctx.validate_states(se3)
            assert np.array_equal(got, ref), f"{oname}: {_bad(got, ref)}"
            gm.preprocessed.close()
    finally:
        ctx.close()


# ---- 4. preprocessing --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("origin", ORIGINS)
@pytest.mark.parametrize("point", PRE_POINTS)
def test_preprocessing(contexts, point, origin):
    pos = FO.ORIGINS[origin]
    exp = _expected(point, pos)
    L, verts = exp[-1], exp[4][3]
    assert 0 < L["_counts"].sum() < len(verts)             # some vertices in, some out, at this origin too
    cells = _check_point(contexts, point, pos, float64=origin != "utm", expected=exp)
    print(f"preprocessing {point}/{origin}: {cells} cells of {len(LAYERS)} layers")


@pytest.mark.parametrize("origin", ORIGINS)
def test_change_from(contexts, origin):
    """The shift between two maps is lround((pos_new - pos_old) / res) of two large numbers."""
    _check_change_from(contexts, (97, 61), FO.ORIGINS[origin], shifts=((3, -2), (None, -1)))


# ---- 5. position-free kernels stay position-free -----------------------------------------------------------------------------
RECT = (9, 11, 61, 53)
N_YAW = 7


@pytest.mark.parametrize("objective", [0, 1])
def test_fields_do_not_depend_on_the_position(contexts, objective):
    """No map position enters a weight of field.h or clearance.h (the planar step is res * (-dr)): one mask on one
    installed height layer gives the same bits at origin zero and at the UTM origin."""
    ctx = contexts()
    bits = np.random.default_rng(71).random(RECT[2:] + (N_YAW,)) < 0.9
    mask = (bits.astype(np.uint32) << np.arange(N_YAW, dtype=np.uint32)).sum(axis=2).astype(np.uint32)
    nodes = np.argwhere(bits)
    src = tuple(int(v) for v in nodes[len(nodes) // 3])
    got = {}
    for oname, pos in (("zero", FO.ZERO), ("utm", FO.ORIGINS["utm"])):
        ctx.upload_map(FO.map_at("p120", pos))
        with ctx.cost_field(mask, N_YAW, [src], rect=RECT, objective=objective) as f:
            plain = f.dist()
        with ctx.clearance_cost_field(mask, N_YAW, [src], rect=RECT, objective=objective, radius_cells=5, margin=0.15,
                                      gain=3.0) as f:
            clear = f.dist()
        got[oname] = (plain, clear)
    for k, what in enumerate(("cost_field", "clearance_cost_field")):
        d0, d1 = got["zero"][k], got["utm"][k]
        fin = np.isfinite(d0)
        assert fin.sum() > 1000 and len(np.unique(d0[fin])) > 100, what
        assert np.array_equal(d0.view(np.uint64), d1.view(np.uint64)), f"{what}: {int((d0 != d1).sum())} values differ"
    assert not np.array_equal(got["zero"][0], got["zero"][1])       # the clearance term is in play
    print(f"fields objective {objective}: {got['zero'][0].size} values each, bit-equal between origin zero and utm")


# ---- 6. the roadmap's neighbour search ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("origin", ["far", "utm"])
def test_roadmap_knn(contexts, origin):
    """The grid hash subtracts pos - len / 2 from every vertex: kNN lists and distances against the brute force."""
    from art_planner_amd.roadmap import Roadmap
    pos = FO.ORIGINS[origin]
    gm = FO.map_at("p160", pos)
    ctx = contexts()
    ctx.upload_map(gm)
    acc = FO.states("p160", pos)[FO.oracle_labels("p160", pos) != 0]
    corners = []
    for sx, sy in ((-1, -1), (1, 1)):
        cx, cy = gm.pos_x + sx * 0.5 * gm.len_x, gm.pos_y + sy * 0.5 * gm.len_y
        corners.append(acc[np.argmin(np.hypot(acc[:, 0] - cx, acc[:, 1] - cy))])
    rm = Roadmap(ctx, corners[0], corners[1], n_milestones=3000, seed=7)
    try:
        nv, k, d = _check_roadmap_knn(rm, 0)
    finally:
        rm.close()
    assert nv == 3002
    V = d["verts"]
    assert np.array_equal(V[0], corners[0]) and np.array_equal(V[1], corners[1])
    half = 0.5 * gm.len_x + 1.0
    assert (np.abs(V[:, 0] - gm.pos_x) < half).all() and (np.abs(V[:, 1] - gm.pos_y) < half).all()
    print(f"roadmap p160/{origin}: {nv} vertices, k = {k}")
