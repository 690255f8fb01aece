"""The robot-dependent kernels across box sizes, offsets and tilts (-m gpu): every geometry of tests/robot_geometry.py
through validity (batch and few-state), the box checker, the vertex count, the three edge rules in every form, the
sampler, reachability maps with their halo, and the preprocessing.

The suite's other robots are the two presets and one scaled-up ANYmal: no torso offset in the plane, one aspect ratio per
box, one value of each sampler limit.  tests/test_robot_geometry_ref.py pins on the CPU that the table's inputs mix labels
and exits, reach the table tiers the presets do not, and that the torso offset decides labels term by term.  The oracle,
the edge answers and the restatements take the robot as an argument, so the requirement is that of
tests/test_gpu_parity.py, unchanged: every comparison EXACT but the sampler's (the bar of tests/test_sampler_sweep.py) and
the lastValid states' (1e-12, tests/test_far_origin.py).

One context per geometry; every test installs the fine map, then the coarse one on the same context, so every second
upload sizes the LDS downwards and the next one upwards again."""
from types import SimpleNamespace

import numpy as np
import pytest

import oracle_py as O
import preprocess_restated as P
import robot_geometry as RG
from test_far_origin import STATE_TOL, _assert_edges, _bad, _in_calls
from test_preprocess_sweep import LAYERS, _compare, _device, _float64_violations, _inputs, _pt
from test_reachability import cells_finite, check_every_label, check_halo_grown_recompute, halo_cells, mask_bits
from test_sampler_sweep import assert_states

pytestmark = pytest.mark.gpu

GEOS = list(RG.GEOMETRIES)
MAPS = list(RG.MAPS)                      # fine first
# the sampler reads reach_z and the two limits: the other geometries share its inputs with yaml.  level IS the exact-zero
# case (both limits 0.0 keep its valid share at 0.33 / 0.36: tests/test_robot_geometry_ref.py)
SAMPLER_GEOS = ["yaml", "flat", "tall", "steep", "level"]
HALO_GEOS = ["offset", "bigfeet", "tall"]
PRE_GEOS = ["tiny", "bigfeet", "wide"]
N_FEW = 512
RECT = (0, 0, 48, 48)                     # the map's corner: feet and torsos leave the map along two sides
N_YAW = 4


@pytest.fixture(scope="module")
def contexts():
    """One context per geometry, made on first use, closed at the end."""
    from art_planner_amd.context import Context
    made = {}

    def get(name):
        if name not in made:
            made[name] = Context(0, RG.params_of(name))
        return made[name]

    yield get
    for c in made.values():
        c.close()


# ---- states, boxes, vertex count -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GEOS)
def test_states(contexts, name):
    ctx = contexts(name)
    for mname in MAPS:
        se3, ref, ref_detail = RG.states(name, mname), RG.oracle_labels(name, mname), RG.oracle_details(name, mname)
        ctx.upload_map(RG.map_of(mname), sampler=False)
        valid, detail = ctx.validate_states(se3, want_detail=True)
        print(f"states {name}/{mname}: {len(se3)} states, {int((valid != ref).sum())} labels and "
              f"{int((detail[:, :5] != ref_detail[:, :5]).any(axis=1).sum())} details differ from the oracle")
        assert np.array_equal(valid, ref), f"{mname}: {_bad(valid, ref)}"
        assert np.array_equal(detail[:, :5], ref_detail[:, :5]), mname
        # without the details the list takes the batch pipeline (classify, stream passes, tail), not the wave-per-state kernel
        batch = ctx.validate_states(se3)
        assert np.array_equal(batch, ref), f"{mname} batch pipeline: {_bad(batch, ref)}"


@pytest.mark.parametrize("name", GEOS)
def test_few_state_path(contexts, name):
    ctx = contexts(name)
    for mname in MAPS:
        se3, ref = RG.states(name, mname)[:N_FEW], RG.oracle_labels(name, mname)[:N_FEW]
        assert 0 < ref.sum() < N_FEW
        ctx.upload_map(RG.map_of(mname), sampler=False)
        got, _ = _in_calls(lambda lo, hi: ctx.validate_states(se3[lo:hi]), N_FEW, (16,))
        got = np.concatenate(got)
        assert np.array_equal(got, ref), f"{mname}: {_bad(got, ref)}"


@pytest.mark.parametrize("name", GEOS)
def test_boxes(contexts, name):
    """The states' own torso and foot boxes against either layer: hit and exit code."""
    ctx = contexts(name)
    rob = RG.robot_of(name)
    for mname in MAPS:
        gm = RG.map_of(mname)
        ctx.upload_map(gm, sampler=False)
        torso, feet = RG.state_boxes(name, mname)
        for slot, layer in ((0, "elevation"), (1, "elevation_masked")):
            of = O.OracleField(gm[layer], gm.len_x, gm.len_y, gm.pos_x, gm.pos_y)
            for kind, side, poses in (("torso", rob.torso, torso), ("foot", rob.foot, feet)):
                ho, eo, _ = of.check_boxes(side, poses, want_detail=True)
                hg, eg = ctx.check_boxes(slot, side, poses, want_exit_codes=True)
                assert np.array_equal(hg, ho), f"{mname} slot {slot} {kind}: {_bad(hg, ho)}"
                assert np.array_equal(eg, eo), f"{mname} slot {slot} {kind}: exit codes, {_bad(eg, eo)}"


@pytest.mark.parametrize("name", GEOS)
def test_vertex_count(contexts, name):
    import torch
    ctx = contexts(name)
    rob = RG.robot_of(name)
    for mname in MAPS:
        gm = RG.map_of(mname)
        ctx.upload_map(gm, sampler=False)
        se3 = RG.states(name, mname)
        _, want = O.OracleMap(gm).states_valid(rob, se3, want_vertices=True)
        got = ctx.algorithmic_vertices_dev(torch.from_numpy(se3).cuda())
        print(f"vertices {name}/{mname}: {got} (oracle {want})")
        assert want > 0 and got == want, mname


# ---- edges -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GEOS)
def test_edges(contexts, name):
    ctx = contexts(name)
    tol = STATE_TOL
    try:
        for mname in MAPS:
            a, b = RG.edge_pairs(name, mname)
            ref = RG.oracle_edges(name, mname)
            ctx.upload_map(RG.map_of(mname), sampler=False)
            every = np.arange(len(a))
            lv = ctx.check_motions_last_valid(a, b)
            with np.errstate(invalid="ignore"):
                worst = float(np.nanmax(np.abs(lv[2] - ref["lv_st"])))
            print(f"edges {name}/{mname}: {len(a)} pairs, lastValid states within {worst:.2e} of the oracle's")
            _assert_edges(ref, every, f"{mname} two passes", tol, cm=ctx.check_motions(a, b), lv=lv,
                          interp=ctx.check_edges_interp(a, b))
            ctx.set_edge_passes(False, 0)
            _assert_edges(ref, every, f"{mname} single pass", tol, cm=ctx.check_motions(a, b),
                          lv=ctx.check_motions_last_valid(a, b), interp=ctx.check_edges_interp(a, b))
            ctx.set_edge_passes(True, 0)
            # the few-edges kernel: calls of 64, 1, 2 and 33 edges
            m = 400
            ctx.set_few_edges(True)
            cm, _ = _in_calls(lambda lo, hi: ctx.check_motions(a[lo:hi], b[lo:hi]), m, (64, 1, 2, 33))
            _assert_edges(ref, np.arange(m), f"{mname} few edges", tol, cm=np.concatenate(cm))
    finally:
        ctx.set_edge_passes(True, 0)
        ctx.set_few_edges(True)


# ---- sampler ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SAMPLER_GEOS)
def test_sampler(contexts, name):
    ctx = contexts(name)
    rob = RG.robot_of(name)
    for mname in MAPS:
        gm = RG.map_of(mname)
        ctx.upload_map(gm)
        so, rc = O.OracleSampler(gm).sample(rob, RG.SEED, RG.FIRST, RG.N_STATES)
        assert np.array_equal(so, RG.states(name, mname))
        sg = ctx.sample_states(RG.SEED, RG.FIRST, RG.N_STATES)
        print(f"sampler {name}/{mname}: max |diff| per number {np.abs(sg - so).max(axis=0)}")
        assert_states(sg, so, rc, gm, f"{name}/{mname} sample_states")
    if name != "yaml":      # the limits and reach_z are in play: the states are not the preset's
        assert not np.array_equal(RG.states(name, "fine"), RG.states("yaml", "fine"))


# ---- reachability ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GEOS)
def test_reachability(contexts, name):
    ctx = contexts(name)
    rob = RG.robot_of(name)
    for mname in MAPS:
        gm = RG.map_of(mname)
        ctx.upload_map(gm)
        assert cells_finite(gm, RECT).all()
        mask = check_every_label(ctx, gm, N_YAW, rob, RECT)     # poses, every bit against the oracle and validate_states
        bits = int(mask_bits(mask, N_YAW).sum())
        print(f"reachability {name}/{mname}: {mask.size * N_YAW} bits, {bits} set")
        assert 0 < bits < mask.size * N_YAW
        assert ctx.reachability_halo() == halo_cells(rob, gm.res)


@pytest.mark.parametrize("name", HALO_GEOS)
def test_halo_grown_recompute_equals_a_full_recompute(contexts, name):
    ctx = contexts(name)
    gm = RG.map_of("fine")
    ctx.upload_map(gm)
    full0 = ctx.reachability_map(8)
    # the 10 x 12 block with the most valid poses on and around it (two cells to every side): an obstacle there changes
    # masks inside and outside the block
    near = np.zeros((gm.rows + 1, gm.cols + 1), np.int64)
    near[1:, 1:] = mask_bits(full0, 8).sum(axis=2).cumsum(axis=0).cumsum(axis=1)
    score = near[14:, 16:] - near[:-14, 16:] - near[14:, :-16] + near[:-14, :-16]     # 14 x 16 windows by their corner
    r0, c0 = np.unravel_index(np.argmax(score), score.shape)
    block = (int(r0) + 2, int(c0) + 2, 10, 12)
    full0, full1, halo = check_halo_grown_recompute(ctx, gm, 8, block, full0=full0)
    assert halo == halo_cells(RG.robot_of(name), gm.res)
    written = np.zeros(full0.shape, bool)
    written[block[0]:block[0] + block[2], block[1]:block[1] + block[3]] = True
    changed = full1 != full0
    print(f"halo {name}: {halo} cells, {int(changed.sum())} masks changed, {int((changed & ~written).sum())} outside the block")
    assert (changed & ~written).any()   # the halo is not 0: cells next to the block change too
    assert not changed.all()            # and the grown rectangle is not the whole map's worth of change


# ---- preprocessing ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", [0.1, 0.05])
@pytest.mark.parametrize("name", PRE_GEOS)
def test_preprocessing(contexts, name, res):
    """One 61 x 53 map through preprocess_map under the geometry: bit-equal to the restatement given the same robot numbers,
    and inside the float64 bounds.  tiny: reach and wall sizes of 0 cells at 0.1 m, 1 at 0.05 m; bigfeet: min_wall < 0, the
    3 x 3 rectangle cv::erode takes for an empty kernel."""
    r = RG.robot_of(name)
    rob = SimpleNamespace(torso_length=r.torso_length, torso_width=r.torso_width, reach_x=r.reach_x, reach_y=r.reach_y,
                          unknown_space_untraversable=r.unknown_space_untraversable)
    reach, wall = P.reach_sizes(rob, res)
    if name == "tiny":
        assert (reach, wall) == ((0, 0) if res == 0.1 else (1, 1))
    if name == "bigfeet":
        assert wall < 0 and P.disk(wall).shape == (3, 3) and P.disk(wall).all()
    pt = _pt((61, 53), res)
    prm = P.params("yaml")
    rows, cols = pt["shape"]
    pos = (0.7, -0.3)
    geom = (rows * res, cols * res) + pos
    elev, trav, obs, verts = _inputs(pt, pos=pos)
    # an untraversable strip wider than the widest reach disk (bigfeet at 0.05 m: 19 cells): the closing by the reach
    # would otherwise fill every hole of this map, and the wall erosion after it would have nothing to move
    trav = trav.copy()
    trav[:, :24] = 0.0
    L = P.preprocess(elev, *geom, traversability=trav, observed=obs, vertices=verts, prm=prm, rob=rob)
    for what in ("_hole", "_wall", "_keep"):                   # the comparison cannot pass on an all-pass map
        assert L[what].any() and not L[what].all(), what
    f = L["traversability_sample_filter"]
    assert (f > 0.5).any() and (f <= 0.5).any()
    closed = P.erode(P.dilate(L["traversability_thresholded"], reach), reach)
    if name == "bigfeet" or (name, res) == ("tiny", 0.1):      # size <= 0: the 3 x 3 rectangle moves the strip's edge
        assert np.array_equal(f, P.erode(closed, 0)) and (f != closed).any()
    pp = _device(contexts(name), pt, elev, trav, obs, verts, pos)
    got, bad = _compare(pp, L, f"{name}@{res}")
    bad += _float64_violations(got, L, elev, geom, prm, rob)
    pp.close()
    assert not bad, bad
    print(f"preprocessing {name}@{res}: reach {reach}, wall {wall}, {sum(got[k].size for k in LAYERS)} cells")
