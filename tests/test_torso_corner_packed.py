"""The torso stream pass (PASS 0 of resolve_boxes_kernel) against the C oracle (-m gpu).

A wavefront takes a chunk of torso boxes, reads the chunk's headers together (lane k: the state of box k and that state's
label; a ballot gives the boxes still worth checking) and then gives each live box its vertex stream and, when the stream
finds nothing, the list-free corner stage; boxes it cannot finish leave for the staged pass from their own slot of the
chunk.  The label of a torso box is "(f) a colliding vertex lies inside the box OR the plane stage yields a contact":
existence tests.  Only states whose four feet pass depend on the torso pass for their label, so every input below is chosen
on the CPU with the oracle such that among THOSE states the torso is decided by a vertex, by a plane contact and by
nothing (each at least 100 times, asserted here); batch sizes cover empty sub-queues, sub-queues shorter than a chunk and
a last chunk that is not full; terraces give corner candidates with coplanar partners (the box goes to the staged pass
from its own chunk slot); a band of unknown cells gives records that are forwarded without streaming; edges run the same
kernel on interpolated states.  Labels and verdicts must be BIT-EQUAL to the oracle's.  (The file is named after the form
of the corner stage that was measured with these tests and not kept: four open boxes a round on 16-lane groups,
profiles/torso_corner_packed.txt.)"""
import copy

import numpy as np
import pytest

import common
import oracle_py as O
from synthetic import make_map

pytestmark = pytest.mark.gpu

N = 1 << 15
SEED_MAP = 3
MIN_EACH = 100
EXIT_VERTEX, EXIT_PLANE, EXIT_NONE = 5, 6, 8
# make_map(100, 0.04, seed=3), the sampler's first 2^15 states (seed 42): torso exits among the states over the map whose
# four feet pass
#   yaml      771 vertex, 129 plane contact, 298 nothing
#   defaults  625 vertex, 366 plane contact, 604 nothing


@pytest.fixture(scope="module")
def gm1():
    return make_map(100, 0.04, seed=SEED_MAP)


def _terraced(gm, step=0.05):
    """Both height layers quantised to terraces: large families of exactly coplanar triangles, so that corner candidates
    have partners and the partner table cannot rule them out."""
    out = copy.deepcopy(gm)
    for name in ("elevation", "elevation_masked"):
        a = out[name].astype(np.float64)
        q = np.where(np.isfinite(a), np.round(a / step) * step, a)
        out.layers[name] = np.asfortranarray(q.astype(np.float32))
    return out


@pytest.fixture(scope="module")
def gm_terraced():
    return _terraced(make_map(200, 0.04, seed=SEED_MAP))


def _ctx(kind, gm, sampler=True):
    from art_planner_amd.context import Context
    c = Context(0, kind)
    c.upload_map(gm, sampler=sampler)
    return c


def _torso_exits_behind_passing_feet(om, rob, se3):
    """The oracle's exit code of the torso box of every state whose five boxes lie over the map and whose four foot boxes
    touch (the states whose label the torso decides)."""
    poses, inside = om.state_poses(rob, se3)
    feet_hit = om.feet.check_boxes(rob.foot, poses[:, 1:5].reshape(-1, 16)).reshape(-1, 4)
    _, ec, _ = om.body.check_boxes(rob.torso, poses[:, 0].reshape(-1, 16), want_detail=True)
    return ec[feet_hit.all(axis=1) & (inside != 0).all(axis=1)]


def _count_exits(ec):
    return {name: int((ec == code).sum()) for name, code in (("vertex", EXIT_VERTEX), ("plane", EXIT_PLANE), ("none", EXIT_NONE))}


def _sampled_and_validated(ctx, n):
    """One fused sample + validate batch: (states, labels) on the host."""
    import torch
    se3 = torch.empty((n, 7), dtype=torch.float64, device="cuda:0")
    valid = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    ctx.use_torch_stream()
    ctx.sample_and_validate_dev(42, 0, n, se3, valid)
    torch.cuda.synchronize()
    return se3.cpu().numpy(), valid.cpu().numpy()


@pytest.mark.parametrize("rname", ["yaml", "defaults"])
def test_all_three_torso_outcomes_behind_passing_feet(gm1, rname):
    """Perlin terrain + obstacles, 2^15 states of the sampler, both robots: the labels of the fused step and of
    validate_states equal the oracle's, and among the states whose feet pass the oracle decides at least MIN_EACH
    torso boxes by each of the three outcomes of the kernel's two stages."""
    rob = O.robot(rname)
    om = O.OracleMap(gm1)
    ctx = _ctx(rname, gm1)
    se3, fused = _sampled_and_validated(ctx, N)
    counts = _count_exits(_torso_exits_behind_passing_feet(om, rob, se3))
    print("torso boxes behind passing feet, by the oracle's exit:", counts)
    assert min(counts.values()) >= MIN_EACH, counts   # the map must keep exercising every branch
    ref = om.states_valid(rob, se3)
    assert np.array_equal(fused, ref), f"sample_and_validate_dev: {(fused != ref).sum()} mismatches"
    vg = ctx.validate_states(se3)
    assert np.array_equal(vg, ref), f"validate_states: {(vg != ref).sum()} mismatches"
    assert 0 < ref.sum() < N
    ctx.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000, 16 * 64 * 8 + 1])
def test_chunk_and_round_edges(gm1, n):
    """Batch sizes around the wavefront, the chunk and the 16 sub-queues: empty sub-queues, sub-queues shorter than a
    chunk, a last chunk that is not full (fewer headers than lanes that read them), chunks with one, two and three
    boxes still open after their streams."""
    rob = O.robot("yaml")
    om = O.OracleMap(gm1)
    ctx = _ctx("yaml", gm1)
    se3, fused = _sampled_and_validated(ctx, n)
    ref = om.states_valid(rob, se3)
    assert np.array_equal(fused, ref), f"n = {n}: {(fused != ref).sum()} mismatches"
    vg = ctx.validate_states(se3)
    assert np.array_equal(vg, ref), f"n = {n}, validate_states: {(vg != ref).sum()} mismatches"
    ctx.close()


def test_partner_planes_reach_the_staged_pass(gm_terraced):
    """Terraces: corner candidates with coplanar partners (corner stage result 2).  Such a torso box must reach the
    staged pass (queue 6) from its own slot of the chunk: labels equal the oracle's and the staged pass ran.  On the
    CPU: the oracle decides torso boxes of feet-passing states by a plane contact here (236 of them, with 2 706 by a
    vertex and 1 068 by nothing, counted when this test was written; at least MIN_EACH asserted)."""
    rob = O.robot("yaml")
    om = O.OracleMap(gm_terraced)
    ctx = _ctx("yaml", gm_terraced, sampler=False)
    rng = np.random.default_rng(21)
    se3 = common.random_states(gm_terraced, N, rng, z_off=(0.0, 0.03), tilt=0.15, spread=0.5)
    counts = _count_exits(_torso_exits_behind_passing_feet(om, rob, se3))
    print("torso boxes behind passing feet, by the oracle's exit:", counts)
    assert counts["plane"] >= MIN_EACH, counts
    vg = ctx.validate_states(se3)
    cnt = ctx.pipeline_counters()
    vo = om.states_valid(rob, se3)
    assert np.array_equal(vg, vo), f"{(vg != vo).sum()} mismatches"
    print("pipeline counters:", cnt)
    assert cnt["torso_staged_pass"] > 0, cnt          # the result-2 path was taken
    assert 0.02 < vg.mean() < 0.98
    ctx.close()


def test_unknown_cells_are_forwarded_without_streaming(gm_terraced):
    """The same map with a band of unknown (NaN) rows: torso records that are not known to be all finite, which the
    streaming pass forwards to the staged pass without streaming.  Labels equal the oracle's."""
    gm = copy.deepcopy(gm_terraced)
    for name in ("elevation", "elevation_masked"):
        a = np.array(gm[name], dtype=np.float32, order="F")
        a[80:110, :] = np.nan
        gm.layers[name] = np.asfortranarray(a)
    rob = O.robot("yaml")
    ctx = _ctx("yaml", gm, sampler=False)
    rng = np.random.default_rng(5)
    se3 = common.random_states(gm, N, rng, z_off=(0.02, 0.12), tilt=0.15, spread=0.5)
    vg = ctx.validate_states(se3)
    cnt = ctx.pipeline_counters()
    vo = O.OracleMap(gm).states_valid(rob, se3)
    assert np.array_equal(vg, vo), f"{(vg != vo).sum()} mismatches"
    print("pipeline counters:", cnt)
    assert cnt["torso_staged_pass"] > 0, cnt
    assert 0.02 < vg.mean() < 0.9
    ctx.close()


def _pair_edges(acc, want, max_gap=3):
    """The benchmark's pairing rule: accepted state i with accepted states i + 1 .. i + max_gap when their lateral
    distance is below 2 m."""
    ii, jj = [], []
    for d in range(1, max_gap + 1):
        a, b = acc[:-d], acc[d:]
        near = np.flatnonzero(np.hypot(a[:, 0] - b[:, 0], a[:, 1] - b[:, 1]) < 2.0)
        ii.append(near)
        jj.append(near + d)
        if sum(len(x) for x in ii) >= want:
            break
    return np.concatenate(ii)[:want], np.concatenate(jj)[:want]


def test_edges_between_accepted_states(gm1):
    """2^12 edges between accepted states less than 2 m apart through check_motions_dev (edge batches expand into states
    and run the same kernel): verdicts equal the oracle's checkMotion, both verdicts occur."""
    import torch
    rob = O.robot("yaml")
    om = O.OracleMap(gm1)
    ctx = _ctx("yaml", gm1)
    se3, labels = _sampled_and_validated(ctx, N)
    acc = se3[labels != 0]
    n = 1 << 12
    ii, jj = _pair_edges(acc, n, max_gap=16)   # ~400 accepted states on this 4 m map: gaps up to 16 give 2^12 pairs
    assert len(ii) == n, len(ii)
    s1, s2 = acc[ii], acc[jj]
    a, b = torch.from_numpy(np.ascontiguousarray(s1)).cuda(), torch.from_numpy(np.ascontiguousarray(s2)).cuda()
    v = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    ctx.check_motions_dev(a, b, v)
    torch.cuda.synchronize()
    eg = v.cpu().numpy()
    eo, _ = om.check_motions(rob, s1, s2)
    assert np.array_equal(eg, eo), f"{(eg != eo).sum()} verdicts differ"
    print("valid edges:", int(eo.sum()), "of", n)
    assert 0 < eo.sum() < n
    ctx.close()
