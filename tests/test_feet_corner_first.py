"""feet_stream_kernel runs a foot box's corner stage BEFORE its vertex stream (-m gpu), labels against the C oracle.

The label of a foot box that exits (b)-(e) do not decide is "(f) a colliding vertex lies inside the box OR the plane
stage yields a contact": two independent existence tests, so the kernel may run them in either order.  It runs the
list-free corner stage first and streams the window only for the boxes the corners leave open, after compacting them
within the wavefront's chunk.  Every input below is chosen on the CPU with the oracle so that each branch of that kernel
is provably taken: boxes the oracle decides by a vertex, by a plane contact and by nothing (each at least 100 times,
asserted here), corner candidates with coplanar partners (terraces: the box is streamed and then queued for the list
pass), windows with unknown cells (records without a table verdict, which the kernel leaves to the lane scan), the
expansion of edges (the same kernel on interpolated states) and the defaults robot (other window shapes).  Labels and
verdicts must be BIT-EQUAL to the oracle's."""
import copy

import numpy as np
import pytest

import common
import oracle_py as O
from synthetic import make_map

pytestmark = pytest.mark.gpu

N = 1 << 15
SEED_MAP = 3            # make_map(100, 0.04, seed=3): of the 4 * 2^15 foot boxes of the sampler's states the oracle decides
MIN_EACH = 100          # 21 175 by a vertex, 12 453 by a plane contact, 14 389 by nothing (yaml robot); asserted below
EXIT_VERTEX, EXIT_PLANE, EXIT_NONE = 5, 6, 8


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
    return _terraced(make_map(200, 0.04, seed=SEED_MAP))   # 8 m wide: room for states that are valid


def _ctx(kind, gm, sampler=True):
    from art_planner_amd.context import Context
    c = Context(0, kind)
    c.upload_map(gm, sampler=sampler)
    return c


def _foot_exit_codes(om, rob, se3):
    """The oracle's exit code of each of the four foot boxes of every state: (n, 4)."""
    poses, _ = om.state_poses(rob, se3)
    _, ec, _ = om.feet.check_boxes(rob.foot, poses[:, 1:5].reshape(-1, 16), want_detail=True)
    return ec.reshape(-1, 4)


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
def test_vertex_plane_and_nothing_boxes_on_perlin_terrain(gm1, rname):
    """Perlin terrain + obstacles, 2^15 states of the sampler, both robots (the defaults robot's foot box is 0.5 x 0.2 x
    0.3: other windows): the labels of the fused step and of validate_states equal the oracle's, and the oracle decides
    at least MIN_EACH foot boxes by each of the three exits the kernel's two stages produce."""
    rob = O.robot(rname)
    om = O.OracleMap(gm1)
    ctx = _ctx(rname, gm1)
    se3, fused = _sampled_and_validated(ctx, N)
    ec = _foot_exit_codes(om, rob, se3)
    counts = {name: int((ec == code).sum()) for name, code in (("vertex", EXIT_VERTEX), ("plane", EXIT_PLANE), ("none", EXIT_NONE))}
    print("foot boxes by the oracle's exit:", counts)
    assert min(counts.values()) >= MIN_EACH, counts   # the map must keep exercising every branch
    ref = om.states_valid(rob, se3)
    assert np.array_equal(fused, ref), f"sample_and_validate_dev: {(fused != ref).sum()} mismatches"
    vg = ctx.validate_states(se3)
    assert np.array_equal(vg, ref), f"validate_states: {(vg != ref).sum()} mismatches"
    assert 0 < ref.sum() < N
    ctx.close()


def test_partner_planes_are_streamed_then_queued(gm_terraced):
    """Terraces: corner candidates with coplanar partners (corner stage result 2).  Such a box still gets its stream and
    is queued for the list pass only when the stream finds no vertex: labels equal the oracle's and the list pass ran.
    The number of boxes queued is the same on two consecutive calls.  That number is only defined for a batch in which
    the kernel fails no state itself (a box of a state that another foot has already failed is skipped, and which of two
    feet comes first is a matter of timing), so the repeated batch holds the states none of whose feet the oracle decides
    by EXIT_NONE."""
    rob = O.robot("yaml")
    om = O.OracleMap(gm_terraced)
    ctx = _ctx("yaml", gm_terraced, sampler=False)
    rng = np.random.default_rng(21)
    se3 = common.random_states(gm_terraced, N, rng, z_off=(0.0, 0.03), tilt=0.15, spread=0.5)
    vg = ctx.validate_states(se3)
    cnt = ctx.pipeline_counters()
    vo = om.states_valid(rob, se3)
    assert np.array_equal(vg, vo), f"{(vg != vo).sum()} mismatches"
    print("pipeline counters:", cnt)
    assert cnt["feet_partner_pass"] > 0, cnt          # the rr = 2 path was taken
    assert 0.02 < vg.mean() < 0.98
    keep = ~(_foot_exit_codes(om, rob, se3) == EXIT_NONE).any(axis=1)
    sub = se3[keep]
    assert len(sub) > N // 8
    queued = []
    for _ in range(2):
        v2 = ctx.validate_states(sub)
        assert np.array_equal(v2, vo[keep])
        queued.append(ctx.pipeline_counters()["feet_partner_pass"])
    print("queued for the list pass, twice:", queued)
    assert queued[0] > 0 and queued[0] == queued[1], queued
    ctx.close()


def test_unknown_cells_stay_with_the_lane_scan(gm_terraced):
    """The same map with a band of unknown (NaN) rows: foot records without a table verdict, which the kernel must leave
    alone (classify lists them for the lane scan).  Labels equal the oracle's."""
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
    vo = O.OracleMap(gm).states_valid(rob, se3)
    assert np.array_equal(vg, vo), f"{(vg != vo).sum()} mismatches"
    assert 0.02 < vg.mean() < 0.9
    ctx.close()


def test_edges_between_accepted_states(gm1):
    """2^12 pairs of accepted states through check_motions_dev (edge batches expand into states and run the same
    kernel): verdicts equal the oracle's checkMotion, both verdicts occur."""
    import torch
    rob = O.robot("yaml")
    om = O.OracleMap(gm1)
    ctx = _ctx("yaml", gm1)
    se3, labels = _sampled_and_validated(ctx, N)
    acc = se3[labels != 0]
    assert len(acc) >= 64
    rng = np.random.default_rng(11)
    n = 1 << 12
    s1, s2 = acc[rng.integers(0, len(acc), n)], acc[rng.integers(0, len(acc), n)]
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
