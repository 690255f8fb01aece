"""feet_stream_kernel's pre-pass (two lanes per box, the box's lowest corner) on the GPU (-m gpu): labels and verdicts
BIT-EQUAL to the C oracle's.

The pre-pass settles a box as "touches" from one corner and hands the rest to the full 16-lane corner stage, four boxes
a round (see lane_corner_probe in box_check.h and its restatement, feet_prepass_ref.py, whose soundness the CPU test
test_feet_prepass_ref.py checks against the oracle).  Here the shipped kernel runs the inputs of that test: the
sampler's 2^15 states on make_map(100, 0.04, seed=3) and 2^15 random states on the terraced 200-cell map, both robots,
through the fused step, validate_states and 2^12 edges; batch sizes and sub-queue fills around the chunk of 32 boxes and
the pre-pass's lane masks; records without a table verdict; states with a foot that fails; and one batch 20 times.

Not built here: a foot window wider than the partner table's radius.  The radius is ceil(box diagonal / sample spacing)
+ 3 and a window spans at most that many cells, and a layer whose radius would pass 63 is refused at upload with the
window tile, so no accepted robot or spacing produces one; the restatement's CPU test covers the rule instead."""
import copy

import numpy as np
import pytest

import common
import feet_prepass_ref as P
import oracle_py as O
from synthetic import make_map

pytestmark = pytest.mark.gpu

N = 1 << 15
EXIT_VERTEX, EXIT_PLANE, EXIT_NONE = 5, 6, 8


def _ctx(kind, gm, sampler=True):
    from art_planner_amd.context import Context
    c = Context(0, kind)
    c.upload_map(gm, sampler=sampler)
    return c


def _fused(ctx, n):
    import torch
    se3 = torch.empty((n, 7), dtype=torch.float64, device="cuda:0")
    valid = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    ctx.use_torch_stream()
    ctx.sample_and_validate_dev(42, 0, n, se3, valid)
    torch.cuda.synchronize()
    return se3.cpu().numpy(), valid.cpu().numpy()


@pytest.fixture(scope="module")
def gm1():
    return make_map(100, 0.04, seed=3)


@pytest.fixture(scope="module")
def gm_terraced():
    return P.terraced(make_map(200, 0.04, seed=3))


@pytest.fixture(scope="module")
def perlin_yaml(gm1):
    """The sampler's 2^15 states on the Perlin map (yaml robot) with everything the oracle and the restatement say about
    them, computed once: states, the fused step's labels, oracle labels, per-foot exit codes and probe decisions."""
    rob = O.robot("yaml")
    om = O.OracleMap(gm1)
    ctx = _ctx("yaml", gm1)
    se3, fused = _fused(ctx, N)
    ctx.close()
    ref = om.states_valid(rob, se3)
    fp = P.foot_poses(om, rob, se3)
    _, ec, _ = om.feet.check_boxes(rob.foot, fp, want_detail=True)
    R = P.foot_radius(rob, gm1.res)
    decided, _ = P.probe(om.feet, rob.foot, fp, P.partner_flags(om.feet, R), R)
    return dict(rob=rob, om=om, se3=se3, fused=fused, ref=ref, ec=ec.reshape(-1, 4), decided=decided.reshape(-1, 4))


def test_fused_step_and_validate_states_on_perlin_terrain_yaml(gm1, perlin_yaml):
    d = perlin_yaml
    neg = np.isin(d["ec"], (EXIT_VERTEX, EXIT_PLANE, EXIT_NONE))
    print("foot boxes with negative exits", int(neg.sum()), "of which the restatement's probe decides", int((d["decided"] & neg).sum()))
    assert (d["decided"] & neg).sum() >= 100 and (~d["decided"] & neg).sum() >= 100
    assert np.array_equal(d["fused"], d["ref"]), f"sample_and_validate_dev: {(d['fused'] != d['ref']).sum()} mismatches"
    ctx = _ctx("yaml", gm1)
    vg = ctx.validate_states(d["se3"])
    ctx.close()
    assert np.array_equal(vg, d["ref"]), f"validate_states: {(vg != d['ref']).sum()} mismatches"
    assert 0 < d["ref"].sum() < N


def test_fused_step_and_validate_states_on_perlin_terrain_defaults(gm1):
    rob = O.robot("defaults")
    om = O.OracleMap(gm1)
    ctx = _ctx("defaults", gm1)
    se3, fused = _fused(ctx, N)
    ref = om.states_valid(rob, se3)
    assert np.array_equal(fused, ref), f"sample_and_validate_dev: {(fused != ref).sum()} mismatches"
    vg = ctx.validate_states(se3)
    ctx.close()
    assert np.array_equal(vg, ref), f"validate_states: {(vg != ref).sum()} mismatches"
    assert 0 < ref.sum() < N


@pytest.mark.parametrize("rname", ["yaml", "defaults"])
def test_terraces_flagged_candidates_go_to_the_partner_pass(gm_terraced, rname):
    """Terraces: nearly every candidate under a corner is flagged, the probe refuses them and the boxes take the full stage,
    their stream and the list pass."""
    rob = O.robot(rname)
    om = O.OracleMap(gm_terraced)
    ctx = _ctx(rname, gm_terraced, sampler=False)
    se3 = common.random_states(gm_terraced, N, np.random.default_rng(21), z_off=(0.0, 0.03), tilt=0.15, spread=0.5)
    vg = ctx.validate_states(se3)
    cnt = ctx.pipeline_counters()
    ctx.close()
    vo = om.states_valid(rob, se3)
    assert np.array_equal(vg, vo), f"{(vg != vo).sum()} mismatches"
    print("pipeline counters:", cnt)
    assert cnt["feet_partner_pass"] > 0, cnt
    assert 0.02 < vg.mean() < 0.98


def test_edges_between_accepted_states(gm1, perlin_yaml):
    import torch
    d = perlin_yaml
    acc = d["se3"][d["ref"] != 0]
    rng = np.random.default_rng(11)
    n = 1 << 12
    s1, s2 = acc[rng.integers(0, len(acc), n)], acc[rng.integers(0, len(acc), n)]
    ctx = _ctx("yaml", gm1)
    a, b = torch.from_numpy(np.ascontiguousarray(s1)).cuda(), torch.from_numpy(np.ascontiguousarray(s2)).cuda()
    v = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    ctx.use_torch_stream()
    ctx.check_motions_dev(a, b, v)
    torch.cuda.synchronize()
    eg = v.cpu().numpy()
    ctx.close()
    eo, _ = d["om"].check_motions(d["rob"], s1, s2)
    assert np.array_equal(eg, eo), f"{(eg != eo).sum()} verdicts differ"
    assert 0 < eo.sum() < n


def test_small_batches_and_sub_queue_fills_around_the_chunk(gm1, perlin_yaml):
    """Batches of 1, 7, 33 and 65 states, and batches that put exactly 1, 31, 32 and 33 boxes into one foot sub-queue (a
    batch of at most 64 states is one classify workgroup, whose boxes all go to sub-queue 0): the chunk's tail and the
    pre-pass's lane masks.  How many foot boxes a state queues is measured per state first (classify decides that per
    state), then the batches are put together from those numbers and the counter of the batch must be the target."""
    d = perlin_yaml
    ctx = _ctx("yaml", gm1, sampler=False)
    for n in (1, 7, 33, 65):
        for first in (0, 1000, 20000):
            vg = ctx.validate_states(d["se3"][first:first + n])
            assert np.array_equal(vg, d["ref"][first:first + n]), (n, first)
    # calls of up to 16 states take the latency path, not this kernel: a state is measured as a batch of 17 copies of it
    cand = np.arange(600)
    per_state = []
    for i in cand:
        vg = ctx.validate_states(np.repeat(d["se3"][i:i + 1], 17, axis=0))
        assert (vg == d["ref"][i]).all()
        q = int(ctx.pipeline_counters()["feet_queued"])
        assert q % 17 == 0, q
        per_state.append(q // 17)
    per_state = np.array(per_state)
    print("foot boxes queued per state:", np.bincount(per_state, minlength=5).tolist())
    pad = cand[per_state == 0]
    assert len(pad) >= 24
    for target in (1, 31, 32, 33):
        # subset sum over the candidates
        reach = {0: []}
        for k, q in enumerate(per_state):
            if q == 0:
                continue
            for s, members in list(reach.items()):
                if s + q <= target and s + q not in reach:
                    reach[s + q] = members + [k]
            if target in reach:
                break
        assert target in reach, (target, np.bincount(per_state).tolist())
        idx = cand[reach[target]]
        assert len(idx) <= 40
        idx = np.concatenate([idx, pad[:24]])      # states that queue no foot box: more than 16 states, at most 64
        vg = ctx.validate_states(d["se3"][idx])
        cnt = ctx.pipeline_counters()
        print("target", target, "states", len(idx), "counters", cnt)
        assert cnt["feet_queued"] == target, cnt
        assert np.array_equal(vg, d["ref"][idx])
    ctx.close()


def test_unknown_cells_stay_with_the_lane_scan(gm_terraced, gm1):
    """A band of NaN rows, on the terraced and on the Perlin map: foot records without a table verdict, which the pre-pass
    must leave alone like the rounds do (classify lists them for the lane scan)."""
    for gm0, seed in ((gm_terraced, 5), (make_map(200, 0.04, seed=3), 6)):
        gm = copy.deepcopy(gm0)
        for name in ("elevation", "elevation_masked"):
            a = np.array(gm[name], dtype=np.float32, order="F")
            a[80:110, :] = np.nan
            gm.layers[name] = np.asfortranarray(a)
        rob = O.robot("yaml")
        ctx = _ctx("yaml", gm, sampler=False)
        se3 = common.random_states(gm, N, np.random.default_rng(seed), z_off=(0.02, 0.12), tilt=0.15, spread=0.5)
        vg = ctx.validate_states(se3)
        ctx.close()
        vo = O.OracleMap(gm).states_valid(rob, se3)
        assert np.array_equal(vg, vo), f"{(vg != vo).sum()} mismatches"
        assert 0.02 < vg.mean() < 0.9


def test_states_with_a_failing_foot_and_settled_feet(gm1, perlin_yaml):
    """Every state of the batch has a foot that the oracle ends with EXIT_NONE (it fails the state) and another that the
    probe settles: boxes of states that fail while their chunk is in flight.  Every label is 0, call after call."""
    d = perlin_yaml
    neg = np.isin(d["ec"], (EXIT_VERTEX, EXIT_PLANE, EXIT_NONE))
    pick = (d["ec"] == EXIT_NONE).any(axis=1) & (d["decided"] & neg).any(axis=1)
    sub = d["se3"][pick]
    print("states with a failing foot and a settled foot:", len(sub))
    assert len(sub) >= 100
    assert not d["ref"][pick].any()
    ctx = _ctx("yaml", gm1, sampler=False)
    for _ in range(3):
        assert not ctx.validate_states(sub).any()
    ctx.close()


def test_one_batch_twenty_times(gm1, perlin_yaml):
    d = perlin_yaml
    ctx = _ctx("yaml", gm1, sampler=False)
    sub = d["se3"][:1 << 13]
    for _ in range(20):
        assert np.array_equal(ctx.validate_states(sub), d["ref"][:1 << 13])
    ctx.close()
