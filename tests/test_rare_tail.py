"""The two tails of the batch validity step on the GPU (-m gpu): the five-launch full tail and rare_boxes_kernel, the one
launch that takes a batch's few leftover boxes (queues 4, 6 and 5) to their labels.  Labels are always BIT-EQUAL to the C
oracle's, whichever tail ran.

Maps: the C2-style Perlin terrain at 100 x 100 (next to nothing left over, the regime the rare tail is for); the terraced
map of test_feet_prepass.py (queues 5, 6 and 2 populated: the list pass and the exact grouping must agree); bands of NaN
rows like the one of the existing suites (thousands of boxes in queues 4 and 6: the rare tail's slow-but-correct case); a
flat map (every queue empty).  Auto mode is followed across map uploads and a change of regime through Context.last_tail().  Every window fits the LDS
tile: nothing here raises the capacity error."""
import copy

import numpy as np
import pytest

import common
import feet_prepass_ref as P
import oracle_py as O
from synthetic import make_map

pytestmark = pytest.mark.gpu

FULL, RARE = 1, 2
N = 1 << 13


def _ctx(gm, sampler=False, mode=0):
    from art_planner_amd.context import Context
    c = Context(0, "yaml")
    c.upload_map(gm, sampler=sampler)
    c.set_tail_mode(mode)
    return c


def _nan_bands(gm0, bands):
    gm = copy.deepcopy(gm0)
    for name in ("elevation", "elevation_masked"):
        a = np.array(gm[name], dtype=np.float32, order="F")
        for lo, hi in bands:
            a[lo:hi, :] = np.nan
        gm.layers[name] = np.asfortranarray(a)
    return gm


def _case(gm, n, seed, z_off=(0.0, 0.05)):
    """States and their oracle labels, computed once."""
    se3 = common.random_states(gm, n, np.random.default_rng(seed), z_off=z_off, tilt=0.15, spread=0.5)
    return dict(gm=gm, se3=se3, ref=O.OracleMap(gm).states_valid(O.robot("yaml"), se3))


@pytest.fixture(scope="module")
def perlin():
    return _case(make_map(100, 0.04, seed=1234), 3 * (1 << 12), 31)


@pytest.fixture(scope="module")
def nan_bands():
    """The band of NaN rows of test_feet_prepass.py, twelve times across the 200-cell map, 2^15 states: boxes that straddle
    a band's edge have no table verdict (queue 4) or no all-finite window (queue 6) -- tens of thousands of them."""
    gm = _nan_bands(make_map(200, 0.04, seed=3), [(r, r + 6) for r in range(8, 200, 16)])
    return _case(gm, 1 << 15, 6, z_off=(0.02, 0.12))


def _both_modes(case, n):
    out = {}
    for mode in (FULL, RARE):
        ctx = _ctx(case["gm"], mode=mode)
        lab = ctx.validate_states(case["se3"][:n])
        assert ctx.last_tail() == mode
        out[mode] = (lab, ctx.pipeline_counters())
        ctx.close()
    return out


def test_perlin_map_full_and_rare_tail_equal_the_oracle(perlin):
    got = _both_modes(perlin, N)
    ref = perlin["ref"][:N]
    print("counters, full tail:", got[FULL][1], "rare tail:", got[RARE][1])
    assert np.array_equal(got[FULL][0], ref), f"full tail: {(got[FULL][0] != ref).sum()} mismatches"
    assert np.array_equal(got[RARE][0], ref), f"rare tail: {(got[RARE][0] != ref).sum()} mismatches"
    assert 0 < ref.sum() < N


def test_terraced_map_list_pass_and_exact_grouping_agree():
    gm = P.terraced(make_map(200, 0.04, seed=3))
    n = 1 << 15
    se3 = common.random_states(gm, n, np.random.default_rng(21), z_off=(0.0, 0.03), tilt=0.15, spread=0.5)
    case = dict(gm=gm, se3=se3)
    got = _both_modes(case, n)
    ref = O.OracleMap(gm).states_valid(O.robot("yaml"), se3)
    cf, cr = got[FULL][1], got[RARE][1]
    print("counters, full tail:", cf, "rare tail:", cr)
    # the premise of the case: the full tail's list pass and exact grouping both have work here
    assert cf["feet_partner_pass"] >= 1000 and cf["exact_grouping"] > 0, cf
    # the rare tail takes the same boxes from queue 5, pushes nothing to queue 3, and every box it groups is counted
    assert cr["feet_partner_pass"] > 0 and cr["feet_plane_stage"] == 0, cr
    assert 0 < cr["exact_grouping"] <= cr["feet_partner_pass"] + cr["torso_staged_pass"], cr
    assert np.array_equal(got[FULL][0], ref), f"full tail: {(got[FULL][0] != ref).sum()} mismatches"
    assert np.array_equal(got[RARE][0], ref), f"rare tail: {(got[RARE][0] != ref).sum()} mismatches"
    assert 0.02 < ref.mean() < 0.98


def test_nan_bands_thousands_of_boxes_through_the_rare_tail(nan_bands):
    case = nan_bands
    n = len(case["se3"])
    got = _both_modes(case, n)
    ref = case["ref"]
    cr = got[RARE][1]
    print("counters, full tail:", got[FULL][1], "rare tail:", cr)
    # the premise of the case: thousands of boxes in queues 4 and 6 together, neither of them a handful
    assert cr["feet_lane_scan"] + cr["torso_staged_pass"] >= 2000, cr
    assert cr["feet_lane_scan"] >= 100 and cr["torso_staged_pass"] >= 100, cr
    assert cr["feet_plane_stage"] == 0, cr         # queue 3 stays empty
    assert cr["exact_grouping"] <= cr["feet_lane_scan"] + cr["torso_staged_pass"], cr
    assert np.array_equal(got[RARE][0], ref), f"rare tail: {(got[RARE][0] != ref).sum()} mismatches"
    assert np.array_equal(got[FULL][0], ref), f"full tail: {(got[FULL][0] != ref).sum()} mismatches"
    assert 0 < ref.sum() < n


def test_auto_mode_across_a_regime_change(perlin, nan_bands):
    """Three batches on the finite map, the NaN-band map uploaded, three batches there, and back to the finite map.  Every
    batch equals the oracle.  The first call after an upload takes the full tail; after that the count the previous batch
    left decides.  The rare grid has one wavefront per workgroup and between 1 and 16 workgroups per CU (by LDS), so a
    count of at most the number of CUs is on the rare side of the rule for every tile size and a count above 16 x CUs on
    the full side: the finite batches must leave the former, the NaN-band batches the latter, and the tails must follow."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    m = 1 << 12
    ctx = _ctx(perlin["gm"])
    taken = []
    for case, finite in ((perlin, True), (nan_bands, False), (perlin, True)):
        if taken:
            ctx.upload_map(case["gm"], sampler=False)
        for k in range(3):
            # the finite map: three different batches; the NaN-band map: its 2^15 states three times
            sl = slice(k * m, (k + 1) * m) if finite else slice(None)
            lab = ctx.validate_states(case["se3"][sl])   # returns with the labels: the batch is done
            ref = case["ref"][sl]
            assert np.array_equal(lab, ref), (len(taken), int((lab != ref).sum()))
            cnt = ctx.pipeline_counters()
            # what the call's last kernel reports: queues 4, 6, 5 and, where the full tail filled it, queue 2
            left = cnt["feet_lane_scan"] + cnt["torso_staged_pass"] + cnt["feet_partner_pass"]
            if ctx.last_tail() == FULL:
                left += cnt["exact_grouping"]
            taken.append((ctx.last_tail(), int(left)))
    ctx.close()
    print("(tail, leftover boxes) per batch:", taken, "CUs:", cus)
    tails = [t for t, _ in taken]
    counts = [c for _, c in taken]
    assert all(c <= cus for c in counts[0:3] + counts[6:9]), (counts, cus)   # the rare side of the rule, whatever the tile
    assert all(c > 16 * cus for c in counts[3:6]), (counts, cus)            # the full side
    assert tails[0:3] == [FULL, RARE, RARE], tails     # after the first upload
    assert tails[3:6] == [FULL, FULL, FULL], tails     # after the upload: full; then by the count: full
    assert tails[6:9] == [FULL, RARE, RARE], tails     # back: after the upload full, then by the count again


def test_edges_same_verdicts_with_either_tail():
    import torch
    gm = make_map(100, 0.04, seed=1234)
    n = 1 << 10
    verdicts = {}
    s1 = s2 = None
    for mode in (FULL, RARE):
        ctx = _ctx(gm, sampler=True, mode=mode)
        ctx.use_torch_stream()
        if s1 is None:
            ns = 1 << 15
            se3 = torch.empty((ns, 7), dtype=torch.float64, device="cuda:0")
            valid = torch.empty(ns, dtype=torch.uint8, device="cuda:0")
            ctx.sample_and_validate_dev(42, 0, ns, se3, valid)
            torch.cuda.synchronize()
            acc = se3[valid != 0]
            assert len(acc) >= 64
            g = torch.Generator().manual_seed(5)
            s1 = acc[torch.randint(0, len(acc), (n,), generator=g).cuda()].contiguous()
            s2 = acc[torch.randint(0, len(acc), (n,), generator=g).cuda()].contiguous()
        v = torch.empty(n, dtype=torch.uint8, device="cuda:0")
        ctx.check_motions_dev(s1, s2, v)
        torch.cuda.synchronize()
        assert ctx.last_tail() == mode
        verdicts[mode] = v.cpu().numpy()
        ctx.close()
    assert np.array_equal(verdicts[FULL], verdicts[RARE]), f"{(verdicts[FULL] != verdicts[RARE]).sum()} verdicts differ"
    assert 0 < verdicts[FULL].sum() < n


def test_flat_map_every_queue_empty():
    gm = make_map(100, 0.04, seed=1234, flat=True)
    se3 = common.random_states(gm, 1 << 12, np.random.default_rng(33), z_off=(0.0, 0.05), tilt=0.15, spread=0.5)
    ctx = _ctx(gm, mode=RARE)
    lab = ctx.validate_states(se3)
    cnt = ctx.pipeline_counters()
    ctx.close()
    print("counters:", cnt)
    assert cnt["feet_lane_scan"] == 0 and cnt["torso_staged_pass"] == 0 and cnt["feet_partner_pass"] == 0, cnt
    ref = O.OracleMap(gm).states_valid(O.robot("yaml"), se3)
    assert np.array_equal(lab, ref), f"{(lab != ref).sum()} mismatches"
