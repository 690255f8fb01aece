"""The full-width motion-cost network (network.py, n9convNetwork3LR: grid-1563-blind, grid-1975-blind, grid-1992-perceptive):
blob version 2, the numpy oracle against the reference class's fixtures (CPU), the HIP path at 32 / 64 channels against
both (GPU), and switching networks on one context."""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np
import pytest

import common

sys.path.insert(0, os.path.join(common.ROOT, "oracle"))
sys.path.insert(0, os.path.join(common.ROOT, "tools"))
sys.path.insert(0, os.path.join(common.ROOT, "scripts"))
import motion_cost_oracle as mo  # noqa: E402
import convert_weights as cw  # noqa: E402
from test_mfma_hazard import needs_hipcc  # noqa: E402

GOLD = np.load(os.path.join(common.GOLDEN_DIR, "motion_cost_full.npz"))
GOLD120 = np.load(os.path.join(common.GOLDEN_DIR, "motion_cost_full_120.npz"))
# the reference full-width network's own torch.half-vs-float32 error on the inputs below (make_golden_cost_full.py)
ANCHOR = json.load(open(os.path.join(common.GOLDEN_DIR, "motion_cost_full_fp16_anchor.json")))["cases"]
ANCHOR_FACTOR = 1.0   # as for the light network (tests/test_motion_cost.py)
FULL_BYTES, LIGHT_BYTES = 4141140, 2333524
ERR_INVALID_ARG, ERR_NO_MAP = -1, -4


def _params_full():
    return mo.random_params(0, cw.SHAPES_FULL)


# ---- CPU ---------------------------------------------------------------------------------------------------------------
def test_full_blob_has_version_2_and_the_light_blob_is_unchanged():
    b = cw.to_blob(_params_full())
    assert b[:4] == b"ARMC" and b[4] == 2 and b[5:8] == b"\0\0\0"
    assert len(b) == FULL_BYTES == 8 + 4 * 1035283
    light = cw.to_blob(mo.random_params(0))
    assert light[4] == 1 and len(light) == LIGHT_BYTES
    assert hashlib.sha256(light).hexdigest().startswith("b994b33616867687")
    # random_params' default table is still the light one, the explicit one gives the same draw
    assert all(np.array_equal(v, mo.random_params(0, cw.SHAPES)[k]) for k, v in mo.random_params(0).items())


def test_to_blob_refuses_an_unknown_width():
    p = _params_full()
    p["init_conv1.weight"] = np.zeros((40, 1, 3, 3), np.float32)
    with pytest.raises(ValueError):
        cw.to_blob(p)


def test_library_reports_both_blob_sizes():
    from art_planner_amd import _capi
    L = _capi.load()
    assert L.artp_cost_blob_bytes() == LIGHT_BYTES
    assert L.artp_cost_blob_bytes_version(1) == LIGHT_BYTES
    assert L.artp_cost_blob_bytes_version(2) == FULL_BYTES
    assert L.artp_cost_blob_bytes_version(0) == 0 and L.artp_cost_blob_bytes_version(3) == 0


def test_convert_weights_main_on_a_full_width_state_dict(tmp_path, monkeypatch):
    """A checkpoint in the reference's state_dict layout at network.py's shapes (BatchNorm counters included) converts to the
    version-2 blob of the same parameters."""
    torch = pytest.importorskip("torch")
    p = _params_full()
    sd = {k: torch.from_numpy(v.copy()) for k, v in p.items()}
    for name in list(cw.SHAPES_FULL):
        if name not in cw.WITH_BIAS:
            sd[name + "_bn.num_batches_tracked"] = torch.tensor(0)
    ck, out = tmp_path / "grid-full.pt", tmp_path / "grid-full.armc"
    torch.save(sd, ck)
    monkeypatch.setattr(sys, "argv", ["convert_weights.py", str(ck), str(out)])
    cw.main()
    assert out.read_bytes() == cw.to_blob(p)


@pytest.mark.parametrize("g,F", [(GOLD, 32), (GOLD120, 36)], ids=["112", "120"])
def test_oracle_matches_reference_full_network_golden(g, F):
    p = _params_full()
    crop = g["crop"].astype(np.float32)
    res = float(g["res"])
    L = crop.shape[0] * res
    f = mo.cnn_features(p, crop)
    assert f.shape == (64, F, F)
    assert np.abs(f - g["features"]).max() < 1e-3
    c = mo.fc_costs(p, g["features"], g["edges"], res, L, L)
    assert np.abs(c - g["costs"]).max() < 1e-4


FULL_KERNELS = ["fc_cost_mfma_full_kernel", "conv345_kernelILi12ELb1ELb1ELi32ELi64", "conv_ksplit_kernelILi15ELi15ELi64ELi64"]


@needs_hipcc
def test_full_width_mfma_kernels_keep_the_measured_distances(tmp_path):
    """scripts/mfma_hazard_check.py over the full network's MFMA kernels: one MFMA shape each, no hazard below the minima."""
    import mfma_hazard_check as H
    asm = H.compile_asm(str(tmp_path / "artp.s"))
    res = H.check_file(asm, FULL_KERNELS)
    for k in FULL_KERNELS:
        assert any(k in n for n, _, _ in res), f"{k} not found in the assembly"
    assert not [(n, v) for n, _, viol in res for v in viol]
    assert all(r["shapes"] == {"16x16x32"} and r["mix"] is None for _, r, _ in res)


# ---- GPU ---------------------------------------------------------------------------------------------------------------
def _ctx(blob):
    from art_planner_amd.context import Context
    ctx = Context(0, "yaml")
    ctx.cost_load_weights(blob)
    return ctx


def _update(ctx, elv, res):
    ctx.cost_update_map(np.ascontiguousarray(elv, np.float32), res, elv.shape[0] * res, elv.shape[1] * res)


def _assert_within_reference_half_error(f_hwc, ref_chw, c, c_ref, case):
    a = ANCHOR[case]
    ref = np.transpose(ref_chw, (1, 2, 0))
    assert f_hwc.shape == ref.shape, (case, f_hwc.shape, ref.shape)
    fe = np.abs(f_hwc - ref)
    ce = np.abs(c - c_ref)
    cex = (ce - 2e-3 * np.abs(c_ref)).max(axis=1)
    got = {"feat_err_max": float(fe.max()), "feat_err_mean": float(fe.mean()), "feat_err_q999": float(np.quantile(fe, 0.999)),
           "cost_err_max": float(ce.max()), "cost_err_mean": float(ce.mean()),
           "cost_excess_over_2e-3_rel_q99": float(np.quantile(cex, 0.99)), "cost_excess_over_2e-3_rel_max": float(cex.max())}
    for k, v in got.items():
        assert v <= ANCHOR_FACTOR * a[k], (case, k, v, "reference half-vs-float32:", a[k])


def _map_edges(gm, n):
    rng = np.random.default_rng(n)
    B = 20000
    s = rng.uniform(-0.55 * gm.len_x, 0.55 * gm.len_x, (B, 2))
    d = rng.uniform(-0.6, 0.6, (B, 2))
    return np.stack([s[:, 0] + d[:, 0], s[:, 1] + d[:, 1], rng.uniform(-np.pi, np.pi, B), s[:, 0], s[:, 1],
                     rng.uniform(-np.pi, np.pi, B)], 1).astype(np.float32)


@pytest.mark.gpu
def test_gpu_full_blob_loads_with_the_mfma_fc_path():
    ctx = _ctx(cw.to_blob(_params_full()))
    assert ctx.cost_feature_channels() == 64
    fp = ctx.cost_fc_path()
    assert fp["mfma"] == 1 and fp["selfcheck"] == 1, fp
    assert fp["max_abs_diff"] < 1e-4
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("g,case", [(GOLD, "golden_112"), (GOLD120, "golden_120")], ids=["112", "120"])
def test_gpu_full_features_and_costs_match_reference_golden(g, case):
    """112^2 -> 32^2 and 120^2 -> 36^2 (partial tiles in every kernel) against the reference network.py in float32, within the
    reference's own half-vs-float32 error."""
    ctx = _ctx(cw.to_blob(_params_full()))
    _update(ctx, g["crop"].astype(np.float32), float(g["res"]))
    f = ctx.cost_features()
    c = ctx.cost_query(g["edges"])
    _assert_within_reference_half_error(f, g["features"], c, g["costs"], case)
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n,F", [(400, 176), (800, 376), (141, 46), (97, 24)])
def test_gpu_full_features_and_costs_match_oracle_at_c3_c4_and_odd_sizes(n, F):
    """C3, C4 and two odd sizes against the numpy oracle (pinned on network.py at 112^2 / 120^2), then 20 000 edge costs
    against the oracle fed with the ORACLE's features, under the same anchor rule as the light network."""
    from synthetic import make_map
    gm = make_map(n, 0.04, seed=1234 if n == 400 else 77)
    elv = np.ascontiguousarray(gm["elevation"][::-1, ::-1]).astype(np.float16).astype(np.float32)
    p = _params_full()
    ref = mo.cnn_features(p, elv)
    assert ref.shape == (64, F, F)
    ctx = _ctx(cw.to_blob(p))
    _update(ctx, elv, gm.res)
    f = ctx.cost_features()
    e = _map_edges(gm, n)
    c = ctx.cost_query(e)
    co = mo.fc_costs(p, ref, e, gm.res, gm.len_x, gm.len_y)
    _assert_within_reference_half_error(f, ref, c, co, f"map_{n}")
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mfma", [True, False], ids=["mfma", "fp32"])
def test_gpu_full_fc_paths_match_the_oracle_on_the_devices_features(mfma):
    """Both FC forms (the MFMA hi / lo kernel and the fp32 VALU one) against the float32 oracle's FCpart fed with the
    device's own feature map: the MLP alone, to fp32 accuracy."""
    p = _params_full()
    ctx = _ctx(cw.to_blob(p))
    ctx.cost_set_fc_path(mfma)
    assert ctx.cost_fc_path()["mfma"] == int(mfma)
    crop = GOLD["crop"].astype(np.float32)
    res = float(GOLD["res"])
    _update(ctx, crop, res)
    f = ctx.cost_features()
    c = ctx.cost_query(GOLD["edges"])
    L = crop.shape[0] * res
    co = mo.fc_costs(p, np.transpose(f, (2, 0, 1)), GOLD["edges"], res, L, L)
    err = np.abs(c - co)
    assert (err <= 1e-4 + 1e-4 * np.abs(co)).all(), float(err.max())
    ctx.close()


@pytest.mark.gpu
def test_gpu_light_full_light_on_one_context_equals_a_fresh_light_context():
    """Switching networks leaves nothing behind: the light results after light -> full -> light are bit for bit those of a
    fresh light context; the full results in between are those of a fresh full context."""
    light, full = cw.to_blob(mo.random_params(0)), cw.to_blob(_params_full())
    crop = GOLD["crop"].astype(np.float32)
    res = float(GOLD["res"])
    e = GOLD["edges"]

    def run(ctx):
        _update(ctx, crop, res)
        return ctx.cost_features(), ctx.cost_query(e)

    fresh_l = _ctx(light)
    fl, cl = run(fresh_l)
    fresh_l.close()
    fresh_f = _ctx(full)
    ff, cf = run(fresh_f)
    fresh_f.close()
    ctx = _ctx(light)
    run(ctx)
    ctx.cost_load_weights(full)
    f2, c2 = run(ctx)
    assert f2.shape == (32, 32, 64) and np.array_equal(f2, ff) and np.array_equal(c2, cf)
    ctx.cost_load_weights(light)
    f3, c3 = run(ctx)
    assert f3.shape == (32, 32, 48) and np.array_equal(f3, fl) and np.array_equal(c3, cl)
    assert ctx.cost_fc_path()["selfcheck"] == 1
    ctx.close()


@pytest.mark.gpu
def test_gpu_no_query_is_answered_from_the_other_networks_features():
    """A load that switches the network drops the feature map: queries and feature reads answer ARTP_ERR_NO_MAP until the
    next map update, in both directions.  Reloading the same network keeps the map (as before)."""
    light, full = cw.to_blob(mo.random_params(0)), cw.to_blob(_params_full())
    crop = GOLD["crop"].astype(np.float32)
    res = float(GOLD["res"])
    e = np.ascontiguousarray(GOLD["edges"][:64])
    out = np.empty((64, 3), np.float32)
    for first, second in ((light, full), (full, light)):
        ctx = _ctx(first)
        _update(ctx, crop, res)
        ctx.cost_query(e)
        ctx.cost_load_weights(second)
        assert ctx.L.artp_cost_query(ctx.h, e.ctypes.data, 64, out.ctypes.data) == ERR_NO_MAP
        fh, fw = C.c_int(0), C.c_int(0)
        ch = ctx.cost_feature_channels()
        assert ctx.L.artp_cost_get_features_c(ctx.h, None, ch, C.byref(fh), C.byref(fw)) == ERR_NO_MAP
        _update(ctx, crop, res)
        ctx.cost_query(e)
        ctx.cost_load_weights(second)          # the same network again: the map stays
        assert ctx.L.artp_cost_query(ctx.h, e.ctypes.data, 64, out.ctypes.data) == 0
        ctx.close()


@pytest.mark.gpu
def test_gpu_get_features_refuses_while_the_full_network_is_loaded():
    """artp_cost_get_features is the 48-channel getter: with the full network loaded it refuses (ARTP_ERR_INVALID_ARG) and
    writes nothing; artp_cost_get_features_c with the wrong count refuses too."""
    ctx = _ctx(cw.to_blob(_params_full()))
    _update(ctx, GOLD["crop"].astype(np.float32), float(GOLD["res"]))
    fh, fw = C.c_int(-7), C.c_int(-7)
    buf = np.full(32 * 32 * 48, 123.0, np.float32)
    assert ctx.L.artp_cost_get_features(ctx.h, buf.ctypes.data, C.byref(fh), C.byref(fw)) == ERR_INVALID_ARG
    assert (buf == 123.0).all() and fh.value == -7 and fw.value == -7
    assert ctx.L.artp_cost_get_features_c(ctx.h, buf.ctypes.data, 48, C.byref(fh), C.byref(fw)) == ERR_INVALID_ARG
    assert (buf == 123.0).all()
    assert ctx.L.artp_cost_get_features_c(ctx.h, None, 64, C.byref(fh), C.byref(fw)) == 0 and (fh.value, fw.value) == (32, 32)
    ctx.close()


@pytest.mark.gpu
def test_gpu_learned_cost_roadmap_priced_by_the_full_network():
    """objective 2 (PRMMotionCostMaintainer::updateEdges) with the full network loaded, no other change: every priced edge's
    cost is the weighted chain sum of its sub-edges' own artp_cost_query rows (infinite past the risk threshold)."""
    import oracle_py as O
    from art_planner_amd.context import Context
    from art_planner_amd.roadmap import Roadmap
    from synthetic import make_map
    gm = make_map(200, 0.04, seed=5)
    ctx = Context(0, "yaml")
    ctx.upload_map(gm)
    se3 = ctx.sample_states(99, 0, 1 << 16)
    cand = se3[ctx.validate_states(se3) != 0]

    def near(x, y):
        return cand[np.argmin(np.hypot(cand[:, 0] - x, cand[:, 1] - y))]

    start, goal = near(gm.pos_x - 2.6, gm.pos_y - 2.6), near(gm.pos_x + 2.6, gm.pos_y + 2.6)
    ctx.cost_load_weights(cw.to_blob(_params_full()))
    elv = np.ascontiguousarray(gm["elevation"][::-1, ::-1]).astype(np.float32)
    ctx.cost_update_map(elv, gm.res, gm.len_x, gm.len_y, gm.pos_x, gm.pos_y)
    w, thr = (0.25, 1.0, 5.0), 0.55
    rm = Roadmap(ctx, start, goal, n_milestones=1200, seed=5, k_neighbors=60, objective=2, cost_weights=w, risk_threshold=thr)
    d = rm.export()
    V, E = d["verts"], d["edges"].astype(np.int64)

    def yaw(q):
        return np.float32(np.arctan2(2 * (q[3] * q[2] + q[0] * q[1]), 1 - 2 * (q[1] ** 2 + q[2] ** 2)))

    rows, owner = [], []
    sel = np.concatenate([np.nonzero(d["edge_interp"] > 0)[0][:400], np.nonzero(d["edge_interp"] == 0)[0][:400]])
    assert (d["edge_interp"][sel] > 0).sum() > 50
    for e in sel:
        a, b, ni = V[E[e, 0]], V[E[e, 1]], int(d["edge_interp"][e])
        pts = [a] + [O.interpolate(a, b, s / (ni + 1)) for s in range(1, ni + 1)] + [b]
        for s0, s1 in zip(pts[:-1], pts[1:]):
            rows.append([s1[0], s1[1], yaw(s1[3:]), s0[0], s0[1], yaw(s0[3:])])
            owner.append(e)
    c3 = ctx.cost_query(np.array(rows, np.float32)).astype(np.float64)
    owner = np.array(owner)
    for e in sel:
        r = c3[owner == e]
        ref = np.inf if (r[:, 2] > np.float32(thr)).any() else (r[:, 0] * np.float32(w[0]) + r[:, 1] * np.float32(w[1])
                                                                + r[:, 2] * np.float32(w[2])).sum()
        got = d["edge_cost"][e]
        assert (np.isinf(ref) and np.isinf(got)) or abs(got - ref) <= 1e-5 * max(1.0, abs(ref)), (e, got, ref)
    assert np.isfinite(d["edge_cost"]).any()
    path, cost, _ = rm.solve()
    if path is not None:
        assert np.isfinite(cost) and cost > 0
    rm.close()
    ctx.close()
