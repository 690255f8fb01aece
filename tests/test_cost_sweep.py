"""The motion-cost feature extractor at every kernel form it ships (GPU).

cost_run_cnn (artp_capi.hip) picks conv345_kernel's tile edge (12 / 16 / 18) and the 15 x 15 layer's form (8-row tiles in
512-thread workgroups, or 8-, 9- or 10-row tiles in 256-thread ones; the full-width network: 8 / 512 or 6 / 256) from the
map size and the device's CU count.  The sweep searches shapes that reach every form on THIS device, confirms each with
artp_cost_debug_forms, and holds the features on probe parameters to the exact restatement of tests/cost_exact_ref.py bit
for bit, on the seeded random parameters to the existing tolerance bars, plus the query geometry, both entry points, one
context's buffers across shrinking, growing and transposed maps, and the size limits."""
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import common

sys.path.insert(0, os.path.join(common.ROOT, "oracle"))
sys.path.insert(0, os.path.join(common.ROOT, "tools"))
import convert_weights as cw  # noqa: E402
import cost_exact_ref as R  # noqa: E402
import motion_cost_oracle as mo  # noqa: E402
from test_cost_exact_ref import MIN_BRANCH_RATE  # noqa: E402
from test_motion_cost import _assert_features_close  # noqa: E402

pytestmark = pytest.mark.gpu

RES = 0.04
ERR_INVALID_ARG = -1
PROBES = [("positive", "dense"), ("mixed", "impulse"), ("mixed", "signed")]   # (parameter set, map)


def _cdiv(a, b):
    return -(-a // b)


def expected_forms(H, W, ncu, net):
    """cost_run_cnn's / cost_run_cnn_full's choice restated: (net, conv345 tile edge, 15 x 15 tile rows, its threads)."""
    h5, w5 = (H - 4) // 2 - 8, (W - 4) // 2 - 8
    hf, wf = h5 - 14, w5 - 14
    tiles8 = _cdiv(wf, 16) * _cdiv(hf, 8)
    if net == 2:
        return (2, 12, 8, 512) if tiles8 <= ncu else (2, 12, 6, 256)

    def rounds_cost(t):
        return _cdiv(_cdiv(w5, t) * _cdiv(h5, t), ncu) * (t + 8) ** 2
    t_best = 16
    for t in (12, 18):
        if rounds_cost(t) < rounds_cost(t_best):
            t_best = t
    if tiles8 <= ncu:
        return (1, t_best, 8, 512)
    best, best_cost = 8, None
    for tr in (8, 9, 10):
        c = _cdiv(_cdiv(wf, 16) * _cdiv(hf, tr), 2 * ncu) * tr
        if best_cost is None or c < best_cost:
            best, best_cost = tr, c
    return (1, t_best, best, 256)


WANTED = [(1, "tile", 12), (1, "tile", 16), (1, "tile", 18), (1, "rows", (8, 512)), (1, "rows", (8, 256)),
          (1, "rows", (9, 256)), (1, "rows", (10, 256)), (2, "rows", (8, 512)), (2, "rows", (6, 256))]


def _form_keys(f):
    return [(f[0], "tile", f[1]), (f[0], "rows", (f[2], f[3]))]


def sweep_shapes(ncu):
    """The smallest non-square shape that reaches each wanted form (tall and wide in turn), then the edge shapes."""
    cands = sorted({(h, w) for h in range(54, 1400) for w in (h + 17, h - 17, h + 1) if w >= 54},
                   key=lambda s: (s[0] * s[1], s))
    chosen = []
    for i, want in enumerate(WANTED):
        for s in cands:
            if (s[0] < s[1]) == (i % 2 == 0) and want in _form_keys(expected_forms(*s, ncu, want[0])):
                chosen.append(s)                          # wide and tall in turn: both orientations
                break
        else:
            raise AssertionError(f"no shape reaches {want} on {ncu} CUs")
    edges = [(54, 54), (54, 55), (55, 54), (97, 800), (800, 97), (500, 500), (800, 800), (121, 96), (96, 121)]
    # wf mod 16 = 1 and 15, hf mod (the 15 x 15 tile height) = 1 and tile - 1
    for cond in (lambda hf, wf, tr: wf % 16 == 1, lambda hf, wf, tr: wf % 16 == 15,
                 lambda hf, wf, tr: hf % tr == 1, lambda hf, wf, tr: hf % tr == tr - 1):
        for n in range(60, 200):
            s = (n, n + 3)
            hf, wf = R.feature_shape(*s)
            if cond(hf, wf, expected_forms(*s, ncu, 1)[2]):
                edges.append(s)
                break
    out = []
    for s in chosen + edges:
        if s not in out:
            out.append(s)
    return out


@pytest.fixture(scope="module")
def device():
    import torch
    from art_planner_amd.context import Context
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    shapes = sweep_shapes(ncu)
    probes = {(net, kind): R.probe_params(net, kind) for net in (1, 2) for kind in ("positive", "mixed")}
    real = {net: mo.random_params(0, R.shapes_of(net)) for net in (1, 2)}
    blobs = {k: cw.to_blob(p) for k, p in list(probes.items()) + [((net, "real"), p) for net, p in real.items()]}
    ctx = Context(0, "yaml")
    yield {"ncu": ncu, "shapes": shapes, "probes": probes, "real": real, "blobs": blobs, "ctx": ctx}
    ctx.close()


def _compute(jobs):
    def run(key):
        p, m, exact = jobs[key]
        st = {}
        f = R.restate(p, m, round_half=exact, stats=st)
        return key, f, st
    with ThreadPoolExecutor(4) as ex:     # numpy and torch release the GIL
        return {k: (f, st) for k, f, st in ex.map(run, list(jobs))}


@pytest.fixture(scope="module")
def exact_refs(device):
    """Every (shape, network, probe set) exact restatement, computed once."""
    return _compute({(s, net, kind, mk): (device["probes"][(net, kind)], R.probe_map(mk, *s), True)
                     for s in device["shapes"] for net in (1, 2) for kind, mk in PROBES})


@pytest.fixture(scope="module")
def real_refs(device):
    """Every (shape, network) float64 feature map of the seeded random parameters, computed once."""
    return _compute({(s, net): (device["real"][net], _terrain(*s), False) for s in device["shapes"] for net in (1, 2)})


def _terrain(H, W):
    """A smooth terrain with steps, rounded to fp16 (the device's input rounding), as in test_motion_cost."""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    t = 0.4 * np.sin(x / 9.0) * np.cos(y / 13.0) + 0.25 * ((x + 2 * y) % 37 > 20) + 0.002 * ((x * 7 + y * 3) % 11)
    return t.astype(np.float16).astype(np.float32)


def _update(ctx, m, cx=0.0, cy=0.0, res=RES):
    ctx.cost_update_map(np.ascontiguousarray(m, np.float32), res, m.shape[0] * res, m.shape[1] * res, cx, cy)


def _edges(H, W, n, seed, cx=0.0, cy=0.0, res=RES):
    """n edges whose starts cover the whole map and 15 % beyond each side (both clamps)."""
    rng = np.random.default_rng(seed)
    Lx, Ly = H * res, W * res
    s = np.stack([rng.uniform(-0.65 * Lx, 0.65 * Lx, n) + cx, rng.uniform(-0.65 * Ly, 0.65 * Ly, n) + cy], 1)
    d = rng.uniform(-0.6, 0.6, (n, 2))
    return np.stack([s[:, 0] + d[:, 0], s[:, 1] + d[:, 1], rng.uniform(-np.pi, np.pi, n), s[:, 0], s[:, 1],
                     rng.uniform(-np.pi, np.pi, n)], 1).astype(np.float32)


def _hwc(ref_chw):
    return np.transpose(ref_chw, (1, 2, 0)).astype(np.float32)


def test_every_shipped_form_is_reached(device):
    """Each wanted form is reported by artp_cost_debug_forms at some sweep shape, and the report is cost_run_cnn's rule."""
    ctx, seen, table = device["ctx"], set(), []
    for net in (1, 2):
        ctx.cost_load_weights(device["blobs"][(net, "mixed")])
        for s in device["shapes"]:
            _update(ctx, R.probe_map("signed", *s))
            f = ctx.cost_debug_forms()
            got = (f["net"], f["c345_tile"], f["conv15_rows"], f["conv15_threads"])
            assert got == expected_forms(*s, device["ncu"], net), (s, net, got)
            seen.update(_form_keys(got))
            table.append((s, got))
    missing = [w for w in WANTED if w not in seen]
    assert not missing, (device["ncu"], missing)
    print(f"\n{device['ncu']} CUs: " + "; ".join(f"{h}x{w} -> {g}" for (h, w), g in table))


@pytest.mark.parametrize("net", [1, 2])
def test_exact_probe_features_are_bit_equal_at_every_shape(device, exact_refs, net):
    """Every sweep shape, every probe set: the device's features are the exact restatement, bit for bit."""
    ctx, bad = device["ctx"], []
    for kind in ("positive", "mixed"):
        ctx.cost_load_weights(device["blobs"][(net, kind)])
        for s in device["shapes"]:
            for k2, mk in PROBES:
                if k2 != kind:
                    continue
                ref, st = exact_refs[(s, net, kind, mk)]
                if kind == "mixed":
                    assert all(v["neg"] >= MIN_BRANCH_RATE and v["pos"] >= MIN_BRANCH_RATE for v in st.values()), (s, st)
                _update(ctx, R.probe_map(mk, *s))
                f = ctx.cost_features()
                r = _hwc(ref)
                assert f.shape == r.shape, (s, f.shape, r.shape)
                if not np.array_equal(f, r):
                    diff = np.argwhere(f != r)
                    bad.append((s, kind, mk, len(diff), tuple(diff[0]), tuple(diff[-1]), float(f[tuple(diff[0])]),
                                float(r[tuple(diff[0])])))
    assert not bad, bad


@pytest.mark.parametrize("net", [1, 2])
def test_random_params_features_and_costs_at_every_shape(device, real_refs, net):
    """The seeded random parameters at every sweep shape: features within the existing bar of the float64 network, and
    20 000 edge costs (the whole map and both clamps) on the device's own features within 5e-5 of motion_cost_oracle."""
    ctx = device["ctx"]
    ctx.cost_load_weights(device["blobs"][(net, "real")])
    p = device["real"][net]
    for i, s in enumerate(device["shapes"]):
        m = _terrain(*s)
        _update(ctx, m)
        f = ctx.cost_features()
        _assert_features_close(f, real_refs[(s, net)][0].astype(np.float32), f"{s} net {net}")
        e = _edges(*s, 20000, seed=i)
        c = ctx.cost_query(e)
        co = mo.fc_costs(p, np.transpose(f, (2, 0, 1)), e, RES, s[0] * RES, s[1] * RES)
        assert np.abs(c - co).max() < 5e-5, (s, float(np.abs(c - co).max()))


@pytest.mark.parametrize("res", [0.02, 0.04, 0.1, 0.3])
@pytest.mark.parametrize("centre", [(0.0, 0.0), (3.7, -1.25), (1000.3, -2500.7)])
def test_query_cells_equal_the_oracle(device, res, centre):
    """cost_query_cells against motion_cost_oracle.query_cells, bit for bit: non-square feature maps, a map centre away
    from the origin (a large one included), starts on feature-cell borders +- 1 float32 ulp after the centre shift, and
    starts far outside the map on every side."""
    ctx = device["ctx"]
    ctx.cost_load_weights(device["blobs"][(1, "real")])
    cx, cy = centre
    for H, W in ((131, 110), (110, 131)):
        _update(ctx, _terrain(H, W), cx, cy, res)
        F = R.feature_shape(H, W)
        Lx, Ly = H * res, W * res
        fr = 2 * res
        rb, cb = int((Lx / res - 48) / 2 * 0.5), int((Ly / res - 48) / 2 * 0.5)
        k = np.arange(-3, max(F) + 3, dtype=np.float64)
        bx = (cx + (k - rb) * fr).astype(np.float32)
        by = (cy + (k - cb) * fr).astype(np.float32)
        n = min(len(bx), len(by))
        sx = np.concatenate([bx, np.nextafter(bx, np.float32(np.inf)), np.nextafter(bx, np.float32(-np.inf)),
                             np.float32([cx - 1e4, cx + 1e4, cx])])
        j = np.arange(len(bx)) % n
        sy = np.concatenate([by[j], np.nextafter(by, np.float32(-np.inf))[j][::-1], np.nextafter(by, np.float32(np.inf))[j],
                             np.float32([cy + 1e4, cy - 1e4, cy])])
        e = np.zeros((len(sx), 6), np.float32)
        e[:, 3], e[:, 4] = sx, sy
        e[:, 0], e[:, 1] = sx + 0.1, sy - 0.1
        rng = np.random.default_rng(5)
        e2 = _edges(H, W, 4000, 11, cx, cy, res)
        far = rng.uniform(-1e4, 1e4, (200, 1)).astype(np.float32)   # far outside, both clamps (the target moves along)
        e2[:100, [0, 3]] += far[:100]
        e2[100:200, [1, 4]] += far[100:]
        e = np.concatenate([e, e2])
        rows, cols = ctx.cost_query_cells(e)
        r, c = mo.query_cells(e, res, Lx, Ly, F, cx, cy)
        assert np.array_equal(rows, r) and np.array_equal(cols, c), (H, W, res, centre, int((rows != r).sum()), int((cols != c).sum()))
        assert rows.min() == 1 and rows.max() == F[0] - 2 and cols.min() == 1 and cols.max() == F[1] - 2
        # and the costs with a centre: the oracle on the device's own features
        f = ctx.cost_features()
        cst = ctx.cost_query(e2)
        co = mo.fc_costs(device["real"][1], np.transpose(f, (2, 0, 1)), e2, res, Lx, Ly, cx, cy)
        assert np.abs(cst - co).max() < 5e-5, float(np.abs(cst - co).max())


def test_device_entry_points_equal_the_host_ones(device):
    """artp_cost_update_map_dev on a torch tensor and artp_cost_query_dev give the host forms' bits, both networks."""
    import torch
    from art_planner_amd.context import Context
    for net in (1, 2):
        a, b = Context(0, "yaml"), Context(0, "yaml")
        for c in (a, b):
            c.cost_load_weights(device["blobs"][(net, "real")])
        H, W = 233, 190
        m = _terrain(H, W)
        _update(a, m, 1.5, -2.0)
        t = torch.from_numpy(m).cuda()
        torch.cuda.synchronize()
        b.cost_update_map_dev(t, RES, H * RES, W * RES, 1.5, -2.0)
        b.synchronize()
        assert np.array_equal(a.cost_features(), b.cost_features())
        assert a.cost_debug_forms() == b.cost_debug_forms()
        e = _edges(H, W, 5000, 3, 1.5, -2.0)
        ch = a.cost_query(e)
        et = torch.from_numpy(e).cuda()
        out = torch.full((len(e), 3), float("nan"), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        b.cost_query_dev(et, out)
        b.synchronize()
        assert np.array_equal(out.cpu().numpy(), ch)
        a.close()
        b.close()


SEQUENCE = [(800, 800), (54, 54), (97, 800), (800, 97), (500, 500)]


def test_one_context_reuses_its_buffers_across_shapes_and_networks(device):
    """One context: 800^2 -> 54^2 -> 97 x 800 -> 800 x 97 -> 500^2 with the light network, then the full one and the same
    sequence.  Each step's features, costs and forms are the bits of a fresh context given that shape alone (d_act is
    zeroed only when allocated, d_feat never: nothing of an earlier map may leak into a later one)."""
    from art_planner_amd.context import Context
    ctx = Context(0, "yaml")
    for net in (1, 2):
        ctx.cost_load_weights(device["blobs"][(net, "real")])
        for i, s in enumerate(SEQUENCE):
            m = _terrain(*s) + np.float32(0.25 * i)
            e = _edges(*s, 4096, 100 + i)
            _update(ctx, m)
            f, c, fm = ctx.cost_features(), ctx.cost_query(e), ctx.cost_debug_forms()
            fresh = Context(0, "yaml")
            fresh.cost_load_weights(device["blobs"][(net, "real")])
            _update(fresh, m)
            assert np.array_equal(f, fresh.cost_features()), (net, s)
            assert np.array_equal(c, fresh.cost_query(e)), (net, s)
            assert fm == fresh.cost_debug_forms(), (net, s)
            fresh.close()
    ctx.close()


@pytest.mark.parametrize("net", [1, 2])
def test_size_limits(device, net):
    """53 rows or 53 columns are refused with ARTP_ERR_INVALID_ARG; the refused update changes nothing a query sees.
    54 x 54 (a 3 x 3 feature map) is accepted and every query gathers cell (1, 1)."""
    from art_planner_amd._capi import ArtpError
    from art_planner_amd.context import Context
    ctx = Context(0, "yaml")
    ctx.cost_load_weights(device["blobs"][(net, "real")])
    H, W = 140, 121
    _update(ctx, _terrain(H, W), 0.7, -0.3)
    e = _edges(H, W, 3000, 9, 0.7, -0.3)
    before = (ctx.cost_features(), ctx.cost_query(e), ctx.cost_query_cells(e), ctx.cost_debug_forms())
    for s in ((53, 54), (54, 53), (53, 53), (53, 400), (400, 53)):
        with pytest.raises(ArtpError) as ei:
            _update(ctx, _terrain(*s) + np.float32(1), 5.0, 5.0, 0.1)
        assert ei.value.status == ERR_INVALID_ARG, (s, ei.value.status)
        after = (ctx.cost_features(), ctx.cost_query(e), ctx.cost_query_cells(e), ctx.cost_debug_forms())
        assert np.array_equal(after[0], before[0]) and np.array_equal(after[1], before[1])
        assert np.array_equal(after[2][0], before[2][0]) and np.array_equal(after[2][1], before[2][1])
        assert after[3] == before[3]
    _update(ctx, _terrain(54, 54))
    assert ctx.cost_features().shape[:2] == (3, 3)
    e = _edges(54, 54, 2000, 10)
    rows, cols = ctx.cost_query_cells(e)
    assert (rows == 1).all() and (cols == 1).all()
    ctx.close()
