"""Validity entry points across map spacings and across map changes on one context (-m gpu), against the C oracle.

Every validity kernel sizes its LDS from the map's sample spacing (size_scratch): the window tile, the kept-triangle
list (at most 4096), the partner hash table and the dynamic LDS of the few-state, few-edge and resident kernels.  The
sweep runs every entry point from the finest spacing an upload accepts up to 0.3 m (foot windows of a cell or two), on
a map that holds a Perlin part, a ramp, terraces and a NaN margin, with random states and with torsos that graze the
ramp: their windows keep more triangles than the LDS list holds.  The map-change test installs maps of other spacings
on ONE context with persistent latency on, so that the resident kernels restart with another LDS size.

The oracle allocates its buffers per window, so it is exact at any spacing: labels must be BIT-EQUAL."""
import math

import numpy as np
import pytest

import common
import kept_triangles as KT
import oracle_py as O
from synthetic import GridMap, cumulative_distribution, perlin_terrain

ARTP_ERR_CAPACITY = -5
EXTENT = 9.6          # metres per side: at most 480 cells
RAMP_SLOPE = 0.3      # dh/dx of the ramp part
FEET_RAISE = -0.4     # the feet's layer over the ramp part, relative to the body's (the feet sit ~0.4 m lower)
SPACINGS = [0.025, 0.03, 0.035, 0.05, 0.07, 0.1, 0.2, 0.3]


# ---- maps -------------------------------------------------------------------------------------------------------------
def _diag(rob):
    t = math.sqrt(rob.torso_length ** 2 + rob.torso_width ** 2 + rob.torso_height ** 2)
    f = math.sqrt(rob.reach_x ** 2 + rob.reach_y ** 2 + rob.reach_z ** 2)
    return max(t, f)


def _maxdim(rob, n, res):
    """size_scratch's window tile for an n x n map of cell size res (sample spacing len / (n - 1) in float)."""
    s = float(np.float32(np.float32(n * res) / (np.float32(n) - np.float32(1.0))))
    return min(int(math.ceil(_diag(rob) / s)) + 4, n)


def finest_accepted(rob):
    """(n, res): the finest cell size of an EXTENT-wide map whose window tile still fits 64 samples, and one step finer."""
    d = _diag(rob)
    n = int(round(EXTENT / (d / 60.0)))
    res = EXTENT / n
    while _maxdim(rob, n, res) > 64:
        n -= 1
        res = EXTENT / n
    while _maxdim(rob, n + 1, EXTENT / (n + 1)) <= 64:
        n += 1
        res = EXTENT / n
    return n, res, n + 1, EXTENT / (n + 1)


def composite_map(n, res, seed=7, pos=(0.3, -0.2), cols=None):
    """One map, four kinds: a ramp (h = RAMP_SLOPE * x) over the half with y > pos_y, Perlin terrain and its
    terraces over the other half, a NaN margin (unknown space) around all of it.  Derived layers: elevation_masked =
    elevation (+ FEET_RAISE over the ramp), sampler layers from the elevation (normals, a probability that follows the terrain's smoothness)."""
    cols = cols or n
    gm = GridMap(n, cols, res, pos[0], pos[1])
    x = gm.cell_x()[:, None].astype(np.float64)
    y = gm.cell_y()[None, :].astype(np.float64)
    per = perlin_terrain(max(n, cols), res, seed, n_boxes=6)[:n, :cols].astype(np.float64)
    terr = np.round(per / 0.05) * 0.05
    h = np.where(y > pos[1], RAMP_SLOPE * x + 0 * y, np.where(x > pos[0], per, terr))
    m = max(2, int(round(0.4 / res)))
    if n > 4 * m and cols > 4 * m:
        h[:m, :] = np.nan
        h[-m:, :] = np.nan
        h[:, :m] = np.nan
        h[:, -m:] = np.nan
    h = h.astype(np.float32)
    gm.add("elevation", h)
    # the feet's layer lies FEET_RAISE off the ramp: a torso that grazes the ramp then has its feet on the ground, so
    # its state's label is the torso's verdict (and the batch pipeline does not skip the torso box)
    gm.add("elevation_masked", np.where(y > pos[1], h + np.float32(FEET_RAISE), h).astype(np.float32))
    hf = np.where(np.isfinite(h), h, 0.0).astype(np.float64)
    gx, gy = np.gradient(hf, res) if min(n, cols) > 1 else (np.zeros_like(hf), np.zeros_like(hf))
    nz = 1.0 / np.sqrt(1.0 + gx * gx + gy * gy)
    gm.add("normal_x", (-gx * nz).astype(np.float32))
    gm.add("normal_y", (-gy * nz).astype(np.float32))
    gm.add("normal_z", nz.astype(np.float32))
    gm.add("plane_fit_std_dev", np.full((n, cols), 0.01, np.float32))
    prob = np.where(np.isfinite(h), nz, 0.0).astype(np.float32)
    gm.add("sample_probability", prob)
    cp, cr = cumulative_distribution(prob)
    gm.layers["cum_prob"] = np.asfortranarray(cp)
    gm.layers["cum_prob_rowwise"] = np.ascontiguousarray(cr, np.float32)
    return gm


# ---- states -----------------------------------------------------------------------------------------------------------
def _quat_from_R(R):
    """(x, y, z, w) of a rotation matrix (Shepperd)."""
    t = np.trace(R)
    if t > 0:
        s = math.sqrt(t + 1.0) * 2
        return np.array([(R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s, 0.25 * s])
    i = int(np.argmax(np.diag(R)))
    j, k = (i + 1) % 3, (i + 2) % 3
    s = math.sqrt(1.0 + R[i, i] - R[j, j] - R[k, k]) * 2
    q = np.zeros(4)
    q[i] = 0.25 * s
    q[j] = (R[j, i] + R[i, j]) / s
    q[k] = (R[k, i] + R[i, k]) / s
    q[3] = (R[k, j] - R[j, k]) / s
    return q


def _rot(axis, a):
    c, s = math.cos(a), math.sin(a)
    if axis == 0:
        return np.array([[1, 0, 0], [0, c, -s], [0, s, c]])
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])


def grazing_states(gm, rob, n, rng, part="torso"):
    """States on the ramp part whose torso (part="torso") or feet (part="feet") box lies parallel to the ramp, yawed
    about 45 degrees, tilted against it by a fraction of a degree, its lowest corner a few mm above or below the ramp
    (the feet's: the feet's layer).
    A torso's window then keeps nearly every triangle, every triangle has coplanar partners, and no sample lies inside
    the box (the exact grouping decides)."""
    nrm = np.array([-RAMP_SLOPE, 0.0, 1.0]) / math.hypot(RAMP_SLOPE, 1.0)
    half = np.array([rob.torso_length, rob.torso_width, rob.torso_height]) / 2 if part == "torso" else \
        np.array([rob.reach_x, rob.reach_y, rob.reach_z]) / 2
    # the box's offset in the body frame, as the oracle places it (state = the feet plane, see random_states)
    poses, _ = O.OracleMap(gm).state_poses(rob, np.array([[gm.pos_x, gm.pos_y, 0.0, 0.0, 0.0, 0.0, 1.0]]))
    off = poses[0, 0 if part == "torso" else 1, :3].astype(np.float64) - [gm.pos_x, gm.pos_y, 0.0]
    corners = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]) * half
    out = np.empty((n, 7))
    m = 1.5 + 0.4                                                          # margin + half a torso
    for i in range(n):
        yaw = math.pi / 4 + rng.choice([0.0, math.pi / 2, math.pi, -math.pi / 2]) + rng.normal(0, 0.05)
        d = np.array([math.cos(yaw), math.sin(yaw), 0.0])
        e1 = d - d.dot(nrm) * nrm
        e1 /= np.linalg.norm(e1)
        R = np.stack([e1, np.cross(nrm, e1), nrm], axis=1) @ _rot(0, rng.normal(0, 0.004)) @ _rot(1, rng.normal(0, 0.004))
        px = gm.pos_x + rng.uniform(-gm.len_x / 2 + m, gm.len_x / 2 - m)
        py = gm.pos_y + rng.uniform(0.9, max(1.0, gm.len_y / 2 - m))
        on = np.array([px, py, RAMP_SLOPE * px + (FEET_RAISE if part == "feet" else 0.0)])
        delta = rng.uniform(-0.003, 0.006)
        low = (corners @ R.T @ nrm).min()
        centre = on + nrm * (delta - low)                                  # the box's lowest corner delta above the ramp
        out[i, :3] = centre - R @ off
        out[i, 3:] = _quat_from_R(R)
    return out


def kept_counts(gm, rob, se3):
    """Kept triangles of every state's torso window (numpy, the rule of grp_compact_triangles)."""
    om = O.OracleMap(gm)
    poses, inside = om.state_poses(rob, se3)
    return np.array([KT.kept_triangles(om.body, rob.torso, poses[i, 0]) if inside[i, 0] else 0
                     for i in range(len(se3))])


# ---- the entry points -------------------------------------------------------------------------------------------------
def _ctx(rob_kind):
    from art_planner_amd.context import Context
    return Context(0, rob_kind)


def _near(se3, rng, step):
    """Edge end points a short way from se3 (keeps the oracle's per-edge state count small)."""
    s2 = se3.copy()
    s2[:, :2] += rng.normal(0, step, (len(se3), 2))
    s2[:, 2] += rng.normal(0, step / 4, len(se3))
    q = s2[:, 3:] + rng.normal(0, 0.05, (len(se3), 4))
    s2[:, 3:] = q / np.linalg.norm(q, axis=1, keepdims=True)
    return s2


def run_entry_points(ctx, gm, rob, states, edges, n_sample=3000, tag=""):
    """Every validity entry point of ctx on (states, edges); returns a dict of results.  ctx has gm installed."""
    import torch
    s1, s2 = edges
    out = {}
    ctx.set_persistent_latency(False)
    out["host"] = ctx.validate_states(states)
    t = torch.from_numpy(np.ascontiguousarray(states)).cuda()
    v = torch.empty(len(states), dtype=torch.uint8, device="cuda")
    ctx.validate_states_dev(t, v)
    ctx.synchronize()
    out["dev"] = v.cpu().numpy()
    k = min(len(states), 320)
    out["few"] = np.concatenate([ctx.validate_states(states[i:i + 16]) for i in range(0, k, 16)])
    out["sample"] = ctx.sample_and_validate(11, 777, n_sample)
    ctx.set_few_edges(True)
    out["edges"] = ctx.check_motions(s1, s2)
    m = min(len(s1), 384)
    out["few_edges"] = np.concatenate([ctx.check_motions(s1[i:i + 64], s2[i:i + 64]) for i in range(0, m, 64)])
    out["interp"] = ctx.check_edges_interp(s1[:1500], s2[:1500])
    ctx.set_persistent_latency(True)
    q = min(len(states), 64)
    svc = []
    i = 0
    while i < q:
        w = 1 + (i // 3) % 2
        svc.append(ctx.validate_states(states[i:i + w]))
        i += w
    out["svc"] = np.concatenate(svc)
    pool = []
    i = 0
    while i < 48:
        w = 1 + (i // 3) % 2
        pool.append(ctx.check_motions(s1[i:i + w], s2[i:i + w]))
        i += w
    out["pool"] = np.concatenate(pool)
    st = ctx.persistent_latency_stats()
    assert st["requests"] > 0, f"{tag}: the resident kernels were not used"
    ctx.set_persistent_latency(False)
    return out


def oracle_answers(gm, rob, states, edges, n_sample=3000):
    s1, s2 = edges
    om = O.OracleMap(gm)
    valid = om.states_valid(rob, states)
    so, _ = O.OracleSampler(gm).sample(rob, 11, 777, n_sample)
    return {"valid": valid, "sample_se3": so, "sample_valid": om.states_valid(rob, so),
            "edges": om.check_motions(rob, s1, s2)[0], "interp": om.edges_interp_valid(rob, s1[:1500], s2[:1500])}


def assert_matches_oracle(got, ref, tag):
    def eq(a, b, what):
        a, b = np.asarray(a), np.asarray(b)
        assert a.shape == b.shape and np.array_equal(a, b), f"{tag}: {what}: {int((a != b).sum())} of {b.size} differ"
    v = ref["valid"]
    eq(got["host"], v, "validate_states (host)")
    eq(got["dev"], v, "validate_states_dev")
    eq(got["few"], v[:len(got["few"])], "few-state path")
    eq(got["svc"], v[:len(got["svc"])], "resident service")
    se3, sv = got["sample"]
    assert np.abs(se3 - ref["sample_se3"]).max() < 1e-12, f"{tag}: sampled states differ"
    eq(sv, ref["sample_valid"], "sample_and_validate")
    e = ref["edges"]
    eq(got["edges"], e, "check_motions (batch)")
    eq(got["few_edges"], e[:len(got["few_edges"])], "few-edge path")
    eq(got["pool"], e[:len(got["pool"])], "resident edge pool")
    eq(got["interp"][0], ref["interp"][0], "check_edges_interp verdicts")
    eq(got["interp"][1], ref["interp"][1], "check_edges_interp counts")


def make_inputs(gm, rob, seed, n_random=2500, n_graze=400, n_edges=4200):
    rng = np.random.default_rng(seed)
    rs = common.random_states(gm, n_random, rng, z_off=(0.02, 0.1), tilt=0.2, spread=0.5)
    gt = grazing_states(gm, rob, n_graze, rng, "torso")
    gf = grazing_states(gm, rob, n_graze // 4, rng, "feet")
    # interleaved, so that every prefix (few-state, service) holds grazing states too
    states = np.empty((len(rs) + len(gt) + len(gf), 7))
    states[0::2][:len(gt) + len(gf)] = np.concatenate([gt, gf])
    rest = np.ones(len(states), bool)
    rest[0::2][:len(gt) + len(gf)] = False
    states[rest] = rs
    base = np.concatenate([states, states])[:n_edges]
    s2 = _near(base, rng, 0.15)
    return states, gt, (base, s2)


# ---- tests ------------------------------------------------------------------------------------------------------------
def test_kept_triangle_helper_matches_the_oracle():
    """The numpy kept-triangle count equals the oracle's (artp_oracle_last_num_tri) for every box that reaches the
    triangle stage, on a ramp, a Perlin map with NaN holes and terraces, at three spacings."""
    import ctypes as C
    L = O.lib()
    L.artp_oracle_last_num_tri.restype = C.c_uint
    rob = O.robot("yaml")
    reached = 0
    for res in (0.03, 0.05, 0.1):
        gm = composite_map(int(round(6.0 / res)), res, seed=3)
        om = O.OracleMap(gm)
        rng = np.random.default_rng(1)
        se3 = np.concatenate([grazing_states(gm, rob, 20, rng), common.random_states(gm, 60, rng)])
        poses, inside = om.state_poses(rob, se3)
        for i in range(len(se3)):
            if not inside[i, 0]:
                continue
            _, ec, _ = om.body.check_boxes(rob.torso, poses[i, 0][None], want_detail=True)
            if ec[0] not in (6, 8):      # EXIT_PLANE / EXIT_NONE: the triangle list was built
                continue
            reached += 1
            assert KT.kept_triangles(om.body, rob.torso, poses[i, 0]) == L.artp_oracle_last_num_tri(), (res, i)
    assert reached >= 30


def test_grazing_torsos_overflow_the_lds_list_at_fine_spacings():
    """The constructed set reaches the edge it is built for: below ~0.031 m (YAML robot) torso windows on the ramp keep
    more than 4096 triangles; at 0.05 m none does."""
    rob = O.robot("yaml")
    rng = np.random.default_rng(2)
    gm = composite_map(int(round(EXTENT / 0.025)), EXTENT / round(EXTENT / 0.025))
    kc = kept_counts(gm, rob, grazing_states(gm, rob, 40, rng))
    assert (kc > KT.LDS_LIST_CAP).mean() > 0.5, kc
    gm = composite_map(int(round(EXTENT / 0.05)), 0.05)
    assert kept_counts(gm, rob, grazing_states(gm, rob, 40, rng)).max() <= KT.LDS_LIST_CAP


@pytest.mark.gpu
@pytest.mark.parametrize("rname", ["yaml", "defaults"])
def test_upload_accepts_the_finest_fitting_spacing_and_refuses_the_next(rname):
    rob = O.robot(rname)
    n, res, n2, res2 = finest_accepted(rob)
    ctx = _ctx(rname)
    ctx.upload_map(composite_map(n, res), sampler=False)
    gm2 = composite_map(n2, res2)
    rc = ctx.L.artp_upload_layer(ctx.h, 0, np.asfortranarray(gm2["elevation"]).ctypes.data, n2, n2, gm2.len_x,
                                 gm2.len_y, gm2.pos_x, gm2.pos_y)
    assert rc == ARTP_ERR_CAPACITY, rc
    ctx.close()


def _sweep_points():
    pts = []
    for rname in ("yaml", "defaults"):
        n, res, _, _ = finest_accepted(O.robot(rname))
        pts.append((rname, n, res))
        for s in SPACINGS:
            if s >= res:
                pts.append((rname, int(round(EXTENT / s)), EXTENT / round(EXTENT / s)))
    return pts


@pytest.mark.gpu
@pytest.mark.parametrize("rname,n,res", _sweep_points(), ids=lambda v: f"{v:.4f}" if isinstance(v, float) else str(v))
def test_resolution_sweep(rname, n, res):
    """Every validity entry point equals the oracle at this spacing: validate_states (host, > 16 states, and _dev),
    the few-state path, the resident service, sample_and_validate, check_motions (two-pass batch, few-edge, resident
    pool) and check_edges_interp.  At the spacings where grazing torsos keep more than 4096 triangles, those boxes
    really reach the exact grouping."""
    rob = O.robot(rname)
    gm = composite_map(n, res, seed=11)
    states, graze, edges = make_inputs(gm, rob, seed=int(res * 1e4))
    ref = oracle_answers(gm, rob, states, edges)
    ctx = _ctx(rname)
    ctx.upload_map(gm)
    got = run_entry_points(ctx, gm, rob, states, edges, tag=f"{rname}@{res:.4f}")
    assert_matches_oracle(got, ref, f"{rname}@{res:.4f}")
    kc = kept_counts(gm, rob, graze[:60])
    if res < 0.03 and rname == "yaml" or res < 0.024:
        assert (kc > KT.LDS_LIST_CAP).any(), kc.max()
    if kc.max() > 1024:
        # the long lists go through the exact-grouping stage of the batch pipeline
        ctx.validate_states(graze)
        assert ctx.pipeline_counters()["exact_grouping"] > 0
    # torso boxes alone through artp_check_boxes (wave_check_box): hits and misses, equal to the oracle's
    om = O.OracleMap(gm)
    poses, inside = om.state_poses(rob, graze)
    tp = poses[inside[:, 0] != 0, 0]
    want = om.body.check_boxes(rob.torso, tp)
    assert np.array_equal(ctx.check_boxes(0, rob.torso, tp), want)
    assert 0 < want.mean() < 1
    assert 0 < ref["valid"].mean() < 1
    ctx.close()


@pytest.mark.gpu
def test_map_changes_on_one_context_with_persistent_latency():
    """One context, persistent latency on, maps of other spacings installed one after the other (0.1 m, 0.04 m, the
    finest accepted, 0.3 m, a non-square 0.04 m map at another origin).  After each install every entry point equals the
    oracle and a fresh context given the same map; the resident kernels restart with the LDS of the NEW map."""
    rob = O.robot("yaml")
    nf, rf, _, _ = finest_accepted(rob)
    maps = [composite_map(96, 0.1, seed=21), composite_map(240, 0.04, seed=22), composite_map(nf, rf, seed=23),
            composite_map(32, 0.3, seed=24), composite_map(200, 0.04, seed=25, pos=(-2.5, 3.0), cols=280)]
    ctx = _ctx("yaml")
    ctx.set_persistent_latency(True)
    for k, gm in enumerate(maps):
        tag = f"map {k} ({gm.rows}x{gm.cols} @ {gm.res:.4f})"
        states, graze, edges = make_inputs(gm, rob, seed=100 + k, n_random=1200, n_graze=200, n_edges=4100)
        ref = oracle_answers(gm, rob, states, edges, n_sample=2000)
        ctx.upload_map(gm)
        got = run_entry_points(ctx, gm, rob, states, edges, n_sample=2000, tag=tag)
        # persistent latency stays on between maps: the first calls after the install restart the resident kernels
        ctx.set_persistent_latency(True)
        one = np.concatenate([ctx.validate_states(states[i:i + 1]) for i in range(8)])
        two = np.concatenate([ctx.check_motions(edges[0][i:i + 2], edges[1][i:i + 2]) for i in range(0, 8, 2)])
        assert np.array_equal(one, ref["valid"][:8]), tag
        assert np.array_equal(two, ref["edges"][:8]), tag
        assert_matches_oracle(got, ref, tag)
        fresh = _ctx("yaml")
        fresh.upload_map(gm)
        got_f = run_entry_points(fresh, gm, rob, states, edges, n_sample=2000, tag=tag + " fresh")
        for key in got:
            a, b = got[key], got_f[key]
            if isinstance(a, tuple):
                assert all(np.array_equal(x, y) for x, y in zip(a, b)), (tag, key)
            else:
                assert np.array_equal(a, b), (tag, key)
        fresh.close()
        ctx.set_persistent_latency(True)
    ctx.close()


@pytest.mark.gpu
def test_two_contexts_on_different_spacings_interleave():
    """The dynamic-LDS opt-in belongs to the kernel, not to the context: a context on a fine map keeps working after
    another context uploads a coarse map, through every path (batch, few-state, service, few-edge, pool)."""
    rob = O.robot("yaml")
    nf, rf, _, _ = finest_accepted(rob)
    fine, coarse = composite_map(nf, rf, seed=31), composite_map(32, 0.3, seed=32)
    a, b = _ctx("yaml"), _ctx("yaml")
    a.upload_map(fine)
    states, _, edges = make_inputs(fine, rob, seed=33, n_random=600, n_graze=100, n_edges=4100)
    ref = oracle_answers(fine, rob, states, edges, n_sample=1000)
    a.set_persistent_latency(True)
    a.validate_states(states[:1])
    b.upload_map(coarse)
    b.set_persistent_latency(True)
    b.validate_states(states[:1])
    b.check_motions(edges[0][:1], edges[1][:1])
    a.upload_map(fine)        # a map write: a's resident kernels restart
    b.upload_map(coarse)      # ... after b has asked for less LDS again
    got = run_entry_points(a, fine, rob, states, edges, n_sample=1000, tag="fine after coarse")
    assert_matches_oracle(got, ref, "fine after coarse")
    a.close()
    b.close()
