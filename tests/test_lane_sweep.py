"""Every front end on lanes 1 to 3 (artp_set_lane): a context's lanes own their stream, counters and scratch, and since
the lanes became one lane_state every front end reaches them through ctx->lane.

A scenario is a function of (ctx, step): step() moves to the lane the plan gives the next step, waits for everything
queued so far (a _dev result made on one lane and read on another is the caller's to order), and the scenario then issues
one call.  sweep() runs the scenario on a fresh context with every step on lane 0 (once per scenario), then on another
fresh context under the lane plan, and compares everything the scenario returns byte for byte: every front end here is
deterministic.  Before a lane-plan run lane 2 gets live buffers -- a 65-state validate_states batch and a whole-map
reachability_map at 16 headings on the 97 x 61 map -- and answers the same two calls again afterwards: the same bytes.

Lane plans: all steps on lane 1, all on lane 3, alternating 1, 3, 1, 3.  The lane-0 run of every scenario is tied to the
project's references where the scenario's module has one (step.baseline), and the conditions a scenario needs of its
inputs are asserted on the inputs before the device runs."""
import os
import sys

import numpy as np
import pytest

import common
import oracle_py as O
import preprocess_restated as P
from test_lane_order import GEOM, POS, sampler_inputs

sys.path.insert(0, os.path.join(common.ROOT, "oracle"))
sys.path.insert(0, os.path.join(common.ROOT, "tools"))
import motion_cost_oracle as mo  # noqa: E402
import convert_weights as cw  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PLANS = {
    "lane1": lambda i: 1,
    "lane3": lambda i: 3,
    "alternating": lambda i: (1, 3)[i % 2],
}


# ---- the helper -----------------------------------------------------------------------------------------------------------
class Step:
    def __init__(self, ctx, lane_of, baseline):
        self.ctx, self.lane_of, self.baseline, self.i, self.lanes = ctx, lane_of, baseline, 0, []

    def __call__(self):
        self.ctx.synchronize()
        lane = self.lane_of(self.i)
        self.ctx.set_lane(lane)
        assert self.ctx.lane == lane
        self.lanes.append(lane)
        self.i += 1


def flat(obj, path="r"):
    """Everything a scenario returned as (where, bytes) pairs."""
    if isinstance(obj, dict):
        return [p for k in sorted(obj) for p in flat(obj[k], f"{path}.{k}")]
    if isinstance(obj, (list, tuple)):
        return [p for i, v in enumerate(obj) for p in flat(v, f"{path}[{i}]")]
    if obj is None:
        return [(path, b"None")]
    if hasattr(obj, "cpu"):
        obj = obj.cpu().numpy()
    a = np.ascontiguousarray(obj)
    return [(path, str(a.dtype).encode() + str(a.shape).encode() + a.tobytes())]


def _lane2(ctx):
    """Lane 2's two calls on the 97 x 61 map; leaves the context on lane 0."""
    gm = sampler_inputs()["old"]
    ctx.synchronize()
    ctx.set_lane(2)
    ctx.upload_map(gm)
    se3 = common.random_states(gm, 65, np.random.default_rng(31))
    out = [ctx.validate_states(se3), ctx.reachability_map(16)]
    ctx.set_lane(0)
    return out


_BASELINE = {}


def _run(scenario, lane_of, baseline):
    from art_planner_amd.context import Context
    ctx = Context(0, "yaml")
    try:
        first = None if baseline else _lane2(ctx)
        step = Step(ctx, lane_of, baseline)
        out = flat(scenario(ctx, step))
        ctx.synchronize()
        assert step.i >= 2 and set(step.lanes) == ({0} if baseline else {lane_of(i) for i in range(step.i)})
        if first is not None:
            again = _lane2(ctx)
            assert flat(again) == flat(first), "lane 2's answers changed after the other lanes ran"
            assert 0 < first[0].sum() < 65 and first[1].any()
    finally:
        ctx.close()
    return out


def sweep(name, plan):
    if name not in _BASELINE:               # the lane-0 run: once per scenario, shared by the three plans
        _BASELINE[name] = _run(SCENARIOS[name], lambda i: 0, True)
    base = _BASELINE[name]
    got = _run(SCENARIOS[name], PLANS[plan], False)
    assert [p for p, _ in got] == [p for p, _ in base]
    bad = [p for (p, a), (_, b) in zip(base, got) if a != b]
    assert not bad, f"{len(bad)} of {len(base)} results differ from the lane-0 run: {bad[:8]}"


def _bits(d):
    return np.ascontiguousarray(d).view(np.uint64)


# ---- 1. reachability ------------------------------------------------------------------------------------------------------
REACH_RECT = (13, 9, 41, 33)


def reachability(ctx, step):
    from test_reachability import check_every_label
    gm = sampler_inputs()["old"]
    n_yaw = 7
    for rect in (None, REACH_RECT):
        cells = gm.rows * gm.cols if rect is None else rect[2] * rect[3]
        assert (cells * n_yaw) % 64 != 0 and cells % 2 == 1
    step()
    ctx.upload_map(gm)
    out = []
    for rect in (None, REACH_RECT):
        step()
        out.append(ctx.reachability_map(n_yaw, rect))
        step()
        out.append(ctx.reachability_poses(n_yaw, rect))
        if step.baseline:
            assert np.array_equal(check_every_label(ctx, gm, n_yaw, rect=rect), out[-2])
    assert np.array_equal(out[2], out[0][REACH_RECT[0]:REACH_RECT[0] + REACH_RECT[2], REACH_RECT[1]:REACH_RECT[1] + REACH_RECT[3]])
    return out


# ---- 2. clearance ---------------------------------------------------------------------------------------------------------
def clearance(ctx, step):
    import clearance_ref as CR
    from test_clearance_ref import random_words
    n_yaw = 7
    mask = random_words((37, 45), n_yaw, 41, 0.9)          # 3 x 3 tiles of 16 cells: the corner (16, 16) lies inside
    assert ((mask[12:20, 12:20] & 0x7f) != 0x7f).any() and ((mask[12:20, 12:20] & 0x7f) != 0).any()
    out = []
    for R in (5, 17):
        step()
        out.append(ctx.clearance_map(mask, n_yaw, R))
        if step.baseline:
            assert np.array_equal(out[-1], CR.clearance_map(mask, n_yaw, R, 0, False))
    return out


# ---- 3 .. 5. cost fields --------------------------------------------------------------------------------------------------
def _shift_inputs(n_yaw=7, shift=(-3, 5)):
    """test_cost_field_shift's world, windows and rectangle; the masks of the four states of the scenario."""
    import test_cost_field_shift as TS
    si, sj = shift
    old_c, new_c = TS.corners(si, sj)
    bits = TS.world_bits(n_yaw)
    src = TS.overlap_sources(si, sj, n_yaw)

    def keep_sources(b):
        for r, c, k in src:
            b[old_c[0] + TS.RECT[0] + r, old_c[1] + TS.RECT[1] + c, k] = True

    keep_sources(bits)
    # the update: flips around the corner where four tiles of the rectangle meet (local cell (16, 16))
    edited = bits.copy()
    r0, c0 = old_c[0] + TS.RECT[0] + 16, old_c[1] + TS.RECT[1] + 16
    block = edited[r0 - 5:r0 + 5, c0 - 6:c0 + 6]
    block ^= np.random.default_rng(7).random(block.shape) < 0.3
    keep_sources(edited)
    old_b, upd_b, new_b = TS.rect_bits(bits, old_c), TS.rect_bits(edited, old_c), TS.rect_bits(edited, new_c)
    assert (old_b & ~upd_b).sum() > 0 and (upd_b & ~old_b).sum() > 0            # the update removes and adds nodes
    ch = np.argwhere((old_b != upd_b).any(axis=2))
    assert ch[:, 0].min() < 16 <= ch[:, 0].max() and ch[:, 1].min() < 16 <= ch[:, 1].max()   # ... in all four tiles
    return TS, old_c, new_c, src, old_b, upd_b, new_b, (si, sj)


def plain_field(ctx, step):
    from test_cost_field_update import pack
    n_yaw = 7
    TS, old_c, new_c, src, old_b, upd_b, new_b, (si, sj) = _shift_inputs(n_yaw)
    kw = dict(rect=TS.RECT, objective=1)
    out = {}
    step()
    TS.install(ctx, old_c)
    step()
    f = ctx.cost_field(pack(old_b), n_yaw, src, **kw)
    try:
        out["dist0"] = _bits(f.dist())
        step()
        st = f.update(pack(upd_b))
        out["update"] = [st[k] for k in ("changed_words", "removed_nodes", "added_nodes", "dead_nodes", "reached_nodes")]
        assert st["removed_nodes"] == int((old_b & ~upd_b).sum()) and st["added_nodes"] == int((upd_b & ~old_b).sum())
        out["dist1"] = _bits(f.dist())
        with ctx.cost_field(pack(upd_b), n_yaw, src, **kw) as fresh:
            assert np.array_equal(out["dist1"], _bits(fresh.dist()))
        step()
        TS.install(ctx, new_c)
        step()
        st = f.shift(pack(new_b))
        assert (st["shift_rows"], st["shift_cols"]) == (si, sj) and st["left_nodes"] > 0
        out["shift"] = [st[k] for k in TS.STAT_KEYS]
        now = TS.moved(src, si, sj)
        out["dist2"] = _bits(f.dist())
        with ctx.cost_field(pack(new_b), n_yaw, now, **kw) as fresh:
            want = fresh.dist()
            assert np.array_equal(out["dist2"], _bits(want))
        fin = np.argwhere(np.isfinite(want))
        assert len(fin) > 1000
        targets = [tuple(int(v) for v in t) for t in fin[np.random.default_rng(3).integers(0, len(fin), 16)]]
        far = max(targets, key=lambda t: want[t])
        nodes = f.path(far)[0]
        assert len(nodes) >= 6
        step()
        out["blocked"] = f.block_moves(nodes[1:4], nodes[2:5])
        assert out["blocked"] == 3
        out["dist3"] = _bits(f.dist())
        step()
        plan = f.plan(targets, max_rounds=8)
        out["plan"] = [(p[0], p[1], p[2], p[3]) for p in plan]
        out["plan_blocked"] = f.blocked_count()
        step()
        out["unblocked"] = f.unblock()
        out["dist4"] = _bits(f.dist())
        assert np.array_equal(out["dist4"], out["dist2"])
        paths = [f.path(t)[1] for t in targets[:6]]
        step()
        out["simplify"] = f.simplify(paths, window=8)
        step()
        out["dist5"] = _bits(f.dist())
        step()
        out["path"] = f.path(far)
    finally:
        f.close()
    return out


def learned_field(ctx, step):
    import test_cost_field_learned as TL
    from test_cost_field import device_map
    from test_cost_field_learned_update import bump
    n_yaw = 7
    elev = TL.perlin_terrain(TL.N, TL.RES, seed=11) * np.float32(0.2)
    elev2 = elev + bump()
    mask = TL.random_mask(TL.RECT[2:], n_yaw, 5)
    src = [tuple(int(v) for v in np.argwhere(((mask[..., None] >> np.arange(n_yaw)) & 1) != 0)[40])]
    kw = dict(rect=TL.RECT, **TL.WEIGHTS)
    geom = (TL.RES, TL.N * TL.RES, TL.N * TL.RES) + TL.POS
    out = {}
    step()
    device_map(ctx, elev, TL.RES, pos=TL.POS)
    step()
    ctx.cost_load_weights(TL.blob(1, "real"))
    step()
    ctx.cost_update_map(np.ascontiguousarray(elev[::-1, ::-1]), *geom)
    step()
    f = ctx.learned_cost_field(mask, n_yaw, src, **kw)
    try:
        out["dist0"] = _bits(f.dist())
        assert np.isfinite(f.dist()).sum() > 1000
        step()
        ctx.cost_update_map(np.ascontiguousarray(elev2[::-1, ::-1]), *geom)
        step()
        st = f.update_learned()
        out["stats"] = [st[k] for k in ("changed_slots", "repriced_slots", "dead_nodes", "reached_nodes")]
        assert st["changed_slots"] > 0
        out["dist1"] = _bits(f.dist())
        assert not np.array_equal(out["dist0"], out["dist1"])
        with ctx.learned_cost_field(mask, n_yaw, src, **kw) as fresh:
            assert np.array_equal(out["dist1"], _bits(fresh.dist()))
    finally:
        f.close()
    return out


def clearance_field(ctx, step):
    from test_cost_field_update import pack
    n_yaw = 7
    TS, old_c, new_c, src, old_b, upd_b, new_b, _ = _shift_inputs(n_yaw)
    kw = dict(rect=TS.RECT, objective=1, margin=0.2, gain=2.0, radius_cells=5)
    out = {}
    step()
    TS.install(ctx, old_c)
    step()
    f = ctx.clearance_cost_field(pack(old_b), n_yaw, src, **kw)
    try:
        out["dist0"] = _bits(f.dist())
        step()
        st = f.update_clearance(pack(upd_b))
        out["stats"] = [st[k] for k in ("changed_words", "removed_nodes", "added_nodes", "reached_nodes")]
        out["dist1"] = _bits(f.dist())
        step()
        out["d2"] = f.clearance()
        with ctx.clearance_cost_field(pack(upd_b), n_yaw, src, **kw) as fresh:
            assert np.array_equal(out["dist1"], _bits(fresh.dist())) and np.array_equal(out["d2"], fresh.clearance())
        assert not np.array_equal(out["dist0"], out["dist1"])
    finally:
        f.close()
    return out


# ---- 6, 7. roadmap and trees ----------------------------------------------------------------------------------------------
_sq200 = {}


def sq200():
    """test_graph_sweep's smallest map and the valid states nearest its corners (made once, on a context of their own)."""
    if not _sq200:
        from art_planner_amd.context import Context
        from synthetic import make_map
        gm = make_map(200, 0.04, seed=5)
        ctx = Context(0, "yaml")
        ctx.upload_map(gm)
        se3 = ctx.sample_states(99, 0, 1 << 16)
        acc = se3[ctx.validate_states(se3) != 0]
        ctx.close()
        corners = []
        for sx, sy in ((-1, -1), (1, 1), (1, -1), (-1, 1), (0, 0), (-1, 0), (0, 1)):
            cx, cy = gm.pos_x + sx * 0.4 * gm.len_x, gm.pos_y + sy * 0.4 * gm.len_y
            corners.append(acc[np.argmin(np.hypot(acc[:, 0] - cx, acc[:, 1] - cy))])
        _sq200.update(gm=gm, corners=corners)
    return _sq200["gm"], _sq200["corners"]


ROADMAP_PATCH = (80, 60, 40, 40)


def roadmap(ctx, step):
    from art_planner_amd.roadmap import Roadmap
    gm, corners = sq200()
    r0, c0, nr, nc = ROADMAP_PATCH
    patch = gm["elevation"][r0:r0 + nr, c0:c0 + nc] + np.float32(0.8)
    out = {}
    step()
    ctx.upload_map(gm)
    step()
    rm = Roadmap(ctx, corners[0], corners[1], n_milestones=3000, seed=7)
    try:
        out["built"] = rm.export()
        step()
        out["solve0"] = rm.solve()
        step()
        out["grow"] = rm.grow(500)
        assert rm.stats()["vertices"] == 3502
        step()
        ctx.update_layer_rects(0, [patch], [(r0, c0)])
        step()
        rv = rm.revalidate()
        out["revalidate"] = rv
        assert rv["invalid_vertices"] > 0 and rv["valid_edges_after"] < rv["valid_edges_before"]   # the patch is in the way
        step()
        rm.set_query(corners[2], corners[3])
        step()
        out["solve1"] = rm.solve()
        step()
        many = rm.solve_many(corners[2], np.stack([corners[k] for k in (0, 1, 4, 5, 6)]))
        out["many"] = [many["status"], many["cost"], many["paths"], many["stats"]]
        path = out["solve1"][0] if out["solve1"][0] is not None else out["solve0"][0]
        assert path is not None and len(path) >= 3
        step()
        out["simplify"] = rm.simplify(path)
        st = rm.stats()
        out["stats"] = [st[k] for k in ("vertices", "candidate_edges", "valid_edges", "removed_edges", "k", "samples_drawn")]
        out["final"] = rm.export()
    finally:
        rm.close()
    return out


def trees(variant):
    def scenario(ctx, step):
        from art_planner_amd.tree import Tree
        gm, corners = sq200()
        out = []
        step()
        ctx.upload_map(gm)
        step()
        tree = Tree(ctx, corners[0], corners[1], variant, seed=17, first_index=1000, batch=256)
        try:
            for _ in range(4):
                step()
                out.append(tree.grow(1))
                out.append(tree.export())
                out.append(tree.export_checked())
            assert out[-2]["verts"].shape[0] > 100
        finally:
            tree.close()
        return out
    return scenario


# ---- 8. preprocessing -----------------------------------------------------------------------------------------------------
def preprocessing(ctx, step):
    from test_preprocess_sweep import LAYERS
    s = sampler_inputs()
    elev, trav = s["elev"], s["trav"]
    rows, cols = elev.shape
    out = {}
    step()
    pm = ctx.preprocess_map(elev, *GEOM, traversability=trav)
    out["layers"] = {name: pm.layer(name) for name in LAYERS}
    if step.baseline:
        L = P.preprocess(elev, *GEOM, traversability=trav)
        for name in LAYERS:
            assert np.array_equal(out["layers"][name], L[name], equal_nan=True), name
    holes = np.zeros(elev.shape, bool)
    holes[:3, :4] = holes[-2:, -5:] = holes[:4, -1] = holes[-1, :2] = True          # the four corners
    holes[0, 20:30] = holes[rows // 2: rows // 2 + 6, 0] = holes[-3:, cols // 2] = True   # along the borders
    holes[rows // 3: rows // 3 + 9, cols // 3: cols // 3 + 7] = True
    holed = np.array(elev)
    holed[holes] = np.nan
    for mode in (0, 1):
        step()
        filled, n = ctx.inpaint_layer(holed, mode)
        assert n == holes.sum() and np.isfinite(filled).all()
        out[f"inpaint{mode}"] = filled
    e2 = np.array(elev)
    e2[10:20, 5:17] += np.float32(0.2)
    step()
    pm2 = ctx.preprocess_map(e2, GEOM[0], GEOM[1], POS[0] + 3 * 0.04, POS[1] - 2 * 0.04, traversability=trav)
    step()
    upd, rect, cnt = pm2.change_from(pm, 0.05)
    assert 0 < cnt < rows * cols
    out["change"] = [upd, np.array(rect), cnt]
    step()
    pm2.install()
    step()
    se3 = ctx.sample_states(3, 0, 4099)
    out["sampled"] = [se3, ctx.validate_states(se3)]
    assert 0 < out["sampled"][1].sum() < 4099
    pm.close()
    pm2.close()
    return out


# ---- 9. motion cost -------------------------------------------------------------------------------------------------------
def motion_cost(ctx, step):
    g = np.load(os.path.join(common.GOLDEN_DIR, "motion_cost.npz"))
    crop, res = g["crop"].astype(np.float32), float(g["res"])
    L = crop.shape[0] * res
    rng = np.random.default_rng(2)
    B = 70000
    assert 1000 <= (1 << 16) < B                     # artp_cost_query_dev: four lanes per edge up to 2^16 edges, one above
    s = rng.uniform(-0.55 * L, 0.55 * L, (B, 2))
    d = rng.uniform(-0.6, 0.6, (B, 2))
    edges = np.stack([s[:, 0] + d[:, 0], s[:, 1] + d[:, 1], rng.uniform(-np.pi, np.pi, B), s[:, 0], s[:, 1],
                      rng.uniform(-np.pi, np.pi, B)], 1).astype(np.float32)
    nets = {1: mo.random_params(0), 2: mo.random_params(0, cw.SHAPES_FULL)}
    out = []
    for net, mfma in ((1, True), (1, False), (2, True)):
        step()
        ctx.cost_set_fc_path(mfma)
        ctx.cost_load_weights(cw.to_blob(nets[net]))
        assert ctx.cost_fc_path()["mfma"] == int(mfma)
        step()
        ctx.cost_update_map(crop, res, L, L)
        assert ctx.cost_debug_forms()["net"] == net
        step()
        small = ctx.cost_query(edges[:1000])
        step()
        big = ctx.cost_query(edges)
        assert np.array_equal(big[:1000], small)   # whichever kernel: an edge's cost does not depend on the batch around it
        step()
        cells = ctx.cost_query_cells(edges[:1000])
        step()
        feats = ctx.cost_features()
        if step.baseline:
            ref = mo.fc_costs(nets[net], np.transpose(feats, (2, 0, 1)), edges[:4096], res, L, L)
            err = np.abs(big[:4096] - ref)       # test_motion_cost.py's bound for the light network, test_motion_cost_full.py's
            assert err.max() < 5e-5 if net == 1 else (err <= 1e-4 + 1e-4 * np.abs(ref)).all()
        out.append([small, big, cells[0], cells[1], feats])
    return out


# ---- 10. bitmap exchange --------------------------------------------------------------------------------------------------
def bitmap_exchange(ctx, step):
    import torch
    gm = sampler_inputs()["old"]
    n, seed, base = 4099, 7, 1234
    words = (n + 63) // 64
    t = dict(se3=torch.zeros((n, 7), dtype=torch.float64, device=DEV), valid=torch.zeros(n, dtype=torch.uint8, device=DEV),
             compact=torch.zeros((n, 7), dtype=torch.float64, device=DEV), cnt=torch.zeros(4, dtype=torch.int64, device=DEV),
             idx=torch.full((n,), -1, dtype=torch.int32, device=DEV), bits=torch.zeros((2, words), dtype=torch.int64, device=DEV),
             idx2=torch.full((n,), -1, dtype=torch.int32, device=DEV), mat=torch.zeros((2, n, 7), dtype=torch.float64, device=DEV),
             counts=torch.zeros(2, dtype=torch.int64, device=DEV), at=torch.zeros((n, 7), dtype=torch.float64, device=DEV))
    torch.cuda.synchronize()
    step()
    ctx.upload_map(gm)
    step()
    ctx.sample_and_validate_dev(seed, base, n, t["se3"], t["valid"])
    step()
    ctx.compact_valid_dev(t["se3"], t["valid"], t["compact"], t["cnt"][0:1])
    step()
    ctx.compact_valid_indices_dev(t["valid"], t["idx"], t["cnt"][1:2])
    step()
    ctx.pack_valid_bits_dev(t["valid"], t["bits"][0])
    step()
    ctx.pack_valid_bits_dev(t["valid"], t["bits"][1])
    step()
    ctx.indices_from_bits_dev(t["bits"][0], n, t["idx2"], t["cnt"][2:3])
    step()
    ctx.materialise_from_bits_dev(seed, t["bits"], n, [base, base], n, t["mat"], t["counts"])
    step()
    ctx.sample_states_at_dev(seed, base, t["idx"], t["cnt"][1:2], n, t["at"])
    ctx.synchronize()
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in t.items()}
    valid, se3 = out["valid"], out["se3"]
    pos = np.flatnonzero(valid)
    c = len(pos)
    assert 0 < c < n
    if step.baseline:
        assert np.array_equal(valid, O.OracleMap(gm).states_valid(O.robot("yaml"), se3))
        assert list(out["cnt"][:3]) == [c, c, c] and list(out["counts"]) == [c, c]
        assert np.array_equal(out["compact"][:c], se3[pos]) and np.array_equal(out["at"][:c], se3[pos])
        assert np.array_equal(out["idx"][:c], pos) and np.array_equal(out["idx2"][:c], pos)
        assert np.array_equal(out["mat"][0, :c], se3[pos]) and np.array_equal(out["mat"][1, :c], se3[pos])
    return out


SCENARIOS = {
    "reachability": reachability,
    "clearance": clearance,
    "plain_field": plain_field,
    "learned_field": learned_field,
    "clearance_field": clearance_field,
    "roadmap": roadmap,
    "tree_rrt_star": trees("rrt_star"),
    "tree_inf_rrt_star": trees("inf_rrt_star"),
    "tree_rrt_sharp": trees("rrt_sharp"),
    "preprocessing": preprocessing,
    "motion_cost": motion_cost,
    "bitmap_exchange": bitmap_exchange,
}


@pytest.mark.parametrize("plan", list(PLANS))
@pytest.mark.parametrize("name", list(SCENARIOS))
def test_front_end_on_other_lanes_equals_lane_0(name, plan):
    sweep(name, plan)


# ---- 11. objects sharing one lane -----------------------------------------------------------------------------------------
def test_objects_taking_turns_on_one_lane_equal_each_object_alone():
    """A tree, a roadmap and a plain field on lane 1 of one context, a call each in turn, three times round: nothing an
    object left in the lane's scratch may be needed by its next call.  Against each object alone on a fresh context."""
    from art_planner_amd.context import Context
    from art_planner_amd.roadmap import Roadmap
    from art_planner_amd.tree import Tree
    from test_cost_field_update import pack
    gm, corners = sq200()
    n_yaw, rect = 7, (60, 50, 61, 53)
    rng = np.random.default_rng(12)
    masks = [rng.random(rect[2:] + (n_yaw,)) < 0.7]
    for i in range(3):
        nxt = masks[-1].copy()
        blk = nxt[10 + 3 * i:22 + 3 * i, 9:23]
        blk ^= rng.random(blk.shape) < 0.2
        masks.append(nxt)
    src = [(30, 26, 0)]
    for m in masks:
        m[30, 26, 0] = True
    assert all((a != b).any() for a, b in zip(masks, masks[1:]))

    def run(which):
        ctx = Context(0, "yaml")
        ctx.upload_map(gm)
        ctx.set_lane(1)
        tree = Tree(ctx, corners[0], corners[1], "rrt_star", seed=17, batch=256) if "tree" in which else None
        rm = Roadmap(ctx, corners[0], corners[1], n_milestones=3000, seed=7) if "roadmap" in which else None
        f = ctx.cost_field(pack(masks[0]), n_yaw, src, rect=rect, objective=1) if "field" in which else None
        out = {}
        for i in range(3):
            if tree:
                tree.grow(1)
                out[f"tree{i}"] = [tree.export(), tree.export_checked()]
            if rm:
                rm.grow(200)
                out[f"roadmap{i}"] = [rm.export(), rm.solve()[:2]]
            if f:
                f.update(pack(masks[i + 1]))
                out[f"field{i}"] = _bits(f.dist())
        for o in (tree, rm, f):
            if o:
                o.close()
        ctx.close()
        return out

    together = run(("tree", "roadmap", "field"))
    for which in ("tree", "roadmap", "field"):
        alone = run((which,))
        assert sorted(alone) == sorted(k for k in together if k.startswith(which))
        for k, v in alone.items():
            assert flat(v) == flat(together[k]), k
    assert not np.array_equal(together["field0"], together["field2"])


# ---- 12. overlap without host waits ---------------------------------------------------------------------------------------
def test_four_lanes_in_flight_without_host_waits():
    """reachability_map_dev on lane 1, clearance_map_dev on lane 3, sample_and_validate_dev of 4099 states on lane 2 and
    cost_query_dev of 1000 edges on lane 0, issued back to back three times with one synchronize() at the end: every result
    equals the one the same call gives alone on lane 0."""
    import torch
    from art_planner_amd.context import Context
    from test_clearance_ref import random_words
    gm = sampler_inputs()["old"]
    g = np.load(os.path.join(common.GOLDEN_DIR, "motion_cost.npz"))
    crop, res = g["crop"].astype(np.float32), float(g["res"])
    L = crop.shape[0] * res
    n_yaw, n = 7, 4099
    ctx = Context(0, "yaml")
    ctx.upload_map(gm)
    ctx.cost_load_weights(cw.to_blob(mo.random_params(0)))
    ctx.cost_update_map(crop, res, L, L)
    cmask = random_words((37, 45), n_yaw, 41, 0.9)
    cmask_t = torch.from_numpy(np.asfortranarray(cmask).T.copy().view(np.int32)).to(DEV).T
    rng = np.random.default_rng(2)
    s = rng.uniform(-0.55 * L, 0.55 * L, (1000, 2))
    d = rng.uniform(-0.6, 0.6, (1000, 2))
    edges = torch.tensor(np.stack([s[:, 0] + d[:, 0], s[:, 1] + d[:, 1], rng.uniform(-3, 3, 1000), s[:, 0], s[:, 1],
                                   rng.uniform(-3, 3, 1000)], 1).astype(np.float32), device=DEV)

    def tensors():
        return dict(reach=torch.full((gm.rows * gm.cols,), -1, dtype=torch.int32, device=DEV),
                    d2=torch.full((37 * 45 * n_yaw,), -1, dtype=torch.int16, device=DEV),
                    se3=torch.full((n, 7), -7.0, dtype=torch.float64, device=DEV),
                    valid=torch.full((n,), 7, dtype=torch.uint8, device=DEV),
                    cost=torch.full((1000, 3), -7.0, dtype=torch.float32, device=DEV))

    def issue(t, lanes):
        ctx.set_lane(lanes[0])
        ctx.reachability_map_dev(t["reach"], n_yaw)
        ctx.set_lane(lanes[1])
        ctx.clearance_map_dev(cmask_t, n_yaw, t["d2"], 5)
        ctx.set_lane(lanes[2])
        ctx.sample_and_validate_dev(11, 500, n, t["se3"], t["valid"])
        ctx.set_lane(lanes[3])
        ctx.cost_query_dev(edges, t["cost"])

    ref = tensors()
    torch.cuda.synchronize()
    issue(ref, (0, 0, 0, 0))                 # sequential, all on lane 0
    ctx.synchronize()
    want = flat({k: v for k, v in ref.items()})
    labels = ref["valid"].cpu().numpy()
    assert np.array_equal(labels, O.OracleMap(gm).states_valid(O.robot("yaml"), ref["se3"].cpu().numpy()))
    assert 0 < labels.sum() < n and (ref["reach"] != 0).any().item() and (ref["d2"] > 0).any().item()
    rounds = [tensors() for _ in range(3)]
    torch.cuda.synchronize()
    for t in rounds:
        issue(t, (1, 3, 2, 0))
    ctx.synchronize()
    torch.cuda.synchronize()
    for i, t in enumerate(rounds):
        got = flat({k: v for k, v in t.items()})
        assert [p for (p, a), (_, b) in zip(want, got) if a != b] == [], i
    ctx.close()
