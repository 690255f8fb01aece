"""artp_roadmap_solve_many / Roadmap.solve_many: one start, many goals, one lazy search on the kept roadmap.

Every goal's answer is checked against the sequential one -- set_query(start, goal) + solve() per goal on an identically
built second roadmap -- for constructions 0, 1 and 2 with the Euclidean and the directional objective and the learned
cost; the paths against the exported graph, the CPU oracle's motion validator and a bitwise left fold of the edge costs;
the roadmap's state before / after; determinism; the edge cases of the C ABI; and a 10 000-milestone roadmap with 1 024
goals."""
import os
import sys

import numpy as np
import pytest

import common
import oracle_py as O

pytestmark = pytest.mark.gpu

W_LEARNED = (0.25, 1.0, 5.0)
THR_LEARNED = 0.55


@pytest.fixture(scope="module")
def setup():
    from art_planner_amd.context import Context
    from synthetic import make_map
    sys.path.insert(0, os.path.join(common.ROOT, "oracle"))
    sys.path.insert(0, os.path.join(common.ROOT, "tools"))
    import motion_cost_oracle as mo
    import convert_weights
    gm = make_map(200, 0.04, seed=5)
    ctx = Context(0, "yaml")
    ctx.upload_map(gm)
    ctx.cost_load_weights(convert_weights.to_blob(mo.random_params(0)))
    elv = np.ascontiguousarray(gm["elevation"][::-1, ::-1]).astype(np.float32)
    ctx.cost_update_map(elv, gm.res, gm.len_x, gm.len_y, gm.pos_x, gm.pos_y)
    se3 = ctx.sample_states(99, 0, 1 << 16)
    ok = ctx.validate_states(se3) != 0
    valid, invalid = se3[ok], se3[~ok]

    def near(xy):
        return valid[np.argmin(np.hypot(valid[:, 0] - xy[0], valid[:, 1] - xy[1]))]

    start = near((gm.pos_x - 2.6, gm.pos_y - 2.6))
    goal = near((gm.pos_x + 2.6, gm.pos_y + 2.6))
    # goals spread over the map: every n-th valid state of a second stream, plus invalid states
    s2 = ctx.sample_states(11, 0, 1 << 14)
    ok2 = ctx.validate_states(s2) != 0
    spread = s2[ok2][:: max(1, int(ok2.sum()) // 43)][:43]
    yield gm, ctx, start, goal, spread, invalid[:3]
    ctx.close()


def _build(ctx, start, goal, construction, objective, n=1500):
    from art_planner_amd.roadmap import Roadmap
    kw = {}
    if objective == 2:
        kw = dict(cost_weights=W_LEARNED, risk_threshold=THR_LEARNED)
    return Roadmap(ctx, start, goal, n_milestones=n, seed=5, construction=construction, objective=objective, **kw)


def _goals(rm, start, spread, invalid):
    """spread goals, 3 invalid states, and the 2 roadmap vertices nearest the start (near goals: in its k-list)"""
    V = rm.export()["verts"]
    dq = np.abs(V[2:, 3:] @ start[3:])
    d = np.linalg.norm(V[2:, :3] - start[:3], axis=1) + np.where(dq > 1 - 1e-9, 0.0, np.arccos(np.minimum(dq, 1.0)))
    return np.concatenate([spread, invalid, V[2 + np.argsort(d, kind="stable")[:2]]])


def _sequential(rm, start, goals):
    """set_query + solve per goal: (status, cost, path, prefix edge costs {(u, v): cost} of that query)"""
    from art_planner_amd import _capi
    out = []
    for g in goals:
        try:
            rm.set_query(start, g)
        except _capi.ArtpError as e:
            assert e.status == -1
            out.append((1, np.inf, None, {}))
            continue
        d = rm.export()
        pre = {(int(u), int(v)): d["edge_cost"][i] for i, (u, v) in enumerate(d["edges"]) if u < 2}
        try:
            path, cost, _ = rm.solve()
        except _capi.ArtpError as e:
            assert e.status == -5
            out.append((3, np.inf, None, pre))
            continue
        out.append((0 if path is not None else 2, cost, path, pre))
    return out


def _ids(V, start, goal, path):
    """vertex ids of a path's states: 0 = start, 1 = goal, the exported row otherwise"""
    rows = {V[i].tobytes(): i for i in range(2, len(V))}
    ids = []
    for i, s in enumerate(path):
        if i == 0:
            assert np.array_equal(s, start)
            ids.append(0)
        elif i == len(path) - 1:
            assert np.array_equal(s, goal)
            ids.append(1)
        else:
            assert s.tobytes() in rows, "interior path state is not an exported vertex"
            ids.append(rows[s.tobytes()])
    return ids


CASES = [(c, o) for o in (0, 1) for c in (0, 1, 2)] + [(0, 2), (2, 2)]


@pytest.mark.parametrize("construction,objective", CASES)
def test_solve_many_equals_sequential_queries(setup, construction, objective):
    gm, ctx, start, goal, spread, invalid = setup
    A = _build(ctx, start, goal, construction, objective)
    Bm = _build(ctx, start, goal, construction, objective)
    goals = _goals(A, start, spread, invalid)
    _, cost0, _ = A.solve()
    before = A.export()
    res = A.solve_many(start, goals)
    after = A.export()
    seq = _sequential(Bm, start, goals)
    st, cost, paths = res["status"], res["cost"], res["paths"]
    assert res["stats"]["fallback"] >= 2
    assert (st == 1).sum() >= 3 and (st == 0).sum() >= 20

    # the verdicts the answers rest on are direction-symmetric (the equality assumes it: DESIGN.md)
    V = before["verts"]
    pairs = set()
    for p in list(paths) + [s[2] for s in seq]:
        if p is not None:
            pairs.update((p[i].tobytes(), p[i + 1].tobytes()) for i in range(len(p) - 1))
    E = after["edges"]
    gone = np.nonzero(after["edge_removed"] & (E[:, 0] >= 2))[0]
    pairs.update((V[E[e, 0]].tobytes(), V[E[e, 1]].tobytes()) for e in gone)
    s1 = np.array([np.frombuffer(a) for a, _ in pairs])
    s2 = np.array([np.frombuffer(b) for _, b in pairs])
    assert np.array_equal(ctx.check_motions(s1, s2), ctx.check_motions(s2, s1))

    # 1. the sequential answers
    for i, (ss, cs, _, _) in enumerate(seq):
        assert st[i] == ss, (i, st[i], ss)
        if ss == 0:
            assert abs(cost[i] - cs) <= 1e-12 * abs(cs), (i, cost[i], cs)
        else:
            assert np.isinf(cost[i]) and paths[i] is None

    # 2. the paths: exported vertices joined by exported edges, valid motions, the cost a left fold of the edge costs
    key = {(int(u), int(v)): e for e, (u, v) in enumerate(E)}
    om, rob = O.OracleMap(gm), O.robot("yaml")
    m1, m2 = [], []
    for i, p in enumerate(paths):
        if p is None:
            continue
        ids = _ids(V, start, goals[i], p)
        assert len(ids) >= 2
        c = None
        for a, b in zip(ids[:-1], ids[1:]):
            u, v = min(a, b), max(a, b)
            if u < 2:
                w = seq[i][3][(u, v)]  # the query's own edge: as set_query evaluates it for this goal
            else:
                e = key[(u, v)]
                assert after["edge_valid"][e] and not after["edge_removed"][e]
                w = after["edge_cost"][e]
            c = w if c is None else c + w
        assert c == cost[i], (i, c, cost[i])
        m1.append(p[:-1])
        m2.append(p[1:])
    s1, s2 = np.concatenate(m1), np.concatenate(m2)
    assert om.check_motions(rob, s1, s2)[0].all()

    # 3. the roadmap: only new removals on roadmap edges; its own query answers as before
    for f in ("verts", "knn", "knn_dist", "edges", "edge_valid", "edge_interp", "edge_cost"):
        assert np.array_equal(before[f], after[f], equal_nan=f in ("knn_dist", "edge_cost")), f
    new = after["edge_removed"].astype(bool) & ~before["edge_removed"].astype(bool)
    assert (after["edge_removed"] >= before["edge_removed"]).all()
    assert (E[new, 0] >= 2).all()
    _, cost1, _ = A.solve()
    assert cost1 == cost0
    A.close()
    Bm.close()


@pytest.mark.parametrize("construction,objective", [(0, 0), (2, 1), (1, 2)])
def test_solve_many_is_deterministic(setup, construction, objective):
    gm, ctx, start, goal, spread, invalid = setup
    out = []
    for _ in range(2):
        rm = _build(ctx, start, goal, construction, objective)
        r = rm.solve_many(start, _goals(rm, start, spread, invalid))
        out.append(r)
        rm.close()
    a, b = out
    assert np.array_equal(a["status"], b["status"])
    assert a["cost"].tobytes() == b["cost"].tobytes()
    assert a["stats"] == b["stats"]
    for p, q in zip(a["paths"], b["paths"]):
        assert (p is None and q is None) or p.tobytes() == q.tobytes()


def test_solve_many_edge_cases(setup):
    from art_planner_amd import _capi
    gm, ctx, start, goal, spread, invalid = setup
    rm = _build(ctx, start, goal, 0, 0)
    goals = _goals(rm, start, spread, invalid)
    full = rm.solve_many(start, goals)
    # costs only
    r = rm.solve_many(start, goals, paths=False)
    assert r["paths"] is None
    assert np.array_equal(r["status"], full["status"]) and r["cost"].tobytes() == full["cost"].tobytes()
    # a path buffer too small: ARTP_ERR_CAPACITY with statuses, costs and offsets filled
    n = len(goals)
    g = np.ascontiguousarray(goals)
    s = np.ascontiguousarray(start)
    status = np.full(n, 99, np.int32)
    cost = np.zeros(n)
    off = np.zeros(n + 1, np.uint64)
    buf = np.zeros((2, 7))
    rc = rm.L.artp_roadmap_solve_many(rm.h, s.ctypes.data, g.ctypes.data, n, status.ctypes.data, cost.ctypes.data,
                                      off.ctypes.data, buf.ctypes.data, 2, None)
    assert rc == -5
    assert np.array_equal(status, full["status"]) and cost.tobytes() == full["cost"].tobytes()
    lens = [0 if p is None else len(p) for p in full["paths"]]
    assert np.array_equal(off, np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64))
    # Python retries with the reported size
    small = rm.solve_many(start, goals, cap_states=2)
    assert all((p is None and q is None) or np.array_equal(p, q) for p, q in zip(small["paths"], full["paths"]))
    # no goals
    r = rm.solve_many(start, np.zeros((0, 7)))
    assert len(r["status"]) == 0 and r["paths"] == [] and r["stats"]["rounds"] == 0
    # an invalid start: refused, nothing changes
    before = rm.export()
    with pytest.raises(_capi.ArtpError) as e:
        rm.solve_many(invalid[0], goals)
    assert e.value.status == -1
    after = rm.export()
    for f in before:
        assert before[f].tobytes() == after[f].tobytes(), f
    rm.close()


def test_solve_many_at_scale():
    """C2: 10 000 milestones, 1 024 goals in one call; 32 of them against the sequential queries."""
    from art_planner_amd.context import Context
    from art_planner_amd.roadmap import Roadmap
    from synthetic import make_map
    gm = make_map(400, 0.04, seed=1234)
    ctx = Context(0, "yaml")
    ctx.upload_map(gm)
    se3 = ctx.sample_states(99, 0, 1 << 17)
    valid = se3[ctx.validate_states(se3) != 0]
    start, goal = valid[0], valid[1]
    goals = valid[2:][:: max(1, (len(valid) - 2) // 1024)][:1024]
    assert len(goals) == 1024
    A = Roadmap(ctx, start, goal, n_milestones=10000, seed=1)
    Bm = Roadmap(ctx, start, goal, n_milestones=10000, seed=1)
    res = A.solve_many(start, goals)
    assert (res["status"] == 0).sum() > 512
    pick = np.arange(0, 1024, 32)
    seq = _sequential(Bm, start, goals[pick])
    for j, i in enumerate(pick):
        assert res["status"][i] == seq[j][0], (i, res["status"][i], seq[j][0])
        if seq[j][0] == 0:
            assert abs(res["cost"][i] - seq[j][1]) <= 1e-12 * seq[j][1]
    A.close()
    Bm.close()
    ctx.close()
