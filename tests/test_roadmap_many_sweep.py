"""artp_roadmap_solve_many against an independent restatement of its lazy rounds and limits (tests/many_ref.py).

Roadmap A takes the call; an identically built roadmap B only supplies inputs: per goal, B.set_query(start, goal) +
export() gives the two neighbour lists and the query's own edge costs (B.solve is never called, but for the one near goal
of the max_replans family, whose contract is the sequential answer).  The lists are checked against many_ref.classify and
graph_ref.check_knn_rows; the weights are taken as given (the edge sweep tests them) and the verdicts come from
ctx.check_motions (the edge sweep covers it).

Every family asserts, for the far goals, status, cost and path ids bit for bit against many_ref.rounds, together with
stats rounds / removed / motions and the new edge_removed flags; for every goal, status and cost against many_ref.eager
(all invalid edges deleted up front); every path's motions, and its cost as a left fold; and that the roadmap's own query
is untouched.  Lines starting with MANY_SWEEP print the measured figures DESIGN.md section 10 quotes."""
import math

import numpy as np
import pytest

import graph_ref as G
import many_ref as M
from test_graph_sweep import SSSP_MIN_VERTICES, _ring_map
from test_roadmap_many import THR_LEARNED, W_LEARNED, _ids, setup  # noqa: F401  (setup: the 200 x 200 map's fixture)

pytestmark = pytest.mark.gpu


def _corner(valid, x, y):
    return valid[np.argmin(np.hypot(valid[:, 0] - x, valid[:, 1] - y))]


@pytest.fixture(scope="module")
def env(setup):  # noqa: F811
    gm, ctx, start, goal, spread, invalid = setup
    s2 = ctx.sample_states(11, 0, 1 << 14)
    pool = s2[ctx.validate_states(s2) != 0]
    # the roadmap's own query: the two other corners, so that restoring it is visible
    own = (_corner(pool, gm.pos_x + 2.6, gm.pos_y - 2.6), _corner(pool, gm.pos_x - 2.6, gm.pos_y + 2.6))
    s3 = ctx.sample_states(12, 0, 1 << 12)
    bad = s3[ctx.validate_states(s3) == 0]
    assert len(pool) > 2000 and len(bad) >= 8
    return {"gm": gm, "ctx": ctx, "start": start, "own": own, "pool": pool, "invalid": bad, "cache": {}}


def _roadmap(ctx, own, n, construction=0, objective=0, k_neighbors=0, max_replans=1000, zero_cost=False, seed=5):
    from art_planner_amd.roadmap import Roadmap
    kw = {}
    if objective == 2:
        kw = dict(cost_weights=(0.0, 0.0, 0.0), risk_threshold=1.0) if zero_cost else \
            dict(cost_weights=W_LEARNED, risk_threshold=THR_LEARNED)
    return Roadmap(ctx, own[0], own[1], n_milestones=n, seed=seed, construction=construction, objective=objective,
                   k_neighbors=k_neighbors, max_replans=max_replans, **kw)


def _usable(valid, cost):
    return np.where((np.asarray(valid) != 0) & np.isfinite(cost) & (cost >= 0.0), cost, np.inf)


def _motions(ctx, a, b):
    if len(a) == 0:
        return np.zeros(0, bool)
    return ctx.check_motions(a, b) != 0


def _inputs(B, start, goals, ok, vinvalid=None):
    """per valid goal: set_query on B + export -> the two knn rows, their distances, the query's own edges {(u, v): w};
    vinvalid: the vertices the current map invalidates (no list may hold them)"""
    exclude = None if vinvalid is None else np.flatnonzero(vinvalid)
    out = []
    for g in range(len(goals)):
        if not ok[g]:
            out.append(None)
            continue
        B.set_query(start, goals[g])
        d = B.export()
        E = d["edges"]
        fk = int((E[:, 0] < 2).sum())
        w = _usable(d["edge_valid"][:fk], d["edge_cost"][:fk])
        G.check_knn_rows(d["verts"], np.arange(2), d["knn"][:2], d["knn_dist"][:2], d["knn"].shape[1],
                         exclude=exclude)
        out.append({"row": d["knn"][:2].astype(np.int64), "dist": d["knn_dist"][:2].copy(),
                    "pre": {(int(E[e, 0]), int(E[e, 1])): float(w[e]) for e in range(fk)}})
    return out


def _pick_far(V, start, k, pool, n, vinvalid=None, chunk=64):
    """the first n states of pool that the reference calls far, with a classification margin > 1e-9"""
    out = []
    for c0 in range(0, len(pool), chunk):
        C = M.classify(V, vinvalid, start, pool[c0:c0 + chunk], k)
        for i in np.flatnonzero(~C["near"] & (C["margin"] > 1e-9)):
            out.append(pool[c0 + i])
            if len(out) == n:
                return np.array(out)
    raise AssertionError(f"only {len(out)} far goals in the pool, {n} wanted")


def _check(ctx, A, B, start, goals, *, label, pristine, max_replans=1000, vinvalid=None, inputs=None,
           near_status=None, cost0=None, own_solve=True):
    """One solve_many call on A against the reference; returns (result, simulator output or None, details).
    pristine: A's verdict cache holds nothing for this map and edge list (never solved, or stale), so the motions the call
    checks are exactly the simulator's; otherwise cached verdicts may only save some."""
    goals = np.ascontiguousarray(goals, np.float64).reshape(-1, 7)
    ng = len(goals)
    before = A.export()
    V, k = before["verts"], before["knn"].shape[1]
    nv = len(V)
    ok = ctx.validate_states(goals) != 0
    C = M.classify(V, vinvalid, start, goals, k)
    amb = ok & ~((C["margin"] > 1e-9) | (C["d_start_goal"] == 0.0))
    assert not amb.any(), ("ambiguous near / far goals", np.flatnonzero(amb), C["margin"][amb])
    near = ok & C["near"]
    far = np.flatnonzero(ok & ~C["near"])
    inp = inputs if inputs is not None else _inputs(B, start, goals, ok, vinvalid)

    # the lists of the far goals: the reference's, id for id
    def padded(ids):
        return np.concatenate([ids, np.full(k - len(ids), G.NONE, np.int64)])
    for g in far:
        assert np.array_equal(inp[g]["row"][0], padded(C["start_ids"])), (g, "the start's list")
        assert np.array_equal(inp[g]["row"][1], padded(C["goal_ids"][g])), (g, "the goal's list")
        assert np.abs(inp[g]["dist"][1][:len(C["goal_dist"][g])] - C["goal_dist"][g]).max(initial=0.0) <= 1e-11

    # the graph of the rounds: usable roadmap edges with both ends >= 2, one verdict per direction
    E = before["edges"].astype(np.int64)
    fk = int((E[:, 0] < 2).sum())
    eu, ev = E[fk:, 0], E[fk:, 1]
    w = _usable(before["edge_valid"][fk:] & (before["edge_removed"][fk:] == 0), before["edge_cost"][fk:])
    fin = np.flatnonzero(np.isfinite(w))
    fwd, bwd = np.ones(len(w), bool), np.ones(len(w), bool)
    fwd[fin] = _motions(ctx, V[eu[fin]], V[ev[fin]])
    bwd[fin] = _motions(ctx, V[ev[fin]], V[eu[fin]])
    n_dir = int((fwd != bwd).sum())
    sn = C["start_ids"]
    S0 = np.concatenate([start[None], V[1:]])
    s_fwd = _motions(ctx, np.repeat(start[None], len(sn), 0), V[sn])
    s_bwd = _motions(ctx, V[sn], np.repeat(start[None], len(sn), 0))
    n_dir += int((s_fwd != s_bwd).sum())

    sim = None
    sw = None
    if len(far):
        sw = np.array([inp[far[0]]["pre"][(0, int(n))] for n in sn])
        for g in far:
            assert all(inp[g]["pre"][(0, int(n))] == sw[t] for t, n in enumerate(sn)), (g, "start edge costs differ")
        atts = [(C["goal_ids"][g], np.array([inp[g]["pre"][(1, int(n))] for n in C["goal_ids"][g]])) for g in far]
        S = np.concatenate([S0, goals[far]])

        def verdict(src, dst):
            return _motions(ctx, S[src], S[dst])
        sim = M.rounds(nv, eu, ev, w, (sn, sw), atts, verdict, max_replans)

    res = A.solve_many(start, goals)
    after = A.export()
    st, cost, paths, stats = res["status"], res["cost"], res["paths"], res["stats"]
    print(f"MANY_SWEEP {label}: goals {ng} valid {int(ok.sum())} near {int(near.sum())} stats {stats} "
          f"status counts {np.bincount(st, minlength=4).tolist()}")
    assert np.all(st[~ok] == 1) and np.all(np.isinf(cost[~ok])) and all(paths[g] is None for g in np.flatnonzero(~ok))
    assert np.all(st[ok] != 1)
    assert stats["fallback"] == int(near.sum())

    ids_of = {int(g): _ids(V, start, goals[g], paths[g]) for g in np.flatnonzero(st == 0)}

    # removals: the simulator's; a near goal's own solve may have removed (invalid) roadmap edges before the rounds
    new = np.flatnonzero((after["edge_removed"][fk:] != 0) & (before["edge_removed"][fk:] == 0))
    assert np.all(after["edge_removed"] >= before["edge_removed"])
    assert not (after["edge_removed"][:fk] != before["edge_removed"][:fk]).any()
    extra = []
    if sim is not None:
        extra = sorted(set(new.tolist()) - set(sim["removed_edges"]))
        if extra:
            assert near.any(), "edges removed that no round of the reference removes"
            assert not (fwd[extra] & bwd[extra]).any(), "the fallback removed a valid edge"
            w2 = w.copy()
            w2[extra] = np.inf
            sim = M.rounds(nv, eu, ev, w2, (sn, sw), atts, verdict, max_replans)
        assert sorted(set(sim["removed_edges"]) | set(extra)) == new.tolist()
        assert stats["rounds"] == sim["rounds"], (stats, sim["rounds"])
        assert stats["removed"] == sim["removed"], (stats, sim["removed"])
        if pristine:
            assert stats["motions"] == sim["motions"], (stats, sim["motions"])
        else:
            assert stats["motions"] <= sim["motions"], (stats, sim["motions"])
        for i, g in enumerate(far):
            assert st[g] == sim["status"][i], (g, st[g], sim["status"][i])
            assert cost[g].tobytes() == sim["cost"][i].tobytes(), (g, cost[g], sim["cost"][i])
            if st[g] == 0:
                want = sim["paths"][i][:-1] + [1]
                assert ids_of[int(g)] == want, (g, "path ids", ids_of[int(g)], want)
            else:
                assert paths[g] is None
    else:
        assert (stats["rounds"], stats["removed"], stats["motions"]) == (0, 0, 0)

    # every goal against the eager graph, the edges whose two directions disagree once kept and once deleted
    picks = {"kept": lambda a, b: a | b, "deleted": lambda a, b: a & b}
    eager_far = {}
    if len(far):  # one search per variant for all far goals
        lens = [len(a[0]) for a in atts]
        an_all = np.concatenate([a[0] for a in atts])
        g_all = np.repeat(goals[far], lens, 0)
        cut = np.cumsum(lens)[:-1]
        a_f, a_b = _motions(ctx, V[an_all], g_all), _motions(ctx, g_all, V[an_all])
        n_dir += int((a_f != a_b).sum())
        for both, pick in picks.items():
            if both == "deleted" and n_dir == 0:
                eager_far[both] = eager_far["kept"]
                continue
            eager_far[both] = M.eager(nv, eu, ev, w, (sn, sw), atts, pick(fwd, bwd), pick(s_fwd, s_bwd),
                                      np.split(pick(a_f, a_b), cut))

    def eager_of(g, both):
        pick = picks[both]
        if not C["near"][g]:
            i = int(np.flatnonzero(far == g)[0])
            return int(eager_far[both][0][i]), float(eager_far[both][1][i]), 0
        # a near goal's own query graph: the goal is vertex 1, its edges and (0, 1) join the roadmap's
        pre = inp[g]["pre"]
        Sg = np.concatenate([start[None], goals[g][None], V[2:]])
        p1 = [(u, v) for (u, v) in pre if u == 1]
        p0 = [(u, v) for (u, v) in pre if u == 0]
        e1u, e1v = np.array([p[0] for p in p1], np.int64), np.array([p[1] for p in p1], np.int64)
        f1, b1 = _motions(ctx, Sg[e1u], Sg[e1v]), _motions(ctx, Sg[e1v], Sg[e1u])
        n0 = np.array([p[1] for p in p0], np.int64)
        f0 = _motions(ctx, np.repeat(start[None], len(n0), 0), Sg[n0])
        b0 = _motions(ctx, Sg[n0], np.repeat(start[None], len(n0), 0))
        s, c = M.eager(nv, np.concatenate([eu, e1u]), np.concatenate([ev, e1v]),
                       np.concatenate([w, [pre[p] for p in p1]]), (n0, np.array([pre[p] for p in p0])),
                       [(np.array([1]), np.array([0.0]))], np.concatenate([pick(fwd, bwd), pick(f1, b1)]),
                       pick(f0, b0), [np.array([True])])
        return int(s[0]), float(c[0]), int((f1 != b1).sum() + (f0 != b0).sum())

    n_skip = 0
    for g in np.flatnonzero(ok):
        if st[g] == 3:  # a limit, not a property of the graph: the far ones are the simulator's, the near ones the caller's
            if C["near"][g]:
                assert near_status is not None and near_status.get(int(g)) == 3, (g, "near goal with status 3")
            continue
        if near_status is not None and int(g) in near_status:
            assert st[g] == near_status[int(g)]
        s_k, c_k, nd = eager_of(g, "kept")
        n_dir += nd
        s_d, c_d = (s_k, c_k) if n_dir == 0 else eager_of(g, "deleted")[:2]
        if (s_k, c_k) != (s_d, c_d):
            n_skip += 1
            continue
        assert st[g] == s_k, (g, st[g], s_k)
        if s_k == 0:
            if C["near"][g]:
                assert abs(cost[g] - c_k) <= 1e-12 * abs(c_k), (g, cost[g], c_k)
            else:
                assert cost[g] == c_k, (g, cost[g], c_k)
        else:
            assert np.isinf(cost[g])
    print(f"MANY_SWEEP {label}: direction-dependent verdicts {n_dir}, goals left out of the eager comparison {n_skip}")
    assert n_skip <= math.ceil(0.01 * ng)

    deepest = _check_paths(ctx, res, ids_of, inp, (eu, ev, w), after["edge_removed"][fk:], vinvalid)
    print(f"MANY_SWEEP {label}: deepest path {deepest} hops")
    for f in ("verts", "knn", "knn_dist", "edges", "edge_valid", "edge_interp", "edge_cost"):  # the query prefix stays
        assert np.array_equal(before[f], after[f], equal_nan=f in ("knn_dist", "edge_cost")), f
    if own_solve:
        _check_own_query(ctx, A, after, max_replans, cost0)
    return res, sim, {"far": far, "near": np.flatnonzero(near), "ok": ok, "class": C, "deepest": deepest, "inputs": inp,
                      "before": before, "after": after}


def _check_paths(ctx, res, ids_of, inp, graph, removed_after, vinvalid):
    """every returned path: exported vertices joined by usable edges that are still there, valid motions, no invalid
    vertex, the cost the left fold of its edge costs; returns the deepest path's hops"""
    eu, ev, w = graph
    key = {(int(a), int(b)): e for e, (a, b) in enumerate(zip(eu, ev))}
    m1, m2, deepest = [], [], 0
    for g in np.flatnonzero(res["status"] == 0):
        p, ids = res["paths"][g], ids_of[int(g)]
        deepest = max(deepest, len(ids) - 1)
        ws = []
        for a, b in zip(ids[:-1], ids[1:]):
            u, v = min(a, b), max(a, b)
            if u < 2:
                ws.append(inp[g]["pre"][(u, v)])
            else:
                e = key[(u, v)]
                assert np.isfinite(w[e]) and not removed_after[e]
                ws.append(w[e])
        assert G.left_fold(ws) == res["cost"][g], (g, G.left_fold(ws), res["cost"][g])
        if vinvalid is not None:
            assert not np.asarray(vinvalid, bool)[[i for i in ids if i >= 2]].any(), (g, "path through an invalid vertex")
        m1.append(p[:-1])
        m2.append(p[1:])
    if m1:
        assert _motions(ctx, np.concatenate(m1), np.concatenate(m2)).all()
    return deepest


def _check_own_query(ctx, A, after, max_replans, cost0):
    """the roadmap's own solve() after the call: what it was before (cost0), and the eager answer of its own graph"""
    from art_planner_amd import _capi
    try:
        _, own_cost, _ = A.solve()
    except _capi.ArtpError as e:  # the roadmap's own query runs out of removals where max_replans is the subject
        assert e.status == -5 and max_replans < 1000 and cost0 is None
        return
    if cost0 is not None:
        assert own_cost == cost0
    V = after["verts"]
    Ea = after["edges"].astype(np.int64)
    wa = _usable(after["edge_valid"] & (after["edge_removed"] == 0), after["edge_cost"])
    fa = np.flatnonzero(np.isfinite(wa))
    of, ob = _motions(ctx, V[Ea[fa, 0]], V[Ea[fa, 1]]), _motions(ctx, V[Ea[fa, 1]], V[Ea[fa, 0]])
    refs = []
    for okk in (of | ob, of & ob):  # edges whose two directions disagree once kept, once deleted
        ww = wa.copy()
        ww[fa[~okk]] = np.inf
        refs.append(M.dijkstra(len(V), Ea[:, 0], Ea[:, 1], ww)[1])
    if refs[0] == refs[1]:
        assert (np.isinf(own_cost) and np.isinf(refs[0])) or abs(own_cost - refs[0]) <= 1e-12 * refs[0]


# ---- a. goal counts --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_goals", [1, 63, 64, 65, 255, 256, 257])
def test_goal_counts(env, n_goals):
    """the attach kernel's ng + 1 slots and the 256-lane blocks of the path / resolve kernels, far goals only"""
    ctx, start = env["ctx"], env["start"]
    A = _roadmap(ctx, env["own"], 600)
    if "a" not in env["cache"]:
        B = _roadmap(ctx, env["own"], 600)
        d = A.export()
        goals = _pick_far(d["verts"], start, d["knn"].shape[1], env["pool"], 257)
        env["cache"]["a"] = (goals, _inputs(B, start, goals, np.ones(257, bool)))
        B.close()
    goals, inp = env["cache"]["a"]
    res, sim, info = _check(ctx, A, None, start, goals[:n_goals], label=f"a goals={n_goals}", pristine=True,
                            inputs=inp[:n_goals])
    assert len(info["far"]) == n_goals and res["stats"]["fallback"] == 0 and (res["status"] == 0).sum() > 0.5 * n_goals
    A.close()


# ---- b. k regimes ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k_nb", [1, 56, 57, 63, 64, 65, 128])
def test_k_regimes(env, k_nb):
    """kk = min(k + 8, 64): margin 8 up to k = 56, a shrinking margin to 63, host brute force from 64"""
    ctx, start = env["ctx"], env["start"]
    A = _roadmap(ctx, env["own"], 300, k_neighbors=k_nb)
    B = _roadmap(ctx, env["own"], 300, k_neighbors=k_nb)
    d = A.export()
    assert d["knn"].shape[1] == k_nb
    # the pool's states nearest the start first: the nearest far goals are the ones most likely to be in reach
    pool = env["pool"][:1500]
    pool = pool[np.argsort(G.se3_distance(start[None], pool)[0], kind="stable")]
    goals = np.concatenate([_pick_far(d["verts"], start, k_nb, pool, 24), env["invalid"][:1]])
    res, sim, info = _check(ctx, A, B, start, goals, label=f"b k={k_nb}", pristine=True)
    assert len(info["far"]) == 24 and res["status"][-1] == 1
    if k_nb > 1:  # (k = 1 leaves the roadmap in pieces: the reference decides)
        assert (res["status"] == 0).sum() >= 4, "no k regime without solved far goals"
    A.close()
    B.close()


def test_fewer_candidates_than_the_shortlist(env):
    """20 milestones, k = 15: the shortlist asks for 23 of 20 candidates (have < kk); near is what the reference says"""
    ctx, start = env["ctx"], env["start"]
    A = _roadmap(ctx, env["own"], 20, k_neighbors=15)
    B = _roadmap(ctx, env["own"], 20, k_neighbors=15)
    assert A.export()["knn"].shape[1] == 15
    goals = env["pool"][100:148]
    res, sim, info = _check(ctx, A, B, start, goals, label="b 20 milestones k=15", pristine=True)
    assert len(info["far"]) + len(info["near"]) == 48
    A.close()
    B.close()


def test_every_goal_near_on_a_tiny_roadmap(env):
    """5 milestones: every list is shorter than k, every valid goal goes through set_query + solve, no round runs"""
    ctx, start = env["ctx"], env["start"]
    A = _roadmap(ctx, env["own"], 5)
    B = _roadmap(ctx, env["own"], 5)
    goals = np.concatenate([env["pool"][200:212], env["invalid"][:2]])
    res, sim, info = _check(ctx, A, B, start, goals, label="b 5 milestones", pristine=True)
    assert sim is None and res["stats"]["fallback"] == 12 and res["stats"]["rounds"] == 0
    A.close()
    B.close()


# ---- c. constructions and objectives ---------------------------------------------------------------------------------

@pytest.mark.parametrize("construction,objective", [(0, 0), (1, 0), (2, 0), (0, 1), (1, 1), (2, 1), (0, 2), (2, 2)])
def test_constructions_and_objectives(env, construction, objective):
    ctx, start = env["ctx"], env["start"]
    A = _roadmap(ctx, env["own"], 800, construction, objective)
    B = _roadmap(ctx, env["own"], 800, construction, objective)
    d = A.export()
    goals = _pick_far(d["verts"], start, d["knn"].shape[1], env["pool"][300:], 64)
    res, sim, info = _check(ctx, A, B, start, goals, label=f"c construction={construction} objective={objective}",
                            pristine=True)
    assert (res["status"] == 0).sum() >= 16
    if construction == 2:
        assert res["stats"]["removed"] > 0
    A.close()
    B.close()


# ---- d. ties ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("construction", [0, 2])
def test_total_ties(env, construction):
    """The learned objective with weights (0, 0, 0): every usable edge costs exactly 0, every vertex ties with every
    other, and the paths are the hop rule's and the smallest-predecessor rule's alone.  Goals on roadmap vertices, the
    start on a roadmap vertex, one goal twice."""
    ctx = env["ctx"]
    A = _roadmap(ctx, env["own"], 600, construction, 2, zero_cost=True)
    B = _roadmap(ctx, env["own"], 600, construction, 2, zero_cost=True)
    d = A.export()
    V, k = d["verts"], d["knn"].shape[1]
    fin = np.isfinite(d["edge_cost"])
    assert fin.sum() > 1000 and np.all(d["edge_cost"][fin] == 0.0)
    start = V[2 + int(np.argmin(G.se3_distance(env["start"][None], V[2:])[0]))].copy()
    on_vertex = V[2 + np.argsort(-G.se3_distance(start[None], V[2:])[0], kind="stable")[:8]]
    free = _pick_far(V, start, k, env["pool"][300:], 40)
    goals = np.concatenate([free, on_vertex, free[:1]])
    res, sim, info = _check(ctx, A, B, start, goals, label=f"d ties construction={construction}", pristine=True)
    solved = res["status"] == 0
    assert solved.sum() >= 20 and np.all(res["cost"][solved] == 0.0)
    assert res["status"][-1] == res["status"][0] and res["cost"][-1] == res["cost"][0]
    if res["status"][0] == 0:
        assert np.array_equal(res["paths"][-1], res["paths"][0])
    assert set(info["far"].tolist()) >= set(range(40, 48)), "the goals on roadmap vertices are far from the start"
    if construction == 2:
        assert res["stats"]["removed"] > 0
    A.close()
    B.close()


# ---- e. max_replans --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("max_replans", [0, 1, 2, 1000])
def test_max_replans(env, max_replans):
    """Construction 2's direct edges are of unknown validity: the rounds remove edges, and a goal with more than
    max_replans removals on its paths ends with status 3 -- exactly the simulator's goals."""
    from art_planner_amd import _capi
    ctx, start = env["ctx"], env["start"]
    A = _roadmap(ctx, env["own"], 800, 2, 0, max_replans=max_replans)
    B = _roadmap(ctx, env["own"], 800, 2, 0, max_replans=max_replans)
    d = A.export()
    V, k = d["verts"], d["knn"].shape[1]
    goals = _pick_far(V, start, k, env["pool"][300:], 64)
    near_status = None
    if max_replans == 0:
        # one near goal whose sequential answer is "too many removals": the contract of a near goal is B's own solve
        cand = np.concatenate([V[2 + np.argsort(G.se3_distance(start[None], V[2:])[0], kind="stable")[:k - 1]],
                               env["pool"]])
        Cc = M.classify(V, None, start, cand, k)
        cand = cand[Cc["near"] & (Cc["margin"] > 1e-9)]
        cand = cand[np.argsort(-G.se3_distance(start[None], cand)[0], kind="stable")][:200]
        for c in cand:
            B.set_query(start, c)
            try:
                B.solve()
            except _capi.ArtpError as e:
                assert e.status == -5
                goals = np.concatenate([goals, c[None]])
                near_status = {64: 3}
                break
        assert near_status is not None, "no near goal with a removal on its first path among the near candidates"
    res, sim, info = _check(ctx, A, B, start, goals, label=f"e max_replans={max_replans}", pristine=True,
                            max_replans=max_replans, near_status=near_status)
    n3 = int((res["status"] == 3).sum())
    assert sim["removed"] > 0
    if max_replans == 0:
        assert n3 >= 2 and res["status"][64] == 3 and list(info["near"]) == [64]
    if max_replans == 1000:
        assert n3 == 0
    print(f"MANY_SWEEP e max_replans={max_replans}: status 3 for {n3} goals, most removals of a goal "
          f"{int(sim['removals'].max())}")
    A.close()
    B.close()


# ---- f. unreachable goals --------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ring():
    from art_planner_amd.context import Context
    gm, (cx, cy) = _ring_map()
    ctx = Context(0, "yaml")
    ctx.upload_map(gm)
    se3 = ctx.sample_states(3, 0, 1 << 15)
    okv = ctx.validate_states(se3) != 0
    acc, bad = se3[okv], se3[~okv]
    r = np.maximum(np.abs(acc[:, 0] - cx), np.abs(acc[:, 1] - cy))
    inside, outside = acc[r < 1.3], acc[r > 3.4]
    assert len(inside) >= 40 and len(outside) >= 400 and len(bad) >= 16
    own = (outside[0], outside[1])
    yield {"ctx": ctx, "inside": inside, "outside": outside, "invalid": bad, "own": own}
    ctx.close()


@pytest.mark.parametrize("case", ["start_outside", "start_inside", "start_inside_goals_outside", "all_invalid"])
def test_unreachable_and_invalid_goals(ring, case):
    """A ring no motion crosses around a pocket: goals on the other side of it are ARTP_GOAL_UNREACHABLE."""
    ctx = ring["ctx"]
    A = _roadmap(ctx, ring["own"], 1500)
    B = _roadmap(ctx, ring["own"], 1500)
    d = A.export()
    V, k = d["verts"], d["knn"].shape[1]
    inside = ring["inside"]
    if case in ("start_outside", "all_invalid"):
        start, n_in = ring["outside"][5], 12
    else:  # from a corner of the pocket, the goals farthest from it first: few states of the pocket are far
        start, n_in = inside[np.argmin(inside[:, 0] + inside[:, 1])], 4
        inside = inside[np.argsort(-G.se3_distance(start[None], inside)[0], kind="stable")][:-1]
    g_in = _pick_far(V, start, k, inside, n_in)
    g_out = _pick_far(V, start, k, ring["outside"][10:], 20)
    goals = {"start_outside": np.concatenate([g_in, g_out]), "start_inside": np.concatenate([g_out, g_in]),
             "start_inside_goals_outside": g_out, "all_invalid": ring["invalid"][:16]}[case]
    res, sim, info = _check(ctx, A, B, start, goals, label=f"f {case}", pristine=True)
    st = res["status"]
    if case == "start_outside":
        assert np.all(st[:12] == 2) and np.all(st[12:] == 0)
    elif case == "start_inside":
        assert np.all(st[:20] == 2) and (st[20:] == 0).sum() >= 1 and len(st) == 24
    elif case == "start_inside_goals_outside":
        # far goals enter many_device_solve, no attachment is in reach: total == 0 ends the loop before round 1
        assert len(info["far"]) == 20 and sim["rounds"] == 0 and res["stats"]["rounds"] == 0 and np.all(st == 2)
    else:
        assert sim is None and np.all(st == 1)
        assert res["stats"] == {"rounds": 0, "removed": 0, "motions": 0, "fallback": 0}
    A.close()
    B.close()


# ---- g. state carried between calls ------------------------------------------------------------------------------------

@pytest.mark.parametrize("construction", [0, 2])
def test_the_same_call_twice(env, construction):
    """The second call finds the first call's verdicts in the cache and its removals in the roadmap: equal answers from
    fewer motions.  "removed == 0" holds for the second call only when it drops no attachment: the start's edges and the
    goals' attachments belong to the call, not to the roadmap, so the ones the motion check rejects are found, and counted
    in stats.removed, by every call (measured: 4 with construction 0, whose edge evaluation and motion check disagree on
    them); and the way to a vertex whose attachment is about to be dropped again runs through the thinned graph, over
    edges the first call never had on a path (measured: 2 new roadmap removals with construction 2).  What is asserted
    is the simulator's count, exactly, fewer removals than the first call made, and 0 where nothing is dropped."""
    ctx, start = env["ctx"], env["start"]
    A = _roadmap(ctx, env["own"], 800, construction, 0)
    B = _roadmap(ctx, env["own"], 800, construction, 0)
    d = A.export()
    goals = _pick_far(d["verts"], start, d["knn"].shape[1], env["pool"][300:], 64)
    r1, sim1, info = _check(ctx, A, B, start, goals, label=f"g first call construction={construction}", pristine=True,
                            own_solve=False)
    r2, sim2, info2 = _check(ctx, A, None, start, goals, label=f"g second call construction={construction}",
                             pristine=False, inputs=info["inputs"])
    assert r2["stats"]["removed"] == sim2["removed"] == \
        len(sim2["removed_edges"]) + len(sim2["removed_start"]) + len(sim2["dropped"])
    print(f"MANY_SWEEP g second call construction={construction}: removed again {r2['stats']['removed']} of which "
          f"roadmap edges {len(sim2['removed_edges'])}, first call {r1['stats']['removed']}")
    if not sim2["dropped"] and not sim2["removed_start"]:
        assert r2["stats"]["removed"] == 0
    if construction == 0:
        assert sim2["removed_edges"] == []
    else:
        assert len(sim1["removed_edges"]) > 0 and r2["stats"]["removed"] < r1["stats"]["removed"]
    assert 0 < r2["stats"]["motions"] < r1["stats"]["motions"]
    assert np.array_equal(r1["status"], r2["status"]) and r1["cost"].tobytes() == r2["cost"].tobytes()
    A.close()
    B.close()


def test_call_after_the_roadmaps_own_solve(env):
    """A.solve() fills the verdict cache (valid for this map and edge list): the call reads it, and checks fewer motions"""
    ctx, start = env["ctx"], env["start"]
    A = _roadmap(ctx, env["own"], 800, 2, 0)
    B = _roadmap(ctx, env["own"], 800, 2, 0)
    for cand in env["pool"][::97][:16]:  # a query of its own from the same start that solves after lazy removals
        A.set_query(start, cand)
        path0, cost0, rep0 = A.solve()
        if path0 is not None and rep0 > 0:
            break
    assert path0 is not None and rep0 > 0
    d = A.export()
    goals = _pick_far(d["verts"], start, d["knn"].shape[1], env["pool"][300:], 64)
    res, sim, _ = _check(ctx, A, B, start, goals, label="g after solve", pristine=False, cost0=cost0)
    assert res["stats"]["motions"] < sim["motions"], "no cached verdict was used"
    A.close()
    B.close()


def test_call_after_a_map_change_and_revalidate(env):
    """A block raised in the middle of the map, then revalidate(): some vertices are invalid for every list, edge
    usability is the re-evaluated one, the verdict cache is stale.  No path visits an invalid vertex."""
    ctx, gm, start = env["ctx"], env["gm"], env["start"]
    A = _roadmap(ctx, env["own"], 800)
    B = _roadmap(ctx, env["own"], 800)
    A.solve()  # verdicts of the old map in the cache
    ix = int(0.5 * gm.len_x / gm.res)
    iy = int(0.5 * gm.len_y / gm.res)
    r0, c0 = ix - 20, iy - 20
    saved = []
    for slot, name in ((0, "elevation"), (1, "elevation_masked")):
        patch0 = np.asfortranarray(gm[name][r0:r0 + 40, c0:c0 + 40])
        saved.append((slot, patch0))
        patch = (np.where(np.isfinite(patch0), patch0, np.float32(0)) + np.float32(0.6) if slot == 0
                 else np.full_like(patch0, -np.inf))
        ctx.update_layer_rect(slot, np.asfortranarray(patch), r0, c0)
    try:
        info = A.revalidate()
        B.revalidate()
        V = A.export()["verts"]
        vinvalid = ctx.validate_states(V) == 0
        vinvalid[:2] = False
        assert vinvalid.sum() >= 1 and info["invalid_vertices"] >= vinvalid.sum()
        pool = env["pool"][300:]
        pool = pool[ctx.validate_states(pool) != 0]
        goals = _pick_far(V, start, A.export()["knn"].shape[1], pool, 64, vinvalid=vinvalid)
        res, sim, _ = _check(ctx, A, B, start, goals, label="g after revalidate", pristine=True, vinvalid=vinvalid)
        assert (res["status"] == 0).sum() >= 16
    finally:
        for slot, patch0 in saved:
            ctx.update_layer_rect(slot, patch0, r0, c0)
    A.close()
    B.close()


# ---- h. the device-search threshold ------------------------------------------------------------------------------------

def test_fallback_restore_at_the_device_search_threshold(env):
    """ARTP_SSSP_MIN_VERTICES milestones: the near goals' solve runs the device search and the restore drops its device
    graph; afterwards the roadmap's own solve() is what it was, bit for bit."""
    ctx, start = env["ctx"], env["start"]
    A = _roadmap(ctx, env["own"], SSSP_MIN_VERTICES)
    B = _roadmap(ctx, env["own"], SSSP_MIN_VERTICES)
    for cand in env["pool"][::97][:16]:  # a query of its own that has a path
        A.set_query(start, cand)
        path0, cost0, _ = A.solve()
        if path0 is not None:
            break
    assert path0 is not None
    d = A.export()
    V, k = d["verts"], d["knn"].shape[1]
    assert len(V) >= SSSP_MIN_VERTICES
    nearest = V[2 + np.argsort(G.se3_distance(start[None], V[2:])[0], kind="stable")[:2]]
    goals = np.concatenate([_pick_far(V, start, k, env["pool"][300:], 64), nearest])
    res, sim, info = _check(ctx, A, B, start, goals, label="h threshold", pristine=False, cost0=cost0)
    assert res["stats"]["fallback"] == 2 and np.all(res["status"][64:] == 0)
    A.close()
    B.close()
