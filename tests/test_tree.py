"""The batch-synchronous tree planners (include/artp_c.h artp_tree_*: rrt_star, inf_rrt_star, rrt_sharp).  OMPL is not
available here, so every stage is checked against an independent restatement: the sampler and the interpolation against
the C oracle, nearest / near sets against numpy brute force, motion verdicts against the CPU oracle's discrete motion
validator, costs against a numpy PathLengthObjective, the RRT# costs against scipy's Dijkstra."""
import numpy as np
import pytest

import common
import oracle_py as O

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF


def _se3_distance(a, b):
    """OMPL SE3StateSpace::distance: R^3 L2 + SO3 arc length."""
    dp = np.sqrt(((a[:, None, :3] - b[None, :, :3]) ** 2).sum(-1))
    dq = np.abs((a[:, None, 3:] * b[None, :, 3:]).sum(-1))
    arc = np.where(dq > 1.0 - 1e-9, 0.0, np.arccos(np.minimum(dq, 1.0)))
    return dp + arc


def _yaw(q):  # getYawFromSO3: the double atan2 rounded to float
    return np.float64(np.float32(np.arctan2(2.0 * (q[:, 3] * q[:, 2] + q[:, 0] * q[:, 1]),
                                            1.0 - 2.0 * (q[:, 1] ** 2 + q[:, 2] ** 2))))


def _motion_cost(a, b, objective, lon=0.5, lat=0.1, ang=0.5):
    """PathLengthObjective::motionCost (path_length_objective.cpp:26-70), rows a -> b."""
    a, b = np.atleast_2d(a), np.atleast_2d(b)
    d = b[:, :3] - a[:, :3]
    if objective == 0:
        return np.sqrt((d ** 2).sum(-1)) / lon
    y1, y2 = _yaw(a[:, 3:]), _yaw(b[:, 3:])
    dy = np.abs(y1 - y2)
    dy = np.where(dy > np.pi, 2 * np.pi - dy, dy)
    lon_d = np.cos(y1) * d[:, 0] + np.sin(y1) * d[:, 1]
    lat_d = -np.sin(y1) * d[:, 0] + np.cos(y1) * d[:, 1]
    return np.maximum(np.maximum(np.abs(lon_d) / lon, np.abs(lat_d) / lat), dy / ang)


def _h(a, b):
    return np.sqrt(((np.atleast_2d(b)[:, :3] - np.atleast_2d(a)[:, :3]) ** 2).sum(-1)) / 0.5


def _k(n):
    return int(np.ceil(1.1 * (np.e + np.e / 6.0) * np.log(n + 1)))


def _check_tree_shape_and_fold(d):
    """Parent array: a tree rooted at 0 (no cycles, every vertex reaches 0); cost == the left fold of the edge costs
    from the root, bit for bit."""
    par, ec, cost = d["parent"].astype(np.int64), d["edge_cost"], d["cost"]
    n = len(par)
    assert par[0] == NONE and cost[0] == 0.0
    fold = np.full(n, np.nan)
    fold[0] = 0.0
    for v in range(1, n):
        chain = []
        u = v
        while u != 0 and np.isnan(fold[u]):
            chain.append(u)
            assert len(chain) <= n and 0 <= par[u] < n, f"vertex {v}: parent chain does not reach the root"
            u = int(par[u])
        for w in reversed(chain):
            fold[w] = fold[par[w]] + ec[w]
    assert np.array_equal(fold, cost), "cost-to-come differs from the left fold along the parents"


def _range(ctx, gm):
    elev = gm["elevation"]
    fin = elev[np.isfinite(elev)]
    ez = float(fin.max()) - float(fin.min()) + ctx.params.reach_z
    return 0.2 * (np.sqrt((2 * gm.len_x) ** 2 + (2 * gm.len_y) ** 2 + ez ** 2) + 0.5 * np.pi)


def _valid_state_near(ctx, xy):
    se3 = ctx.sample_states(99, 0, 1 << 16)
    cand = se3[ctx.validate_states(se3) != 0]
    return cand[np.argmin(np.hypot(cand[:, 0] - xy[0], cand[:, 1] - xy[1]))]


@pytest.fixture(scope="module")
def setup200():
    from art_planner_amd.context import Context
    from synthetic import make_map
    gm = make_map(200, 0.04, seed=5)
    ctx = Context(0, "yaml")
    ctx.upload_map(gm)
    start = _valid_state_near(ctx, (gm.pos_x - 2.6, gm.pos_y - 2.6))
    goal = _valid_state_near(ctx, (gm.pos_x + 2.6, gm.pos_y + 2.6))
    yield gm, ctx, start, goal
    ctx.close()


@pytest.fixture(scope="module")
def setup_c1():
    """BASELINE config C1's query: flat 100 x 100 @ 0.1 m, (-4, -4, yaw 0) -> (4, 4)."""
    from art_planner_amd.context import Context
    from synthetic import make_map
    gm = make_map(100, 0.1, flat=True)
    ctx = Context(0, "yaml")
    ctx.upload_map(gm)
    probe = ctx.sample_states(1, 0, 64)
    z0 = float(probe[ctx.validate_states(probe) != 0][0, 2])
    s = np.array([-4.0, -4.0, z0, 0, 0, 0, 1.0])
    g = np.array([4.0, 4.0, z0, 0, 0, 0, 1.0])
    yield gm, ctx, s, g
    ctx.close()


def _grow_per_batch(tree, n):
    """Exports (tree, checked motions) before the first batch and after each of n batches."""
    out = [(tree.export(), tree.export_checked(), tree.solve()[1])]
    for _ in range(n):
        tree.grow(1)
        out.append((tree.export(), tree.export_checked(), tree.solve()[1]))
    return out


@pytest.mark.parametrize("objective", [0, 1])
def test_rrt_star_stages_against_restatements(setup200, objective):
    from art_planner_amd.tree import Tree
    gm, ctx, start, goal = setup200
    rob, om = O.robot("yaml"), O.OracleMap(gm)
    smp = O.OracleSampler(gm)
    B, seed, first = 256, 17, 1000
    tree = Tree(ctx, start, goal, "rrt_star", seed=seed, first_index=first, batch=B, objective=objective)
    rng_ = _range(ctx, gm)
    hist = _grow_per_batch(tree, 4)
    tree.close()
    verdict_u, verdict_v, verdict_ok, verdict_V = [], [], [], None
    for b in range(1, len(hist)):
        P, _, _ = hist[b - 1]
        C_, L, _ = hist[b]
        n_pre, n_now = len(P["verts"]), len(C_["verts"])
        assert n_now > n_pre
        V = C_["verts"]
        assert np.array_equal(V[:n_pre], P["verts"]) and np.all(C_["born"][n_pre:] == b - 1)
        # 1. the samples: the CPU sampler's states of this batch (slot 0 = the goal while it is not a vertex)
        samp, _ = smp.sample(rob, seed, first + (b - 1) * B, B)
        dev = ctx.sample_states(seed, first + (b - 1) * B, B)
        assert np.abs(samp - dev).max() < 1e-12
        goal_in = hist[b - 1][2] < np.inf
        if not goal_in:
            samp[0] = goal
        # 2. nearest (brute force) and steering
        D = _se3_distance(samp, P["verts"])
        nn = np.argmin(D, axis=1)
        dn = D[np.arange(B), nn]
        xnew = np.array([O.interpolate(P["verts"][nn[s]], samp[s], rng_ / dn[s]) if dn[s] > rng_ else samp[s]
                         for s in range(B)])
        # the new vertices are steered samples, in slot order
        dx = np.abs(V[n_pre:, None, :] - xnew[None, :, :]).max(-1)
        slot = np.argmin(dx, axis=1)
        assert dx[np.arange(len(slot)), slot].max() <= 1e-12
        assert np.all(np.diff(slot) > 0)
        # motions of this batch
        sel = L["batch"] == b - 1
        lu, lv, lok = L["u"][sel].astype(np.int64), L["v"][sel].astype(np.int64), L["valid"][sel]
        k = _k(n_pre)
        for j, v in enumerate(range(n_pre, n_now)):
            mine = np.flatnonzero(lv == v)
            us = lu[mine]
            # the first motion is the one from the nearest vertex (a tie in distance may pick the other id)
            s = slot[j]
            assert us[0] == nn[s] or abs(D[s, us[0]] - dn[s]) < 1e-12
            assert lok[mine[0]] == 1
            # near set: the exact k nearest pre-batch vertices of x_new (plus the nearest)
            Dx = _se3_distance(V[v:v + 1], P["verts"])[0]
            order = np.lexsort((np.arange(n_pre), Dx))[:k]
            want = set(order.tolist()) | {int(us[0])}
            got = set(us.tolist())
            if got != want:  # only near-ties may differ
                kth = Dx[order[-1]]
                assert all(abs(Dx[u] - kth) < 1e-12 for u in got ^ want), (b, v)
            assert len(us) == len(got)
            # parent choice: argmin over the valid candidates of cost(u) + c(u, x_new) with pre-batch costs
            ok_u = us[lok[mine] == 1]
            vals = P["cost"][ok_u] + _motion_cost(P["verts"][ok_u], np.repeat(V[v:v + 1], len(ok_u), 0), objective)
            par = int(C_["parent"][v])
            assert par in ok_u.tolist()
            assert P["cost"][par] + _motion_cost(P["verts"][par], V[v], objective)[0] <= vals.min() * (1 + 1e-12) + 1e-15
        # rewiring: with the costs parent choice gave the new vertices, no valid motion (u pre-batch, v new) is left
        # that would have lowered cost(u) below what u got
        cv0 = np.full(n_now, np.nan)
        cv0[n_pre:] = P["cost"][C_["parent"][n_pre:]] + C_["edge_cost"][n_pre:]
        got_u = P["cost"].copy()
        rew = np.flatnonzero(C_["parent"][1:n_pre] != P["parent"][1:n_pre]) + 1
        assert np.all(C_["parent"][rew] >= n_pre)
        got_u[rew] = cv0[C_["parent"][rew]] + C_["edge_cost"][rew]
        m = (lok == 1) & (lv != NONE) & (lv >= n_pre)
        cand = cv0[lv[m]] + _motion_cost(V[lv[m]], P["verts"][lu[m]], objective)
        assert np.all(got_u[lu[m]] <= cand * (1 + 1e-12) + 1e-15)
        assert np.all(got_u[rew] < P["cost"][rew])
        # edge costs: the numpy PathLengthObjective
        ref = _motion_cost(V[C_["parent"][1:]], V[1:], objective)
        assert np.all(np.abs(C_["edge_cost"][1:] - ref) <= 1e-12 * np.maximum(ref, 1e-300))
        _check_tree_shape_and_fold(C_)
        # the goal is a vertex once a batch steered exactly onto it (and only then)
        if hist[b][2] < np.inf:
            gid = np.flatnonzero((V == goal).all(1))
            assert len(gid) == 1 and C_["cost"][gid[0]] == hist[b][2]
        else:
            assert not (V == goal).all(1).any()
        keep = lv != NONE
        verdict_u.append(lu[keep])
        verdict_v.append(lv[keep])
        verdict_ok.append(lok[keep])
        verdict_V = V
    # verdicts: every tree edge and up to 2e4 checked motions against the oracle's discrete motion validator
    final = hist[-1][0]
    V = final["verts"]
    par = final["parent"][1:].astype(np.int64)
    assert om.check_motions(rob, V[par], V[1:])[0].all()
    u, v, ok = np.concatenate(verdict_u), np.concatenate(verdict_v), np.concatenate(verdict_ok)
    assert 0.02 < ok.mean() < 0.999
    sub = np.random.default_rng(0).choice(len(u), min(len(u), 20000), replace=False)
    vo = om.check_motions(rob, verdict_V[u[sub]], verdict_V[v[sub]])[0]
    assert np.array_equal(vo.astype(np.uint8), ok[sub])


def test_rrt_sharp_costs_are_shortest_paths(setup200):
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import dijkstra
    from art_planner_amd.tree import Tree
    gm, ctx, start, goal = setup200
    tree = Tree(ctx, start, goal, "rrt_sharp", seed=5, batch=512)
    for _ in range(4):
        tree.grow(1)
        d, L = tree.export(), tree.export_checked()
        _check_tree_shape_and_fold(d)
        V, n = d["verts"], len(d["verts"])
        m = (L["valid"] == 1) & (L["v"] != NONE)
        u, v = L["u"][m].astype(np.int64), L["v"][m].astype(np.int64)
        w_uv, w_vu = _motion_cost(V[u], V[v], 0), _motion_cost(V[v], V[u], 0)
        W = csr_matrix((np.concatenate([w_uv, w_vu]), (np.concatenate([u, v]), np.concatenate([v, u]))), shape=(n, n))
        ref = dijkstra(W, directed=True, indices=0)
        assert np.abs(d["cost"] - ref).max() <= 1e-9 * max(1.0, ref.max())
        # the parent is a predecessor on a shortest path
        par = d["parent"][1:].astype(np.int64)
        assert np.abs(d["cost"][par] + _motion_cost(V[par], V[1:], 0) - d["cost"][1:]).max() < 1e-9
    tree.close()


def test_inf_rrt_star_rejection_and_pruning(setup_c1):
    from art_planner_amd.tree import Tree
    gm, ctx, s, g = setup_c1
    tree = Tree(ctx, s, g, "inf_rrt_star", seed=3, batch=512)
    hist = _grow_per_batch(tree, 10)
    st = tree.stats()
    tree.close()
    fb = st["first_solution_batch"]
    assert fb is not None and fb < 8
    costs = [h[2] for h in hist]
    assert all(b <= a for a, b in zip(costs[1:], costs[2:]))
    n_pruned_checked = 0
    for b in range(fb + 2, len(hist)):
        P, _, c_best = hist[b - 1]
        C_, L, _ = hist[b]
        V = C_["verts"]
        new = np.flatnonzero(C_["born"] == b - 1)
        assert np.all(_h(s, V[new]) + _h(V[new], g) < c_best)
        # no vertex pruned before this batch is a nearest / near candidate in it
        used = L["u"][L["batch"] == b - 1]
        pruned = np.flatnonzero(P["pruned"])
        assert not np.isin(used, pruned).any()
        n_pruned_checked += len(pruned)
        # pruning rule after the batch
        cb = hist[b][2]
        h_all = _h(s, V) + _h(V, g)
        expect = h_all >= cb
        expect[0] = False
        expect[st["goal"]] = False
        prev = np.zeros(len(V), bool)
        prev[:len(P["pruned"])] = P["pruned"] != 0
        assert np.array_equal(C_["pruned"] != 0, expect | prev)
    assert n_pruned_checked > 0
    assert st["pruned"] > 0


# Batch budget of the convergence test, from a measured run (profiles/tree_time.txt, C1 at B = 1024: every variant
# reaches the goal in batch 1 at the straight-line cost, 1.0000 x, and holds it through batch 30)
CONVERGENCE_BATCHES = 10


@pytest.mark.parametrize("variant", ["rrt_star", "inf_rrt_star", "rrt_sharp"])
def test_convergence_on_flat_c1(setup_c1, variant):
    from art_planner_amd.tree import Tree
    gm, ctx, s, g = setup_c1
    optimum = np.linalg.norm(g[:3] - s[:3]) / 0.5
    tree = Tree(ctx, s, g, variant, seed=42, batch=1024)
    best = []
    for _ in range(CONVERGENCE_BATCHES):
        tree.grow(1)
        best.append(tree.solve()[1])
    path, cost = tree.solve()
    assert all(b <= a for a, b in zip(best, best[1:])), best
    assert cost <= 1.03 * optimum, (variant, cost, optimum, best)
    assert np.array_equal(path[0], s) and np.array_equal(path[-1], g)
    # the simplified path is never costlier
    _, c_simple = tree.simplify(path)
    assert c_simple <= cost * (1 + 1e-9)
    tree.close()


@pytest.mark.parametrize("variant", ["rrt_star", "inf_rrt_star", "rrt_sharp"])
def test_deterministic_exports(setup200, variant):
    from art_planner_amd.tree import Tree
    gm, ctx, start, goal = setup200
    outs = []
    for _ in range(2):
        t = Tree(ctx, start, goal, variant, seed=9, batch=1024)
        t.grow(5)
        d, L = t.export(), t.export_checked()
        outs.append(b"".join(a.tobytes() for a in list(d.values()) + list(L.values())) + repr(t.stats()).encode())
        t.close()
    assert outs[0] == outs[1]


def test_invalid_arguments(setup200):
    from art_planner_amd.tree import Tree
    from art_planner_amd._capi import ArtpError
    gm, ctx, start, goal = setup200
    with pytest.raises(ArtpError) as e:
        Tree(ctx, start, goal, "rrt_star", objective=2)
    assert e.value.status == -1
    bad = start.copy()
    bad[2] += 5.0  # far above the ground: the feet cannot reach it
    with pytest.raises(ArtpError) as e:
        Tree(ctx, bad, goal, "rrt_star")
    assert e.value.status == -1 and "start" in str(e.value)
    t = Tree(ctx, start, goal, "rrt_star", batch=64)
    assert t.solve() == (None, float("inf"))
    st = t.stats()
    assert st["vertices"] == 1 and st["goal"] is None and st["first_solution_batch"] is None
    with pytest.raises(ArtpError):
        t.grow(0)  # no budget at all
    t.close()


def test_plan_time_and_max_vertices(setup_c1):
    from art_planner_amd.tree import Tree
    gm, ctx, s, g = setup_c1
    t = Tree(ctx, s, g, "rrt_star", batch=256, max_vertices=600)
    out = t.grow(1000)
    assert out["vertices"] == 600 and out["batches"] < 1000
    t.close()
    t = Tree(ctx, s, g, "rrt_star", batch=256, plan_time=0.01)
    out = t.grow(0)
    assert out["batches"] >= 1
    t.close()
