"""The batch-synchronous tree planners (include/artp_c.h artp_tree_*: rrt_star, inf_rrt_star, rrt_sharp).  OMPL is not
available here, so every stage is checked against an independent restatement: the sampler and the interpolation against
the C oracle, nearest / near sets against numpy brute force, motion verdicts against the CPU oracle's discrete motion
validator, costs against a numpy PathLengthObjective, the RRT# costs against scipy's Dijkstra."""
import numpy as np
import pytest

import oracle_py as O
from graph_ref import NONE, check_tree_batches, check_tree_shape_and_fold as _check_tree_shape_and_fold
from graph_ref import grow_per_batch as _grow_per_batch, motion_cost as _motion_cost

pytestmark = pytest.mark.gpu


def _h(a, b):
    return np.sqrt(((np.atleast_2d(b)[:, :3] - np.atleast_2d(a)[:, :3]) ** 2).sum(-1)) / 0.5


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


@pytest.mark.parametrize("objective", [0, 1])
def test_rrt_star_stages_against_restatements(setup200, objective):
    from art_planner_amd.tree import Tree
    gm, ctx, start, goal = setup200
    rob, om = O.robot("yaml"), O.OracleMap(gm)
    B, seed, first = 256, 17, 1000
    tree = Tree(ctx, start, goal, "rrt_star", seed=seed, first_index=first, batch=B, objective=objective)
    hist = _grow_per_batch(tree, 4)
    tree.close()
    u, v, ok, verdict_V = check_tree_batches(ctx, gm, hist, B, seed, first, objective, goal)
    # verdicts: every tree edge and up to 2e4 checked motions against the oracle's discrete motion validator
    final = hist[-1][0]
    V = final["verts"]
    par = final["parent"][1:].astype(np.int64)
    assert om.check_motions(rob, V[par], V[1:])[0].all()
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
