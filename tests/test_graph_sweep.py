"""The planners' graph kernels across sizes, shapes and limits, against float64 numpy / scipy restatements
(tests/graph_ref.py):
  1. the roadmap's k-NN grid (knn_cell_ids / knn_permute / knn_kernel, the edge keys and their sort / unique) against a
     (distance, index) brute force: square, non-square and one-cell grids, 1 .. 40 000 milestones, k from 1 to the
     128 clamp, construction 2's predecessor lists, set_query and grow;
  2. the device shortest paths of roadmaps of >= ARTP_SSSP_MIN_VERTICES (30 000) vertices against scipy's Dijkstra, and
     the reported cost against the left fold of the path's edge costs, bit for bit: every objective, lazy removals,
     a re-validated map, an unreachable goal, and both sides of the threshold;
  3. the tree planners at ragged and limit batch sizes (1 .. 65 536), a full 64-entry near set, inf_rrt_star's pruned
     vertices, and rrt_sharp's single-workgroup search over a log of more than 50 000 motions."""
import numpy as np
import pytest

import graph_ref as G
import oracle_py as O

pytestmark = pytest.mark.gpu

SSSP_MIN_VERTICES = 30000  # roadmap.h ARTP_SSSP_MIN_VERTICES


def _crop(gm, i0, j0, nr, nc):
    """nr x nc crop of a map (rows != cols), the sampler's distribution recomputed (test_gpu_parity's non-square map)."""
    from synthetic import GridMap, cumulative_distribution
    out = GridMap(nr, nc, gm.res)
    out.pos_x = float(gm.cell_x()[i0:i0 + nr].mean())
    out.pos_y = float(gm.cell_y()[j0:j0 + nc].mean())
    for k, v in gm.layers.items():
        if v.ndim == 2:
            out.layers[k] = np.asfortranarray(v[i0:i0 + nr, j0:j0 + nc])
    cp, cr = cumulative_distribution(out["sample_probability"])
    out.layers["cum_prob"] = np.asfortranarray(cp)
    out.layers["cum_prob_rowwise"] = np.ascontiguousarray(cr, np.float32)
    return out


def _ring_map():
    """Flat 16 x 16 m map with a 1.6 m wide ring of untraversable raised terrain around a 3 x 3 m pocket: no valid state
    and no motion crosses it."""
    from synthetic import make_map
    gm = make_map(400, 0.04, flat=True)
    n = gm.rows
    c = n // 2 + 100                      # pocket centre: 4 m towards -x, -y of the map centre (rows / cols grow that way)
    inner, outer = 37, 37 + 40
    ii, jj = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    cheb = np.maximum(np.abs(ii - c), np.abs(jj - c))
    ring = (cheb > inner) & (cheb <= outer)
    for name in ("elevation", "elevation_masked"):
        lay = np.array(gm[name], np.float32)
        lay[ring] = np.float32(0.6) if name == "elevation" else -np.inf
        gm.layers[name] = np.asfortranarray(lay)
    centre = (float(gm.cell_x()[c]), float(gm.cell_y()[c]))
    return gm, centre


def _make(name):
    from synthetic import make_map
    if name == "sq200":
        return make_map(200, 0.04, seed=5)
    if name == "crop300x90":
        return _crop(make_map(400, 0.04, seed=1234), 40, 150, 300, 90)
    if name == "crop90x300":
        return _crop(make_map(400, 0.04, seed=1234), 150, 40, 90, 300)
    if name == "tiny":
        return make_map(30, 0.1, flat=True)
    if name == "flat100":
        return make_map(100, 0.1, flat=True)
    if name == "sq400":
        return make_map(400, 0.04, seed=1234)
    if name == "sq800":
        return make_map(800, 0.04, seed=77)
    raise KeyError(name)


class _Maps:
    """One context per map, made on first use; four valid states nearest the map's corners."""

    def __init__(self):
        self.cache = {}

    def __call__(self, name):
        if name not in self.cache:
            from art_planner_amd.context import Context
            gm = _make(name)
            ctx = Context(0, "yaml")
            ctx.upload_map(gm)
            se3 = ctx.sample_states(99, 0, 1 << 16)
            acc = se3[ctx.validate_states(se3) != 0]
            corners = []
            for sx, sy in ((-1, -1), (1, 1), (1, -1), (-1, 1)):
                cx, cy = gm.pos_x + sx * 0.5 * gm.len_x, gm.pos_y + sy * 0.5 * gm.len_y
                corners.append(acc[np.argmin(np.hypot(acc[:, 0] - cx, acc[:, 1] - cy))])
            self.cache[name] = (gm, ctx, corners)
        return self.cache[name]

    def close(self):
        for _, ctx, _ in self.cache.values():
            ctx.close()
        self.cache.clear()


@pytest.fixture(scope="module")
def maps():
    m = _Maps()
    yield m
    m.close()


def _rows(nv, n_check, seed=0):
    """every row, or start, goal, the first 64 and a seeded subset of n_check rows"""
    if nv <= n_check:
        return np.arange(nv)
    sub = np.random.default_rng(seed).choice(np.arange(64, nv), n_check, replace=False)
    return np.unique(np.concatenate([np.arange(64), sub]))


def _check_roadmap_knn(rm, k_neighbors, construction=0, n_check=3200):
    st, d = rm.stats(), rm.export()
    nv, k = int(st["vertices"]), int(st["k"])
    assert k == G.roadmap_k(k_neighbors, nv), (k, k_neighbors, nv)
    V = d["verts"]
    k_of = G.construction2_k_of(k_neighbors, nv) if construction == 2 else np.full(nv, k)
    rows = _rows(nv, n_check)
    G.check_knn_rows(V, rows, d["knn"][rows], d["knn_dist"][rows], k_of[rows], pred_only=construction == 2)
    # candidate edges: the sorted unique symmetrised pairs (construction 2: (predecessor, i), predecessor < i)
    assert np.array_equal(d["edges"], G.symmetrised_edges(d["knn"]))
    if construction == 2:
        m = d["knn"] != G.NONE
        assert np.all(d["knn"][m] < np.repeat(np.arange(nv), k).reshape(nv, k)[m])
    return nv, k, d


KNN_CASES = [
    ("sq200", 1, 0), ("sq200", 2, 0), ("sq200", 5, 0), ("sq200", 63, 0), ("sq200", 64, 0), ("sq200", 65, 0),
    ("sq200", 3000, 0), ("sq200", 3000, 1), ("sq200", 3000, 127), ("sq200", 3000, 128), ("sq200", 3000, 200),
    ("sq200", 5, 7), ("sq200", 63, 1000),
    ("crop300x90", 3000, 0), ("crop90x300", 3000, 0), ("crop300x90", 3000, 128), ("crop90x300", 65, 100),
    ("tiny", 1, 0), ("tiny", 2, 0), ("tiny", 5, 0), ("tiny", 5, 50),
    ("sq800", 40000, 0),
]


@pytest.mark.parametrize("name,n_ms,k_nb", KNN_CASES)
def test_roadmap_knn_against_bruteforce(maps, name, n_ms, k_nb):
    """Start and goal sit at opposite corners: their rings walk to the grid's edge (clamped cells)."""
    from art_planner_amd.roadmap import Roadmap
    gm, ctx, corners = maps(name)
    rm = Roadmap(ctx, corners[0], corners[1], n_milestones=n_ms, seed=7, k_neighbors=k_nb)
    nv, k, d = _check_roadmap_knn(rm, k_nb)
    rm.close()
    assert nv == n_ms + 2
    assert np.array_equal(d["verts"][0], corners[0]) and np.array_equal(d["verts"][1], corners[1])
    if k_nb >= 128 and nv > 128:
        assert k == 128
    if k_nb >= nv:
        assert k == nv - 1 and np.all(d["knn"] != G.NONE)
    if name == "tiny" and n_ms == 1:
        assert G.knn_grid_dims(gm.len_x, gm.len_y, nv) == (1, 1)


@pytest.mark.parametrize("n_ms", [3000, 20000])
def test_construction_2_predecessor_lists_against_bruteforce(maps, n_ms):
    from art_planner_amd.roadmap import Roadmap
    gm, ctx, corners = maps("sq200")
    rm = Roadmap(ctx, corners[0], corners[1], n_milestones=n_ms, seed=42, construction=2)
    nv, k, d = _check_roadmap_knn(rm, 0, construction=2)
    rm.close()
    assert nv == n_ms + 2


def test_set_query_and_grow_lists_against_bruteforce(maps):
    """set_query: rows 0 and 1 (the host's partial_sort) are the brute force's, the edges touching them are their
    symmetrised pairs and every other edge stays; grow: the rebuilt lists are the brute force over the new vertex set."""
    from art_planner_amd.roadmap import Roadmap
    gm, ctx, corners = maps("sq200")
    rm = Roadmap(ctx, corners[0], corners[1], n_milestones=3000, seed=3)
    before = rm.export()
    rm.set_query(corners[2], corners[3])
    st, d = rm.stats(), rm.export()
    k = int(st["k"])
    V = d["verts"]
    assert np.array_equal(V[0], corners[2]) and np.array_equal(V[1], corners[3])
    assert np.array_equal(V[2:], before["verts"][2:])
    G.check_knn_rows(V, np.arange(2), d["knn"][:2], d["knn_dist"][:2], k)
    q = np.full_like(d["knn"], G.NONE)
    q[:2] = d["knn"][:2]
    head = G.symmetrised_edges(q)
    old = before["edges"][before["edges"][:, 0] >= 2]
    assert np.array_equal(d["edges"], np.concatenate([head, old]))
    out = rm.grow(1000)
    assert out["kept"] == 3000 and out["dropped"] == 0
    nv, k2, d2 = _check_roadmap_knn(rm, 0)
    assert nv == 4002 and np.array_equal(d2["verts"][:3002], V)
    rm.close()


# ---- 2. device shortest paths -----------------------------------------------------------------------------------------

def _check_solve(rm, path, cost, n_vertices_min=SSSP_MIN_VERTICES):
    """cost == scipy's Dijkstra over the usable edges within 1e-12 relative; bit-equal to the left fold of the path's
    edge costs; every consecutive pair a usable edge.  Returns the scipy distance of the goal."""
    from scipy.sparse.csgraph import dijkstra
    e = rm.export()
    nv = len(e["verts"])
    assert nv >= n_vertices_min
    w = e["edge_cost"]
    ok = (e["edge_valid"] != 0) & (e["edge_removed"] == 0) & np.isfinite(w) & (w >= 0.0)
    eu, ev = e["edges"][:, 0].astype(np.int64), e["edges"][:, 1].astype(np.int64)
    W = G.min_weight_csr(eu[ok], ev[ok], w[ok], nv)
    ref = dijkstra(W, directed=False, indices=0)[1]
    if path is None:
        assert np.isinf(ref) and np.isinf(cost)
        return ref
    assert abs(cost - ref) <= 1e-12 * ref, (cost, ref)
    assert np.array_equal(path[0], e["verts"][0]) and np.array_equal(path[-1], e["verts"][1])
    row = {e["verts"][i].tobytes(): i for i in range(nv - 1, 1, -1)}
    idx = np.array([0] + [row[p.tobytes()] for p in path[1:-1]] + [1], np.int64)
    a, b = np.minimum(idx[:-1], idx[1:]), np.maximum(idx[:-1], idx[1:])
    keys = (eu << 32) | ev
    pos = np.searchsorted(keys, (a << 32) | b)
    assert np.all(pos < len(keys)) and np.array_equal(keys[np.minimum(pos, len(keys) - 1)], (a << 32) | b)
    assert ok[pos].all(), "the path uses an edge that is not usable"
    assert G.left_fold(w[pos]) == cost, "cost differs from the left fold of the path's edge costs"
    return ref


def _corner_pair(ctx, gm):
    se3 = ctx.sample_states(1001, 0, 8000)  # a stream no roadmap here draws its milestones from
    acc = se3[ctx.validate_states(se3) != 0]
    return acc[np.argmin(acc[:, 0] + acc[:, 1])], acc[np.argmax(acc[:, 0] + acc[:, 1])]


@pytest.mark.parametrize("objective", [0, 1])
def test_device_search_objectives_and_revalidate(maps, objective):
    from art_planner_amd.roadmap import Roadmap
    gm, ctx, _ = maps("sq400")
    s, g = _corner_pair(ctx, gm)
    rm = Roadmap(ctx, s, g, n_milestones=34000, seed=11, objective=objective)
    path, cost, rep = rm.solve()
    assert path is not None
    _check_solve(rm, path, cost)
    assert rep == int(rm.export()["edge_removed"].sum())
    if objective == 1:
        rm.close()
        return
    # a block raised under the middle of the plan, then revalidate and search again
    mid = path[len(path) // 2]
    ix = int((gm.pos_x + 0.5 * gm.len_x - mid[0]) / gm.res)
    iy = int((gm.pos_y + 0.5 * gm.len_y - mid[1]) / gm.res)
    r0, c0 = max(ix - 10, 0), max(iy - 10, 0)
    saved = []
    for slot, name in ((0, "elevation"), (1, "elevation_masked")):
        patch0 = np.asfortranarray(gm[name][r0:r0 + 20, c0:c0 + 20])
        saved.append((slot, patch0))
        patch = (np.where(np.isfinite(patch0), patch0, np.float32(0)) + np.float32(0.6) if slot == 0
                 else np.full_like(patch0, -np.inf))
        ctx.update_layer_rect(slot, np.asfortranarray(patch), r0, c0)
    try:
        info = rm.revalidate()
        assert info["valid_edges_after"] < info["valid_edges_before"]
        path2, cost2, _ = rm.solve()
        assert path2 is not None and cost2 > cost
        _check_solve(rm, path2, cost2)
    finally:
        for slot, patch0 in saved:
            ctx.update_layer_rect(slot, patch0, r0, c0)
    rm.close()


def test_device_search_lazy_removals(maps):
    """construction 2 puts direct edges of unknown validity into the graph: the lazy path check removes edges and the
    device search runs again over the remaining ones, round after round."""
    from art_planner_amd.roadmap import Roadmap
    gm, ctx, _ = maps("sq400")
    s, g = _corner_pair(ctx, gm)
    rm = Roadmap(ctx, s, g, n_milestones=SSSP_MIN_VERTICES, seed=21, construction=2, max_replans=100000)
    path, cost, rep = rm.solve()
    assert rep > 0 and rep == int(rm.export()["edge_removed"].sum())
    assert path is not None
    _check_solve(rm, path, cost)
    rm.close()


def test_device_search_learned_objective(maps):
    import os
    import sys
    import common
    sys.path.insert(0, os.path.join(common.ROOT, "oracle"))
    sys.path.insert(0, os.path.join(common.ROOT, "tools"))
    import motion_cost_oracle as mo
    import convert_weights
    from art_planner_amd.roadmap import Roadmap
    gm, ctx, _ = maps("sq400")
    ctx.cost_load_weights(convert_weights.to_blob(mo.random_params(0)))
    elv = np.ascontiguousarray(gm["elevation"][::-1, ::-1]).astype(np.float32)
    ctx.cost_update_map(elv, gm.res, gm.len_x, gm.len_y, gm.pos_x, gm.pos_y)
    s, g = _corner_pair(ctx, gm)
    rm = Roadmap(ctx, s, g, n_milestones=SSSP_MIN_VERTICES, seed=5, k_neighbors=16, objective=2,
                 cost_weights=(0.25, 1.0, 5.0), risk_threshold=0.55)
    fin = np.isfinite(rm.export()["edge_cost"])
    assert 0.02 < fin.mean() < 0.98
    path, cost, _ = rm.solve()
    _check_solve(rm, path, cost)
    rm.close()


def test_device_search_unreachable_goal():
    from art_planner_amd.context import Context
    from art_planner_amd.roadmap import Roadmap
    gm, (cx, cy) = _ring_map()
    ctx = Context(0, "yaml")
    try:
        ctx.upload_map(gm)
        se3 = ctx.sample_states(3, 0, 1 << 16)
        acc = se3[ctx.validate_states(se3) != 0]
        g = acc[np.argmin(np.hypot(acc[:, 0] - cx, acc[:, 1] - cy))]
        assert np.hypot(g[0] - cx, g[1] - cy) < 0.5
        s = acc[np.argmax(np.hypot(acc[:, 0] - cx, acc[:, 1] - cy))]
        rm = Roadmap(ctx, s, g, n_milestones=SSSP_MIN_VERTICES, seed=9)
        path, cost, rep = rm.solve()
        assert path is None and np.isinf(cost)
        _check_solve(rm, path, cost)
        rm.close()
    finally:
        ctx.close()


@pytest.mark.parametrize("n_ms", [SSSP_MIN_VERTICES - 3, SSSP_MIN_VERTICES - 2])
def test_search_on_both_sides_of_the_device_threshold(maps, n_ms):
    """29 999 vertices: the host search; 30 000: the device search.  Both equal scipy's."""
    from art_planner_amd.roadmap import Roadmap
    gm, ctx, _ = maps("sq400")
    s, g = _corner_pair(ctx, gm)
    rm = Roadmap(ctx, s, g, n_milestones=n_ms, seed=31)
    path, cost, _ = rm.solve()
    assert path is not None
    _check_solve(rm, path, cost, n_vertices_min=n_ms + 2)
    rm.close()


# ---- 3. tree planners --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,n_batches", [(1, 45), (63, 12), (65, 12), (1000, 3)])
def test_rrt_star_ragged_batches(maps, B, n_batches):
    """Query counts that are not a multiple of the k-NN kernel's four waves, pre-batch vertex counts across its
    256-row tiles."""
    from art_planner_amd.tree import Tree
    gm, ctx, corners = maps("flat100")
    seed, first = 17, 500
    tree = Tree(ctx, corners[0], corners[1], "rrt_star", seed=seed, first_index=first, batch=B)
    hist = G.grow_per_batch(tree, n_batches)
    tree.close()
    G.check_tree_batches(ctx, gm, hist, B, seed, first, 0, corners[1], allow_empty=B == 1)
    if B > 1:
        assert len(hist[-1][0]["verts"]) > 256


def test_rrt_star_largest_batch(maps):
    """TREE_MAX_BATCH = 65 536 samples in one batch (the compaction's 64 flags per lane); 65 537 is refused."""
    from art_planner_amd.tree import Tree
    from art_planner_amd._capi import ArtpError
    gm, ctx, corners = maps("sq200")
    with pytest.raises(ArtpError):
        Tree(ctx, corners[0], corners[1], "rrt_star", batch=65537)
    B, seed, first = 65536, 23, 0
    tree = Tree(ctx, corners[0], corners[1], "rrt_star", seed=seed, first_index=first, batch=B, max_vertices=200000)
    hist = G.grow_per_batch(tree, 1)
    tree.close()
    assert len(hist[-1][0]["verts"]) > 1000
    u, v, ok, V = G.check_tree_batches(ctx, gm, hist, B, seed, first, 0, corners[1], max_vertices=200000, n_sub=300)
    om = O.OracleMap(gm)
    sub = np.random.default_rng(1).choice(len(u), min(len(u), 20000), replace=False)
    assert np.array_equal(om.check_motions(O.robot("yaml"), V[u[sub]], V[v[sub]])[0].astype(np.uint8), ok[sub])


def test_full_wave_near_set(maps):
    """rewire_factor with tree_k(rewire_factor, max_vertices) == TREE_KMAX = 64: accepted, and once the tree is large
    enough every new vertex has a full 64-entry near set; the next factor up (65) is refused."""
    from art_planner_amd.tree import Tree
    from art_planner_amd._capi import ArtpError
    gm, ctx, corners = maps("flat100")
    cap = 2000
    rf = 63.95 / ((G.E + G.E / 6.0) * np.log(cap + 1.0))
    assert G.tree_k(rf, cap) == 64
    rf65 = 64.5 / ((G.E + G.E / 6.0) * np.log(cap + 1.0))
    assert G.tree_k(rf65, cap) == 65
    with pytest.raises(ArtpError):
        Tree(ctx, corners[0], corners[1], "rrt_star", batch=256, max_vertices=cap, rewire_factor=rf65)
    B, seed, first = 256, 29, 0
    tree = Tree(ctx, corners[0], corners[1], "rrt_star", seed=seed, first_index=first, batch=B, max_vertices=cap,
                rewire_factor=rf)
    n_batches = 0
    while G.tree_k(rf, tree.stats()["vertices"]) < 64:
        tree.grow(1)
        n_batches += 1
        assert n_batches < 40 and tree.stats()["vertices"] < cap
    hist = G.grow_per_batch(tree, 1)
    tree.close()
    G.check_tree_batches(ctx, gm, hist, B, seed, first, 0, corners[1], rewire_factor=rf, max_vertices=cap,
                         batch0=n_batches)
    P, (C_, L, _) = hist[0][0], hist[1]
    n_pre = len(P["verts"])
    sel = (L["batch"] == n_batches) & (L["v"] != G.NONE) & (L["v"] >= n_pre)
    per_v = np.bincount(L["v"][sel].astype(np.int64) - n_pre)
    assert len(per_v) == len(C_["verts"]) - n_pre and np.all(per_v == 64)


def test_inf_rrt_star_pruned_vertices_are_no_candidates(maps):
    from art_planner_amd.tree import Tree
    gm, ctx, corners = maps("flat100")
    s, g = corners[0], corners[1]
    B, seed, first = 1000, 3, 0
    tree = Tree(ctx, s, g, "inf_rrt_star", seed=seed, first_index=first, batch=B)
    hist = G.grow_per_batch(tree, 8)
    st = tree.stats()
    tree.close()
    assert st["first_solution_batch"] is not None and st["pruned"] > 0
    G.check_tree_batches(ctx, gm, hist, B, seed, first, 0, g, variant=1, allow_empty=True)
    assert any(h[0]["pruned"].any() for h in hist[:-1])


def test_rrt_sharp_long_log(maps):
    """tree_sssp_kernel (one 1024-lane workgroup) over a log of more than 50 000 motions: the costs are scipy's directed
    Dijkstra over the valid logged motions and the left fold along the parents."""
    from scipy.sparse.csgraph import dijkstra
    from art_planner_amd.tree import Tree
    gm, ctx, corners = maps("sq200")
    tree = Tree(ctx, corners[0], corners[1], "rrt_sharp", seed=5, batch=1024)
    while True:
        tree.grow(1)
        if tree.stats()["motions_checked"] >= 50000:
            break
    d, L = tree.export(), tree.export_checked()
    tree.close()
    assert len(L["u"]) >= 50000
    G.check_tree_shape_and_fold(d)
    V, n = d["verts"], len(d["verts"])
    m = (L["valid"] == 1) & (L["v"] != G.NONE)
    u, v = L["u"][m].astype(np.int64), L["v"][m].astype(np.int64)
    W = G.min_weight_csr(np.concatenate([u, v]), np.concatenate([v, u]),
                         np.concatenate([G.motion_cost(V[u], V[v], 0), G.motion_cost(V[v], V[u], 0)]), n)
    ref = dijkstra(W, directed=True, indices=0)
    assert np.all(np.isfinite(ref))
    assert np.all(np.abs(d["cost"] - ref) <= 1e-12 * np.maximum(ref, 1.0))
    par = d["parent"][1:].astype(np.int64)
    assert np.array_equal(d["cost"][par] + d["edge_cost"][1:], d["cost"][1:])
