"""Float64 numpy restatements of the planners' graph operations, the reference of tests/test_graph_sweep.py and
tests/test_tree.py: OMPL's SE3 distance, PathLengthObjective::motionCost, the k rules of the roadmap and the tree
planners, a (distance, index) brute-force k-NN computed in row chunks, the checks of a device k-NN list against it,
and the tree-shape / cost-fold check.  Nothing here runs on the GPU; the self-tests are tests/test_graph_ref.py."""
import math

import numpy as np

NONE = 0xFFFFFFFF
# so3_arc_length: dq > 1 - 1e-9 counts as the same rotation (arc 0); pairs this close to the cut-off may take either
# branch on the device (the quaternion dot product may be contracted into FMAs there)
ARC_CUT = 1.0 - 1e-9
ARC_AMBIGUOUS = 1e-15
E = 2.718281828459045


def _dq(a, b):
    return np.abs((a[:, None, 3:] * b[None, :, 3:]).sum(-1))


def se3_distance(a, b):
    """OMPL SE3StateSpace::distance: R^3 L2 + SO3 arc length, rows of a x rows of b."""
    dp = np.sqrt(((a[:, None, :3] - b[None, :, :3]) ** 2).sum(-1))
    dq = _dq(a, b)
    arc = np.where(dq > ARC_CUT, 0.0, np.arccos(np.minimum(dq, 1.0)))
    return dp + arc


def _se3_distance_both(a, b):
    """(distance, the other branch's distance where dq is within ARC_AMBIGUOUS of the cut-off, else nan)"""
    dp = np.sqrt(((a[:, None, :3] - b[None, :, :3]) ** 2).sum(-1))
    dq = _dq(a, b)
    acos = np.arccos(np.minimum(dq, 1.0))
    d = dp + np.where(dq > ARC_CUT, 0.0, acos)
    amb = np.abs(dq - ARC_CUT) <= ARC_AMBIGUOUS
    alt = np.where(amb, dp + np.where(dq > ARC_CUT, acos, 0.0), np.nan)
    return d, alt


def yaw(q):
    """getYawFromSO3: the double atan2 rounded to float."""
    return np.arctan2(2.0 * (q[:, 3] * q[:, 2] + q[:, 0] * q[:, 1]),
                      1.0 - 2.0 * (q[:, 1] ** 2 + q[:, 2] ** 2)).astype(np.float32).astype(np.float64)


def motion_cost(a, b, objective, lon=0.5, lat=0.1, ang=0.5):
    """PathLengthObjective::motionCost (path_length_objective.cpp:26-70), rows a -> b."""
    a, b = np.atleast_2d(a), np.atleast_2d(b)
    d = b[:, :3] - a[:, :3]
    if objective == 0:
        return np.sqrt((d ** 2).sum(-1)) / lon
    y1, y2 = yaw(a[:, 3:]), yaw(b[:, 3:])
    dy = np.abs(y1 - y2)
    dy = np.where(dy > np.pi, 2 * np.pi - dy, dy)
    lon_d = np.cos(y1) * d[:, 0] + np.sin(y1) * d[:, 1]
    lat_d = -np.sin(y1) * d[:, 0] + np.cos(y1) * d[:, 1]
    return np.maximum(np.maximum(np.abs(lon_d) / lon, np.abs(lat_d) / lat), dy / ang)


def tree_k(rewire_factor, n):
    """RRTstar's k_rrt_: ceil(rewire_factor (e + e / 6) ln (n + 1)), the same double operations as the library."""
    return int(math.ceil(rewire_factor * (E + E / 6.0) * math.log(float(n) + 1.0)))


def k_tree_default(n):
    """tree_k at the default rewire factor 1.1"""
    return int(np.ceil(1.1 * (np.e + np.e / 6.0) * np.log(n + 1)))


def roadmap_kstar(n):
    """KStarStrategy for SE3: ceil(e (1 + 1/6) ln n)."""
    return int(math.ceil(E * (1.0 + 1.0 / 6.0) * math.log(float(n))))


def roadmap_k(k_neighbors, nv):
    """The k of a roadmap of nv vertices (roadmap_connect): k*(nv) unless given, at most nv - 1, at least 1, at most 128."""
    k = int(k_neighbors) if k_neighbors > 0 else roadmap_kstar(nv)
    k = min(k, nv - 1)
    k = max(k, 1)
    return min(k, 128)


def construction2_k_of(k_neighbors, nv):
    """k_i of construction 2: k*(i + 1) (or k_neighbors), at most i, at most the roadmap's k."""
    k = roadmap_k(k_neighbors, nv)
    out = np.empty(nv, np.int64)
    for i in range(nv):
        ki = int(k_neighbors) if k_neighbors else roadmap_kstar(i + 1)
        out[i] = min(ki, i, k)
    return out


def knn_grid_dims(len_x, len_y, nv):
    """(gx, gy) of the roadmap's k-NN grid (roadmap_connect: about three vertices per cell)."""
    h = math.sqrt(len_x * len_y * 3.0 / float(nv))
    h = max(h, max(len_x, len_y) / 2048.0)
    inv_h = 1.0 / h
    return max(1, int(math.ceil(len_x * inv_h))), max(1, int(math.ceil(len_y * inv_h)))


def knn_bruteforce(V, rows, k_of, pred_only=False, exclude=None, chunk=64):
    """The k nearest of every query row among the vertices V (not itself; with pred_only the smaller indices only; never
    an `exclude`d vertex), ascending by (distance, index) -- np.lexsort over the full candidate row, in chunks of rows.
    k_of: one k per row.  Returns (idx [n, kmax] with NONE, dist [n, kmax] with +inf)."""
    rows = np.asarray(rows, np.int64)
    k_of = np.broadcast_to(np.asarray(k_of, np.int64), rows.shape)
    kmax = int(k_of.max(initial=0))
    nv = len(V)
    idx = np.full((len(rows), max(kmax, 1)), NONE, np.uint32)[:, :kmax]
    dist = np.full((len(rows), max(kmax, 1)), np.inf)[:, :kmax]
    ids = np.arange(nv)
    for c0 in range(0, len(rows), chunk):
        r = rows[c0:c0 + chunk]
        D = se3_distance(V[r], V)
        D[np.arange(len(r)), r] = np.inf
        if pred_only:
            D[ids[None, :] >= r[:, None]] = np.inf
        if exclude is not None:
            D[:, exclude] = np.inf
        for t in range(len(r)):
            order = np.lexsort((ids, D[t]))
            kk = int(k_of[c0 + t])
            order = order[:kk]
            order = order[np.isfinite(D[t, order])]
            idx[c0 + t, :len(order)] = order
            dist[c0 + t, :len(order)] = D[t, order]
    return idx, dist


def check_knn_rows(V, rows, got_idx, got_dist, k_of, pred_only=False, exclude=None, tol=1e-11, chunk=64):
    """Device k-NN lists (rows of got_idx / got_dist, row length k_row >= k_of) against the brute force:
      * the distances match the brute force slot by slot within tol (1e-11: the same double formula; the quaternion dot
        product may be contracted into FMAs and acos magnifies one ulp of dq near 1 to ~1e-12);
      * every reported distance is the distance of the reported vertex (either branch where dq sits at the cut-off);
      * every row ascends by (distance, index), has no repeats, no self and only allowed candidates;
      * a neighbour differs from the brute force's only at a distance tie within tol;
      * unused slots are NONE / +inf, exactly when fewer than k candidates exist.
    Returns the number of slots whose neighbour differs from the brute force's (ties)."""
    rows = np.asarray(rows, np.int64)
    k_of = np.broadcast_to(np.asarray(k_of, np.int64), rows.shape)
    k_row = got_idx.shape[1]
    assert got_dist.shape == got_idx.shape and np.all(k_of <= k_row)
    nv = len(V)
    ids = np.arange(nv)
    n_tie = 0
    for c0 in range(0, len(rows), chunk):
        r = rows[c0:c0 + chunk]
        D, alt = _se3_distance_both(V[r], V)
        allowed = np.ones(D.shape, bool)
        allowed[np.arange(len(r)), r] = False
        if pred_only:
            allowed &= ids[None, :] < r[:, None]
        if exclude is not None:
            allowed[:, exclude] = False
        for t in range(len(r)):
            i, kk = int(r[t]), int(k_of[c0 + t])
            gi, gd = got_idx[c0 + t], got_dist[c0 + t]
            n_cand = int(allowed[t].sum())
            n_use = min(kk, n_cand)
            assert np.all(gi[n_use:] == NONE) and np.all(np.isinf(gd[n_use:])), (i, "unused slots", gi, gd)
            gi, gd = gi[:n_use].astype(np.int64), gd[:n_use]
            assert np.all(gi < nv), (i, "missing neighbour", gi)
            assert np.all(allowed[t, gi]), (i, "not a candidate", gi[~allowed[t, gi]])
            assert len(np.unique(gi)) == n_use, (i, "repeated neighbour")
            # ascending by (distance, index)
            asc = (gd[1:] > gd[:-1]) | ((gd[1:] == gd[:-1]) & (gi[1:] > gi[:-1]))
            assert asc.all(), (i, "not ascending", gi, gd)
            # the reported distance is the reported vertex's
            true = D[t, gi]
            ok = np.abs(gd - true) <= tol
            a_ = alt[t, gi]
            ok |= np.isfinite(a_) & (np.abs(gd - a_) <= tol)
            assert ok.all(), (i, "distance", gi[~ok], gd[~ok], true[~ok])
            # the brute force's list
            Dm = np.where(allowed[t], D[t], np.inf)
            if 0 < n_use < nv:  # the lexsort of the whole row, restricted to the entries up to the n_use-th distance
                cand = np.flatnonzero(Dm <= np.partition(Dm, n_use - 1)[n_use - 1])
                order = cand[np.lexsort((cand, Dm[cand]))][:n_use]
            else:
                order = np.lexsort((ids, Dm))[:n_use]
            ref_d = Dm[order]
            if np.isfinite(alt[t, order]).any() or (np.isfinite(alt[t]) & allowed[t] &
                                                     (Dm <= (ref_d[-1] if n_use else -1.0) + 1e-4)).any():
                continue  # a pair at the arc cut-off inside the list: either branch is right, the order may differ
            assert np.all(np.abs(gd - ref_d) <= tol), (i, "slot distances", np.abs(gd - ref_d).max())
            diff = gi != order
            assert np.all(np.abs(true[diff] - ref_d[diff]) <= tol), (i, "neighbour differs without a tie")
            n_tie += int(diff.sum())
    return n_tie


def symmetrised_edges(knn):
    """Sorted unique (min, max) pairs of every (row, listed neighbour)."""
    nv, k = knn.shape
    i = np.repeat(np.arange(nv, dtype=np.uint64), k)
    j = knn.reshape(-1).astype(np.uint64)
    m = j != NONE
    i, j = i[m], j[m]
    keys = np.unique((np.minimum(i, j) << np.uint64(32)) | np.maximum(i, j))
    return np.stack([(keys >> np.uint64(32)).astype(np.uint32), (keys & np.uint64(NONE)).astype(np.uint32)], 1)


def left_fold(ws):
    """((0 + w1) + w2) + ... in double, in order."""
    acc = 0.0
    for w in ws:
        acc = float(np.float64(acc) + np.float64(w))
    return acc


def min_weight_csr(u, v, w, n):
    """csr (n x n) of the edges u -> v with weight w; repeated pairs keep their smallest weight (csr_matrix would sum)."""
    from scipy.sparse import csr_matrix
    u, v, w = np.asarray(u, np.int64), np.asarray(v, np.int64), np.asarray(w, np.float64)
    order = np.lexsort((w, v, u))
    u, v, w = u[order], v[order], w[order]
    first = np.ones(len(u), bool)
    first[1:] = (u[1:] != u[:-1]) | (v[1:] != v[:-1])
    return csr_matrix((w[first], (u[first], v[first])), shape=(n, n))


def check_tree_shape_and_fold(d):
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


def tree_range(ctx, gm):
    """OMPL's default range of the tree planners: 0.2 x the space's maximum extent."""
    elev = gm["elevation"]
    fin = elev[np.isfinite(elev)]
    ez = float(fin.max()) - float(fin.min()) + ctx.params.reach_z
    return 0.2 * (np.sqrt((2 * gm.len_x) ** 2 + (2 * gm.len_y) ** 2 + ez ** 2) + 0.5 * np.pi)


def grow_per_batch(tree, n):
    """Exports (tree, checked motions, best cost) before the first batch and after each of n batches."""
    out = [(tree.export(), tree.export_checked(), tree.solve()[1])]
    for _ in range(n):
        tree.grow(1)
        out.append((tree.export(), tree.export_checked(), tree.solve()[1]))
    return out


def check_tree_batches(ctx, gm, hist, B, seed, first, objective, goal, variant=0, rewire_factor=1.1,
                       max_vertices=100000, batch0=0, n_sub=None, sub_seed=0, allow_empty=False):
    """Every stage of every batch of an rrt_star / inf_rrt_star history (grow_per_batch; hist[0] after batch0 batches)
    against its restatement: the sampler, nearest unpruned vertex (brute force) and steering, informed rejection, new
    vertices in slot order, near sets (the exact k nearest unpruned pre-batch vertices), parent choice, rewiring, edge
    costs and the cost fold.  n_sub: the per-vertex checks (near set, parent) on a seeded subset of that many new
    vertices per batch; allow_empty: a batch may add no vertex.  Returns the logged motions with a vertex (u, v, valid) and the final vertices."""
    import oracle_py as O
    rob = O.robot("yaml")
    smp = O.OracleSampler(gm)
    rng_ = tree_range(ctx, gm)
    kmax = max(1, tree_k(rewire_factor, max_vertices))
    pick = np.random.default_rng(sub_seed)
    verdict_u, verdict_v, verdict_ok, verdict_V = [], [], [], None
    for b in range(1, len(hist)):
        batch = batch0 + b - 1
        P, _, c_prev = hist[b - 1]
        C_, L, _ = hist[b]
        n_pre, n_now = len(P["verts"]), len(C_["verts"])
        assert n_now > n_pre or (allow_empty and n_now == n_pre)
        V = C_["verts"]
        assert np.array_equal(V[:n_pre], P["verts"]) and np.all(C_["born"][n_pre:] == batch)
        # 1. the samples: the CPU sampler's states of this batch (slot 0 = the goal while it is not a vertex; with one
        # sample per batch only every 20th batch)
        samp, _ = smp.sample(rob, seed, first + batch * B, B)
        dev = ctx.sample_states(seed, first + batch * B, B)
        assert np.abs(samp - dev).max() < 1e-12
        goal_in = c_prev < np.inf
        if not goal_in and (B > 1 or batch % 20 == 0):
            samp[0] = goal
        # 2. nearest unpruned pre-batch vertex (brute force) and steering
        pruned = P["pruned"] != 0
        D = se3_distance(samp, P["verts"])
        D[:, pruned] = np.inf
        nn = np.argmin(D, axis=1)
        dn = D[np.arange(B), nn]
        alive = dn > 0.0
        xnew = np.array([O.interpolate(P["verts"][nn[s]], samp[s], rng_ / dn[s]) if dn[s] > rng_ else samp[s]
                         for s in range(B)])
        # 3. informed rejection (inf_rrt_star with a solution): h(s, x) + h(x, g) < c_best survives
        if variant == 1 and goal_in:
            hs = np.sqrt(((xnew[:, :3] - V[0, :3]) ** 2).sum(-1)) / 0.5
            hg = np.sqrt(((goal[:3] - xnew[:, :3]) ** 2).sum(-1)) / 0.5
            alive &= hs + hg < c_prev
        # motions of this batch: the first motions of the survivors in slot order, then the near motions
        sel = L["batch"] == batch
        lu, lv, lok = L["u"][sel].astype(np.int64), L["v"][sel].astype(np.int64), L["valid"][sel]
        slots = np.flatnonzero(alive)
        m1 = len(slots)
        assert len(lu) >= m1, "fewer first motions logged than samples survived"
        fu, fv, fok = lu[:m1], lv[:m1], lok[:m1]
        tie = np.abs(D[slots, np.minimum(fu, n_pre - 1)] - dn[slots]) < 1e-12
        assert np.all((fu == nn[slots]) | (tie & (fu < n_pre))), "first motion not from the nearest vertex"
        # the new vertices are the steered survivors whose first motion is valid, in slot order
        kept = fv != NONE
        assert np.array_equal(fv[kept], np.arange(n_pre, n_now)), "new vertices out of slot order"
        assert np.all(fok[kept] == 1)
        ok_first = fok == 1
        assert np.array_equal(kept, ok_first & (np.cumsum(ok_first) <= n_now - n_pre))
        assert np.abs(V[n_pre:] - xnew[slots[kept]]).max(initial=0.0) <= 1e-12
        k = max(1, min(tree_k(rewire_factor, n_pre), kmax))
        js = np.arange(n_now - n_pre)
        if n_sub is not None and len(js) > n_sub:
            js = np.sort(pick.choice(len(js), n_sub, replace=False))
        near_lu, near_lv = lu[m1:], lv[m1:]
        for j in js:
            v = n_pre + int(j)
            mine = np.flatnonzero(near_lv == v)
            us = np.concatenate([[fu[kept][j]], near_lu[mine]])
            uok = np.concatenate([[1], lok[m1:][mine]])
            # near set: the exact k nearest unpruned pre-batch vertices of x_new (plus the nearest)
            Dx = se3_distance(V[v:v + 1], P["verts"])[0]
            Dx[pruned] = np.inf
            order = np.lexsort((np.arange(n_pre), Dx))[:k]
            order = order[np.isfinite(Dx[order])]
            want = set(order.tolist()) | {int(us[0])}
            got = set(us.tolist())
            assert not (got & set(np.flatnonzero(pruned).tolist())), (batch, v, "pruned vertex as a candidate")
            if got != want:  # only near-ties may differ
                kth = Dx[order[-1]]
                assert all(abs(Dx[u] - kth) < 1e-12 for u in got ^ want), (batch, v)
            assert len(us) == len(got)
            # parent choice: argmin over the valid candidates of cost(u) + c(u, x_new) with pre-batch costs
            ok_u = us[uok == 1]
            vals = P["cost"][ok_u] + motion_cost(P["verts"][ok_u], np.repeat(V[v:v + 1], len(ok_u), 0), objective)
            par = int(C_["parent"][v])
            assert par in ok_u.tolist()
            assert P["cost"][par] + motion_cost(P["verts"][par], V[v], objective)[0] <= vals.min() * (1 + 1e-12) + 1e-15
        # rewiring: with the costs parent choice gave the new vertices, no valid motion (u pre-batch, v new) is left
        # that would have lowered cost(u) below what u got
        cv0 = np.full(n_now, np.nan)
        cv0[n_pre:] = P["cost"][C_["parent"][n_pre:]] + C_["edge_cost"][n_pre:]
        got_u = P["cost"].copy()
        rew = np.flatnonzero(C_["parent"][1:n_pre] != P["parent"][1:n_pre]) + 1
        assert np.all(C_["parent"][rew] >= n_pre)
        got_u[rew] = cv0[C_["parent"][rew]] + C_["edge_cost"][rew]
        m = (lok == 1) & (lv != NONE) & (lv >= n_pre)
        cand = cv0[lv[m]] + motion_cost(V[lv[m]], P["verts"][lu[m]], objective)
        assert np.all(got_u[lu[m]] <= cand * (1 + 1e-12) + 1e-15)
        assert np.all(got_u[rew] < P["cost"][rew])
        # edge costs: the numpy PathLengthObjective
        ref = motion_cost(V[C_["parent"][1:]], V[1:], objective)
        assert np.all(np.abs(C_["edge_cost"][1:] - ref) <= 1e-12 * np.maximum(ref, 1e-300))
        check_tree_shape_and_fold(C_)
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
    return np.concatenate(verdict_u), np.concatenate(verdict_v), np.concatenate(verdict_ok), verdict_V
