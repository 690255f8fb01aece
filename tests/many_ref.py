"""Restatement of artp_roadmap_solve_many (csrc/roadmap_many.h) in numpy + heapq, the reference of
tests/test_roadmap_many_sweep.py.  Nothing here runs on the GPU or calls the library; the self-tests are
tests/test_many_ref.py.

  classify  which goals are "near" (answered by set_query + solve) and every attachment list;
  shortlist the rule that accepts a goal's device shortlist or sends the goal to the host brute force;
  eager     the order-free answer: shortest left-fold costs over the graph with every invalid edge deleted up front;
  rounds    the lazy rounds of many_device_solve, step for step: dist (the minimum over paths of the left-folded float64
            sum: with weights >= 0 float addition is monotone, so Dijkstra gives the same bits as the label-correcting
            sweeps), hops (BFS over tight edges), the smallest predecessor one hop closer, the attachment argmin in slot
            order with ties to the smaller vertex, every pending path, one verdict per (edge, direction of travel), every
            invalid item removed at once, removals summed per goal against max_replans.

Vertex ids: 0 = the start, 1 = unused (the roadmap's own goal), 2 .. nv - 1 = roadmap vertices, nv + g = goal g."""
import heapq

import numpy as np

import graph_ref as G

NONE = G.NONE
SOLVED, INVALID, UNREACHABLE, TOO_MANY_REMOVALS = 0, 1, 2, 3
LARGE = 5000  # vertices from which dijkstra() uses scipy


def _knn(V, allowed, q, k):
    d = G.se3_distance(np.asarray(q, np.float64)[None], V)[0]
    ids = np.flatnonzero(allowed)
    order = ids[np.lexsort((ids, d[ids]))][:k]
    return order.astype(np.int64), d[order]


def classify(V, vinvalid, start, goals, k):
    """The start's list and every goal's list -- the k nearest of the vertices >= 2 not in vinvalid, ascending
    (distance, id) -- and which goals are near: a list shorter than k, or d(start, goal) <= the k-th distance of either
    list.  margin[g] = min over the two lists of |d(start, goal) - kth| / kth (+inf where a list is short)."""
    V = np.asarray(V, np.float64)
    goals = np.asarray(goals, np.float64).reshape(-1, 7)
    allowed = np.ones(len(V), bool)
    allowed[:2] = False
    if vinvalid is not None and len(vinvalid):
        allowed &= ~np.asarray(vinvalid, bool)
    s_ids, s_d = _knn(V, allowed, start, k)
    g_ids, g_d, near, margin = [], [], np.zeros(len(goals), bool), np.full(len(goals), np.inf)
    dsg = G.se3_distance(np.asarray(start, np.float64)[None], goals)[0] if len(goals) else np.zeros(0)
    for g in range(len(goals)):
        ids, d = _knn(V, allowed, goals[g], k)
        g_ids.append(ids)
        g_d.append(d)
        if len(s_ids) < k or len(ids) < k:
            near[g] = True
            continue
        near[g] = dsg[g] <= s_d[-1] or dsg[g] <= d[-1]
        margin[g] = min(abs(dsg[g] - s_d[-1]) / s_d[-1], abs(dsg[g] - d[-1]) / d[-1])
    return {"start_ids": s_ids, "start_dist": s_d, "goal_ids": g_ids, "goal_dist": g_d, "near": near, "margin": margin,
            "d_start_goal": dsg}


TREE_KMAX = 64  # tree.h: the longest list tree_knn_kernel returns


def shortlist_k(k, mutate=False):
    """kk of artp_roadmap_solve_many: k + 8 candidates, at most TREE_KMAX; no shortlist (host brute force) unless kk > k.
    mutate: the wrong rule "kk = k, shortlist always" of the mutation runs."""
    return min(k, TREE_KMAX) if mutate else min(k + 8, TREE_KMAX)


def shortlist(V, vinvalid, q, k, kk, force=False):
    """A goal's list as step 3 of artp_roadmap_solve_many makes it: the kk nearest allowed vertices (the device's
    shortlist), re-ranked, cut to k, and accepted ("exact") when the shortlist holds every candidate or its last distance
    exceeds the k-th by more than 1e-9; otherwise the brute force over all vertices.  Here both sides use one distance
    formula, so the list is the brute force's either way: what the rule decides is which path made it.
    Returns (ids, dist, exact); exact is None where no shortlist is made (kk <= k and not force)."""
    V = np.asarray(V, np.float64)
    allowed = np.ones(len(V), bool)
    allowed[:2] = False
    if vinvalid is not None and len(vinvalid):
        allowed &= ~np.asarray(vinvalid, bool)
    ids, d = _knn(V, allowed, q, len(V))
    if not (kk > k or force):
        return ids[:k], d[:k], None
    have = min(kk, len(ids))
    cand_d = d[:have][:k]
    exact = have < kk or (len(cand_d) > 0 and d[have - 1] - 1e-9 > cand_d[-1])
    return ids[:k], d[:k], bool(exact)


def _csr(nv, eu, ev, w):
    """directed adjacency (both directions of every finite edge) as python lists: ptr, dst, weight"""
    m = np.isfinite(w)
    src = np.concatenate([eu[m], ev[m]]).astype(np.int64)
    dst = np.concatenate([ev[m], eu[m]]).astype(np.int64)
    ww = np.concatenate([w[m], w[m]])
    order = np.argsort(src, kind="stable")
    ptr = np.zeros(nv + 1, np.int64)
    np.add.at(ptr, src + 1, 1)
    return np.cumsum(ptr).tolist(), dst[order].tolist(), ww[order].tolist()


def dijkstra(nv, eu, ev, w, source=0):
    """dist[v] = the smallest left-folded float64 sum over the paths source -> v (edges with w = +inf do not exist).
    Large graphs without zero weights go through scipy's Dijkstra (the same dist[u] + w in double, so the same bits: the
    self-tests compare the two); graphs with zero weights, where sparse formats make an edge of weight 0 easy to lose,
    stay with heapq."""
    m = np.isfinite(w)
    if nv >= LARGE and m.any() and (np.asarray(w)[m] > 0.0).all():
        from scipy.sparse import csr_matrix
        from scipy.sparse.csgraph import dijkstra as sp_dijkstra
        src = np.concatenate([eu[m], ev[m]])
        dst = np.concatenate([ev[m], eu[m]])
        W = csr_matrix((np.concatenate([w[m], w[m]]), (src, dst)), shape=(nv, nv))
        return sp_dijkstra(W, directed=True, indices=source)
    ptr, dst, ww = _csr(nv, eu, ev, w)
    dist = [np.inf] * nv
    dist[source] = 0.0
    heap = [(0.0, source)]
    while heap:
        d, u = heapq.heappop(heap)
        if d > dist[u]:
            continue
        for i in range(ptr[u], ptr[u + 1]):
            nd = d + ww[i]
            v = dst[i]
            if nd < dist[v]:
                dist[v] = nd
                heapq.heappush(heap, (nd, v))
    return np.array(dist, np.float64)


def _graph(nv, eu, ev, w, start_att):
    """roadmap edges, then the start's edges (0, n): the edge list of many_device_solve"""
    sn, sw = np.asarray(start_att[0], np.int64), np.asarray(start_att[1], np.float64)
    eu = np.concatenate([np.asarray(eu, np.int64), np.zeros(len(sn), np.int64)])
    ev = np.concatenate([np.asarray(ev, np.int64), sn])
    w = np.concatenate([np.asarray(w, np.float64), sw]).copy()
    w[~((w >= 0.0) & np.isfinite(w))] = np.inf
    return eu, ev, w


def _attach(dist, an, aw, tie_smaller=True):
    """(slot, value) of the argmin over the slots of dist[n] + w, ties to the smaller n; (None, inf) without one"""
    best, ba, bn = np.inf, None, None
    for a in range(len(an)):
        n, wa = int(an[a]), float(aw[a])
        if n == NONE or not wa < np.inf or not dist[n] < np.inf:
            continue
        val = float(np.float64(dist[n]) + np.float64(wa))
        if val < best or (val == best and ((n < bn) if tie_smaller else (n > bn))):
            best, ba, bn = val, a, n
    return ba, best


def eager(nv, eu, ev, w, start_att, goal_atts, edge_ok, start_ok, goal_ok):
    """Every invalid edge deleted first.  eu, ev, w: roadmap edges (w = +inf where not usable); start_att = (n, w);
    goal_atts = [(n, w)] per goal; edge_ok / start_ok / goal_ok[g]: one verdict per edge / attachment.
    Returns (status 0 / 2 per goal, cost = min over the valid attachments of dist[n] + w)."""
    sw = np.where(np.asarray(start_ok, bool), np.asarray(start_att[1], np.float64), np.inf)
    w = np.where(np.asarray(edge_ok, bool), np.asarray(w, np.float64), np.inf)
    geu, gev, gw = _graph(nv, eu, ev, w, (start_att[0], sw))
    dist = dijkstra(nv, geu, gev, gw)
    status, cost = np.full(len(goal_atts), UNREACHABLE, np.int32), np.full(len(goal_atts), np.inf)
    for g, (an, aw) in enumerate(goal_atts):
        aw = np.where(np.asarray(goal_ok[g], bool), np.asarray(aw, np.float64), np.inf)
        ba, val = _attach(dist, an, aw)
        if ba is not None:
            status[g], cost[g] = SOLVED, val
    return status, cost


def _hops_pred(nv, eu, ev, w, dist, hop_rule=True, smallest=True, stamp_or=False):
    """hops = the fewest tight edges from the start (tight: v != 0, dist[u] finite, dist[u] + w == dist[v] bit for bit);
    pred[v] = the smallest u with a tight edge u -> v and hops[u] + 1 == hops[v].  hop_rule=False / smallest=False are the
    wrong rules of the self-tests' mutation copies."""
    m = np.isfinite(w)
    src = np.concatenate([eu[m], ev[m]])
    dst = np.concatenate([ev[m], eu[m]])
    ww = np.concatenate([w[m], w[m]])
    with np.errstate(invalid="ignore"):
        tight = (dst != 0) & np.isfinite(dist[src]) & (dist[src] + ww == dist[dst])
    src, dst = src[tight], dst[tight]
    hops = np.full(nv, -1, np.int64)
    hops[0] = 0
    level = 0
    while True:
        front = (hops[src] == level) & (hops[dst] < 0)
        if not front.any():
            break
        hops[dst[front]] = level + 1
        level += 1
    pred = np.full(nv, -1, np.int64)
    ok = hops[src] >= 0
    if hop_rule:
        ok &= hops[src] + 1 == hops[dst]
    if smallest:
        big = np.full(nv, nv, np.int64)
        np.minimum.at(big, dst[ok], src[ok])
        pred = np.where(big < nv, big, -1)
    else:
        np.maximum.at(pred, dst[ok], src[ok])
    pred[0] = -1
    return hops, pred


def rounds(nv, eu, ev, w, start_att, goal_atts, verdict, max_replans, initial=None, mutate=()):
    """The lazy rounds of many_device_solve.

    eu, ev, w     roadmap edges with both ends >= 2, each (u, v) once; w = +inf where the edge is not usable
    start_att     (n, w): the start's attachment list and weights (+inf: not usable)
    goal_atts     [(n, w)] per goal, in slot order
    verdict       callable(src_ids, dst_ids) -> bool[]: asked once per (edge, direction of travel) without a verdict,
                  goal g being vertex nv + g
    initial       {(roadmap edge index, direction): 1 valid | 2 invalid}: verdicts known before the call
    mutate        names of deliberately wrong rules (tests/test_many_ref.py): "attach_tie", "no_hop_rule", "pred_largest",
                  "replans_ge", "count_once"

    Returns status, cost, paths (id lists: 0, vertices, nv + g), froze (the round a goal froze in, -1), removed_edges
    (roadmap edge indices), removed_start (start slots), dropped (set of (goal, slot)), and rounds / removed / motions as
    stats[0..2] count them (start edges and attachments included in removed)."""
    nr = len(eu)
    geu, gev, gw = _graph(nv, eu, ev, w, start_att)
    ne = len(geu)
    edge_of = {(int(a), int(b)): e for e, (a, b) in enumerate(zip(geu, gev))}
    assert len(edge_of) == ne, "an edge is listed twice"
    ng = len(goal_atts)
    an = [np.asarray(a[0], np.int64) for a in goal_atts]
    aw = [np.asarray(a[1], np.float64).copy() for a in goal_atts]
    for a in aw:
        a[~((a >= 0.0) & np.isfinite(a))] = np.inf
    verd = dict(initial or {})          # (edge, direction) -> 1 | 2
    averd = {}                          # (goal, slot) -> 1 | 2
    status = np.full(ng, -1, np.int32)
    cost = np.full(ng, np.inf)
    paths = [None] * ng
    froze = np.full(ng, -1, np.int64)
    removals = np.zeros(ng, np.int64)
    n_rounds = motions = 0
    removed = set()
    while True:
        dist = dijkstra(nv, geu, gev, gw)
        hops, pred = _hops_pred(nv, geu, gev, gw, dist, hop_rule="no_hop_rule" not in mutate,
                                smallest="pred_largest" not in mutate)
        cur = {}
        for g in range(ng):
            if status[g] != -1:
                continue
            ba, val = _attach(dist, an[g], aw[g], tie_smaller="attach_tie" not in mutate)
            if ba is None:
                status[g] = UNREACHABLE
                continue
            chain = [int(an[g][ba])]
            while chain[-1] != 0:
                assert pred[chain[-1]] >= 0 and len(chain) <= nv, "broken predecessor chain"
                chain.append(int(pred[chain[-1]]))
            ids = chain[::-1] + [nv + g]
            items = []
            for a, b in zip(ids[:-2], ids[1:-1]):
                e = edge_of[(min(a, b), max(a, b))]
                items.append(("e", e, 0 if a == geu[e] else 1, a, b))
            items.append(("a", g, ba, ids[-2], ids[-1]))
            cost[g] = val
            cur[g] = (ids, items)
        if not cur:
            break
        n_rounds += 1
        # one claim per (edge, direction) however many paths share it
        ask, seen = [], set()
        for g, (ids, items) in cur.items():
            for it in items:
                key = it[:3]
                known = (verd.get(key[1:]) if it[0] == "e" else averd.get(key[1:])) is not None
                if not known and key not in seen:
                    seen.add(key)
                    ask.append(it)
        if ask:
            ok = np.asarray(verdict(np.array([it[3] for it in ask], np.int64), np.array([it[4] for it in ask], np.int64)))
            assert len(ok) == len(ask)
            for it, o in zip(ask, ok):
                (verd if it[0] == "e" else averd)[it[1:3]] = 1 if o else 2
            motions += len(ask)
        bad_goals = 0
        counted = set()
        for g, (ids, items) in cur.items():
            b = 0
            for it in items:
                if it[0] == "e":
                    if verd[it[1:3]] != 2:
                        continue
                    gw[it[1]] = np.inf
                    removed.add(it[1])
                    if "count_once" in mutate and it[1] in counted:
                        continue
                    counted.add(it[1])
                else:
                    if averd[it[1:3]] != 2:
                        continue
                    aw[g][it[2]] = np.inf
                b += 1
            if b == 0:
                status[g] = SOLVED
                froze[g] = n_rounds - 1
                paths[g] = ids
                continue
            removals[g] += b
            if (removals[g] >= max_replans) if "replans_ge" in mutate else (removals[g] > max_replans):
                status[g] = TOO_MANY_REMOVALS
                cost[g] = np.inf
                continue
            bad_goals += 1
        if bad_goals == 0:
            break
    status[status == -1] = UNREACHABLE
    cost[status != SOLVED] = np.inf
    dropped = {key for key, v in averd.items() if v == 2}
    return {"status": status, "cost": cost, "paths": paths, "froze": froze,
            "removed_edges": sorted(e for e in removed if e < nr),
            "removed_start": sorted(e - nr for e in removed if e >= nr), "dropped": dropped,
            "removals": removals, "rounds": n_rounds, "removed": len(removed) + len(dropped), "motions": motions}
