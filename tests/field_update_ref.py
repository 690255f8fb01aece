"""Reference for the in-place update of a cost-to-go field: the four steps of artp_field_update
restated in numpy on lattice_ref.Lattice, one vector operation over all edges per sweep.  Shares nothing with the
library; tests/test_field_update_ref.py checks it against lattice_ref's Dijkstra on the new mask.

A field is (dist, hops), both (nrows, ncols, n_yaw): dist as Lattice.dijkstra gives it, hops = the fewest tight edges
(dist[u] + w == dist[v] bit for bit) from a source, -1 where there is none -- the device's definition, which Dijkstra's
own hop count (the hops of the path that happened to win) need not meet."""
import numpy as np

NONE = -1
BIG = np.iinfo(np.int64).max


def pull_edges(lat, reverse):
    """(pred, node, w) of every edge the search pulls along: forward a -> b gives pred a, node b; reverse the other way."""
    pred, node, wt = [], [], []
    for m in range(10):
        w = lat.w[m].reshape(-1)
        a = np.flatnonzero(np.isfinite(w))
        b = lat.neighbour_index(m).reshape(-1)[a]
        pred.append(b if reverse else a)
        node.append(a if reverse else b)
        wt.append(w[a])
    return np.concatenate(pred), np.concatenate(node), np.concatenate(wt)


def relax_dist(edges, dist):
    """In place to the fixed point of dist[v] = min(dist[v], dist[u] + w); the sweeps it took."""
    pred, node, w = edges
    sweeps = 0
    while True:
        before = dist.copy()
        with np.errstate(invalid="ignore"):
            np.minimum.at(dist, node, before[pred] + w)
        sweeps += 1
        if np.array_equal(before, dist):
            return sweeps


def relax_hops(edges, dist, hops):
    """In place to the fixed point of hops[v] = min(hops[v], hops[u] + 1) over the tight edges with hops[u] known."""
    pred, node, w = edges
    h = np.where(hops == NONE, BIG, hops)
    tight = (dist[pred] + w == dist[node]) & np.isfinite(dist[node])
    p, n = pred[tight], node[tight]
    while True:
        before = h.copy()
        ok = before[p] != BIG
        np.minimum.at(h, n[ok], before[p[ok]] + 1)
        if np.array_equal(before, h):
            break
    hops[:] = np.where(h == BIG, NONE, h)


def unsupport(edges, exists, dist, hops, phase, hop_rule=True):
    """Until nobody dies: a live node that is no source (hops 0) and has no live neighbour u with dist[u] + w == dist[v]
    and hops[u] + 1 == hops[v] dies: dist = +inf (phase 0 only) and hops = NONE.  Returns (deaths, rounds).
    hop_rule=False drops the second condition: the variant that keeps a cut-off island alive."""
    pred, node, w = edges
    deaths = rounds = 0
    while True:
        rounds += 1
        live = exists & np.isfinite(dist)
        if phase == 1:
            live &= hops != NONE
        ok = live[pred] & (dist[pred] + w == dist[node])
        if hop_rule:
            ok &= (hops[pred] != NONE) & (hops[pred] + 1 == hops[node])
        supported = np.zeros(len(dist), bool)
        supported[node[ok]] = True
        die = live & ~supported & (hops != 0)
        if not die.any():
            return deaths, rounds
        deaths += int(die.sum())
        if phase == 0:
            dist[die] = np.inf
        hops[die] = NONE


def compute(lat, sources, reverse=False):
    """(dist, hops) of a new field: Dijkstra's distances and the fewest-tight-edges hop counts."""
    dist, _ = lat.dijkstra(sources, reverse)
    hops = np.full(lat.shape, NONE, np.int64)
    for s in sources:
        hops[tuple(s)] = 0
    relax_hops(pull_edges(lat, reverse), dist.reshape(-1), hops.reshape(-1))
    return dist, hops


def update(lat_new, old_bits, dist, hops, reverse=False, hop_rule=True):
    """Steps 1-4 on copies of (dist, hops), a field of the old mask (old_bits = Lattice.bits of it) with the sources at
    hops 0; lat_new carries the new mask and the new weights.  Returns (dist, hops, stats)."""
    shape = lat_new.shape
    dist, hops = dist.reshape(-1).copy(), hops.reshape(-1).copy()
    old, new = old_bits.reshape(-1), lat_new.bits.reshape(-1)
    assert new[hops == 0].all(), "a source is no longer a node"
    edges = pull_edges(lat_new, reverse)
    # 1. the diff
    gone, added = old & ~new, new & ~old
    dist[gone] = np.inf
    hops[gone] = NONE
    snapshot = dist.copy()
    # 2. unsupport on distances, 3. relax them again
    dead, rounds = unsupport(edges, new, dist, hops, 0, hop_rule)
    relax_dist(edges, dist)
    # 4. hop counts: gone where the distance changed, unsupported at the settled distances, relaxed again
    hops[(dist.view(np.uint64) != snapshot.view(np.uint64)) | added] = NONE
    hop_dead, hop_rounds = unsupport(edges, new, dist, hops, 1, hop_rule)
    relax_hops(edges, dist, hops)
    stats = dict(removed_nodes=int(gone.sum()), added_nodes=int(added.sum()), dead_nodes=dead, hop_dead_nodes=hop_dead,
                 unsupport_rounds=rounds + hop_rounds, reached_nodes=int(np.isfinite(dist).sum()))
    return dist.reshape(shape), hops.reshape(shape), stats
