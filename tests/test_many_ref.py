"""Self-tests of tests/many_ref.py, the restatement of artp_roadmap_solve_many: graphs made by hand with the answers
worked out in the docstrings, `eager` against `rounds` on 200 seeded random graphs whose weights tie as a rule, and
Python copies of the kernel mutations the GPU sweep is run against.  Mutations 1 to 6 each change an answer here (two
further wrong rules, the larger predecessor and removals counted once per edge, are copied as well); mutation 7 changes
no answer, here or on the device, and the last test shows why.  No GPU.

Vertex ids: 0 = the start, 1 unused, 2 .. nv - 1 roadmap vertices, nv + g = goal g.  All weights are multiples of 0.5:
every sum is exact."""
import numpy as np
import pytest

import graph_ref as G
import many_ref as M


class Case:
    def __init__(self, nv, edges, start, goals, invalid=()):
        """edges [(u, v, w)], start [(n, w)], goals [[(n, w), ...]], invalid: unordered vertex pairs whose motion fails"""
        self.nv = nv
        self.eu = np.array([e[0] for e in edges], np.int64)
        self.ev = np.array([e[1] for e in edges], np.int64)
        self.w = np.array([e[2] for e in edges], np.float64)
        self.start = (np.array([a[0] for a in start], np.int64), np.array([a[1] for a in start], np.float64))
        self.goals = [(np.array([a[0] for a in g], np.int64), np.array([a[1] for a in g], np.float64)) for g in goals]
        self.invalid = {frozenset(p) for p in invalid}
        self.asked = []

    def verdict(self, src, dst):
        self.asked += list(zip(src.tolist(), dst.tolist()))
        return np.array([frozenset((a, b)) not in self.invalid for a, b in zip(src.tolist(), dst.tolist())], bool)

    def edge(self, u, v):
        return int(np.flatnonzero((self.eu == u) & (self.ev == v))[0])

    def run(self, max_replans=1000, w=None, **kw):
        self.asked = []
        return M.rounds(self.nv, self.eu, self.ev, self.w if w is None else w, self.start, self.goals, self.verdict,
                        max_replans, **kw)

    def eager(self):
        ok = np.array([frozenset((int(a), int(b))) not in self.invalid for a, b in zip(self.eu, self.ev)], bool)
        sok = np.array([frozenset((0, int(n))) not in self.invalid for n in self.start[0]], bool)
        gok = [np.array([frozenset((int(n), self.nv + g)) not in self.invalid for n in an], bool)
               for g, (an, _) in enumerate(self.goals)]
        return M.eager(self.nv, self.eu, self.ev, self.w, self.start, self.goals, ok, sok, gok)


def diamond():
    """0 -1- 2; 2 -1- 3 -1- 5 and 2 -1- 4 -1- 5; the goal hangs on 5 (1).  Two routes of cost 4: the predecessor of 5 is
    the smaller of 3 and 4, so the path is 0 2 3 5 g."""
    return Case(6, [(2, 3, 1.0), (2, 4, 1.0), (3, 5, 1.0), (4, 5, 1.0)], [(2, 1.0)], [[(5, 1.0)]])


def long_diamond():
    """0 -1- 2; short route 2 -2- 4 -1- 5 (3 hops from the start), long route 2 -1- 6 -1- 3 -1- 5 (4 hops), both cost 4
    at 5.  The smaller predecessor of 5 is 3, but 3 is not one hop closer: hops[5] = 3, hops[3] = 3, hops[4] = 2.  The
    path is 0 2 4 5 g, cost 5."""
    return Case(7, [(2, 4, 2.0), (4, 5, 1.0), (2, 6, 1.0), (3, 6, 1.0), (3, 5, 1.0)], [(2, 1.0)], [[(5, 1.0)]])


def zero_triangle():
    """Zero-weight triangle 0 - 2 - 3 - 0 (the start's edges to 2 and 3, and 2 - 3), goal 0 on 3 (0): every dist is 0 and
    2 <-> 3 is tight both ways; hops[2] = hops[3] = 1, so 3's predecessor is the start: path 0 3 g0, cost 0.
    A second zero triangle 4 - 5 - 6 hangs on the start by 0 -1- 6, goal 1 on 5: hops[6] = 1, hops[4] = hops[5] = 2, the
    predecessor of 5 is 6 (4 is smaller and tight, but not closer): path 0 6 5 g1, cost 1.  Without the hop rule
    pred[5] = 4 and pred[4] = 5: a cycle."""
    return Case(7, [(2, 3, 0.0), (4, 5, 0.0), (4, 6, 0.0), (5, 6, 0.0)], [(2, 0.0), (3, 0.0), (6, 1.0)],
                [[(3, 0.0)], [(5, 0.0)]])


def two_attachments():
    """Start on 2 (1) and 3 (1); the goal's slots are (3, 1) then (2, 1): both give 2, the smaller vertex wins although
    its slot comes second: path 0 2 g."""
    return Case(4, [], [(2, 1.0), (3, 1.0)], [[(3, 1.0), (2, 1.0)]])


def shared_invalid():
    """0 -1- 2 -1- 3 with 2 - 3 invalid, detour 2 -5- 4 -5- 3; goal 0 on 3 (1), goal 1 on 3 (2).
    Round 1: both paths are 0 2 3 g.  Asked: (0,2), (2,3), (3,g0), (3,g1) -- 4 motions, (2,3) once.  2 - 3 is removed
    once and counted for both goals.  Round 2: 0 2 4 3 g, asked (2,4), (4,3).  rounds 2, removed 1, motions 6, costs 12
    and 13."""
    return Case(5, [(2, 3, 1.0), (2, 4, 5.0), (3, 4, 5.0)], [(2, 1.0)], [[(3, 1.0)], [(3, 2.0)]], invalid=[(2, 3)])


def cut_off():
    """0 -1- 2 -1- 3, 2 - 3 invalid, the goal on 3: round 1 removes the only edge, the next search leaves 3 at +inf and
    the goal is unreachable; no path is left, so no second round is counted.  rounds 1, removed 1, motions 3."""
    return Case(4, [(2, 3, 1.0)], [(2, 1.0)], [[(3, 1.0)]], invalid=[(2, 3)])


def two_removals():
    """0 -1- 2; 2 -1- 3 invalid; 2 -2- 4 -2- 3 with 4 - 3 invalid; 2 -5- 5 -5- 3 valid; the goal on 3 (1).
    Round 1: 0 2 3 g loses 2 - 3 (1 removal); round 2: 0 2 4 3 g loses 4 - 3 (2 removals); round 3: 0 2 5 3 g, cost 12.
    b = 2: max_replans 1 gives status 3 after round 2, max_replans 2 and 3 solve it."""
    return Case(6, [(2, 3, 1.0), (2, 4, 2.0), (3, 4, 2.0), (2, 5, 5.0), (3, 5, 5.0)], [(2, 1.0)], [[(3, 1.0)]],
                invalid=[(2, 3), (3, 4)])


def test_smaller_predecessor():
    c = diamond()
    r = c.run()
    assert r["paths"] == [[0, 2, 3, 5, 6]] and r["cost"][0] == 4.0 and r["status"][0] == 0
    assert (r["rounds"], r["removed"], r["motions"]) == (1, 0, 4)


def test_hop_rule():
    c = long_diamond()
    r = c.run()
    assert r["paths"] == [[0, 2, 4, 5, 7]] and r["cost"][0] == 5.0


def test_zero_weight_triangle_has_no_cycle():
    c = zero_triangle()
    r = c.run()
    assert r["paths"] == [[0, 3, 7], [0, 6, 5, 8]]
    assert r["cost"].tolist() == [0.0, 1.0]
    for p in r["paths"]:
        assert len(set(p)) == len(p)


def test_equal_attachments_take_the_smaller_vertex():
    r = two_attachments().run()
    assert r["paths"] == [[0, 2, 4]] and r["cost"][0] == 2.0


def test_shared_invalid_edge_claimed_once_counted_twice_removed_once():
    c = shared_invalid()
    r = c.run()
    assert c.asked.count((2, 3)) == 1 and len(c.asked) == len(set(c.asked)) == 6
    assert r["removals"].tolist() == [1, 1]
    assert r["removed_edges"] == [c.edge(2, 3)] and r["removed"] == 1
    assert (r["rounds"], r["motions"]) == (2, 6)
    assert r["cost"].tolist() == [12.0, 13.0] and r["froze"].tolist() == [1, 1]
    assert r["paths"] == [[0, 2, 4, 3, 5], [0, 2, 4, 3, 6]]


def test_goal_cut_off_by_a_removal():
    r = cut_off().run()
    assert r["status"].tolist() == [2] and np.isinf(r["cost"][0]) and r["paths"] == [None]
    assert (r["rounds"], r["removed"], r["motions"]) == (1, 1, 3)


@pytest.mark.parametrize("max_replans,status", [(1, 3), (2, 0), (3, 0)])
def test_max_replans_around_the_removal_count(max_replans, status):
    c = two_removals()
    r = c.run(max_replans=max_replans)
    assert r["status"].tolist() == [status]
    if status == 0:
        assert r["cost"][0] == 12.0 and r["paths"] == [[0, 2, 5, 3, 6]] and r["rounds"] == 3 and r["removed"] == 2
    else:
        assert np.isinf(r["cost"][0]) and r["rounds"] == 2 and r["removals"][0] == 2


def test_no_goal_reachable_is_zero_rounds():
    """the start's only edge is unusable, one goal hangs on a vertex nothing leads to, one has no attachment at all"""
    c = Case(5, [(3, 4, 1.0)], [(2, np.inf)], [[(3, 1.0)], [(M.NONE, np.inf)]])
    r = c.run()
    assert r["status"].tolist() == [2, 2] and (r["rounds"], r["removed"], r["motions"]) == (0, 0, 0)


def test_dropped_attachment_and_start_edge():
    """Start on 2 (1, invalid) and 3 (2); the goal on 2 (1) and 3 (1, invalid), 2 -1- 3.
    Round 1: 0 2 g (cost 2): the start edge (0, 2) is invalid.  Round 2: 0 3 g (3): the attachment (3, g) is invalid.
    Round 3: 0 3 2 g (4), valid.  removed = 1 start edge + 1 attachment."""
    c = Case(4, [(2, 3, 1.0)], [(2, 1.0), (3, 2.0)], [[(2, 1.0), (3, 1.0)]], invalid=[(0, 2), (3, 4)])
    r = c.run()
    assert r["paths"] == [[0, 3, 2, 4]] and r["cost"][0] == 4.0
    assert r["removed_start"] == [0] and r["dropped"] == {(0, 1)} and r["removed_edges"] == []
    assert (r["rounds"], r["removed"]) == (3, 2)
    st, cost = c.eager()
    assert st.tolist() == [0] and cost[0] == 4.0


def test_known_verdicts_are_not_asked_again():
    c = two_removals()
    full = c.run()
    e = c.edge(2, 5)
    r = c.run(initial={(e, 0): 1})
    assert r["motions"] == full["motions"] - 1 and (2, 5) not in c.asked
    assert r["paths"] == full["paths"] and r["rounds"] == full["rounds"]
    # a cached rejection removes the edge without a motion check
    r = c.run(initial={(c.edge(2, 3), 0): 2})
    assert (2, 3) not in c.asked and r["removed_edges"] == full["removed_edges"] and r["rounds"] == full["rounds"]


def _random_case(seed):
    rng = np.random.default_rng(seed)
    nv = int(rng.integers(30, 201)) + 2
    k = int(rng.integers(2, 6))
    pairs = set()
    for v in range(2, nv):
        for u in rng.choice(np.arange(2, nv), k, replace=False):
            if u != v:
                pairs.add((min(int(u), v), max(int(u), v)))
    pairs = sorted(pairs)
    wts = rng.choice([0.0, 0.5, 1.0, 1.5], len(pairs))
    wts[rng.random(len(pairs)) < 0.05] = np.inf  # not usable
    edges = [(u, v, w) for (u, v), w in zip(pairs, wts)]
    att = lambda: [(int(n), float(rng.choice([0.0, 0.5, 1.0, 1.5]))) for n in rng.choice(np.arange(2, nv), k, replace=False)]
    ng = int(rng.integers(1, 12))
    goals = [att() for _ in range(ng)]
    start = att()
    p_bad = float(rng.choice([0.0, 0.1, 0.3, 0.6]))
    invalid = [p for p in pairs if rng.random() < p_bad]
    invalid += [(0, n) for n, _ in start if rng.random() < p_bad]
    invalid += [(n, nv + g) for g in range(ng) for n, _ in goals[g] if rng.random() < p_bad]
    return Case(nv, edges, start, goals, invalid)


def test_eager_equals_rounds_on_random_graphs():
    """Symmetric verdicts: the lazy rounds end at the shortest left-fold cost over the valid edges, bit for bit, whatever
    the order of the removals; every path is valid, simple, and folds to its cost."""
    seen = {0: 0, 2: 0}
    n_removed = 0
    for seed in range(200):
        c = _random_case(seed)
        r = c.run(max_replans=10 ** 9)
        st, cost = c.eager()
        assert np.array_equal(r["status"], st), seed
        assert r["cost"].tobytes() == cost.tobytes(), seed
        assert len(c.asked) == len(set(c.asked)) == r["motions"]
        n_removed += r["removed"]
        for g, p in enumerate(r["paths"]):
            seen[int(st[g])] += 1
            if p is None:
                continue
            assert len(set(p)) == len(p) and p[0] == 0 and p[-1] == c.nv + g
            ws = []
            for a, b in zip(p[:-1], p[1:]):
                assert frozenset((a, b)) not in c.invalid
                if a == 0:
                    ws.append(c.start[1][list(c.start[0]).index(b)])
                elif b >= c.nv:
                    ws.append(c.goals[g][1][list(c.goals[g][0]).index(a)])
                else:
                    ws.append(c.w[c.edge(min(a, b), max(a, b))])
            assert G.left_fold(ws) == r["cost"][g]
    assert seen[0] > 200 and seen[2] > 20 and n_removed > 200


# ---- Python copies of the kernel mutations of the GPU sweep: each changes an answer of a case above ------------------

def _answer(case, **kw):
    try:
        r = case.run(**kw)
    except AssertionError as e:  # the device's error flag: a broken predecessor chain
        return ("error", str(e))
    return (r["status"].tolist(), r["cost"].tolist(), r["paths"], r["rounds"], r["removed"], r["motions"])


def test_mutation_attach_tie_to_the_larger_vertex():
    assert _answer(two_attachments(), mutate=("attach_tie",)) != _answer(two_attachments())
    assert _answer(two_attachments(), mutate=("attach_tie",))[2] == [[0, 3, 4]]


def test_mutation_pred_without_the_hop_rule():
    assert _answer(long_diamond(), mutate=("no_hop_rule",))[2] == [[0, 2, 6, 3, 5, 7]]
    assert _answer(zero_triangle(), mutate=("no_hop_rule",))[0] == "error"


def test_mutation_larger_predecessor():
    assert _answer(diamond(), mutate=("pred_largest",))[2] == [[0, 2, 4, 5, 6]]


def test_mutation_hops_stamp_or(monkeypatch):
    """`&&` -> `||` in the hops kernel's stamp test: an edge only has work when BOTH ends moved in the previous sweep,
    which never holds in sweep 1 (only the start has moved), so no vertex gets a hop count: every chain is broken."""
    real = M._hops_pred

    def stuck(nv, eu, ev, w, dist, **kw):
        hops, pred = real(nv, eu, ev, w, dist, **kw)
        return np.where(np.arange(nv) == 0, 0, -1), np.full(nv, -1, np.int64)
    monkeypatch.setattr(M, "_hops_pred", stuck)
    assert _answer(diamond())[0] == "error"


def test_mutation_resolve_greater_or_equal():
    c = two_removals()
    assert _answer(c, max_replans=2, mutate=("replans_ge",))[0] == [3] and _answer(c, max_replans=2)[0] == [0]


def test_mutation_removals_counted_once_per_edge():
    """the second goal's removal is not counted: its invalid path passes as solved"""
    c = shared_invalid()
    assert _answer(c, mutate=("count_once",)) != _answer(c)


def test_mutation_removed_flags_ignored():
    """many_device_solve builds its weights without eremoved: an edge removed earlier (here 2 - 3 and 4 - 3) comes back
    with its cost, is checked again and removed again: rounds 3 instead of 1, removed 2 instead of 0"""
    c = two_removals()
    w = c.w.copy()
    w[[c.edge(2, 3), c.edge(3, 4)]] = np.inf
    good, bad = _answer(c, w=w), _answer(c)
    assert good[3:5] == (1, 0) and bad[3:5] == (3, 2) and good[:3] == bad[:3]


def test_mutation_cache_read_at_the_wrong_offset():
    """The verdict cache covers the whole edge list, query prefix first: with `fk` prefix edges the roadmap edge e,
    direction d sits at 2 (fk + e) + d.  Read at 2 e + d instead, the rejection cached for 2 - 3 lands on edge 0 + ... a
    different edge: here the valid 2 - 5 is removed and the goal is lost."""
    c = two_removals()
    fk = 3
    cache = np.zeros(2 * (fk + len(c.eu)), np.uint8)
    cache[2 * (fk + c.edge(2, 3))] = 2
    cache[2 * (fk + c.edge(2, 5))] = 1

    def initial(offset):
        return {(e, d): int(cache[offset + 2 * e + d]) for e in range(len(c.eu)) for d in (0, 1)
                if cache[offset + 2 * e + d]}
    good, bad = _answer(c, initial=initial(2 * fk)), _answer(c, initial=initial(0))
    assert good[:3] == _answer(c)[:3] and good[5] == _answer(c)[5] - 2
    assert bad != good


def test_scipy_and_heapq_searches_agree_bit_for_bit(monkeypatch):
    """random float weights on a graph large enough for the scipy path: the same distances, +inf where unreachable"""
    rng = np.random.default_rng(1)
    nv = M.LARGE + 500
    u = rng.integers(0, nv - 200, 4 * nv)
    v = rng.integers(0, nv - 200, 4 * nv)
    keep = u != v
    u, v = np.minimum(u, v)[keep], np.maximum(u, v)[keep]
    key = np.unique(u * nv + v)
    u, v = key // nv, key % nv
    w = rng.random(len(u)) * 3.0 + 1e-3
    w[rng.random(len(u)) < 0.05] = np.inf
    fast = M.dijkstra(nv, u, v, w)
    monkeypatch.setattr(M, "LARGE", 10 ** 9)
    slow = M.dijkstra(nv, u, v, w)
    assert fast.tobytes() == slow.tobytes() and np.isinf(fast[-1]) and np.isfinite(fast).sum() > nv // 2


def test_mutation_shortlist_of_exactly_k_changes_no_list():
    """Mutation 7 (kk = k, the shortlist always made).  The product's shortlist of k + 8 is accepted wherever the
    (k + 8)-th distance exceeds the k-th by more than 1e-9: the device list is used.  With kk = k the shortlist's last
    entry IS the k-th, `last - 1e-9 > k-th` never holds, and every goal with at least k candidates goes to the host brute
    force; with fewer candidates the shortlist holds them all.  Either way the list is the brute force's: the mutation
    moves work to the host and changes no result, so no comparison of results can catch it."""
    rng = np.random.default_rng(3)
    V = np.concatenate([rng.random((300, 3)) * 8.0, np.tile([0.0, 0.0, 0.0, 1.0], (300, 1))], 1)
    vinvalid = np.zeros(300, bool)
    vinvalid[[5, 17, 170]] = True
    goals = np.concatenate([rng.random((40, 3)) * 8.0, np.tile([0.0, 0.0, 0.0, 1.0], (40, 1))], 1)
    for k in (1, 24, 56, 57, 63, 64, 65, 128):
        C = M.classify(V, vinvalid, goals[0], goals, k)
        kk, kk_mut = M.shortlist_k(k), M.shortlist_k(k, mutate=True)
        assert kk == (k + 8 if k <= 56 else 64) and kk_mut == min(k, 64)
        used = 0
        for g in range(len(goals)):
            ids, d, exact = M.shortlist(V, vinvalid, goals[g], k, kk)
            ids_m, d_m, exact_m = M.shortlist(V, vinvalid, goals[g], k, kk_mut, force=True)
            assert np.array_equal(ids, C["goal_ids"][g]) and np.array_equal(ids_m, ids) and np.array_equal(d_m, d)
            assert (exact is None) == (k >= 64) and exact_m is False
            used += exact is True
        assert used == (len(goals) if k < 64 else 0)
    # fewer candidates than the shortlist: it holds them all, with either kk
    few = V[:12]
    for kk in (M.shortlist_k(15), M.shortlist_k(15, mutate=True)):
        ids, d, exact = M.shortlist(few, None, goals[0], 15, kk, force=True)
        assert exact is True and len(ids) == 10
