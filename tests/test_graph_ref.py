"""Self-tests of tests/graph_ref.py (CPU only): the references of the graph sweep must themselves be right."""
import numpy as np
import pytest

import graph_ref as G


def _states(n, seed, dup=0):
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-1.0, 1.0, (n, 3))
    xyz[:, 2] *= 0.05
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    V = np.concatenate([xyz, q], 1)
    if dup:  # exact copies: distance ties the lists must break by index
        V[n - dup:] = V[:dup]
    return V


def _full_bruteforce(V, k_of, pred_only=False, exclude=None):
    n = len(V)
    D = G.se3_distance(V, V)
    np.fill_diagonal(D, np.inf)
    if pred_only:
        D[np.arange(n)[None, :] >= np.arange(n)[:, None]] = np.inf
    if exclude is not None:
        D[:, exclude] = np.inf
    order = np.argsort(D, axis=1, kind="stable")
    k = int(max(k_of))
    idx = np.full((n, k), G.NONE, np.uint32)
    dist = np.full((n, k), np.inf)
    for i in range(n):
        o = order[i, :k_of[i]]
        o = o[np.isfinite(D[i, o])]
        idx[i, :len(o)] = o
        dist[i, :len(o)] = D[i, o]
    return idx, dist


@pytest.mark.parametrize("pred_only", [False, True])
def test_chunked_bruteforce_equals_the_full_matrix(pred_only):
    V = _states(301, 1, dup=7)
    k_of = G.construction2_k_of(0, len(V)) if pred_only else np.full(len(V), 9)
    ref_i, ref_d = _full_bruteforce(V, k_of, pred_only)
    got_i, got_d = G.knn_bruteforce(V, np.arange(len(V)), k_of, pred_only=pred_only, chunk=37)
    assert np.array_equal(got_i, ref_i) and np.array_equal(got_d, ref_d)
    assert G.check_knn_rows(V, np.arange(len(V)), got_i, got_d, k_of, pred_only=pred_only, chunk=23) == 0


def test_check_knn_rows_rejects_wrong_lists():
    V = _states(200, 2, dup=4)
    rows = np.arange(len(V))
    k = 12
    idx, dist = G.knn_bruteforce(V, rows, k)
    excl = np.array([5, 6, 7])
    ie, de = G.knn_bruteforce(V, rows, k, exclude=excl)
    G.check_knn_rows(V, rows, ie, de, k, exclude=excl)
    with pytest.raises(AssertionError):
        G.check_knn_rows(V, rows, idx, dist, k, exclude=excl)
    # a missed neighbour: the list of one row shifted by one (the true k-th is dropped, a farther one comes in)
    bad_i, bad_d = idx.copy(), dist.copy()
    bad_i[3, 4:], bad_d[3, 4:] = idx[3, 5:].tolist() + [0], dist[3, 5:].tolist() + [0.0]
    full_i, full_d = G.knn_bruteforce(V, rows[3:4], k + 1)
    bad_i[3, -1], bad_d[3, -1] = full_i[0, -1], full_d[0, -1]
    with pytest.raises(AssertionError):
        G.check_knn_rows(V, rows, bad_i, bad_d, k)
    # not ascending
    bad_i, bad_d = idx.copy(), dist.copy()
    bad_i[9, [1, 2]], bad_d[9, [1, 2]] = idx[9, [2, 1]], dist[9, [2, 1]]
    with pytest.raises(AssertionError):
        G.check_knn_rows(V, rows, bad_i, bad_d, k)
    # a distance off by more than 1e-11
    bad_d = dist.copy()
    bad_d[11, 0] += 5e-11
    with pytest.raises(AssertionError):
        G.check_knn_rows(V, rows, idx, bad_d, k)
    # a slot left unused although there are candidates
    bad_i, bad_d = idx.copy(), dist.copy()
    bad_i[0, -1], bad_d[0, -1] = G.NONE, np.inf
    with pytest.raises(AssertionError):
        G.check_knn_rows(V, rows, bad_i, bad_d, k)
    # rows longer than k: the tail must be NONE / inf
    wide_i = np.concatenate([idx, np.full((len(V), 3), G.NONE, np.uint32)], 1)
    wide_d = np.concatenate([dist, np.full((len(V), 3), np.inf)], 1)
    G.check_knn_rows(V, rows, wide_i, wide_d, k)


def test_fewer_candidates_than_k():
    V = _states(6, 3)
    idx, dist = G.knn_bruteforce(V, np.arange(6), 10)
    assert np.all((idx[:, 5:] == G.NONE)) and np.all(np.isinf(dist[:, 5:])) and np.all(idx[:, :5] != G.NONE)
    G.check_knn_rows(V, np.arange(6), idx, dist, 10)


def test_arc_cut_off_pairs_may_take_either_branch():
    a = np.array([[0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0]])
    th = 2 * np.arccos(1.0 - 1e-9)  # dq = cos(th / 2) sits on the cut-off
    b = np.array([[0.3, 0.0, 0.0, 0.0, 0.0, np.sin(th / 2), np.cos(th / 2)]])
    d, alt = G._se3_distance_both(a, b)
    assert np.isfinite(alt[0, 0]) and abs(d[0, 0] - alt[0, 0]) > 1e-6


def test_k_rules():
    assert G.roadmap_k(0, 3002) == int(np.ceil(np.e * (1 + 1 / 6) * np.log(3002)))
    assert G.roadmap_k(200, 5000) == 128 and G.roadmap_k(128, 5000) == 128 and G.roadmap_k(127, 5000) == 127
    assert G.roadmap_k(0, 3) == 2 and G.roadmap_k(50, 7) == 6 and G.roadmap_k(0, 2) == 1
    k_of = G.construction2_k_of(0, 3002)
    k = G.roadmap_k(0, 3002)
    assert k_of[0] == 0 and k_of[1] == 1 and k_of[2] == 2 and k_of.max() == k
    assert all(k_of[i] == min(G.roadmap_kstar(i + 1), i, k) for i in range(0, 3002, 97))
    assert G.tree_k(1.1, 1000) == G.k_tree_default(1000)
    # the grid of a 3-vertex roadmap on a small square map is one cell
    assert G.knn_grid_dims(30 * 0.1, 30 * 0.1, 3) == (1, 1)
    assert G.knn_grid_dims(300 * 0.04, 90 * 0.04, 3002)[0] > G.knn_grid_dims(300 * 0.04, 90 * 0.04, 3002)[1]


def test_symmetrised_edges_and_min_weight_graph():
    knn = np.array([[1, 2, G.NONE], [0, 2, 3], [3, 0, 1], [2, 1, G.NONE]], np.uint32)
    want = sorted({(min(i, int(j)), max(i, int(j))) for i in range(4) for j in knn[i] if j != G.NONE})
    assert [tuple(e) for e in G.symmetrised_edges(knn).tolist()] == want
    W = G.min_weight_csr([0, 0, 1, 0], [1, 1, 2, 1], [3.0, 1.0, 2.0, 5.0], 3)
    assert W[0, 1] == 1.0 and W[1, 2] == 2.0 and W.nnz == 2


def test_left_fold_is_sequential():
    w = [0.1, 0.2, 0.3, 1e-17, 1e16, -1e16]
    acc = 0.0
    for x in w:
        acc += x
    assert G.left_fold(w) == acc
    assert G.left_fold([1.0, 1e16, -1e16]) == 0.0 and G.left_fold([1e16, -1e16, 1.0]) == 1.0
