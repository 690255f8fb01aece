"""CPU suite of the clearance restatement (tests/clearance_ref.py): the shifted-window form against
the brute-force form on small masks, the weight restatement, the numbers of the L-shaped corridor that
tests/test_cost_field_clearance.py relies on, and the new names of the C ABI."""
from collections import deque

import numpy as np
import pytest

import clearance_ref as CR
import lattice_learned_ref as LL
import lattice_ref as LR
from art_planner_amd import _capi


def random_words(shape, n_yaw, seed, p):
    """random low bits with probability p each, random garbage above them"""
    rng = np.random.default_rng(seed)
    bits = rng.random(shape + (n_yaw,)) < p
    low = (bits.astype(np.uint64) << np.arange(n_yaw, dtype=np.uint64)).sum(axis=2)
    high = rng.integers(0, 1 << 32, shape, dtype=np.uint64) & ~np.uint64((1 << n_yaw) - 1) & np.uint64(0xffffffff)
    return (low | high).astype(np.uint32)


@pytest.mark.parametrize("n_yaw,spread", [(1, 0), (2, 0), (2, 1), (7, 0), (7, 1), (7, 3), (16, 2), (32, 16)])
@pytest.mark.parametrize("outside", [False, True])
def test_windows_against_pairwise_distances(n_yaw, spread, outside):
    for seed, shape, R, p in ((1, (12, 9), 3, 0.9), (2, (7, 12), 5, 0.97), (3, (5, 4), 8, 0.8)):
        mask = random_words(shape, n_yaw, seed + 10 * n_yaw, p ** (1.0 / (2 * spread + 1)))
        got = CR.clearance_map(mask, n_yaw, R, spread, outside)
        want = CR.brute_clearance_map(mask, n_yaw, R, spread, outside)
        assert got.dtype == np.uint16 and np.array_equal(got, want)
        # garbage above the low n_yaw bits changes nothing
        assert np.array_equal(got, CR.clearance_map(mask & np.uint32((1 << n_yaw) - 1), n_yaw, R, spread, outside))
        node = CR.planes(mask, n_yaw)
        assert (got[~node] == 0).all()
        if spread == 0:
            assert (got[node] > 0).all()


def test_spread_wraps_around_the_headings():
    # 2 headings: the other heading is both neighbours.  One cell lacks heading 1: with s = 1 it is an obstacle of
    # heading 0 as well, at d2 = 0 for the node it still is.
    m = np.full((5, 5), 3, np.uint32)
    m[2, 2] = 1
    d0, d1 = CR.clearance_map(m, 2, 3, 0), CR.clearance_map(m, 2, 3, 1)
    assert (d0[..., 0] == CR.NONE).all() and d0[2, 2, 1] == 0 and d0[2, 3, 1] == 1 and d0[0, 0, 1] == 8
    assert d1[2, 2, 0] == 0 and d1[2, 2, 1] == 0 and np.array_equal(d1[..., 0][m == 3], d0[..., 1][m == 3])
    # 7 headings: a cell that lacks heading 0 is an obstacle of headings 6, 0 and 1 with s = 1, and of no other
    m = np.full((3, 3), 0x7f, np.uint32)
    m[1, 1] = 0x7e
    d = CR.clearance_map(m, 7, 2, 1)
    assert [int(v) for v in d[1, 0]] == [1, 1, CR.NONE, CR.NONE, CR.NONE, CR.NONE, 1]
    assert [int(v) for v in d[1, 1]] == [0, 0, CR.NONE, CR.NONE, CR.NONE, CR.NONE, 0]
    # s = n_yaw // 2: any missing heading
    assert (CR.clearance_map(m, 7, 2, 3)[1, 0] == 1).all()


def test_the_cap_and_the_outside():
    m = np.ones((9, 9), np.uint32)
    assert (CR.clearance_map(m, 1, 5) == CR.NONE).all()
    d = CR.clearance_map(m, 1, 3, 0, True)[..., 0]
    assert d[0, 0] == 1 and d[2, 5] == 9 and d[3, 3] == CR.NONE and d[4, 4] == CR.NONE
    assert (CR.clearance_map(np.zeros((4, 4), np.uint32), 1, 3) == 0).all()
    # holes at (3, 4) and (4, 4) from a probe with R = 5: 25 counts, 32 does not
    m = np.ones((12, 12), np.uint32)
    m[2 + 3, 3 + 4] = 0
    assert CR.clearance_map(m, 1, 5)[2, 3, 0] == 25
    m = np.ones((12, 12), np.uint32)
    m[2 + 4, 3 + 4] = 0
    assert CR.clearance_map(m, 1, 5)[2, 3, 0] == CR.NONE


def test_weights():
    n_yaw, res = 4, 0.04
    mask = random_words((9, 8), n_yaw, 5, 0.85)
    x, y = -res * np.arange(9), -res * np.arange(8)
    z = np.random.default_rng(1).random((9, 8)).astype(np.float32) * 0.02
    d2 = CR.clearance_map(mask, n_yaw, 4)
    for objective in (0, 1):
        base = LR.Lattice(mask, n_yaw, x, y, z, objective).w
        w0 = CR.weights(base, d2, res, 0.1, 0.0)
        assert np.array_equal(w0.view(np.uint64), base.view(np.uint64))      # gain 0: the base array unchanged
        w = CR.weights(base, d2, res, 0.1, 3.0)
        fin = np.isfinite(base)
        assert np.array_equal(np.isfinite(w), fin) and (w[fin] >= base[fin]).all() and (w[fin] <= 4.0 * base[fin]).all()
        assert (w[fin] > base[fin]).any()
    pen = CR.penalty(np.array([0, 1, 4, 25, CR.NONE], np.uint16), 0.04, 0.2)
    assert pen[0] == 1.0 and pen[1] == 1.0 - 0.04 / 0.2 and pen[2] == 1.0 - (0.04 * 2.0) / 0.2 and pen[3] == 0.0 and pen[4] == 0.0
    f = CR.factors(d2, res, 0.1, 3.0)
    assert np.isnan(f[0][0]).all() and np.isnan(f[7][-1]).all() and not np.isnan(f[8]).any()   # moves that leave the rectangle
    # the larger penalty of the two ends, the same both ways
    a, b = LL.move_slices(9, 8, 4)
    assert np.array_equal(f[4][a], f[3][b])


def corridor():
    m = np.zeros((40, 40), np.uint32)
    m[4:11, 4:35] = 1
    m[4:35, 28:35] = 1
    return m, (7, 4, 0), (34, 31, 0)


def device_path(lat, dist, source, target):
    """field_descend's rule on the reference's distances (forward field): hop counts = fewest tight edges from the source,
    then from the target the first move, in the order of the ten moves, to a tight neighbour one hop closer."""
    hops = np.full(lat.shape, -1, np.int64)
    hops[source] = 0
    q = deque([source])
    while q:
        u = q.popleft()
        for m in range(8):
            v = (u[0] + LR.MOVES[m][0], u[1] + LR.MOVES[m][1], 0)
            if np.isfinite(lat.w[m][u]) and hops[v] < 0 and dist[u] + lat.w[m][u] == dist[v]:
                hops[v] = hops[u] + 1
                q.append(v)
    path = [target]
    while path[-1] != source:
        v = path[-1]
        for j in range(8):
            u = (v[0] + LR.MOVES[j][0], v[1] + LR.MOVES[j][1], 0)
            if not lat.exists(u):
                continue
            if hops[u] + 1 == hops[v] and dist[u] + lat.w[7 - j][u] == dist[v]:
                path.append(u)
                break
        else:
            raise AssertionError("no tight predecessor")
    return path[::-1]


@pytest.mark.parametrize("objective", [0, 1])
def test_the_corridor_numbers(objective):
    """What tests/test_cost_field_clearance.py asserts on the device, on the reference first."""
    res = 0.04
    m, src, tgt = corridor()
    d2 = CR.clearance_map(m, 1, 5)
    base = LR.Lattice(m, 1, -res * np.arange(40), -res * np.arange(40), np.zeros((40, 40)), objective)
    plain, _ = base.dijkstra([src])
    lat = LL.LearnedLattice(m, 1, CR.weights(base.w, d2, res, 4 * res, 4.0))
    weighted, _ = lat.dijkstra([src])
    p0, p1 = device_path(base, plain, src, tgt), device_path(lat, weighted, src, tgt)
    c0 = min(int(d2[v]) for v in p0[3:-3])
    c1 = min(int(d2[v]) for v in p1[3:-3])
    print(f"  objective {objective}: unweighted {len(p0)} states, min d2 {c0}; weighted {len(p1)} states, min d2 {c1}")
    assert c0 <= 2 and c1 > c0
    assert d2[7, 15, 0] == 16            # the corridor's centre line


def test_the_new_names_are_bound():
    for name in ("artp_clearance_params_defaults", "artp_clearance_map", "artp_clearance_map_dev",
                 "artp_field_clearance_params_defaults", "artp_field_compute_clearance", "artp_field_clearance"):
        assert name in _capi.SYMBOLS, name
    import ctypes as C
    assert C.sizeof(_capi.ClearanceParams) == 16
    assert C.sizeof(_capi.FieldClearanceParams) == C.sizeof(_capi.FieldParams) + 16 + 16
