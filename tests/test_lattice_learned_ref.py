"""tests/lattice_learned_ref.py without a device: Dijkstra over hand-made asymmetric weights, the pruning of negative,
NaN and infinite weights, zero-cost edges and the BFS depth, the EdgeMatrix rows and the pricing."""
import numpy as np

import lattice_learned_ref as LL


def line(n, n_yaw=1, fill=np.inf):
    """A 1 x n strip: w[m] filled with `fill`; move 4 is (0, +1), move 3 is (0, -1)."""
    return np.ones((1, n), np.uint32) * ((1 << n_yaw) - 1), np.full((10, 1, n, n_yaw), fill)


def test_asymmetric_weights_give_different_forward_and_reverse_fields():
    mask, w = line(5)
    w[4, 0, :, 0] = [1.0, 2.0, 4.0, 8.0, 99.0]        # rightwards from cell c
    w[3, 0, :, 0] = [99.0, 0.5, 0.25, 0.125, 0.0625]  # leftwards from cell c
    lat = LL.LearnedLattice(mask, 1, w)
    assert np.isinf(lat.w[4, 0, 4, 0]) and np.isinf(lat.w[3, 0, 0, 0])       # they leave the strip
    fwd, hops = lat.dijkstra([(0, 0, 0)])
    assert fwd[0, :, 0].tolist() == [0.0, 1.0, 3.0, 7.0, 15.0] and hops[0, :, 0].tolist() == [0, 1, 2, 3, 4]
    rev, _ = lat.dijkstra([(0, 0, 0)], reverse=True)   # the cost TO the source: leftwards moves, folded from the source end
    assert rev[0, :, 0].tolist() == [0.0, 0.5, 0.75, 0.875, 0.9375]
    mid, _ = lat.dijkstra([(0, 2, 0)])
    assert mid[0, :, 0].tolist() == [0.75, 0.25, 0.0, 4.0, 12.0]


def test_a_one_way_edge():
    mask, w = line(3)
    w[4, 0, :2, 0] = 1.0                               # rightwards only
    lat = LL.LearnedLattice(mask, 1, w)
    assert lat.dijkstra([(0, 0, 0)])[0][0, :, 0].tolist() == [0.0, 1.0, 2.0]
    assert lat.dijkstra([(0, 2, 0)])[0][0, :, 0].tolist() == [np.inf, np.inf, 0.0]
    assert lat.dijkstra([(0, 2, 0)], reverse=True)[0][0, :, 0].tolist() == [2.0, 1.0, 0.0]


def test_negative_nan_and_missing_ends_are_no_edges():
    mask, w = line(6, fill=1.0)
    mask[0, 4] = 0
    w[4, 0, 1, 0] = -1e-300                            # negative: no edge 1 -> 2
    w[3, 0, 2, 0] = np.nan                             # NaN: no edge 2 -> 1
    lat = LL.LearnedLattice(mask, 1, w)
    assert np.isinf(lat.w[4, 0, 1, 0]) and np.isinf(lat.w[3, 0, 2, 0])
    assert np.isinf(lat.w[4, 0, 3, 0]) and np.isinf(lat.w[3, 0, 5, 0]) and np.isinf(lat.w[:, 0, 4, 0]).all()
    d, _ = lat.dijkstra([(0, 0, 0)])
    assert d[0, :, 0].tolist() == [0.0, 1.0, np.inf, np.inf, np.inf, np.inf]
    d, _ = lat.dijkstra([(0, 3, 0)])
    assert d[0, :, 0].tolist() == [np.inf, np.inf, 1.0, 0.0, np.inf, np.inf]
    assert sorted(lat.components()[1].tolist()) == [1, 2, 2]


def test_rotations_are_priced_per_direction():
    mask, w = line(1, n_yaw=4)
    w[8, 0, 0, :] = [1.0, 1.0, 1.0, 1.0]               # k -> k + 1
    w[9, 0, 0, :] = [10.0, 10.0, 10.0, 0.5]            # k -> k - 1
    lat = LL.LearnedLattice(mask, 4, w)
    fwd, _ = lat.dijkstra([(0, 0, 0)])
    assert fwd[0, 0].tolist() == [0.0, 1.0, 2.0, 3.0]
    rev, _ = lat.dijkstra([(0, 0, 0)], reverse=True)   # to heading 0: 3 -> 0 by move 8 costs 1, 1 -> 0 by move 9 costs 10
    assert rev[0, 0].tolist() == [0.0, 3.0, 2.0, 1.0]


def test_zero_cost_edges_and_bfs_depth():
    mask, w = line(5, n_yaw=2, fill=0.0)
    mask[0, 3] = 0b01
    lat = LL.LearnedLattice(mask, 2, w)
    d, _ = lat.dijkstra([(0, 0, 0)])
    assert (d[lat.bits] == 0.0).all() and np.isinf(d[0, 3, 1])
    depth = lat.bfs_depth([(0, 0, 0)])
    assert depth[0, :, 0].tolist() == [0, 1, 2, 3, 4] and depth[0, :, 1].tolist() == [1, 2, 3, -1, 5]


def test_rows_and_pricing():
    poses = np.zeros((2, 3, 2, 7))
    poses[..., 0] = -np.arange(2.0)[:, None, None]
    poses[..., 1] = -np.arange(3.0)[None, :, None]
    yaw = np.array([0.0, np.pi / 2])
    poses[..., 5], poses[..., 6] = np.sin(yaw / 2), np.cos(yaw / 2)
    rows, inside = LL.edge_rows(poses)
    assert rows.shape == (10, 2, 3, 2, 6) and rows.dtype == np.float32
    assert not inside[0, 0].any() and inside[7, 0, :2].all() and not inside[7, 1].any() and inside[8:].all()
    # move 7 = (+1, +1) from (0, 1, k = 1): the target's x, y, yaw first, then the start's
    assert rows[7, 0, 1, 1].tolist() == [-1.0, -2.0, np.float32(np.pi / 2), 0.0, -1.0, np.float32(np.pi / 2)]
    assert rows[8, 1, 2, 0].tolist() == [-1.0, -2.0, np.float32(np.pi / 2), -1.0, -2.0, 0.0]
    assert rows[9, 1, 2, 0, 2] == np.float32(np.pi / 2) and (rows[0, 0] == 0).all()
    c3 = np.float32([[1.0, 2.0, 0.25], [1.0, 2.0, 0.5], [0.1, 0.2, 0.3]])
    w = LL.price(c3, 0.0, 1.0, 5.0, 0.25)
    assert w[0] == 3.25 and np.isinf(w[1]) and np.isinf(w[2])
    f = lambda v: np.float64(np.float32(v))
    assert LL.price(c3, 0.1, 1.0, 5.0, 1.0)[2] == 0.0 + ((f(0.1) * f(0.1) + f(0.2) * 1.0) + f(0.3) * 5.0)
