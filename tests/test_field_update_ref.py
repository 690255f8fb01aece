"""tests/field_update_ref.py, the numpy restatement of artp_field_update's four steps, against
lattice_ref's Dijkstra on the new mask, on 12 x 12 versions of the device cases of tests/test_cost_field_update.py; and the
C ABI of the update without a device.

Both sides fold the same float64 weights of one Lattice, and the least fixed point is unique, so distances must agree bit
for bit; the hop counts must be the fewest-tight-edges counts of a field computed anew."""
import ctypes as C

import numpy as np
import pytest

import field_update_ref as FU
import lattice_ref as LR
from art_planner_amd import _capi

N = 12


def heights(seed):
    return (np.random.default_rng(seed).random((N, N)) * 0.3).astype(np.float32)


def lattice(mask, n_yaw, objective, z):
    return LR.Lattice(mask, n_yaw, -0.1 * np.arange(N), -0.1 * np.arange(N), z, objective)


def serpentine(n_yaw, shortcut):
    """Walls on rows 2, 5, 8 with the way through at alternating ends; shortcut: one more opening in the middle wall."""
    full = np.uint32((1 << n_yaw) - 1)
    m = np.full((N, N), full, np.uint32)
    for i, r in enumerate(range(2, N - 1, 3)):
        m[r, :] = 0
        m[r, N - 1 if i % 2 == 0 else 0] = full
    if shortcut:
        m[5, 8] = full
    return m


def island(n_yaw, joined):
    """Rows 0..5 and rows 7..11, joined by the single cell (6, 4)."""
    full = np.uint32((1 << n_yaw) - 1)
    m = np.full((N, N), full, np.uint32)
    m[6, :] = 0
    if joined:
        m[6, 4] = full
    return m


def run(mask_old, mask_new, n_yaw, objective, sources, reverse, z_old, z_new=None, hop_rule=True):
    z_new = z_old if z_new is None else z_new
    lat_old, lat_new = lattice(mask_old, n_yaw, objective, z_old), lattice(mask_new, n_yaw, objective, z_new)
    dist, hops = FU.compute(lat_old, sources, reverse)
    got_d, got_h, stats = FU.update(lat_new, lat_old.bits, dist, hops, reverse, hop_rule)
    want_d, want_h = FU.compute(lat_new, sources, reverse)
    return got_d, got_h, want_d, want_h, stats


def assert_same(got_d, got_h, want_d, want_h):
    assert np.array_equal(got_d.view(np.uint64), want_d.view(np.uint64))
    assert np.array_equal(got_h, want_h)


def test_update_entry_points_are_exported_and_refuse_a_null_field():
    L = _capi.load()
    mask = np.ones(4, np.uint32)
    rect = np.array([0, 0, 2, 2], np.int32)
    assert L.artp_field_update(None, mask.ctypes.data, 0, rect.ctypes.data, 0) == -1
    assert L.artp_field_update(None, mask.ctypes.data, 0, None, 1) == -1
    s = _capi.FieldUpdateStats()
    assert L.artp_field_update_stats(None, C.byref(s)) == -1
    assert C.sizeof(s) == 10 * 8
    assert [n for n, _ in _capi.FieldUpdateStats._fields_] == [
        "changed_words", "removed_nodes", "added_nodes", "dead_nodes", "hop_dead_nodes", "unsupport_rounds", "dist_rounds",
        "hop_rounds", "tile_launches", "reached_nodes"]
    assert C.sizeof(_capi.FieldStats()) == 8 * 8      # artp_field_stats_t is what it was


def test_hops_of_the_reference_are_the_fewest_tight_edges():
    lat = lattice(np.full((N, N), 0xf, np.uint32), 4, 0, np.zeros((N, N), np.float32))
    dist, hops = FU.compute(lat, [(3, 3, 1)])
    assert hops[3, 3, 1] == 0 and (hops[3, 3, [0, 2]] == 1).all() and hops[3, 3, 3] == 2   # rotations cost 0 but count
    assert (dist[3, 3] == 0.0).all()
    assert hops[3, 6, 1] == 3 and hops[3, 6, 3] == 5


@pytest.mark.parametrize("n_yaw", [1, 4])
@pytest.mark.parametrize("objective", [0, 1])
def test_closing_and_opening_a_shortcut(n_yaw, objective):
    z = heights(1)
    src = [(0, 0, 0)]
    opened, closed = serpentine(n_yaw, True), serpentine(n_yaw, False)
    got_d, got_h, want_d, want_h, st = run(opened, closed, n_yaw, objective, src, False, z)
    assert_same(got_d, got_h, want_d, want_h)
    assert st["removed_nodes"] == n_yaw and st["dead_nodes"] > 0
    before = FU.compute(lattice(opened, n_yaw, objective, z), src)[0]
    assert (got_d[9:] > before[9:]).all() and np.array_equal(got_d[:5], before[:5])   # behind it: the long way round
    got_d, got_h, want_d, want_h, st = run(closed, opened, n_yaw, objective, src, False, z)
    assert_same(got_d, got_h, want_d, want_h)
    assert st["added_nodes"] == n_yaw and st["dead_nodes"] == 0 and np.isfinite(got_d[5, 8]).all()


def test_a_cut_off_island_dies_only_under_the_hop_rule():
    n_yaw, z = 4, heights(2)
    src = [(1, 1, 0)]
    got_d, got_h, want_d, want_h, st = run(island(n_yaw, True), island(n_yaw, False), n_yaw, 0, src, False, z)
    assert_same(got_d, got_h, want_d, want_h)
    assert np.isinf(got_d[6:]).all() and np.isfinite(got_d[:6]).all()
    assert st["dead_nodes"] == 5 * N * n_yaw
    # without hops[u] + 1 == hops[v] the headings of a cell support one another through the rotations of cost 0
    got_d, _, want_d, _, st = run(island(n_yaw, True), island(n_yaw, False), n_yaw, 0, src, False, z, hop_rule=False)
    assert st["dead_nodes"] == 0
    assert np.isfinite(got_d[7:]).all() and np.isinf(want_d[7:]).all()
    # one heading has no rotations: there the distances alone are enough
    got_d, got_h, want_d, want_h, _ = run(island(1, True), island(1, False), 1, 0, src, False, z, hop_rule=False)
    assert np.array_equal(got_d.view(np.uint64), want_d.view(np.uint64))


@pytest.mark.parametrize("n_yaw", [1, 4])
@pytest.mark.parametrize("objective,reverse", [(0, False), (1, False), (1, True)])
def test_random_flips(n_yaw, objective, reverse):
    rng = np.random.default_rng(10 * n_yaw + objective + 2 * reverse)
    z = heights(3)
    bits = rng.random((N, N, n_yaw)) < 0.8
    bits[0, 0] = bits[11, 11] = True
    new = bits.copy()
    flip = rng.random((6, 6, n_yaw)) < 0.15
    new[3:9, 4:10] ^= flip
    pack = lambda b: (b.astype(np.uint32) << np.arange(n_yaw, dtype=np.uint32)).sum(axis=2).astype(np.uint32)
    src = [(0, 0, 0), (11, 11, 0)]
    got_d, got_h, want_d, want_h, st = run(pack(bits), pack(new), n_yaw, objective, src, reverse, z)
    assert st["removed_nodes"] + st["added_nodes"] == int(flip.sum()) > 0
    assert_same(got_d, got_h, want_d, want_h)
    assert st["reached_nodes"] == int(np.isfinite(want_d).sum())


def test_changed_heights_need_no_special_case():
    z = heights(4)
    z2 = z.copy()
    z2[4:8, 4:8] += np.float32(0.3)
    m = np.full((N, N), 0x3, np.uint32)
    got_d, got_h, want_d, want_h, st = run(m, m, 2, 0, [(0, 0, 0)], True, z, z2)
    assert_same(got_d, got_h, want_d, want_h)
    assert st["dead_nodes"] > 0 and st["removed_nodes"] == st["added_nodes"] == 0
