"""tests/field_shift_ref.py, the numpy restatement of artp_field_shift, against
field_update_ref.compute on the new window; and the C ABI of the shift without a device.

A world mask and world heights; the old and the new window are cut from them, so the overlap holds the same cells.  The
new window's top-left corner is the old one's minus the shift: old node (r, c, k) is new node (r + si, c + sj, k).  Both
sides fold the same float64 weights (field_shift_ref.SPACING is exact in binary, see there), and the least fixed point is
unique: distances and fewest-tight-edges hop counts must agree bit for bit."""
import ctypes as C

import numpy as np
import pytest

import field_shift_ref as FS
import field_update_ref as FU
from art_planner_amd import _capi

SHIFTS = [(0, 0), (1, 0), (0, -1), (-3, 5), (7, -6), (2, 2), (-5, -5)]
PAD = 8                                             # world cells around the old window: more than any shift


def assert_same(got_d, got_h, want_d, want_h):
    assert np.array_equal(got_d.view(np.uint64), want_d.view(np.uint64)), int((got_d.view(np.uint64) != want_d.view(np.uint64)).sum())
    assert np.array_equal(got_h, want_h)


def pack(bits):
    n_yaw = bits.shape[2]
    return (bits.astype(np.uint32) << np.arange(n_yaw, dtype=np.uint32)).sum(axis=2).astype(np.uint32)


def test_shift_entry_points_are_exported_and_refuse_a_null_field():
    L = _capi.load()
    mask = np.ones(4, np.uint32)
    assert L.artp_field_shift(None, mask.ctypes.data, 0, 0) == -1
    assert L.artp_field_shift(None, mask.ctypes.data, 0, 1) == -1
    s = _capi.FieldShiftStats()
    assert L.artp_field_shift_stats(None, C.byref(s)) == -1
    names = [n for n, _ in _capi.FieldShiftStats._fields_]
    assert names[:10] == [n for n, _ in _capi.FieldUpdateStats._fields_]
    assert names[10:] == ["shift_rows", "shift_cols", "kept_cells", "left_nodes", "dropped_blocked", "move_ms", "passes_ms"]
    for n, _ in _capi.FieldUpdateStats._fields_:
        assert getattr(_capi.FieldShiftStats, n).offset == getattr(_capi.FieldUpdateStats, n).offset
    assert C.sizeof(s) == 17 * 8
    assert C.sizeof(_capi.FieldUpdateStats()) == 80   # artp_field_update_stats_t is what it was
    assert {"artp_field_shift", "artp_field_shift_stats"} <= set(_capi.SYMBOLS)


def test_move_fills_what_entered():
    a = np.arange(12).reshape(3, 4)
    assert np.array_equal(FS.move(a, 0, 0, -1), a)
    assert np.array_equal(FS.move(a, 1, -1, -1), [[-1, -1, -1, -1], [1, 2, 3, -1], [5, 6, 7, -1]])
    assert (FS.move(a, 3, 0, -1) == -1).all() and (FS.move(a, 0, -4, -1) == -1).all()


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("n_yaw", [1, 4])
@pytest.mark.parametrize("objective", [0, 1])
@pytest.mark.parametrize("size,density", [((14, 14), 0.8), ((40, 33), 0.95)])
def test_a_moved_field_is_repaired_to_the_field_of_the_new_window(size, density, objective, n_yaw, reverse):
    nr, nc = size
    rng = np.random.default_rng(1000 * nr + 10 * n_yaw + objective)
    world_bits = rng.random((nr + 2 * PAD, nc + 2 * PAD, n_yaw)) < density
    src_w = (PAD + 5, PAD + 7)                      # inside every window: rows shift by -5 .. 7, columns by -6 .. 5
    world_bits[src_w] = True
    world = pack(world_bits)
    z = (rng.random(world.shape) * 0.3).astype(np.float32)
    lat_old = FS.window_lattice(world, z, PAD, PAD, nr, nc, n_yaw, objective)
    src_old = (src_w[0] - PAD, src_w[1] - PAD, 0)
    dist, hops = FU.compute(lat_old, [src_old], reverse)
    assert np.isfinite(dist).sum() > 0.5 * world_bits[PAD:PAD + nr, PAD:PAD + nc].sum()
    for si, sj in SHIFTS:
        lat_new = FS.window_lattice(world, z, PAD - si, PAD - sj, nr, nc, n_yaw, objective)
        got_d, got_h, st = FS.shift(lat_new, lat_old.bits, dist, hops, si, sj, reverse)
        want_d, want_h = FU.compute(lat_new, [(src_old[0] + si, src_old[1] + sj, 0)], reverse)
        assert_same(got_d, got_h, want_d, want_h)
        assert st["reached_nodes"] == int(np.isfinite(want_d).sum())
        assert st["kept_cells"] == (nr - abs(si)) * (nc - abs(sj))
        kept = FS.move(np.ones((nr, nc), bool), si, sj, False)
        # the world did not change: nothing differs in the overlap, and what was added lies in the strips that entered
        assert st["removed_nodes"] == 0 and st["added_nodes"] == int(lat_new.bits[~kept].sum())
        assert st["left_nodes"] == int(lat_old.bits[~FS.move(np.ones((nr, nc), bool), -si, -sj, False)].sum())
        if (si, sj) == (0, 0):
            assert st["dead_nodes"] == 0 and np.array_equal(got_d.view(np.uint64), dist.view(np.uint64))


@pytest.mark.parametrize("n_yaw", [1, 4])
@pytest.mark.parametrize("objective", [0, 1])
def test_a_far_arm_whose_bend_left_dies(objective, n_yaw):
    nr, nc, si = 14, 9, 3
    old, new, src, far = FS.u_corridor(nr, nc, n_yaw, 2, si)
    z = (np.random.default_rng(3).random((nr + si, nc)) * 0.2).astype(np.float32)
    world = np.zeros((nr + si, nc), np.uint32)
    world[si:] = old                                # the old window at (si, 0), the new one at (0, 0): nothing but walls enters
    assert np.array_equal(world[:nr], new)
    lat_old = FS.window_lattice(world, z, si, 0, nr, nc, n_yaw, objective)
    lat_new = FS.window_lattice(world, z, 0, 0, nr, nc, n_yaw, objective)
    dist, hops = FU.compute(lat_old, [src])
    far_old = FS.move(far, -si, 0, False)
    assert far.sum() > 0 and np.isfinite(dist[far_old]).all()
    got_d, got_h, st = FS.shift(lat_new, lat_old.bits, dist, hops, si, 0)
    want_d, want_h = FU.compute(lat_new, [(src[0] + si, src[1], 0)])
    assert_same(got_d, got_h, want_d, want_h)
    assert np.isinf(got_d[far]).all()
    assert st["removed_nodes"] == st["added_nodes"] == 0          # no word of the overlap differs: only the border tells
    assert st["dead_nodes"] == int(far.sum()) * n_yaw             # every node of the far arm, and nobody else
    near = (new != 0) & ~far
    assert np.array_equal(got_d[near].view(np.uint64), FS.move(dist, si, 0, np.inf)[near].view(np.uint64))


@pytest.mark.parametrize("n_yaw", [1, 4])
@pytest.mark.parametrize("objective", [0, 1])
def test_an_entering_strip_joins_an_island(objective, n_yaw):
    nr, nc, si = 14, 11, 2
    old, new, src, isl = FS.island(nr, nc, n_yaw, si)
    z = (np.random.default_rng(4).random((nr + si, nc)) * 0.2).astype(np.float32)
    world = np.zeros((nr + si, nc), np.uint32)
    world[si:] = old
    world[:si] = new[:si]
    assert np.array_equal(world[:nr], new)
    lat_old = FS.window_lattice(world, z, si, 0, nr, nc, n_yaw, objective)
    lat_new = FS.window_lattice(world, z, 0, 0, nr, nc, n_yaw, objective)
    dist, hops = FU.compute(lat_old, [src], True)
    assert np.isinf(dist[FS.move(isl, -si, 0, False)]).all()
    got_d, got_h, st = FS.shift(lat_new, lat_old.bits, dist, hops, si, 0, True)
    want_d, want_h = FU.compute(lat_new, [(src[0] + si, src[1], 0)], True)
    assert_same(got_d, got_h, want_d, want_h)
    assert np.isfinite(got_d[isl]).all() and st["dead_nodes"] == 0 and st["added_nodes"] == si * nc * n_yaw
