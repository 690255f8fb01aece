"""tests/field_shift_clearance_ref.py, the numpy restatement of artp_field_shift_clearance, against
the clearance-weighted field computed on the new window; its counts from the slot's side against a hand-made example; and
the C ABI of the call without a device.

A world mask; the old and the new window are cut from it, so the overlap holds the same cells, but not the same
clearances: what lies outside a window is outside the rectangle, so d2 -- and with it the weights -- of the kept nodes
near a border differ between the two windows.  The weights are position-independent otherwise (field_shift_ref.SPACING
is exact in binary, flat ground), and the least fixed point is unique: distances and hop counts must agree bit for bit."""
import ctypes as C
import os

import numpy as np
import pytest

import clearance_ref as CR
import field_shift_clearance_ref as SC
import field_shift_ref as FS
import field_update_ref as FU
import lattice_ref as LR
from art_planner_amd import _capi

NR, NC = 24, 20
SHIFTS = [(1, 0), (-3, 5), (17, -15)]
PAD = 18                                            # world cells around the old window: more than any shift
CLEAR = dict(radius_cells=3, margin=0.3, gain=3.0)  # margin = 2.4 cells: penalties 1, 0 and in between


def test_the_entry_points_are_declared_exported_and_refuse_a_null_field():
    names = ("artp_field_shift_clearance", "artp_field_clearance_shift_stats")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "artp_c.h")).read()
    for name in names:
        assert name in _capi.SYMBOLS, name
        assert f"int {name}(artp_field* f" in header, name
    assert "} artp_field_clearance_shift_stats_t;" in header
    L = _capi.load()
    mask = np.ones(4, np.uint32)
    assert L.artp_field_shift_clearance(None, mask.ctypes.data, 0, 0) == -1
    assert L.artp_field_shift_clearance(None, mask.ctypes.data, 0, 1) == -1
    s = _capi.FieldClearanceShiftStats()
    assert L.artp_field_clearance_shift_stats(None, C.byref(s)) == -1
    fields = [n for n, _ in _capi.FieldClearanceShiftStats._fields_]
    assert fields[:10] == [n for n, _ in _capi.FieldUpdateStats._fields_]
    assert fields[10:] == ["shift_rows", "shift_cols", "kept_cells", "left_nodes", "dropped_blocked", "changed_slots",
                           "weight_tiles", "move_ms", "clearance_ms", "table_ms", "passes_ms"]
    for n, _ in _capi.FieldShiftStats._fields_[:15]:         # the shared counts and the shift's, at the shift's offsets
        assert getattr(_capi.FieldClearanceShiftStats, n).offset == getattr(_capi.FieldShiftStats, n).offset
    assert C.sizeof(s) == 21 * 8
    assert C.sizeof(_capi.FieldShiftStats()) == 17 * 8       # artp_field_shift_stats_t is what it was


def test_the_counts_of_a_hand_made_3_by_3_example():
    """One heading, a 3 x 3 rectangle of nodes, every existing move at 1.0 before and after a move by one row.  Counted by
    hand, in the new rectangle:
      row 0 entered: its slots had +inf and hold an edge now -- 3 at each corner cell, 5 at the middle one: 11
      row 1 was row 0: its three slots towards row 0 were +inf (outside) and hold an edge -- 2 + 3 + 2: 7
      row 2 was row 1: its three slots towards the row below held an edge and are +inf now -- 2 + 3 + 2: 7
    25 in all, the same in both directions (the weights are symmetric), in one tile.  Then the move (1, 1) -> (1, 2) priced
    2.0 afterwards: one more slot -- offset 4 of its origin (1, 1) in a reverse field, offset 3 of its target (1, 2) in a
    forward one; both held 1.0 at the node one row up."""
    w = LR.Lattice(np.ones((3, 3), np.uint32), 1, np.zeros(3), np.zeros(3), np.zeros((3, 3))).w
    ones = np.where(np.isfinite(w), 1.0, np.inf)
    assert int(np.isfinite(ones).sum()) == 4 * 3 + 4 * 5 + 8
    for reverse in (False, True):
        assert SC.changed(ones, ones, 0, 0, reverse) == (0, 0)
        assert SC.changed(ones, ones, 1, 0, reverse) == (25, 1)
        after = ones.copy()
        after[4][1, 1, 0] = 2.0
        assert SC.changed(ones, after, 1, 0, reverse) == (26, 1)
        assert SC.changed(ones, after, 0, 0, reverse) == (1, 1)
    # whose slot it is: the origin's in a reverse field, the target's in a forward one
    assert SC.slot_weights(after, True)[4][1, 1, 0] == 2.0 and SC.slot_weights(after, False)[3][1, 2, 0] == 2.0
    assert (SC.slot_weights(after, False) == 2.0).sum() == 1
    # nothing overlaps: every slot that holds an edge now had +inf
    assert SC.changed(ones, ones, 3, 0, True) == (40, 1)
    # tiles: a 20 x 20 rectangle is 2 x 2 tiles; one changed move from (15, 3) to (16, 3) belongs to tile (0, 0) in a
    # reverse field and to tile (1, 0) in a forward one
    big = LR.Lattice(np.ones((20, 20), np.uint32), 1, np.zeros(20), np.zeros(20), np.zeros((20, 20))).w
    big = np.where(np.isfinite(big), 1.0, np.inf)
    other = big.copy()
    other[6][15, 3, 0] = 3.0
    other[1][4, 17, 0] = 3.0                        # (4, 17) -> (3, 17): tile (0, 1) either way
    assert SC.changed(big, other, 0, 0, True) == (2, 2) and SC.changed(big, other, 0, 0, False) == (2, 2)
    assert SC.slot_weights(other, True)[6][15, 3, 0] == 3.0 and SC.slot_weights(other, False)[1][16, 3, 0] == 3.0


def world_mask(n_yaw, seed):
    """Random per-heading nodes at density 0.9 with a few discs and walls cleared: structure at the scale of the radius."""
    rng = np.random.default_rng(seed)
    shape = (NR + 2 * PAD, NC + 2 * PAD)
    bits = rng.random(shape + (n_yaw,)) < 0.9
    r, c = np.meshgrid(np.arange(shape[0]), np.arange(shape[1]), indexing="ij")
    for _ in range(10):
        r0, c0, rad = rng.integers(0, shape[0]), rng.integers(0, shape[1]), rng.integers(1, 4)
        bits[(r - r0) ** 2 + (c - c0) ** 2 <= rad * rad] = False
    return bits


def pack(bits):
    n_yaw = bits.shape[2]
    return (bits.astype(np.uint32) << np.arange(n_yaw, dtype=np.uint32)).sum(axis=2).astype(np.uint32)


def source(si, sj):
    """A cell of the old window in the middle of the overlap"""
    return ((max(0, -si) + min(NR, NR - si)) // 2, (max(0, -sj) + min(NC, NC - sj)) // 2)


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("objective", [0, 1])
@pytest.mark.parametrize("n_yaw", [1, 7])
def test_a_moved_field_is_repaired_to_the_field_of_the_new_window(n_yaw, objective, reverse):
    bits = world_mask(n_yaw, 100 + n_yaw)
    for si, sj in SHIFTS:
        sr, sc = source(si, sj)
        bits[PAD + sr, PAD + sc, 0] = True
    world = pack(bits)
    lat_old, d2_old = SC.weighted_window(world, PAD, PAD, NR, NC, n_yaw, objective, **CLEAR)
    vals = d2_old[lat_old.bits]
    assert (vals == CR.NONE).any() and ((vals > 0) & (vals < 6)).any()      # penalties 0 and in between (1: no node)
    for si, sj in SHIFTS:
        src = source(si, sj) + (0,)
        dist, hops = FU.compute(lat_old, [src], reverse)
        assert np.isfinite(dist).sum() > 0.5 * lat_old.bits.sum()
        lat_new, d2_new = SC.weighted_window(world, PAD - si, PAD - sj, NR, NC, n_yaw, objective, **CLEAR)
        kept = FS.move(np.ones((NR, NC), bool), si, sj, False)
        # the world did not change, yet kept nodes near the border have another clearance: the outside moved
        assert (FS.move(d2_old, si, sj, 0) != d2_new)[kept].any()
        got_d, got_h, st = SC.shift(lat_new, lat_old, dist, hops, si, sj, reverse)
        now = (src[0] + si, src[1] + sj, 0)
        want_d, want_h = FU.compute(lat_new, [now], reverse)
        assert np.array_equal(got_d.view(np.uint64), want_d.view(np.uint64)), int((got_d.view(np.uint64) != want_d.view(np.uint64)).sum())
        assert np.array_equal(got_h, want_h)
        assert st["reached_nodes"] == int(np.isfinite(want_d).sum())
        assert st["kept_cells"] == (NR - abs(si)) * (NC - abs(sj))
        assert st["removed_nodes"] == 0 and st["added_nodes"] == int(lat_new.bits[~kept].sum())
        # the slots: every edge of a node that entered counts; in the overlap the slots whose weight or existence changed
        s_new = SC.slot_weights(lat_new.w, reverse)
        entered = int(np.isfinite(s_new[:, ~kept]).sum())
        assert entered < st["changed_slots"] < int(np.isfinite(s_new).sum()) + int(np.isfinite(lat_old.w).sum())
        assert 1 <= st["weight_tiles"] <= 4
        # dist is the fold of the new weights: a restated Dijkstra over the restated weights, without the update's steps
        assert np.array_equal(want_d.view(np.uint64), lat_new.dijkstra([now], reverse)[0].view(np.uint64))
