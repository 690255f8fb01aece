"""tests/field_plan_ref.py, the numpy restatement of a blocked-move set on a cost-to-go field (block +
unsupport + relax with blocked slots, on top of field_update_ref.py), against lattice_ref's Dijkstra on the blocked
weights, on the 12 x 12 lattices of tests/test_field_update_ref.py; and the C ABI of the section without a device.

Both sides fold the same float64 weights of one Lattice, and the least fixed point is unique, so distances must agree bit
for bit; the hop counts must be the fewest-tight-edges counts of a field computed anew on the blocked weights."""
import ctypes as C

import numpy as np
import pytest

import field_plan_ref as FP
import field_update_ref as FU
from art_planner_amd import _capi
from test_field_update_ref import N, assert_same, heights, island, lattice, serpentine


def test_plan_entry_points_are_exported_and_refuse_null():
    L = _capi.load()
    for name in ("artp_field_block_moves", "artp_field_unblock", "artp_field_blocked_count", "artp_field_blocked",
                 "artp_field_plan", "artp_field_plan_stats", "artp_field_plan_round_tile_runs"):
        assert name in _capi.SYMBOLS and hasattr(L, name)
    a = np.zeros(3, np.int32)
    n = C.c_uint64(7)
    assert L.artp_field_block_moves(None, a.ctypes.data, a.ctypes.data, 1, C.byref(n)) == -1 and n.value == 0
    n = C.c_uint64(7)
    assert L.artp_field_unblock(None, None, C.byref(n)) == -1 and n.value == 0
    assert L.artp_field_blocked_count(None, C.byref(n)) == -1
    words = np.zeros(4, np.uint16)
    assert L.artp_field_blocked(None, words.ctypes.data) == -1
    st, cost, off = np.zeros(1, np.int32), np.zeros(1), np.zeros(2, np.uint64)
    assert L.artp_field_plan(None, a.ctypes.data, 1, 4, st.ctypes.data, cost.ctypes.data, off.ctypes.data, None, None, 0) == -1
    s = _capi.FieldPlanStats()
    assert L.artp_field_plan_stats(None, C.byref(s)) == -1
    assert L.artp_field_plan_round_tile_runs(None, None, 0, C.byref(C.c_size_t(0))) == -1
    assert C.sizeof(s) == 10 * 8
    assert [n for n, _ in _capi.FieldPlanStats._fields_] == [
        "rounds", "moves_checked", "moves_blocked", "updates", "update_tile_runs", "last_update_tile_runs", "descent_ms",
        "check_ms", "round_ms", "passes_ms"]
    assert C.sizeof(_capi.FieldStats()) == 8 * 8 and C.sizeof(_capi.FieldUpdateStats()) == 10 * 8   # as they were


def test_words_put_a_move_at_its_end_or_at_its_start():
    lat = lattice(np.full((N, N), 0xf, np.uint32), 4, 1, heights(0))
    moves = [((3, 3, 1), (2, 4, 1)),      # move 2 (-1, +1): seen from its end it is offset 5
             ((3, 3, 1), (3, 3, 2)),      # move 8: from its end, offset 9
             ((3, 3, 0), (3, 3, 3))]      # move 9 across the wrap: from its end, offset 8
    fw, rv = FP.words(lat.shape, lat, moves, False), FP.words(lat.shape, lat, moves, True)
    assert fw[2, 4, 1] == 1 << 5 and fw[3, 3, 2] == 1 << 9 and fw[3, 3, 3] == 1 << 8 and int((fw != 0).sum()) == 3
    assert rv[3, 3, 1] == (1 << 2) | (1 << 8) and rv[3, 3, 0] == 1 << 9 and int((rv != 0).sum()) == 2
    assert [FP.back_move(m) for m in range(10)] == [7, 6, 5, 4, 3, 2, 1, 0, 9, 8]


@pytest.mark.parametrize("reverse", [False, True])
def test_at_two_headings_a_rotation_is_both_rotation_moves(reverse):
    """k + 1 and k - 1 are the same heading: Lattice.w holds the rotation as move 8 and as move 9, the device in pull slots
    8 and 9 of its owner.  Blocking it must take both, or the search goes on using the twin."""
    lat = lattice(np.full((N, N), 0x3, np.uint32), 2, 1, heights(6))
    src, tgt = (3, 3, 0), (3, 3, 1)
    move = (tgt, src) if reverse else (src, tgt)
    d0, h0 = FU.compute(lat, [src], reverse)
    assert h0[tgt] == 1
    assert FP.words(lat.shape, lat, [move], reverse)[move[0] if reverse else move[1]] == 0x300
    saved = FP.block(lat, [move])
    assert np.isinf(lat.w[8][move[0]]) and np.isinf(lat.w[9][move[0]])
    want_d, want_h = FU.compute(lat, [src], reverse)
    got_d, got_h, st = FP.repair(lat, d0, h0, reverse)
    assert_same(got_d, got_h, want_d, want_h)
    assert got_d[tgt] > d0[tgt] and got_h[tgt] == 3 and st["dead_nodes"] >= 1   # out, turn there, back
    FP.unblock(lat, saved)
    d, h, _ = FP.repair(lat, got_d, got_h, reverse)
    assert_same(d, h, d0, h0)


def tight_moves(lat, dist, hops, reverse, rng, n):
    """n moves that carry a shortest path: (u -> v) with dist[u] + w == dist[v] and hops[u] + 1 == hops[v], in TRAVEL order."""
    pred, node, w = FU.pull_edges(lat, reverse)
    d, h = dist.reshape(-1), hops.reshape(-1)
    ok = np.flatnonzero((d[pred] + w == d[node]) & np.isfinite(d[node]) & (h[pred] + 1 == h[node]))
    out = []
    for e in ok[rng.permutation(len(ok))[:n]]:
        u, v = np.unravel_index(pred[e], lat.shape), np.unravel_index(node[e], lat.shape)
        out.append((v, u) if reverse else (u, v))
    return [(tuple(int(x) for x in a), tuple(int(x) for x in b)) for a, b in out]


@pytest.mark.parametrize("n_yaw", [1, 4])
@pytest.mark.parametrize("objective,reverse", [(0, False), (1, False), (0, True), (1, True)])
def test_blocking_and_unblocking_against_dijkstra(n_yaw, objective, reverse):
    rng = np.random.default_rng(7 * n_yaw + 2 * objective + reverse)
    z = heights(5)
    mask = serpentine(n_yaw, True)
    src = [(0, 0, 0)]
    lat = lattice(mask, n_yaw, objective, z)
    d0, h0 = FU.compute(lat, src, reverse)
    moves = tight_moves(lat, d0, h0, reverse, rng, 12)
    # objective 0 turns for nothing: a translation is only gone once it is blocked at every heading
    moves += [((a[0], a[1], k), (b[0], b[1], k)) for a, b in moves[:8] if a[:2] != b[:2] for k in range(n_yaw) if k != a[2]]
    # every move from row 4 into the second wall's opening at its end, (5, 0): what lies behind it is left with the
    # opening in the middle of the wall, so the cells next to (5, 0) get a longer way
    gate = [((4, c, k), (5, 0, k)) for c in (0, 1) for k in range(n_yaw)]
    moves += [(b, a) for a, b in gate] if reverse else gate
    a, b = moves[0]
    moves.append((b, a))                                      # both moves of a two-way pair
    # all at once
    saved = FP.block(lat, moves)
    want_d, want_h = FU.compute(lat, src, reverse)
    got_d, got_h, st = FP.repair(lat, d0, h0, reverse)
    assert_same(got_d, got_h, want_d, want_h)
    print(f"  {st['dead_nodes']} nodes died, {int((got_d > d0).sum())} distances rose")
    assert (got_d >= d0).all()
    if objective == 0:        # the heights break the ties; objective 1 at one heading is a grid of equal detours
        assert st["dead_nodes"] > 0 and (got_d > d0).any()
    assert st["removed_nodes"] == st["added_nodes"] == 0
    # one at a time, from the original field
    FP.unblock(lat, saved)
    d, h = d0, h0
    for mv in moves:
        FP.block(lat, [mv])
        d, h, _ = FP.repair(lat, d, h, reverse)
    assert_same(d, h, want_d, want_h)
    # unblocked again: weights that fell, picked up by the relax passes
    FP.unblock(lat, saved)
    d, h, st = FP.repair(lat, d, h, reverse)
    assert_same(d, h, d0, h0)
    assert st["dead_nodes"] == 0


def test_only_the_stated_direction_is_blocked():
    n_yaw, z = 1, np.zeros((N, N), np.float32)
    mask = np.zeros((N, N), np.uint32)
    mask[4, :] = 1                                            # one corridor: every move is a bridge
    lat = lattice(mask, n_yaw, 1, z)
    src = [(4, 0, 0)]
    FP.block(lat, [((4, 5, 0), (4, 6, 0))])
    fw, _ = FU.compute(lat, src, False)
    rv, _ = FU.compute(lat, src, True)
    assert np.isinf(fw[4, 6:]).all() and np.isfinite(fw[4, :6]).all()      # nobody gets past column 5 going out
    assert np.isfinite(rv[4]).all()                                        # coming back uses the other direction


def test_a_blocked_entry_cuts_an_island_off_only_under_the_hop_rule():
    n_yaw, z = 4, heights(2)
    src = [(1, 1, 0)]
    lat = lattice(island(n_yaw, True), n_yaw, 0, z)
    d0, h0 = FU.compute(lat, src)
    entry = [((5, c, k), (6, 4, k)) for c in (3, 4, 5) for k in range(n_yaw)]    # every move onto the joining cell
    FP.block(lat, entry)
    want_d, want_h = FU.compute(lat, src)
    got_d, got_h, st = FP.repair(lat, d0, h0)
    assert_same(got_d, got_h, want_d, want_h)
    assert np.isinf(got_d[6:]).all() and np.isfinite(got_d[:6]).all()
    assert st["dead_nodes"] == (5 * N + 1) * n_yaw
    # without hops[u] + 1 == hops[v] the headings of a cell support one another through the rotations of cost 0
    got_d, _, st = FP.repair(lat, d0, h0, hop_rule=False)
    assert st["dead_nodes"] == 0 and np.isfinite(got_d[7:]).all()
