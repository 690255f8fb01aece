"""The algorithm of artp_field_update_learned without a device: tests/field_update_ref.update, the
four steps of section 13 in numpy, on lattice_learned_ref.LearnedLattice pairs whose WEIGHTS change (with or without the
mask), against field_update_ref.compute on the new lattice.  Both sides fold the same float64 weights and the least fixed
point is unique, so distances agree bit for bit; the hop counts are the fewest-tight-edges counts of a new field.  The four
steps need no new rule for a changed weight: a node whose supporting edge is not tight any more dies and is relaxed again,
a node next to an edge that got cheaper is relaxed.

Also here: the C ABI of the call without a device."""
import ctypes as C

import numpy as np
import pytest

import field_update_ref as FU
import lattice_learned_ref as LL
from art_planner_amd import _capi

NR, NC = 9, 11
# few distinct values, so that ties (several tight predecessors) are the rule; 0, +inf, negative and NaN among them
VALUES = np.array([0.0, 0.0, 0.25, 0.5, 0.5, 1.0, 1.0, 1.5, 3.0, np.inf, -1.0, np.nan])


def pack(bits):
    n_yaw = bits.shape[2]
    return (bits.astype(np.uint64) << np.arange(n_yaw, dtype=np.uint64)).sum(axis=2).astype(np.uint32)


def random_pair(n_yaw, seed):
    """(mask, w) twice: the second with a quarter of the weights drawn again and flips in the middle of the mask.  Every
    weight is drawn on its own: w(a -> b) and w(b -> a) are unrelated."""
    rng = np.random.default_rng(seed)
    bits = rng.random((NR, NC, n_yaw)) < 0.85
    bits[0, 0, 0] = bits[NR - 1, NC - 1, n_yaw - 1] = True
    w = VALUES[rng.integers(0, len(VALUES), (10, NR, NC, n_yaw))]
    new_bits = bits.copy()
    new_bits[2:7, 3:9] ^= rng.random((5, 6, n_yaw)) < 0.2
    redraw = rng.random(w.shape) < 0.25
    new_w = np.where(redraw, VALUES[rng.integers(0, len(VALUES), w.shape)], w)
    return pack(bits), w, pack(new_bits), new_w


def run(old, new, sources, reverse, hop_rule=True):
    dist, hops = FU.compute(old, sources, reverse)
    got_d, got_h, stats = FU.update(new, old.bits, dist, hops, reverse, hop_rule)
    want_d, want_h = FU.compute(new, sources, reverse)
    return got_d, got_h, want_d, want_h, stats, dist


def assert_same(got_d, got_h, want_d, want_h):
    assert np.array_equal(got_d.view(np.uint64), want_d.view(np.uint64))
    assert np.array_equal(got_h, want_h)


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("n_yaw", [1, 2, 3, 7])
def test_random_weights_and_masks(n_yaw, reverse):
    sources = [(0, 0, 0), (NR - 1, NC - 1, n_yaw - 1)]
    moved = 0
    for seed in range(10):
        m0, w0, m1, w1 = random_pair(n_yaw, 1000 * n_yaw + 10 * seed + reverse)
        old, new = LL.LearnedLattice(m0, n_yaw, w0), LL.LearnedLattice(m1, n_yaw, w1)
        assert (old.w != new.w).any() and (m0 != m1).any()
        got_d, got_h, want_d, want_h, st, before = run(old, new, sources, reverse)
        assert_same(got_d, got_h, want_d, want_h)
        assert st["reached_nodes"] == int(np.isfinite(want_d).sum())
        moved += int((before.view(np.uint64) != want_d.view(np.uint64)).sum())
        # the weights alone, on the old mask
        new = LL.LearnedLattice(m0, n_yaw, w1)
        got_d, got_h, want_d, want_h, st, _ = run(old, new, sources, reverse)
        assert_same(got_d, got_h, want_d, want_h)
        assert st["removed_nodes"] == st["added_nodes"] == 0
    assert moved > 10 * n_yaw       # the cases do move the field


def strip(n, fill):
    """A 1 x n strip at one heading: move 4 is (0, +1), move 3 is (0, -1)."""
    return np.ones((1, n), np.uint32), np.full((10, 1, n, 1), fill)


def test_a_region_held_up_by_its_own_zero_cost_edges_dies_with_its_entry_edge():
    mask, w = strip(6, np.inf)
    w[4, 0, 0, 0] = w[4, 0, 1, 0] = 1.0         # 0 -> 1 -> 2: the way in
    w[4, 0, 2:5, 0] = 0.0                       # 2 .. 5: zero-cost edges both ways, each node a tight neighbour of the next
    w[3, 0, 3:6, 0] = 0.0
    old = LL.LearnedLattice(mask, 1, w)
    w2 = w.copy()
    w2[4, 0, 1, 0] = np.inf                     # the entry edge 1 -> 2 goes; the mask stays
    new = LL.LearnedLattice(mask, 1, w2)
    src = [(0, 0, 0)]
    got_d, got_h, want_d, want_h, st, before = run(old, new, src, False)
    assert before[0, :, 0].tolist() == [0.0, 1.0, 2.0, 2.0, 2.0, 2.0]
    assert_same(got_d, got_h, want_d, want_h)
    assert got_d[0, :, 0].tolist() == [0.0, 1.0, np.inf, np.inf, np.inf, np.inf] and st["dead_nodes"] == 4
    # without hops[u] + 1 == hops[v] node 2 is held by node 3 and node 3 by node 2: the region survives (and is wrong)
    got_d, _, want_d, _, st, _ = run(old, new, src, False, hop_rule=False)
    assert st["dead_nodes"] == 0 and got_d[0, :, 0].tolist() == [0.0, 1.0, 2.0, 2.0, 2.0, 2.0]
    assert np.isinf(want_d[0, 2:, 0]).all()


@pytest.mark.parametrize("reverse", [False, True])
def test_a_cheaper_edge_lowers_everything_downstream(reverse):
    mask, w = strip(6, 1.0)
    w[4 if not reverse else 3, 0, 2, 0] = 4.0   # forward: 2 -> 3; reverse (source at the right end): 2 -> 1
    old = LL.LearnedLattice(mask, 1, w)
    w2 = w.copy()
    w2[4 if not reverse else 3, 0, 2, 0] = 0.5
    new = LL.LearnedLattice(mask, 1, w2)
    # forward from cell 0 the edge 2 -> 3 is used; reverse TO cell 0 the edge 2 -> 1 is
    src = [(0, 0, 0)]
    got_d, got_h, want_d, want_h, st, before = run(old, new, src, reverse)
    assert_same(got_d, got_h, want_d, want_h)
    assert st["removed_nodes"] == st["added_nodes"] == 0
    down = slice(3, 6) if not reverse else slice(2, 6)
    assert (got_d[0, down, 0] == before[0, down, 0] - 3.5).all()
    assert np.array_equal(got_d[0, :2, 0], before[0, :2, 0])


def test_update_learned_entry_points_are_exported_and_refuse_a_null_field():
    L = _capi.load()
    mask = np.ones(4, np.uint32)
    rect = np.array([0, 0, 2, 2], np.int32)
    assert L.artp_field_update_learned(None, mask.ctypes.data, 0, rect.ctypes.data) == -1
    assert L.artp_field_update_learned(None, None, 0, None) == -1
    s = _capi.FieldLearnedUpdateStats()
    assert L.artp_field_learned_update_stats(None, C.byref(s)) == -1
    assert C.sizeof(s) == 17 * 8
    names = [n for n, _ in _capi.FieldLearnedUpdateStats._fields_]
    assert names[:10] == [n for n, _ in _capi.FieldUpdateStats._fields_]
    assert names[10:] == ["repriced_slots", "changed_slots", "weight_tiles", "rows_ms", "query_ms", "reprice_ms", "passes_ms"]
    assert C.sizeof(_capi.FieldUpdateStats()) == 10 * 8 and C.sizeof(_capi.FieldLearnedStats()) == 8 * 8   # as they were
