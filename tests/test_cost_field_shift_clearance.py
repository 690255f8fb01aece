"""artp_field_shift_clearance (csrc/clearance.h): a clearance-weighted field carried across a move of
the map by whole cells must hold the bits of a clearance field computed anew on the new map.  artp_field_compute_clearance,
which the call does not touch, is the exact oracle of every case: dist as bit patterns, reached_nodes, edge_costs over ALL
moves of the rectangle (the weight table slot for slot), clearance() -- also against tests/clearance_ref.py -- and some
eight paths with their poses and costs (test_cost_field_clearance_update.snapshot / same).  Every case runs the tiled and
the plain form.

The counts are held against counts made outside the call: the shift's against test_cost_field_shift.expected_counts,
changed_slots and weight_tiles against tests/field_shift_clearance_ref.changed on the edge costs of the field before the
call and of the new field.  That count is what pins the gather of the old slot: a wrong old slot over-flags silently (the
passes then do too much and still reach the fixed point) or under-flags rarely.

The world and the windows are test_cost_field_shift's: 112 x 112 cells at 0.04 m, the map a 72 x 64 window, the field's
rectangle (5, 3, 61, 53).  The world's mask has structure at the scale of the radius -- a dozen discs and a dozen walls of
2 .. 6 cells -- and 5 % per-heading noise."""
import numpy as np
import pytest

import clearance_ref as CR
import field_shift_clearance_ref as SC
import field_shift_ref as FS
import lattice_learned_ref as LL
import lattice_ref as LR
from art_planner_amd import _capi
from synthetic import GridMap, map_from_device, perlin_terrain
from test_cost_field import ROBOT, assert_field, device_map
from test_cost_field_clearance_update import moves_of, same, snapshot, targets_of
from test_cost_field_shift import (MAP, RECT, RES, STAT_KEYS, WORLD, blocked_moves, corners, expected_counts, install, moved,
                                   moved_blocked, rect_bits, world_elev)
from test_cost_field_update import bits_of, pack

pytestmark = pytest.mark.gpu

CLEAR = dict(radius_cells=5, margin=0.15, gain=3.0)
NR, NC = RECT[2], RECT[3]
N_TILES = ((NR + 15) // 16) * ((NC + 15) // 16)
COUNT_KEYS = STAT_KEYS + ("changed_slots", "weight_tiles")


@pytest.fixture(scope="module")
def ctx():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from art_planner_amd.context import Context
    c = Context(0, ROBOT)
    yield c
    c.close()


# ---- helpers ----------------------------------------------------------------------------------------------------
def world_bits(n_yaw, seed=0):
    rng = np.random.default_rng(900 + 10 * n_yaw + seed)
    bits = rng.random((WORLD, WORLD, n_yaw)) >= 0.05
    r, c = np.meshgrid(np.arange(WORLD), np.arange(WORLD), indexing="ij")
    for _ in range(12):
        r0, c0, rad = rng.integers(0, WORLD), rng.integers(0, WORLD), rng.integers(2, 7)
        bits[(r - r0) ** 2 + (c - c0) ** 2 <= rad * rad] = False
    for i in range(12):
        r0, c0, length, thick = rng.integers(0, WORLD), rng.integers(0, WORLD), rng.integers(8, 30), rng.integers(2, 7)
        if i % 2:
            bits[r0:r0 + length, c0:c0 + thick] = False
        else:
            bits[r0:r0 + thick, c0:c0 + length] = False
    return bits


def free_sources(old_b, new_b, si, sj, n_yaw):
    """Two nodes of the old rectangle that stay inside it, near the middle of the overlap, whose cells and the eight
    around them hold the first and the last heading and most of the others in both masks: in open ground, not inside an
    obstacle."""
    was = FS.move(old_b, si, sj, False)
    ends = [0, n_yaw - 1]
    open_ = was[..., ends].all(axis=2) & new_b[..., ends].all(axis=2) & (was.mean(axis=2) > 0.5) & (new_b.mean(axis=2) > 0.5)
    ok = open_.copy()
    for dr in (-1, 0, 1):
        for dc in (-1, 0, 1):
            ok &= FS.move(open_, dr, dc, False)
    kept = FS.move(np.ones((NR, NC), bool), si, sj, False)
    cand = np.argwhere(ok & kept)
    centre = np.argwhere(kept).mean(axis=0)
    cand = cand[np.argsort(((cand - centre) ** 2).sum(axis=1), kind="stable")]
    first = cand[0]
    second = next(c for c in cand if 9 <= ((c - first) ** 2).sum())
    return [(int(first[0]) - si, int(first[1]) - sj, 0), (int(second[0]) - si, int(second[1]) - sj, n_yaw - 1)]


def compare(ctx, fields, new_m, n_yaw, now, reverse, kw, clear, seed=0, words=None, rect=RECT):
    """Every field against ONE new clearance field on the installed map with new_m (and the moves of `words` blocked);
    returns the new field's snapshot."""
    with ctx.clearance_cost_field(new_m, n_yaw, now, **kw, **clear) as fresh:
        if words is not None:
            a, b = blocked_moves(words, n_yaw, reverse)
            if a:
                assert fresh.block_moves(a, b) == len(a)
            assert np.array_equal(fresh.blocked(), words)
        tg = targets_of(fresh.dist(), now, seed)
        want = snapshot(fresh, tg)
    d2_ref = CR.clearance_map(new_m, n_yaw, clear["radius_cells"], clear.get("yaw_spread", 0),
                              bool(clear.get("outside_is_obstacle", False)))
    assert np.array_equal(want["d2"], d2_ref)
    for j, f in enumerate(fields):
        same(ctx, f, snapshot(f, tg), want, new_m, n_yaw, rect, now, reverse, tg, j)
        if words is not None:
            assert np.array_equal(f.blocked(), words) and f.blocked_count() == len(a)
    return want


def edge_array(f):
    a, b = moves_of((f.nrows, f.ncols, f.n_yaw))
    return f.edge_costs(a, b).reshape(10, f.nrows, f.ncols, f.n_yaw)


def same_counts(st, sp):
    for key in COUNT_KEYS:
        assert st[key] == sp[key], key
    assert sp["tile_launches"] == 0


def case(ctx, shift, n_yaw, objective, reverse, refresh=True, clear=CLEAR, edit=True, seed=0):
    """Both forms computed on the old window, carried onto the new one whose mask also differs in a block of the overlap
    (edit); returns the tiled form's stats."""
    si, sj = shift
    old_c, new_c = corners(si, sj)
    bits = world_bits(n_yaw, seed)
    edited = bits.copy()
    if edit:
        block = edited[50:62, 52:66]                            # world cells inside every window of this file
        block ^= np.random.default_rng(7).random(block.shape) < 0.15
    src = free_sources(rect_bits(bits, old_c), rect_bits(edited, new_c), si, sj, n_yaw)
    old_b, new_b = rect_bits(bits, old_c), rect_bits(edited, new_c)
    old_m, new_m = pack(old_b), pack(new_b)
    kw = dict(rect=RECT, objective=objective, reverse=reverse)
    install(ctx, old_c)
    with ctx.clearance_cost_field(old_m, n_yaw, src, **kw, **clear) as ft, \
            ctx.clearance_cost_field(old_m, n_yaw, src, plain_sweeps=True, **kw, **clear) as fp:
        assert ft.stats()["reached_nodes"] > int(old_b.sum()) // 2
        before = edge_array(ft)
        # the property the case relies on: among the kept cells' entries d2 is 0 (no node), the cap, beyond the margin and
        # within it -- penalties 1, 0 and in between
        kept_old = FS.move(np.ones((NR, NC), bool), -si, -sj, False)
        vals = ft.clearance()[kept_old].astype(np.float64)
        pen = 1.0 - RES * np.sqrt(vals) / clear["margin"]
        assert (vals == 0).any() and (vals == CR.NONE).any() and ((vals != CR.NONE) & (pen < 0)).any() and ((pen > 0) & (pen < 1)).any()
        ptr = ft.dist_dev().data_ptr()
        install(ctx, new_c)
        st, sp = ft.shift_clearance(new_m, refresh), fp.shift_clearance(new_m, refresh)
        print(f"  shift {shift}: tiled {st}\n          plain {sp}")
        assert ft.dist_dev().data_ptr() == ptr
        now = moved(src, si, sj)
        want = compare(ctx, [ft, fp], new_m, n_yaw, now, reverse, kw, clear)
        same_counts(st, sp)
        for key, val in expected_counts(old_b, new_b, si, sj).items():
            assert st[key] == val, key
        slots, tiles = SC.changed(before, want["edges"].reshape(before.shape), si, sj, reverse)
        print(f"  changed_slots {st['changed_slots']} (expected {slots}), weight_tiles {st['weight_tiles']} (expected {tiles})")
        assert st["changed_slots"] == slots and st["weight_tiles"] == tiles
        assert st == ft.clearance_shift_stats() and st["dropped_blocked"] == 0
    return st


# ---- cases ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [(0, 0), (1, 0), (0, -1), (-3, 5), (16, 0), (-16, 16), (17, -15), (40, 0)])
def test_shifts_at_7_headings(ctx, shift):
    st = case(ctx, shift, 7, 1, False)
    assert st["removed_nodes"] > 0 and st["changed_slots"] > 0   # the edited block
    if shift != (0, 0):
        assert st["left_nodes"] > 0 and st["added_nodes"] > st["left_nodes"] // 2


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("objective", [0, 1])
@pytest.mark.parametrize("n_yaw", [1, 2, 16, 32])
def test_a_shift_across_headings_objectives_and_directions(ctx, n_yaw, objective, reverse):
    case(ctx, (-3, 5), n_yaw, objective, reverse)


def test_the_outside_as_an_obstacle(ctx):
    """The world does not change, but every kept node within the radius of a border has another distance to the outside:
    the twelve border tiles of the 4 x 4 hold changed weights, the four inner ones none (what entered or left lies within 5
    cells of a border, and moves clearances 5 cells further)."""
    st = case(ctx, (-3, 5), 7, 1, False, clear=dict(CLEAR, outside_is_obstacle=True), edit=False)
    assert N_TILES == 16 and 12 <= st["weight_tiles"] < N_TILES


def test_a_yaw_spread_at_16_headings(ctx):
    case(ctx, (-3, 5), 16, 1, True, clear=dict(CLEAR, yaw_spread=1))


def test_kept_heights_without_refresh(ctx):
    """Objective 0 prices heights.  The new map is raised by 0.3 m in a block of the overlap.  Without refresh_heights the
    kept cells keep the old map's heights and the cells that entered take the new map's: the result is Dijkstra's on the
    weights restated from those merged heights, at the relative 1e-9 test_cost_field_clearance.py derives.  A zero move
    with refresh_heights then gives the new field's bits."""
    n_yaw, (si, sj) = 4, (-3, 5)
    old_c, new_c = corners(si, sj)
    bits = world_bits(n_yaw)
    old_b, new_b = rect_bits(bits, old_c), rect_bits(bits, new_c)
    src = free_sources(old_b, new_b, si, sj, n_yaw)[:1]
    old_m, new_m = pack(old_b), pack(new_b)
    raised = world_elev().copy()
    raised[50:62, 52:66] += np.float32(0.3)
    kw = dict(rect=RECT, objective=0, reverse=True)
    install(ctx, old_c)
    z_old = ctx.reachability_poses(1, RECT)[..., 0, 2]
    with ctx.clearance_cost_field(old_m, n_yaw, src, **kw, **CLEAR) as ft, \
            ctx.clearance_cost_field(old_m, n_yaw, src, plain_sweeps=True, **kw, **CLEAR) as fp:
        gm = install(ctx, new_c, raised)
        z_new = ctx.reachability_poses(1, RECT)[..., 0, 2]
        entered = ~FS.move(np.ones(z_old.shape, bool), si, sj, False)
        z = np.where(entered, z_new, FS.move(z_old, si, sj, np.nan))
        assert (z != z_new).sum() >= 12 * 14 and np.isfinite(z).all()
        st, sp = ft.shift_clearance(new_m, refresh_heights=False), fp.shift_clearance(new_m, refresh_heights=False)
        same_counts(st, sp)
        d, dp = ft.dist(), fp.dist()
        assert np.array_equal(bits_of(d), bits_of(dp))
        x, y = LR.cell_centres(gm, RECT)
        now = moved(src, si, sj)
        d2 = CR.clearance_map(new_m, n_yaw, CLEAR["radius_cells"])
        assert np.array_equal(ft.clearance(), d2)
        w = CR.weights(LR.Lattice(new_m, n_yaw, x, y, z, 0).w, d2, RES, CLEAR["margin"], CLEAR["gain"])
        assert_field(d, LL.LearnedLattice(new_m, n_yaw, w).dijkstra(now, True)[0])
        with ctx.clearance_cost_field(new_m, n_yaw, now, **kw, **CLEAR) as fresh:       # a new field reads the raised block
            assert not np.array_equal(bits_of(fresh.dist()), bits_of(d))
        before = edge_array(ft)
        st = ft.shift_clearance(new_m, refresh_heights=True)      # a zero move that re-reads the heights
        fp.shift_clearance(new_m, refresh_heights=True)
        assert st["shift_rows"] == st["shift_cols"] == 0 and st["changed_words"] == 0 and st["changed_slots"] > 0
        want = compare(ctx, [ft, fp], new_m, n_yaw, now, True, kw, CLEAR)
        assert (st["changed_slots"], st["weight_tiles"]) == SC.changed(before, want["edges"].reshape(before.shape), 0, 0, True)


@pytest.mark.parametrize("objective", [0, 1])
def test_gain_zero_is_the_shifted_plain_field(ctx, objective):
    n_yaw, (si, sj) = 7, (-3, 5)
    old_c, new_c = corners(si, sj)
    bits = world_bits(n_yaw)
    old_b, new_b = rect_bits(bits, old_c), rect_bits(bits, new_c)
    src = free_sources(old_b, new_b, si, sj, n_yaw)
    for reverse in (False, True):
        kw = dict(rect=RECT, reverse=reverse, objective=objective)
        install(ctx, old_c)
        with ctx.clearance_cost_field(pack(old_b), n_yaw, src, radius_cells=5, margin=0.15, gain=0.0, **kw) as f, \
                ctx.cost_field(pack(old_b), n_yaw, src, **kw) as p:
            install(ctx, new_c)
            st, sp = f.shift_clearance(pack(new_b)), p.shift(pack(new_b))
            assert np.array_equal(bits_of(f.dist()), bits_of(p.dist())), reverse
            for key in ("changed_words", "removed_nodes", "added_nodes", "reached_nodes", "left_nodes", "kept_cells", "shift_rows",
                        "shift_cols"):
                assert st[key] == sp[key], key


def corridor_case(ctx, old, new, src, si, n_yaw, reverse):
    """A flat 40 x 40 map moved by si rows; the field covers the whole map.  Returns (dist before, dist after, stats) of the
    tiled form."""
    n = old.shape[0]
    flat = np.zeros((n, n), np.float32)
    kw = dict(objective=1, reverse=reverse)
    clear = dict(radius_cells=3, margin=0.1, gain=3.0)
    device_map(ctx, flat, RES, pos=(0.2, -0.1))
    with ctx.clearance_cost_field(old, n_yaw, [src], **kw, **clear) as ft, \
            ctx.clearance_cost_field(old, n_yaw, [src], plain_sweeps=True, **kw, **clear) as fp:
        d0, before = ft.dist(), edge_array(ft)
        device_map(ctx, flat, RES, pos=(0.2 + si * RES, -0.1))
        st, sp = ft.shift_clearance(new), fp.shift_clearance(new)
        print(f"  tiled {st}\n  plain {sp}")
        now = moved([src], si, 0)
        want = compare(ctx, [ft, fp], new, n_yaw, now, reverse, kw, clear, rect=None)
        same_counts(st, sp)
        assert (st["changed_slots"], st["weight_tiles"]) == SC.changed(before, want["edges"].reshape(before.shape), si, 0, reverse)
    return d0, want["dist"], st


def test_a_far_arm_whose_bend_left_dies(ctx):
    """No word of the overlap differs and nothing enters: the slots of the last kept row that led into the bend go from
    finite to +inf, on top of the flagged border row."""
    n, n_yaw, si = 40, 8, 4
    old, new, src, far = FS.u_corridor(n, n, n_yaw, 3, si)
    before, d, st = corridor_case(ctx, old, new, src, si, n_yaw, False)
    assert np.isfinite(before[FS.move(far, -si, 0, False)]).all() and np.isinf(d[far]).all()
    assert st["changed_words"] == st["removed_nodes"] == st["added_nodes"] == 0
    assert st["dead_nodes"] >= int(far.sum()) * n_yaw > 0
    assert st["left_nodes"] == int((old[n - si:] != 0).sum()) * n_yaw


def test_an_entering_strip_joins_an_island(ctx):
    n, n_yaw, si = 40, 8, 2
    old, new, src, isl = FS.island(n, n, n_yaw, si)
    before, d, st = corridor_case(ctx, old, new, src, si, n_yaw, True)
    assert np.isinf(before[FS.move(isl, -si, 0, False)]).all() and np.isfinite(d[isl]).all()
    assert st["added_nodes"] == si * n * n_yaw and st["removed_nodes"] == 0
    assert st["reached_nodes"] == int((new != 0).sum()) * n_yaw


@pytest.mark.parametrize("reverse", [False, True])
def test_blocked_moves_move_with_their_nodes(ctx, reverse):
    n_yaw, (si, sj) = 7, (6, -4)
    old_c, new_c = corners(si, sj)
    bits = world_bits(n_yaw, seed=1)
    old_b, new_b = rect_bits(bits, old_c), rect_bits(bits, new_c)
    src = free_sources(old_b, new_b, si, sj, n_yaw)[:1]
    kw = dict(rect=RECT, objective=1, reverse=reverse)
    fields = []
    try:
        install(ctx, old_c)
        for form in ({}, dict(plain_sweeps=True)):
            fields.append(ctx.clearance_cost_field(pack(old_b), n_yaw, src, **kw, **form, **CLEAR))
        f = fields[0]
        d0 = f.dist()
        a, b = [], []
        fin = np.argwhere(np.isfinite(d0) & (d0 > 0))
        for t in fin[np.random.default_rng(2).integers(0, len(fin), 12)]:     # on paths: anywhere, most in the overlap
            nodes = f.path(tuple(t))[0]
            for i in range(0, len(nodes) - 1, 4):
                a.append(tuple(nodes[i])), b.append(tuple(nodes[i + 1]))
        full = old_b.all(axis=2)
        for c in range(8, 40):
            # between nodes that leave (rows >= NR - si), and across the line: the last kept row and the first that leaves
            for r0, r1 in ((NR - 2, NR - 3), (NR - si - 1, NR - si)):
                if full[r0, c] and full[r1, c]:
                    for k in (0, 3):
                        a += [(r0, c, k), (r1, c, k)]
                        b += [(r1, c, k), (r0, c, k)]
        for fld in fields:
            fld.block_moves(a, b)
        words, count = f.blocked(), f.blocked_count()
        assert np.array_equal(fields[1].blocked(), words)
        want = moved_blocked(words, si, sj)
        left = ~FS.move(np.ones((NR, NC), bool), -si, -sj, False)            # old cells that leave
        gone = int(np.unpackbits(np.ascontiguousarray(words[left]).view(np.uint8)).sum())
        kept = int(np.unpackbits(np.ascontiguousarray(want).view(np.uint8)).sum())
        assert gone > 0 and kept > 0 and count - gone - kept > 0              # all three kinds are there
        install(ctx, new_c)
        for fld in fields:
            st = fld.shift_clearance(pack(new_b))
            assert st["dropped_blocked"] == count - kept and fld.blocked_count() == kept
        compare(ctx, fields, pack(new_b), n_yaw, moved(src, si, sj), reverse, kw, CLEAR, words=want)
    finally:
        for fld in fields:
            fld.close()


def test_a_shift_an_update_and_a_shift_back(ctx):
    n_yaw, (si, sj) = 4, (-3, 5)
    old_c, new_c = corners(si, sj)
    bits = world_bits(n_yaw, seed=2)
    old_b, new_b = rect_bits(bits, old_c), rect_bits(bits, new_c)
    src = free_sources(old_b, new_b, si, sj, n_yaw)[:1]
    now = moved(src, si, sj)
    kw = dict(rect=RECT, objective=0, reverse=True)
    install(ctx, old_c)
    with ctx.clearance_cost_field(pack(old_b), n_yaw, src, **kw, **CLEAR) as ft, \
            ctx.clearance_cost_field(pack(old_b), n_yaw, src, plain_sweeps=True, **kw, **CLEAR) as fp:
        ptr = ft.dist_dev().data_ptr()
        install(ctx, new_c)
        same_counts(ft.shift_clearance(pack(new_b)), fp.shift_clearance(pack(new_b)))
        compare(ctx, [ft, fp], pack(new_b), n_yaw, now, True, kw, CLEAR, seed=1)
        sub = (14, 14, 4, 4)                                       # over the common corner (16, 16) of four tiles
        edit_b = new_b.copy()
        edit_b[14:18, 14:18] &= np.random.default_rng(3).random((4, 4, n_yaw)) < 0.4
        edit_b[now[0][0], now[0][1], now[0][2]] = True
        for f in (ft, fp):
            assert f.update_clearance(pack(edit_b), sub)["removed_nodes"] > 0
        compare(ctx, [ft, fp], pack(edit_b), n_yaw, now, True, kw, CLEAR, seed=2)
        # back: the old window, with the edit where it lies there
        install(ctx, old_c)
        back_b = old_b.copy()
        back_b[14 + 3:18 + 3, 14 - 5:18 - 5] = edit_b[14:18, 14:18]
        before = edge_array(ft)
        st, sp = ft.shift_clearance(pack(back_b)), fp.shift_clearance(pack(back_b))
        same_counts(st, sp)
        assert (st["shift_rows"], st["shift_cols"]) == (3, -5)
        want = compare(ctx, [ft, fp], pack(back_b), n_yaw, src, True, kw, CLEAR, seed=3)
        assert (st["changed_slots"], st["weight_tiles"]) == SC.changed(before, want["edges"].reshape(before.shape), 3, -5, True)
        for key, val in expected_counts(edit_b, back_b, 3, -5).items():
            assert st[key] == val, key
        assert ft.dist_dev().data_ptr() == ptr


def test_a_zero_shift_is_an_update(ctx):
    n_yaw = 7
    corner, _ = corners(0, 0)
    bits = world_bits(n_yaw)
    edited = bits.copy()
    edited[50:62, 52:66] &= np.random.default_rng(8).random((12, 14, n_yaw)) < 0.8
    old_b, new_b = rect_bits(bits, corner), rect_bits(edited, corner)
    src = free_sources(old_b, new_b, 0, 0, n_yaw)
    old_m, new_m = pack(old_b), pack(new_b)
    install(ctx, corner)
    for objective, refresh, form in ((0, True, {}), (1, False, {}), (0, False, dict(plain_sweeps=True))):
        kw = dict(rect=RECT, objective=objective, **form)
        with ctx.clearance_cost_field(old_m, n_yaw, src, **kw, **CLEAR) as f, \
                ctx.clearance_cost_field(old_m, n_yaw, src, **kw, **CLEAR) as twin:
            zeros = f.clearance_update_stats()
            st, su = f.shift_clearance(new_m, refresh), twin.update_clearance(new_m, None, refresh)
            tg = targets_of(twin.dist(), src, 0)
            same(ctx, f, snapshot(f, tg), snapshot(twin, tg), new_m, n_yaw, RECT, src, False, tg, objective)
            # every count that does not depend on the order in which tiles saw each other's halo
            for key in ("changed_words", "removed_nodes", "added_nodes", "dead_nodes", "hop_dead_nodes", "reached_nodes",
                        "changed_slots", "weight_tiles"):
                assert st[key] == su[key], key
            assert (st["tile_launches"] == 0) == (su["tile_launches"] == 0)
            assert st["removed_nodes"] > 0 and st["changed_slots"] > 0
            assert (st["shift_rows"], st["shift_cols"], st["left_nodes"], st["kept_cells"]) == (0, 0, 0, NR * NC)
            assert f.clearance_update_stats() == zeros               # the update's own record stays its own
            st = f.shift_clearance(new_m, refresh)                   # nothing changes any more
            assert st["changed_words"] == 0 and st["tile_launches"] == 0 and st["changed_slots"] == 0
            compare(ctx, [f], new_m, n_yaw, src, False, kw, CLEAR)


def test_real_masks_and_plan(ctx):
    """Windows of 96 x 96 cells of a 120 x 120 Perlin world through the device's preprocessing, each with its own
    reachability mask.  After the call plan() returns what a new field's plan() returns: checked paths, since the field
    adopted the map version."""
    n, win, n_yaw, (si, sj) = 120, 96, 8, (6, -9)
    elev = perlin_terrain(n, RES, seed=1234, amplitude=0.25)
    clear = dict(radius_cells=4, margin=0.12, gain=2.0)

    def window(top, left):
        raw = GridMap(win, win, RES, 2.0 - top * RES, 1.0 - left * RES)
        raw.add("elevation", np.ascontiguousarray(elev[top:top + win, left:left + win], np.float32))
        raw.add("traversability", np.ones((win, win), np.float32))
        map_from_device(ctx, raw, ROBOT)
        return ctx.reachability_map(n_yaw)

    top, left = 14, 8
    old_m = window(top, left)
    new_m = window(top - si, left - sj)
    both = ((FS.move(old_m, si, sj, 0) & new_m)[..., None] >> np.arange(n_yaw, dtype=np.uint32)) & 1   # nodes of both masks
    cand = np.argwhere(both)
    assert len(cand) > 100
    best = (0, None)                                                            # the candidate that reaches the most nodes
    for r, c, k in cand[::max(1, len(cand) // 8)]:
        with ctx.cost_field(new_m, n_yaw, [(int(r), int(c), int(k))], objective=1, reverse=True) as probe:
            best = max(best, (probe.stats()["reached_nodes"], (int(r), int(c), int(k))))
    src_new = [best[1]]
    src_old = moved(src_new, -si, -sj)
    kw = dict(objective=1, reverse=True)
    window(top, left)
    with ctx.clearance_cost_field(old_m, n_yaw, src_old, **kw, **clear) as f:
        window(top - si, left - sj)
        st = f.shift_clearance(new_m)
        print(f"  {st}")
        with ctx.clearance_cost_field(new_m, n_yaw, src_new, **kw, **clear) as fresh:
            d = fresh.dist()
            assert np.array_equal(bits_of(f.dist()), bits_of(d)) and np.array_equal(f.clearance(), fresh.clearance())
            fin = np.argwhere(np.isfinite(d))
            assert len(fin) > 100
            targets = [tuple(int(v) for v in t) for t in fin[np.random.default_rng(5).integers(0, len(fin), 12)]]
            got, want = f.plan(targets), fresh.plan(targets)
            assert [g[0] for g in got] == [w[0] for w in want] and any(g[0] == 0 for g in got)
            for g, w in zip(got, want):
                assert np.float64(g[3]).view(np.uint64) == np.float64(w[3]).view(np.uint64)
                if g[0] == 0:
                    assert np.array_equal(g[1], w[1]) and np.array_equal(bits_of(g[2]), bits_of(w[2]))
            assert np.array_equal(f.blocked(), fresh.blocked())
            assert np.array_equal(bits_of(f.dist()), bits_of(fresh.dist()))


def test_refusals_leave_the_field_untouched(ctx):
    n_yaw, (si, sj) = 4, (3, -2)
    old_c, new_c = corners(si, sj)
    bits = world_bits(n_yaw, seed=3)
    stay = free_sources(rect_bits(bits, old_c), rect_bits(bits, new_c), si, sj, n_yaw)[0]
    src = [(NR - 2, 20, 1), stay]                                                # the first one leaves with si = 3
    bits[old_c[0] + RECT[0] + NR - 2, old_c[1] + RECT[1] + 20, 1] = True
    old_m, new_m = pack(rect_bits(bits, old_c)), pack(rect_bits(bits, new_c))
    kw = dict(rect=RECT, objective=1)
    ab = moves_of((NR, NC, n_yaw))

    def state(f):
        """snapshot without paths (their poses need the field's own map, which is gone by then), blocked() and all stats"""
        arrays = [bits_of(f.dist()).copy(), bits_of(f.edge_costs(*ab)).copy(), f.blocked().copy()]
        if f is not plain:
            arrays.append(snapshot(f, [])["d2"])
        return arrays, (f.stats(), f.shift_stats(), f.clearance_shift_stats(), f.clearance_update_stats(), f.blocked_count())

    def refused(f, mask, word, call="shift_clearance"):
        before = state(f)
        with pytest.raises(_capi.ArtpError) as e:
            getattr(f, call)(mask)
        assert e.value.status == -1 and word in str(e.value), e.value
        after = state(f)
        assert all(np.array_equal(x, y) for x, y in zip(before[0], after[0])) and before[1] == after[1]

    for form in ({}, dict(plain_sweeps=True)):
        install(ctx, old_c)
        with ctx.clearance_cost_field(old_m, n_yaw, src, **kw, **form, **CLEAR) as f, \
                ctx.clearance_cost_field(old_m, n_yaw, src[1:], **kw, **form, **CLEAR) as g, \
                ctx.cost_field(old_m, n_yaw, src[1:], **kw, **form) as plain:
            for fld in (f, g):
                fld.block_moves([stay], [(stay[0] + 1, stay[1], stay[2])])
            install(ctx, new_c)
            refused(f, new_m, "leaves")                                          # a source that leaves
            gone = rect_bits(bits, new_c).copy()
            gone[stay[0] + si, stay[1] + sj, stay[2]] = False
            refused(g, pack(gone), "not a node")                                 # a source that is no node of the new mask
            refused(g, new_m, "clearance", call="shift")                         # shift still refuses the field
            refused(plain, new_m, "artp_field_compute_clearance")                # a plain field
            device_map(ctx, np.zeros((MAP[0] + 1, MAP[1]), np.float32), RES, pos=(1.0 - new_c[0] * RES, -0.5 - new_c[1] * RES))
            refused(g, new_m, "differs")                                         # a map of another size
            install(ctx, new_c)
            st = g.shift_clearance(new_m)                                        # and a valid call afterwards
            assert (st["shift_rows"], st["shift_cols"]) == (si, sj) and g.blocked_count() == 1
            words = np.zeros((NR, NC, n_yaw), np.uint16)
            words[stay[0] + 1 + si, stay[1] + sj, stay[2]] = 1 << 1              # a forward field: the target owns the move,
            compare(ctx, [g], new_m, n_yaw, moved(src[1:], si, sj), False, kw, CLEAR, words=words)   # its neighbour by offset 1

    # a learned field
    import os
    import sys
    import common
    sys.path.insert(0, os.path.join(common.ROOT, "oracle"))
    sys.path.insert(0, os.path.join(common.ROOT, "tools"))
    import convert_weights as cw
    import cost_exact_ref as R
    import motion_cost_oracle as mo

    def cost_map(corner):
        top, left = corner
        win = world_elev()[top:top + MAP[0], left:left + MAP[1]]
        ctx.cost_update_map(np.ascontiguousarray(win[::-1, ::-1]), RES, MAP[0] * RES, MAP[1] * RES, 1.0 - top * RES, -0.5 - left * RES)

    install(ctx, old_c)
    ctx.cost_load_weights(cw.to_blob(mo.random_params(0, R.shapes_of(1))))
    cost_map(old_c)
    with ctx.learned_cost_field(old_m, n_yaw, src[1:], rect=RECT, risk_threshold=1.0) as lf:
        before = (bits_of(lf.dist()).copy(), bits_of(lf.edge_costs(*ab)).copy(), lf.stats(), lf.clearance_shift_stats())
        install(ctx, new_c)
        cost_map(new_c)
        with pytest.raises(_capi.ArtpError) as e:
            lf.shift_clearance(new_m)
        assert e.value.status == -1 and "artp_field_compute_clearance" in str(e.value)
        after = (bits_of(lf.dist()), bits_of(lf.edge_costs(*ab)), lf.stats(), lf.clearance_shift_stats())
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]) and before[2:] == after[2:]
