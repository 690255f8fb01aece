"""artp_field_shift (csrc/field.h): a cost-to-go field carried across a move of the map by whole
cells must hold the bits of a field computed anew on the new map -- artp_field_compute, which the shift does not touch, is
the exact oracle.  test_cost_field_update.check compares distances (bit patterns), reached_nodes, some twenty paths with
their poses, and the fold of the device's own edge costs along each path.  Every case runs in the tiled and in the plain
form; the two must agree bit for bit and on all counts.

The world: Perlin heights of 112 x 112 cells at 0.04 m and a random per-heading mask of density 0.7 over it.  The map is a
72 x 64 window of the world; its position follows the window, so a window further up the rows is a map moved by whole
cells.  The field's rectangle (5, 3, 61, 53) is odd-sized, not at the origin and no multiple of the 16-cell tile.  Old node
(r, c, k) is new node (r + si, c + sj, k): the new window's corner is the old one's minus the shift."""
import numpy as np
import pytest

import field_shift_ref as FS
import lattice_ref as LR
from art_planner_amd import _capi
from synthetic import GridMap, map_from_device, perlin_terrain
from test_cost_field import ROBOT, assert_field, device_map
from test_cost_field_update import bits_of, check, pack

WORLD, RES = 112, 0.04
MAP = (72, 64)
RECT = (5, 3, 61, 53)
STAT_KEYS = ("changed_words", "removed_nodes", "added_nodes", "dead_nodes", "hop_dead_nodes", "reached_nodes", "shift_rows",
             "shift_cols", "kept_cells", "left_nodes", "dropped_blocked")


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
_elev = {}


def world_elev():
    if "z" not in _elev:
        _elev["z"] = perlin_terrain(WORLD, RES, seed=31) * np.float32(0.6)
    return _elev["z"]


def world_bits(n_yaw, seed=0):
    return np.random.default_rng(500 + 10 * n_yaw + seed).random((WORLD, WORLD, n_yaw)) < 0.7


def corners(si, sj):
    """(top, left) of the old and of the new window: both inside the world for every shift of this file."""
    top, left = (WORLD - MAP[0] + si) // 2, (WORLD - MAP[1] + sj) // 2
    assert 0 <= top <= WORLD - MAP[0] and 0 <= top - si <= WORLD - MAP[0]
    assert 0 <= left <= WORLD - MAP[1] and 0 <= left - sj <= WORLD - MAP[1]
    return (top, left), (top - si, left - sj)


def install(ctx, corner, elev=None):
    """The window at `corner` as the context's map; a window further up the rows lies further along +x."""
    top, left = corner
    z = world_elev() if elev is None else elev
    win = np.ascontiguousarray(z[top:top + MAP[0], left:left + MAP[1]], np.float32)
    return device_map(ctx, win, RES, pos=(1.0 - top * RES, -0.5 - left * RES))


def rect_bits(bits, corner):
    top, left = corner
    return bits[top + RECT[0]:top + RECT[0] + RECT[2], left + RECT[1]:left + RECT[1] + RECT[3]]


def overlap_sources(si, sj, n_yaw):
    """Two nodes of the old rectangle that stay inside it: around the middle of the overlap."""
    r = (max(0, -si) + min(RECT[2], RECT[2] - si)) // 2
    c = (max(0, -sj) + min(RECT[3], RECT[3] - sj)) // 2
    return [(r, c, 0), (min(r + 3, RECT[2] - 1 - max(si, 0)), max(c - 2, max(0, -sj)), n_yaw - 1)]


def moved(nodes, si, sj):
    return [(r + si, c + sj, k) for r, c, k in nodes]


def expected_counts(old_bits, new_bits, si, sj):
    was = FS.move(old_bits, si, sj, False)
    return dict(changed_words=int((was != new_bits).any(axis=2).sum()), removed_nodes=int((was & ~new_bits).sum()),
                added_nodes=int((new_bits & ~was).sum()), left_nodes=int(old_bits.sum()) - int(was.sum()),
                kept_cells=(RECT[2] - abs(si)) * (RECT[3] - abs(sj)), shift_rows=si, shift_cols=sj)


def same_counts(st, sp):
    for key in STAT_KEYS:
        assert st[key] == sp[key], key
    assert sp["tile_launches"] == 0


def case(ctx, shift, n_yaw, objective, reverse, refresh=True):
    """Both forms computed on the old window, shifted onto the new one whose mask also differs in a block of the overlap;
    returns the tiled form's stats."""
    si, sj = shift
    old_c, new_c = corners(si, sj)
    bits = world_bits(n_yaw)
    src = overlap_sources(si, sj, n_yaw)
    for r, c, k in src:
        bits[old_c[0] + RECT[0] + r, old_c[1] + RECT[1] + c, k] = True
    edited = bits.copy()
    block = edited[50:62, 52:66]                                # world cells inside every window of this file
    block ^= np.random.default_rng(7).random(block.shape) < 0.15
    for r, c, k in src:
        edited[old_c[0] + RECT[0] + r, old_c[1] + RECT[1] + c, k] = True
    old_b, new_b = rect_bits(bits, old_c), rect_bits(edited, new_c)
    kw = dict(rect=RECT, objective=objective, reverse=reverse)
    install(ctx, old_c)
    with ctx.cost_field(pack(old_b), n_yaw, src, **kw) as ft, \
            ctx.cost_field(pack(old_b), n_yaw, src, plain_sweeps=True, **kw) as fp:
        install(ctx, new_c)
        st, sp = ft.shift(pack(new_b), refresh), fp.shift(pack(new_b), refresh)
        print(f"  shift {shift}: tiled {st}\n          plain {sp}")
        now = moved(src, si, sj)
        d = check(ctx, ft, pack(new_b), n_yaw, now, **kw)
        dp = check(ctx, fp, pack(new_b), n_yaw, now, **kw)
        assert np.array_equal(bits_of(d), bits_of(dp))
        same_counts(st, sp)
        for key, want in expected_counts(old_b, new_b, si, sj).items():
            assert st[key] == want, key
        assert st == ft.shift_stats() and st["dropped_blocked"] == 0
    return st


# ---- cases ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shift", [(0, 0), (1, 0), (0, -1), (-3, 5), (16, 0), (-16, 16), (17, -15), (40, 0)])
def test_shifts_at_7_headings(ctx, shift):
    st = case(ctx, shift, 7, 1, False)
    assert st["removed_nodes"] > 0                              # the edited block
    if shift != (0, 0):
        assert st["left_nodes"] > 0 and st["added_nodes"] > st["left_nodes"] // 2


@pytest.mark.gpu
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("objective", [0, 1])
@pytest.mark.parametrize("n_yaw", [1, 16])
@pytest.mark.parametrize("shift", [(-3, 5), (17, -15)])
def test_shifts_across_headings_objectives_and_directions(ctx, shift, n_yaw, objective, reverse):
    case(ctx, shift, n_yaw, objective, reverse, refresh=True)


@pytest.mark.gpu
def test_a_shift_at_32_headings(ctx):
    case(ctx, (-16, 16), 32, 1, True)


@pytest.mark.gpu
def test_a_zero_shift_is_an_update(ctx):
    n_yaw = 7
    corner, _ = corners(0, 0)
    bits = world_bits(n_yaw)
    src = overlap_sources(0, 0, n_yaw)
    for r, c, k in src:
        bits[corner[0] + RECT[0] + r, corner[1] + RECT[1] + c, k] = True
    edited = bits.copy()
    edited[50:62, 52:66] &= np.random.default_rng(8).random((12, 14, n_yaw)) < 0.8
    for r, c, k in src:
        edited[corner[0] + RECT[0] + r, corner[1] + RECT[1] + c, k] = True
    old_m, new_m = pack(rect_bits(bits, corner)), pack(rect_bits(edited, corner))
    install(ctx, corner)
    for objective, refresh, form in ((0, True, {}), (1, False, {}), (0, False, dict(plain_sweeps=True))):
        kw = dict(rect=RECT, objective=objective, **form)
        with ctx.cost_field(old_m, n_yaw, src, **kw) as f, ctx.cost_field(old_m, n_yaw, src, **kw) as twin:
            st, su = f.shift(new_m, refresh), twin.update(new_m, None, refresh)
            assert np.array_equal(bits_of(f.dist()), bits_of(twin.dist()))
            # every count that does not depend on the order in which tiles saw each other's halo
            for key in ("changed_words", "removed_nodes", "added_nodes", "dead_nodes", "hop_dead_nodes", "reached_nodes"):
                assert st[key] == su[key], key
            assert (st["tile_launches"] == 0) == (su["tile_launches"] == 0)
            assert st["removed_nodes"] > 0 and st["dead_nodes"] > 0
            assert (st["shift_rows"], st["shift_cols"], st["left_nodes"], st["kept_cells"]) == (0, 0, 0, RECT[2] * RECT[3])
            assert f.stats()["reached_nodes"] == twin.stats()["reached_nodes"]
            st = f.shift(new_m, refresh)                         # nothing changes any more
            assert st["changed_words"] == 0 and st["tile_launches"] == 0 and st["dead_nodes"] == 0
            check(ctx, f, new_m, n_yaw, src, **kw)


@pytest.mark.gpu
def test_kept_heights_without_refresh(ctx):
    """Objective 0 prices heights.  Without refresh_heights the kept cells keep the old map's, the cells that entered take the
    new map's: the result is lattice_ref's on those merged heights and nominal coordinates, at the relative 1e-9 that
    test_cost_field.py derives.  The new map is raised by 0.3 m in a block of the overlap, so the merged heights are neither
    map's."""
    n_yaw, (si, sj) = 4, (-3, 5)
    old_c, new_c = corners(si, sj)
    bits = world_bits(n_yaw)
    src = overlap_sources(si, sj, n_yaw)[:1]
    bits[old_c[0] + RECT[0] + src[0][0], old_c[1] + RECT[1] + src[0][1], 0] = True
    old_m, new_m = pack(rect_bits(bits, old_c)), pack(rect_bits(bits, new_c))
    raised = world_elev().copy()
    raised[50:62, 52:66] += np.float32(0.3)
    kw = dict(rect=RECT, objective=0, reverse=True)
    install(ctx, old_c)
    z_old = ctx.reachability_poses(1, RECT)[..., 0, 2]
    with ctx.cost_field(old_m, n_yaw, src, **kw) as ft, ctx.cost_field(old_m, n_yaw, src, plain_sweeps=True, **kw) as fp:
        gm = install(ctx, new_c, raised)
        z_new = ctx.reachability_poses(1, RECT)[..., 0, 2]
        entered = ~FS.move(np.ones(z_old.shape, bool), si, sj, False)
        z = np.where(entered, z_new, FS.move(z_old, si, sj, np.nan))
        assert (z != z_new).sum() >= 12 * 14 and np.isfinite(z).all()
        st, sp = ft.shift(new_m, refresh_heights=False), fp.shift(new_m, refresh_heights=False)
        same_counts(st, sp)
        d, dp = ft.dist(), fp.dist()
        assert np.array_equal(bits_of(d), bits_of(dp))
        x, y = LR.cell_centres(gm, RECT)
        now = moved(src, si, sj)
        ref = LR.Lattice(new_m, n_yaw, x, y, z, 0).dijkstra(now, True)[0]
        assert_field(d, ref)
        with ctx.cost_field(new_m, n_yaw, now, **kw) as fresh:    # a new field reads the raised block
            assert not np.array_equal(bits_of(fresh.dist()), bits_of(d))
            st = ft.shift(new_m, refresh_heights=True)              # a zero shift that re-reads the heights
            assert st["shift_rows"] == st["shift_cols"] == 0 and st["dead_nodes"] > 0
            assert np.array_equal(bits_of(ft.dist()), bits_of(fresh.dist()))


def corridor_case(ctx, old, new, src, si, n_yaw, reverse):
    """A flat 40 x 40 map moved by si rows; the field covers the whole map.  Returns (dist before, dist after, stats) of the
    tiled form."""
    n = old.shape[0]
    flat = np.zeros((n, n), np.float32)
    kw = dict(objective=1, reverse=reverse)
    device_map(ctx, flat, RES, pos=(0.2, -0.1))
    with ctx.cost_field(old, n_yaw, [src], **kw) as ft, ctx.cost_field(old, n_yaw, [src], plain_sweeps=True, **kw) as fp:
        before = ft.dist()
        device_map(ctx, flat, RES, pos=(0.2 + si * RES, -0.1))
        st, sp = ft.shift(new), fp.shift(new)
        print(f"  tiled {st}\n  plain {sp}")
        now = moved([src], si, 0)
        d = check(ctx, ft, new, n_yaw, now, **kw)
        dp = check(ctx, fp, new, n_yaw, now, **kw)
        assert np.array_equal(bits_of(d), bits_of(dp))
        same_counts(st, sp)
    return before, d, st


@pytest.mark.gpu
def test_a_far_arm_whose_bend_left_dies(ctx):
    """No word of the overlap differs and nothing enters: only the flagged border row makes the tiled form look at the
    nodes whose support left."""
    n, n_yaw, si = 40, 8, 4
    old, new, src, far = FS.u_corridor(n, n, n_yaw, 3, si)
    before, d, st = corridor_case(ctx, old, new, src, si, n_yaw, False)
    assert np.isfinite(before[FS.move(far, -si, 0, False)]).all() and np.isinf(d[far]).all()
    assert st["changed_words"] == st["removed_nodes"] == st["added_nodes"] == 0
    assert st["dead_nodes"] >= int(far.sum()) * n_yaw > 0
    assert st["left_nodes"] == int((old[n - si:] != 0).sum()) * n_yaw


@pytest.mark.gpu
def test_an_entering_strip_joins_an_island(ctx):
    n, n_yaw, si = 40, 8, 2
    old, new, src, isl = FS.island(n, n, n_yaw, si)
    before, d, st = corridor_case(ctx, old, new, src, si, n_yaw, True)
    assert np.isinf(before[FS.move(isl, -si, 0, False)]).all() and np.isfinite(d[isl]).all()
    # (nodes of the last kept row may die: at 8 headings a cheapest path dips into the rows below, which left)
    assert st["added_nodes"] == si * n * n_yaw and st["removed_nodes"] == 0
    assert st["reached_nodes"] == int((new != 0).sum()) * n_yaw


def blocked_moves(words, n_yaw, reverse):
    """The moves (a, b) in travel direction that a field's blocked words hold."""
    a, b = [], []
    for r, c, k in np.argwhere(words != 0):
        for j in range(10):
            if (int(words[r, c, k]) >> j) & 1:
                nb = (r + LR.MOVES[j][0], c + LR.MOVES[j][1], k) if j < 8 else (r, c, (k + (1 if j == 8 else -1)) % n_yaw)
                a.append((r, c, k) if reverse else nb)
                b.append(nb if reverse else (r, c, k))
    return a, b


def moved_blocked(words, si, sj):
    """The blocked words after the move: with their nodes, and a slot cleared whose neighbour lies outside."""
    out = FS.move(words, si, sj, 0)
    nr, nc = out.shape[:2]
    r, c = np.meshgrid(np.arange(nr), np.arange(nc), indexing="ij")
    for j, (dr, dc) in enumerate(LR.MOVES):
        outside = (r + dr < 0) | (r + dr >= nr) | (c + dc < 0) | (c + dc >= nc)
        out[outside] &= np.uint16(~(1 << j) & 0xffff)
    return out


def check_blocked(ctx, f, mask, n_yaw, sources, words, **kw):
    """f against a new field on `mask` with the moves of `words` blocked; returns dist."""
    with ctx.cost_field(mask, n_yaw, sources, **kw) as fresh:
        a, b = blocked_moves(words, n_yaw, bool(kw.get("reverse", False)))
        if a:
            assert fresh.block_moves(a, b) == len(a)
        assert np.array_equal(fresh.blocked(), words) and np.array_equal(f.blocked(), words)
        assert f.blocked_count() == fresh.blocked_count() == len(a)
        d, want = f.dist(), fresh.dist()
        assert np.array_equal(bits_of(d), bits_of(want)), int((bits_of(d) != bits_of(want)).sum())
        assert f.stats()["reached_nodes"] == fresh.stats()["reached_nodes"]
        fin = np.argwhere(np.isfinite(want))
        for t in fin[np.random.default_rng(1).integers(0, len(fin), 8)]:
            p, q = f.path(tuple(t)), fresh.path(tuple(t))
            assert np.array_equal(p[0], q[0]) and np.array_equal(bits_of(p[1]), bits_of(q[1]))
    return d


@pytest.mark.gpu
@pytest.mark.parametrize("reverse", [False, True])
def test_blocked_moves_move_with_their_nodes(ctx, reverse):
    n_yaw, (si, sj) = 7, (6, -4)
    old_c, new_c = corners(si, sj)
    bits = world_bits(n_yaw, seed=1)
    src = overlap_sources(si, sj, n_yaw)[:1]
    bits[old_c[0] + RECT[0] + src[0][0], old_c[1] + RECT[1] + src[0][1], 0] = True
    old_b, new_b = rect_bits(bits, old_c), rect_bits(bits, new_c)
    nr, nc = RECT[2], RECT[3]
    kw = dict(rect=RECT, objective=1, reverse=reverse)
    install(ctx, old_c)
    for form in ({}, dict(plain_sweeps=True)):
        install(ctx, old_c)
        with ctx.cost_field(pack(old_b), n_yaw, src, **kw, **form) as f:
            d0 = f.dist()
            a, b = [], []
            fin = np.argwhere(np.isfinite(d0) & (d0 > 0))
            for t in fin[np.random.default_rng(2).integers(0, len(fin), 12)]:     # on paths: anywhere, most in the overlap
                nodes = f.path(tuple(t))[0]
                for i in range(0, len(nodes) - 1, 4):
                    a.append(tuple(nodes[i])), b.append(tuple(nodes[i + 1]))
            for c in range(10, 30, 3):
                for k in (0, 3):
                    a += [(nr - 2, c, k), (nr - 2, c + 1, k)]                     # between nodes that leave (rows >= nr - si)
                    b += [(nr - 2, c + 1, k), (nr - 2, c, k)]
                    a += [(nr - si - 1, c, k), (nr - si, c, k)]                   # across the line: the last kept row and the
                    b += [(nr - si, c, k), (nr - si - 1, c, k)]                   # first that leaves, both directions
                    a += [(5, -sj, k), (5, -sj - 1, k)]                           # and across the first kept column
                    b += [(5, -sj - 1, k), (5, -sj, k)]
            f.block_moves(a, b)
            words, count = f.blocked(), f.blocked_count()
            want = moved_blocked(words, si, sj)
            left = ~FS.move(np.ones((nr, nc), bool), -si, -sj, False)            # old cells that leave
            gone = int(np.unpackbits(np.ascontiguousarray(words[left]).view(np.uint8)).sum())
            kept = int(np.unpackbits(np.ascontiguousarray(want).view(np.uint8)).sum())
            assert gone > 0 and kept > 0 and count - gone - kept > 0              # all three kinds are there
            install(ctx, new_c)
            st = f.shift(pack(new_b))
            assert st["dropped_blocked"] == count - kept and f.blocked_count() == kept
            check_blocked(ctx, f, pack(new_b), n_yaw, moved(src, si, sj), want, **kw)


@pytest.mark.gpu
def test_a_walk_of_six_shifts(ctx):
    """Six shifts in a row on one field per form, the world's mask edited before each; an update() and a block_moves() in
    between.  dist_dev() stays the same buffer throughout."""
    n_yaw = 4
    bits = world_bits(n_yaw, seed=2)
    corner = (22, 20)
    src = [(30, 24, 1)]
    kw = dict(rect=RECT, objective=0, reverse=True)
    rng = np.random.default_rng(9)
    at = lambda: (corner[0] + RECT[0] + src[0][0], corner[1] + RECT[1] + src[0][1], src[0][2])
    bits[at()] = True
    install(ctx, corner)
    m0 = pack(rect_bits(bits, corner))
    with ctx.cost_field(m0, n_yaw, src, **kw) as ft, ctx.cost_field(m0, n_yaw, src, plain_sweeps=True, **kw) as fp:
        ptr = ft.dist_dev().data_ptr()
        words = np.zeros((RECT[2], RECT[3], n_yaw), np.uint16)
        for step, (si, sj) in enumerate([(3, -2), (-5, 4), (0, 7), (8, 0), (-2, -2), (1, 1)]):
            r0, c0 = rng.integers(30, 70, 2)
            bits[r0:r0 + 9, c0:c0 + 9] ^= rng.random((9, 9, n_yaw)) < 0.2      # the world changes somewhere
            corner = (corner[0] - si, corner[1] - sj)
            src = moved(src, si, sj)
            bits[at()] = True
            install(ctx, corner)
            m = pack(rect_bits(bits, corner))
            st, sp = ft.shift(m), fp.shift(m)
            same_counts(st, sp)
            words = moved_blocked(words, si, sj)
            d = check_blocked(ctx, ft, m, n_yaw, src, words, **kw)
            dp = check_blocked(ctx, fp, m, n_yaw, src, words, **kw)
            assert np.array_equal(bits_of(d), bits_of(dp))
            assert ft.dist_dev().data_ptr() == ptr
            if step == 1:                                                       # a move next to the source, both directions
                a = [src[0], (src[0][0] + 1, src[0][1], src[0][2])]
                for f in (ft, fp):
                    f.block_moves(a, a[::-1])
                words = ft.blocked()
                assert int((words != 0).sum()) == 2
                check_blocked(ctx, ft, m, n_yaw, src, words, **kw)
            if step == 3:                                                       # the mask edited under a map that stays
                bits[corner[0] + RECT[0] + 10:corner[0] + RECT[0] + 25, corner[1] + RECT[1] + 8:corner[1] + RECT[1] + 20] &= \
                    rng.random((15, 12, n_yaw)) < 0.7
                bits[at()] = True
                m = pack(rect_bits(bits, corner))
                for f in (ft, fp):
                    assert f.update(m, (10, 8, 15, 12))["removed_nodes"] > 0
                check_blocked(ctx, ft, m, n_yaw, src, words, **kw)
                check_blocked(ctx, fp, m, n_yaw, src, words, **kw)
        assert ft.blocked_count() == 2 and ft.dist_dev().data_ptr() == ptr


@pytest.mark.gpu
def test_real_masks_plan_and_simplify(ctx):
    """Windows of 96 x 96 cells of a 120 x 120 Perlin world through the device's preprocessing, each with its own
    reachability mask: validity changes along all four borders, not only in the strips that entered.  After the shift,
    plan() returns what a new field's plan() returns, and simplify() accepts the paths."""
    n, win, n_yaw, (si, sj) = 120, 96, 8, (6, -9)
    elev = perlin_terrain(n, RES, seed=1234, amplitude=0.25)

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
    assert len(cand) > 100                                                      # (this robot fits few poses of a 3.84 m map)
    best = (0, None)                                                            # the candidate that reaches the most nodes
    for r, c, k in cand[::max(1, len(cand) // 16)]:
        with ctx.cost_field(new_m, n_yaw, [(int(r), int(c), int(k))], objective=1, reverse=True) as probe:
            best = max(best, (probe.stats()["reached_nodes"], (int(r), int(c), int(k))))
    src_new = [best[1]]
    src_old = moved(src_new, -si, -sj)
    kw = dict(objective=1, reverse=True)
    window(top, left)
    with ctx.cost_field(old_m, n_yaw, src_old, **kw) as f:
        window(top - si, left - sj)
        st = f.shift(new_m)
        print(f"  {st}")
        kept = FS.move(np.ones((win, win), bool), si, sj, False)
        assert (FS.move(old_m, si, sj, 0) != new_m)[kept].any()                  # words of the overlap differ too
        d = check(ctx, f, new_m, n_yaw, src_new, **kw)
        fin = np.argwhere(np.isfinite(d))
        assert len(fin) > 100
        targets = [tuple(int(v) for v in t) for t in fin[np.random.default_rng(5).integers(0, len(fin), 12)]]
        with ctx.cost_field(new_m, n_yaw, src_new, **kw) as fresh:
            got, want = f.plan(targets), fresh.plan(targets)
            assert [g[0] for g in got] == [w[0] for w in want] and any(g[0] == 0 for g in got)
            for g, w in zip(got, want):
                assert np.float64(g[3]).view(np.uint64) == np.float64(w[3]).view(np.uint64)
                if g[0] == 0:
                    assert np.array_equal(g[1], w[1]) and np.array_equal(bits_of(g[2]), bits_of(w[2]))
            assert np.array_equal(f.blocked(), fresh.blocked())
            assert np.array_equal(bits_of(f.dist()), bits_of(fresh.dist()))
            simple, simple_w = f.simplify(got), fresh.simplify(want)
            for g, s, w in zip(got, simple, simple_w):
                if g[0] == 0:
                    assert s[0] == w[0] == 0 and np.array_equal(s[1], w[1]) and np.array_equal(bits_of(s[2]), bits_of(w[2]))


@pytest.mark.gpu
def test_refusals_leave_the_field_untouched(ctx):
    n_yaw, (si, sj) = 4, (3, -2)
    old_c, new_c = corners(si, sj)
    bits = world_bits(n_yaw, seed=3)
    src = [(RECT[2] - 2, 20, 1), (30, 25, 0)]                                    # the first one leaves with si = 3
    for r, c, k in src:
        bits[old_c[0] + RECT[0] + r, old_c[1] + RECT[1] + c, k] = True
    old_m, new_m = pack(rect_bits(bits, old_c)), pack(rect_bits(bits, new_c))
    kw = dict(rect=RECT, objective=1)

    def refused(f, mask, status=-1):
        before = (bits_of(f.dist()).copy(), f.blocked().copy(), f.stats(), f.shift_stats(), f.blocked_count())
        with pytest.raises(_capi.ArtpError) as e:
            f.shift(mask)
        assert e.value.status == status, e.value
        after = (bits_of(f.dist()), f.blocked(), f.stats(), f.shift_stats(), f.blocked_count())
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]) and before[2:] == after[2:]

    for form in ({}, dict(plain_sweeps=True)):
        install(ctx, old_c)
        with ctx.cost_field(old_m, n_yaw, src, **kw, **form) as f, ctx.cost_field(old_m, n_yaw, src[1:], **kw, **form) as g:
            for fld in (f, g):
                fld.block_moves([(30, 25, 0)], [(31, 25, 0)])
            install(ctx, new_c)
            refused(f, new_m)                                                    # a source that leaves
            gone = rect_bits(bits, new_c).copy()
            gone[30 + si, 25 + sj, 0] = False
            refused(g, pack(gone))                                               # a source that is no node of the new mask
            refused(g, new_m[:, :-1], status=None)                               # a mask of the wrong shape: refused in front of the library
            device_map(ctx, np.zeros(MAP, np.float32), RES, pos=(1.0 - (old_c[0] - 70) * RES, -0.5 - old_c[1] * RES))
            refused(g, new_m)                                                    # 70 rows away at 61 rows: no overlap
            device_map(ctx, np.zeros((MAP[0] + 1, MAP[1]), np.float32), RES, pos=(1.0 - new_c[0] * RES, -0.5 - new_c[1] * RES))
            refused(g, new_m)                                                    # a map of another size
            device_map(ctx, np.zeros(MAP, np.float32), RES * 1.25, pos=(1.0 - new_c[0] * RES, -0.5 - new_c[1] * RES))
            refused(g, new_m)                                                    # ... of another resolution
            install(ctx, new_c)
            st = g.shift(new_m)                                                  # and a valid shift afterwards
            assert (st["shift_rows"], st["shift_cols"]) == (si, sj) and g.blocked_count() == 1
            words = np.zeros((RECT[2], RECT[3], n_yaw), np.uint16)
            words[31 + si, 25 + sj, 0] = 1 << 1                                  # a forward field: (31, 25) owns the move onto it,
                                                                                 # its neighbour by offset 1 is (30, 25)
            check_blocked(ctx, g, new_m, n_yaw, moved(src[1:], si, sj), words, **kw)


@pytest.mark.gpu
def test_learned_and_clearance_fields_are_refused(ctx):
    n_yaw, (si, sj) = 4, (2, 1)
    old_c, new_c = corners(si, sj)
    bits = world_bits(n_yaw, seed=4)
    src = [(30, 25, 0)]
    bits[old_c[0] + RECT[0] + 30, old_c[1] + RECT[1] + 25, 0] = True
    old_m, new_m = pack(rect_bits(bits, old_c)), pack(rect_bits(bits, new_c))
    install(ctx, old_c)
    with ctx.clearance_cost_field(old_m, n_yaw, src, rect=RECT, radius_cells=4, margin=0.1) as f:
        before = bits_of(f.dist()).copy()
        install(ctx, new_c)
        with pytest.raises(_capi.ArtpError) as e:
            f.shift(new_m)
        assert e.value.status == -1 and "clearance" in str(e.value)
        assert np.array_equal(bits_of(f.dist()), before) and f.shift_stats()["reached_nodes"] == 0
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
    with ctx.learned_cost_field(old_m, n_yaw, src, rect=RECT, risk_threshold=1.0) as f:
        before = bits_of(f.dist()).copy()
        install(ctx, new_c)
        cost_map(new_c)
        with pytest.raises(_capi.ArtpError) as e:
            f.shift(new_m)
        assert e.value.status == -1 and "learned" in str(e.value)
        assert np.array_equal(bits_of(f.dist()), before) and f.shift_stats()["reached_nodes"] == 0
