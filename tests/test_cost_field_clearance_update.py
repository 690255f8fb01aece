"""artp_field_update_clearance (csrc/clearance.h): a clearance-weighted field brought in place to an
edited mask must hold the bits of a clearance field computed anew on the merged mask.  artp_field_compute_clearance, which
the update does not touch, is the exact oracle of every case: dist as bit patterns, reached_nodes, paths with their poses
and costs, edge_costs over ALL moves of the rectangle (the weight table slot for slot) and clearance() -- the latter also
against tests/clearance_ref.py.  Every case runs the tiled and the plain form.

The update's counts are held against counts made outside it: changed_slots = the (node, move) pairs whose edge cost differs
in its bit pattern between the field before the update and a new field; changed_d2 = the nodes whose reference clearance
differs; clearance_tiles and repriced_slots = the windows of tests/field_update_clearance_ref.py.

refresh_heights: the heights a field reads are the sampler layer's, which artp_update_layer_rect(s) leave alone (see
include/artp_c.h), so that case rewrites them inside sub_rect through artp_upload_sampler_layers, as
tests/test_cost_field_update.py's test_refreshed_heights does."""
import numpy as np
import pytest

import clearance_ref as CR
import field_update_clearance_ref as UR
import lattice_ref as LR
from art_planner_amd import _capi
from test_clearance_ref import corridor
from test_cost_field import assert_field, check_paths, device_map
from test_cost_field_clearance import CLEAR, N, POS, RECT, RES, Setup, all_moves, bits, random_mask
from test_cost_field_update import merged

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def S():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from art_planner_amd.context import Context
    c = Context(0, "yaml")
    yield Setup(c)
    c.close()


_moves = {}


def moves_of(shape):
    if shape not in _moves:
        a, b, _ = all_moves(shape)
        _moves[shape] = (a, b)
    return _moves[shape]


def targets_of(dist, sources, seed):
    rng = np.random.default_rng(seed)
    fin, rest = np.argwhere(np.isfinite(dist)), np.argwhere(~np.isfinite(dist))
    t = [tuple(int(v) for v in x) for x in fin[rng.integers(0, len(fin), 6)]] + [tuple(int(v) for v in sources[0])]
    if len(rest):
        t += [tuple(int(v) for v in x) for x in rest[rng.integers(0, len(rest), 2)]]
    return t


def snapshot(f, targets):
    a, b = moves_of((f.nrows, f.ncols, f.n_yaw))
    return dict(dist=f.dist(), reached=f.stats()["reached_nodes"], edges=f.edge_costs(a, b), d2=f.clearance(),
                paths=[f.path(t) for t in targets])


def same(ctx, f, got, want, cur, n_yaw, rect, sources, reverse, targets, what):
    """One updated field against the new field: every array bit for bit, every path with its poses and its cost."""
    assert np.array_equal(bits(got["dist"]), bits(want["dist"])), (what, int((bits(got["dist"]) != bits(want["dist"])).sum()))
    assert got["reached"] == want["reached"] == int(np.isfinite(want["dist"]).sum()), what
    assert np.array_equal(bits(got["edges"]), bits(want["edges"])), (what, int((bits(got["edges"]) != bits(want["edges"])).sum()))
    assert np.array_equal(got["d2"], want["d2"]), (what, int((got["d2"] != want["d2"]).sum()))
    for p, q in zip(got["paths"], want["paths"]):
        assert (p is None) == (q is None), what
        if p is not None:
            assert np.array_equal(p[0], q[0]) and np.array_equal(bits(p[1]), bits(q[1])), what
            assert np.float64(p[2]).view(np.uint64) == np.float64(q[2]).view(np.uint64), what
    nr, nc = cur.shape
    lat = LR.Lattice(cur, n_yaw, -RES * np.arange(nr), -RES * np.arange(nc), np.zeros((nr, nc)), 1)   # its nodes and moves only
    check_paths(ctx, f, lat, got["dist"], cur, n_yaw, rect, sources, reverse, targets)


def drive(S, n_yaw, sources, mask0, steps, rect=RECT, reverse=False, objective=1, inner=(64,), clear=CLEAR, blocked=None,
          change=None):
    """One field per form (the tiled one per value of `inner`, and the plain one) on mask0, then every step (mask handed
    in, sub_rect, refresh_heights) on all of them; change(i) moves the context's state in front of step i.  After each step
    every field against ONE new field on the merged mask (with `blocked` = (a, b) blocked on all of them).  Returns the
    stats of the first tiled field per step, and the last new field's snapshot."""
    ctx = S.ctx
    kw = dict(rect=rect, reverse=reverse, objective=objective, **clear)
    R, spread = clear["radius_cells"], clear.get("yaw_spread", 0)
    outside = bool(clear.get("outside_is_obstacle", False))
    fields = [ctx.clearance_cost_field(mask0, n_yaw, sources, inner_sweeps=i, **kw) for i in inner]
    fields.append(ctx.clearance_cost_field(mask0, n_yaw, sources, plain_sweeps=True, **kw))
    out, cur, want = [], np.array(mask0, np.uint32), None
    try:
        shape = (fields[0].nrows, fields[0].ncols)
        a, b = moves_of(shape + (n_yaw,))
        if blocked is not None:
            for f in fields:
                f.block_moves(*blocked)
            words = fields[0].blocked()
        for i, (mask, sub, refresh) in enumerate(steps):
            before, d2_before = fields[0].edge_costs(a, b), CR.clearance_map(cur, n_yaw, R, spread, outside)
            assert np.array_equal(fields[0].clearance(), d2_before)
            if change is not None:
                change(i)
            cur = merged(cur, mask, sub)
            stats = [f.update_clearance(mask, sub, refresh) for f in fields]
            print(f"  step {i}: tiled {stats[0]}")
            print(f"          plain {stats[-1]}")
            with ctx.clearance_cost_field(cur, n_yaw, sources, **kw) as fresh:
                if blocked is not None:
                    fresh.block_moves(*blocked)
                tg = targets_of(fresh.dist(), sources, i)
                want = snapshot(fresh, tg)
            d2_ref = CR.clearance_map(cur, n_yaw, R, spread, outside)
            assert np.array_equal(want["d2"], d2_ref)
            for j, f in enumerate(fields):
                same(ctx, f, snapshot(f, tg), want, cur, n_yaw, rect, sources, reverse, tg, (i, j))
                if blocked is not None:
                    assert np.array_equal(f.blocked(), words)
            nothing = stats[0]["changed_words"] == 0 and not refresh     # the call ended after the diff
            for st in stats:
                if blocked is None:      # a blocked move reads +inf whatever its slot holds
                    assert st["changed_slots"] == int((bits(before) != bits(want["edges"])).sum())
                assert st["changed_d2"] == int((d2_before != d2_ref).sum())
                if not nothing:
                    assert st["clearance_tiles"] == UR.clearance_tiles(shape, sub, R)
                    assert st["repriced_slots"] == UR.repriced_slots(shape, sub, R, n_yaw)
                    assert st["weight_tiles"] <= UR.reprice_tiles(shape, sub, R)
                for key in ("changed_words", "removed_nodes", "added_nodes", "dead_nodes", "hop_dead_nodes", "reached_nodes",
                            "clearance_tiles", "changed_d2", "repriced_slots", "changed_slots", "weight_tiles"):
                    assert st[key] == stats[0][key], key
                assert (st["weight_tiles"] > 0) == (st["changed_slots"] > 0)
            assert stats[-1]["tile_launches"] == 0
            out.append(stats[0])
    finally:
        for f in fields:
            f.close()
    return out, want


def source_of(mask, n_yaw, avoid=None):
    """A node of the mask a third of the way through it, outside the cells of `avoid` = (row0, col0, nrows, ncols)"""
    nodes = np.argwhere(CR.planes(mask, n_yaw))
    if avoid is not None:
        r0, c0, nr, nc = avoid
        nodes = nodes[~((nodes[:, 0] >= r0) & (nodes[:, 0] < r0 + nr) & (nodes[:, 1] >= c0) & (nodes[:, 1] < c0 + nc))]
    return tuple(int(v) for v in nodes[len(nodes) // 3])


CORNER = (14, 14, 4, 4)      # over the common corner (16, 16) of four tiles


def corner_flips(mask, n_yaw, seed, sub=CORNER):
    """About three quarters of the cells of sub get a random word xor-ed in: nodes come and go"""
    rng = np.random.default_rng(seed)
    r0, c0, nr, nc = sub
    new = mask.copy()
    cells = rng.random((nr, nc)) < 0.75
    flip = (rng.integers(1, 1 << n_yaw, (nr, nc), dtype=np.uint64)).astype(np.uint32)
    new[r0:r0 + nr, c0:c0 + nc] ^= np.where(cells, flip, np.uint32(0))
    return new


# ---- cases ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("n_yaw", [1, 2, 7, 16, 32])
@pytest.mark.parametrize("objective", [0, 1])
def test_flips_over_a_tile_corner(S, objective, n_yaw, reverse):
    S.perlin()
    mask = random_mask(RECT[2:], n_yaw, 40 + n_yaw, 0.97)
    src = source_of(mask, n_yaw, CORNER)
    new = corner_flips(mask, n_yaw, 500 + n_yaw)
    inner = (64, 1) if (objective, n_yaw) in ((0, 7), (1, 16)) else (64,)
    stats, want = drive(S, n_yaw, [src], mask, [(new, CORNER, False)], reverse=reverse, objective=objective, inner=inner)
    st = stats[0]
    assert 6 <= st["changed_words"] <= 16 and st["changed_d2"] > 0 and st["changed_slots"] > 0
    assert st["clearance_tiles"] == 4 and st["repriced_slots"] == 4 * 2560 * n_yaw
    if n_yaw == 7 and not reverse:       # the new field itself against Dijkstra over restated weights, once per objective
        import lattice_learned_ref as LL
        from test_cost_field import lattice
        base = lattice(S.ctx, S.gm, new, n_yaw, RECT, objective)
        w = CR.weights(base.w, want["d2"], RES, CLEAR["margin"], CLEAR["gain"])
        assert_field(want["dist"], LL.LearnedLattice(new, n_yaw, w).dijkstra([src], reverse)[0])


@pytest.mark.parametrize("which", ["wide", "spread", "outside"])
def test_wide_radius_spread_and_outside(S, which):
    S.perlin()
    n_yaw = 7
    if which == "wide":          # R = 17 is wider than a tile: one cell at (15, 10) reaches tiles 0 .. 2 by 0 .. 1
        clear, p, sub = dict(radius_cells=17, margin=0.6, gain=3.0), 0.995, (15, 10, 1, 1)
    elif which == "spread":
        clear, p, sub = dict(CLEAR, yaw_spread=1), 0.99, (20, 20, 1, 1)
    else:                        # the rectangle's border, where the outside is the nearest obstacle
        clear, p, sub = dict(CLEAR, outside_is_obstacle=True), 0.97, (0, 20, 1, 1)
    mask = random_mask(RECT[2:], n_yaw, 90, p)
    mask[sub[0], sub[1]] = 0x7f
    src = source_of(mask, n_yaw, sub)
    new = mask.copy()
    new[sub[0], sub[1]] = 0x7f ^ 0b100 if which == "spread" else 0         # spread: one heading goes, its neighbours feel it
    stats, _ = drive(S, n_yaw, [src], mask, [(new, sub, False)], clear=clear)
    st = stats[0]
    assert st["changed_words"] == 1 and st["changed_d2"] > (1 if which != "spread" else 2) and st["changed_slots"] > 0
    if which == "wide":
        assert st["clearance_tiles"] == 6 == UR.clearance_tiles(RECT[2:], sub, 17) and st["weight_tiles"] >= 2
    back, _ = drive(S, n_yaw, [src], new, [(mask, sub, False)], clear=clear, reverse=True)     # and the cell coming back
    assert back[0]["added_nodes"] == st["removed_nodes"] > 0


def test_opening_only(S):
    """An obstacle block cleared away: clearances rise and weights fall, no node goes."""
    S.perlin()
    n_yaw = 4
    mask = np.full(RECT[2:], 0xf, np.uint32)
    mask[18:24, 12:20] = 0
    new = np.full(RECT[2:], 0xf, np.uint32)
    sub = (18, 12, 6, 8)
    for reverse in (False, True):
        with S.ctx.clearance_cost_field(mask, n_yaw, [(3, 3, 0)], rect=RECT, reverse=reverse, **CLEAR) as f:
            d_old, a_b = f.dist(), moves_of(RECT[2:] + (n_yaw,))
            w_old = f.edge_costs(*a_b)
        stats, want = drive(S, n_yaw, [(3, 3, 0)], mask, [(new, sub, False)], reverse=reverse)
        st = stats[0]
        assert st["removed_nodes"] == 0 and st["added_nodes"] == 6 * 8 * n_yaw and st["changed_d2"] > 6 * 8 * n_yaw
        fin = np.isfinite(w_old)
        assert (want["edges"][fin] <= w_old[fin]).all() and (want["edges"][fin] < w_old[fin]).any()   # weights only fall
        assert (want["dist"] <= d_old).all() and (want["dist"] < d_old).any()


def test_closing_only(S):
    """A block that cuts the one gap of a wall: the nodes behind it die."""
    S.perlin()
    n_yaw = 4
    mask = np.full(RECT[2:], 0xf, np.uint32)
    mask[:, 20] = 0
    mask[20:24, 20] = 0xf
    new = mask.copy()
    new[20:24, 20] = 0
    stats, want = drive(S, n_yaw, [(3, 3, 0)], mask, [(new, (19, 19, 6, 3), False)])
    st = stats[0]
    behind = (RECT[3] - 21) * RECT[2] * n_yaw
    assert st["added_nodes"] == 0 and st["removed_nodes"] == 4 * n_yaw and st["dead_nodes"] >= behind
    assert np.isinf(want["dist"][:, 21:]).all() and st["reached_nodes"] == 20 * RECT[2] * n_yaw


@pytest.mark.parametrize("objective", [0, 1])
def test_the_corridor_narrowed_by_one_cell(S, objective):
    S.flat(40)
    m, src, tgt = corridor()
    new = m.copy()
    new[4, 4:28] = 0                               # the horizontal arm loses its top row: the centre line moves
    clear = dict(radius_cells=5, margin=4 * RES, gain=4.0)
    with S.ctx.clearance_cost_field(m, 1, [src], objective=objective, **clear) as f:
        before = f.path(tgt)
        f.update_clearance(new, (4, 4, 1, 24))
        with S.ctx.clearance_cost_field(new, 1, [src], objective=objective, **clear) as fresh:
            got, want = f.path(tgt), fresh.path(tgt)
            assert np.array_equal(got[0], want[0]) and np.array_equal(bits(got[1]), bits(want[1])) and got[2] == want[2]
            assert np.array_equal(bits(f.dist()), bits(fresh.dist())) and np.array_equal(f.clearance(), fresh.clearance())
        assert (got[0][:, 0] != 4).all() and got[2] > before[2]     # no state on the lost row; every row of the arm is now within the margin of a wall
    stats, _ = drive(S, 1, [src], m, [(new, (4, 4, 1, 24), False)], rect=None, objective=objective, clear=clear)
    assert stats[0]["removed_nodes"] == 24


def test_refreshed_heights(S):
    ctx, n, n_yaw = S.ctx, 40, 4
    gm = S.flat(n)
    S.key = None                                    # the sampler layers are rewritten below
    mask = np.full((n, n), (1 << n_yaw) - 1, np.uint32)
    mask[5:30, 12] = 0
    src = (20, 2, 1)
    z = np.asfortranarray(ctx.reachability_poses(1)[..., 0, 2], dtype=np.float32)
    bumped = z.copy(order="F")
    bumped[14:24, 20:30] += np.float32(0.3)
    patch = (13, 19, 12, 12)                        # the bumped cells grown by one

    def upload(elev):
        ls = [gm["cum_prob"], np.ascontiguousarray(gm["cum_prob_rowwise"], np.float32), elev, gm["normal_x"],
              gm["normal_y"], gm["normal_z"], gm["plane_fit_std_dev"]]
        ctx._chk(ctx.L.artp_upload_sampler_layers(ctx.h, *[a.ctypes.data for a in ls], n, n, gm.len_x, gm.len_y,
                                                  gm.pos_x, gm.pos_y), "artp_upload_sampler_layers")

    try:
        with ctx.clearance_cost_field(mask, n_yaw, [src], objective=0, **CLEAR) as f:
            d0, w0 = f.dist(), f.edge_costs(*moves_of((n, n, n_yaw)))
            upload(bumped)
            st = f.update_clearance(mask, patch, refresh_heights=False)     # the field keeps its own heights
            assert all(v == 0 for k, v in st.items() if k != "reached_nodes") and st["reached_nodes"] > 0
            assert np.array_equal(bits(f.dist()), bits(d0))
        upload(z)
        stats, want = drive(S, n_yaw, [src], mask, [(mask, patch, True)], rect=None, objective=0,
                            change=lambda i: upload(bumped))
        st = stats[0]
        assert st["changed_words"] == 0 and st["changed_d2"] == 0 and st["changed_slots"] > 0 and st["dead_nodes"] > 0
        assert (want["dist"][16:22, 22:28] != d0[16:22, 22:28]).all()
        assert not np.array_equal(bits(want["edges"]), bits(w0))
    finally:
        upload(z)


def test_junk_outside_sub_rect_is_not_read(S):
    import torch
    S.perlin()
    n_yaw = 8
    old = random_mask(RECT[2:], n_yaw, 3, 0.95)
    junk = random_mask(RECT[2:], n_yaw, 4, 0.5)           # differs from old nearly everywhere
    sub = (12, 9, 11, 17)
    old[1, 1] |= 1
    want = merged(old, junk, sub)
    assert (want != junk).sum() > old.size // 2 and (want != old).any()
    t = torch.from_numpy(np.ascontiguousarray(junk.T).view(np.int32).reshape(-1)).to("cuda:0")   # reachability_map_dev's layout
    for m in (junk, t):
        ctx = S.ctx
        kw = dict(rect=RECT, **CLEAR)
        with ctx.clearance_cost_field(old, n_yaw, [(1, 1, 0)], **kw) as f, ctx.clearance_cost_field(want, n_yaw, [(1, 1, 0)], **kw) as fresh:
            st = f.update_clearance(m, sub)
            assert st["changed_words"] == int(((want ^ old) != 0).sum())
            assert np.array_equal(bits(f.dist()), bits(fresh.dist())) and np.array_equal(f.clearance(), fresh.clearance())
            ab = moves_of(RECT[2:] + (n_yaw,))
            assert np.array_equal(bits(f.edge_costs(*ab)), bits(fresh.edge_costs(*ab)))
    stats, _ = drive(S, n_yaw, [(1, 1, 0)], old, [(junk, sub, False)])
    assert stats[0]["changed_words"] == int(((want ^ old) != 0).sum())


def test_the_same_mask_changes_nothing(S):
    S.perlin()
    n_yaw = 8
    mask = random_mask(RECT[2:], n_yaw, 4, 0.9)
    mask[20, 20] |= 1
    ab = moves_of(RECT[2:] + (n_yaw,))
    for plain in (False, True):
        with S.ctx.clearance_cost_field(mask, n_yaw, [(20, 20, 0)], rect=RECT, plain_sweeps=plain, **CLEAR) as f:
            assert all(v == 0 for v in f.clearance_update_stats().values())        # zeros before the first update
            d, w, d2, reached = f.dist(), f.edge_costs(*ab), f.clearance(), f.stats()["reached_nodes"]
            for sub in (None, (0, 0, 5, 5)):
                st = f.update_clearance(mask, sub)
                assert st == f.clearance_update_stats()
                assert all(v == 0 for k, v in st.items() if k != "reached_nodes"), st
                assert st["reached_nodes"] == reached
            assert np.array_equal(bits(f.dist()), bits(d)) and np.array_equal(bits(f.edge_costs(*ab)), bits(w))
            assert np.array_equal(f.clearance(), d2)


def test_five_updates_in_a_row(S):
    S.perlin()
    n_yaw = 4
    rng = np.random.default_rng(77)
    cur = CR.planes(random_mask(RECT[2:], n_yaw, 78, 0.93), n_yaw)
    cur[22, 19, 0] = True
    from test_cost_field_update import pack
    steps, first = [], pack(cur)
    for i, (r0, c0, nr, nc) in enumerate([(3, 3, 6, 6), (28, 10, 5, 7), (10, 28, 9, 4), (3, 3, 6, 6), (38, 30, 7, 8)]):
        nxt = cur.copy()
        block = nxt[r0:r0 + nr, c0:c0 + nc]
        if i % 2 == 0:
            block &= rng.random(block.shape) < 0.7   # removals
        else:
            block |= rng.random(block.shape) < 0.8   # additions
        steps.append((pack(nxt), (r0, c0, nr, nc), False))
        cur = nxt
    stats, _ = drive(S, n_yaw, [(22, 19, 0)], first, steps, objective=0)
    assert all(s["removed_nodes"] > 0 and s["added_nodes"] == 0 for s in stats[0::2])
    assert all(s["added_nodes"] > 0 and s["removed_nodes"] == 0 for s in stats[1::2])


def test_blocked_moves_are_kept(S):
    S.perlin()
    n_yaw = 7
    mask = random_mask(RECT[2:], n_yaw, 47, 0.97)
    src = source_of(mask, n_yaw, CORNER)
    new = corner_flips(mask, n_yaw, 507)
    kw = dict(rect=RECT, **CLEAR)
    with S.ctx.clearance_cost_field(mask, n_yaw, [src], **kw) as f:
        d = f.dist()
        far = tuple(int(v) for v in np.argwhere(d == d[np.isfinite(d)].max())[0])
        nodes = [tuple(int(v) for v in nd) for nd in f.path(far)[0]]
    inside = lambda v: CORNER[0] <= v[0] < CORNER[0] + 4 and CORNER[1] <= v[1] < CORNER[1] + 4
    pairs = [(a, b) for a, b in zip(nodes[:-1], nodes[1:]) if not inside(a) and not inside(b)]
    assert len(pairs) > 6
    blocked = ([p[0] for p in pairs[2::3]], [p[1] for p in pairs[2::3]])      # tight moves of a shortest path, outside the edit
    drive(S, n_yaw, [src], mask, [(new, CORNER, False)], blocked=blocked)
    with S.ctx.clearance_cost_field(mask, n_yaw, [src], **kw) as f, S.ctx.clearance_cost_field(new, n_yaw, [src], **kw) as fresh:
        assert f.block_moves(*blocked) == len(blocked[0])
        f.update_clearance(new, CORNER)
        assert f.blocked_count() == len(blocked[0])
        assert f.unblock() == len(blocked[0])
        assert np.array_equal(bits(f.dist()), bits(fresh.dist()))             # back at the new unblocked field's bits
        ab = moves_of(RECT[2:] + (n_yaw,))
        assert np.array_equal(bits(f.edge_costs(*ab)), bits(fresh.edge_costs(*ab)))


@pytest.mark.parametrize("objective", [0, 1])
def test_gain_zero_is_the_updated_plain_field(S, objective):
    S.perlin()
    for n_yaw in (1, 7):
        mask = random_mask(RECT[2:], n_yaw, 40 + n_yaw, 0.97)
        src = source_of(mask, n_yaw, CORNER)
        new = corner_flips(mask, n_yaw, 500 + n_yaw)
        for reverse in (False, True):
            kw = dict(rect=RECT, reverse=reverse, objective=objective)
            with S.ctx.clearance_cost_field(mask, n_yaw, [src], radius_cells=5, margin=0.15, gain=0.0, **kw) as f, \
                    S.ctx.cost_field(mask, n_yaw, [src], **kw) as p:
                st, sp = f.update_clearance(new, CORNER), p.update(new, CORNER)
                assert np.array_equal(bits(f.dist()), bits(p.dist())), (n_yaw, reverse)
                assert st["reached_nodes"] == sp["reached_nodes"] and st["changed_words"] == sp["changed_words"] > 0


def test_a_far_corner_stays_local(S):
    ctx, n_yaw = S.ctx, 16
    S.perlin()
    old = np.full((N, N), (1 << n_yaw) - 1, np.uint32)
    old[40:44, 30:60] = 0
    new = old.copy()
    new[92:96, 92:96] = 0
    sub, goal = (92, 92, 4, 4), (2, 2, 0)
    with ctx.clearance_cost_field(old, n_yaw, [goal], reverse=True, **CLEAR) as f:
        fresh = f.stats()
    assert fresh["tiles"] == 36
    stats, _ = drive(S, n_yaw, [goal], old, [(new, sub, False)], rect=None, reverse=True)
    st = stats[0]
    print(f"  update: {st['tile_launches']} tile runs; a new field: {fresh['tile_launches']} + {fresh['hop_tile_launches']}")
    assert st["clearance_tiles"] == UR.clearance_tiles((N, N), sub, 5) == 1
    assert st["repriced_slots"] == UR.repriced_slots((N, N), sub, 5, n_yaw) == 2560 * n_yaw
    assert 0 < st["weight_tiles"] <= UR.reprice_tiles((N, N), sub, 5)
    assert st["tile_launches"] < fresh["tile_launches"] + fresh["hop_tile_launches"]


def test_refusals_leave_the_field_untouched(S):
    ctx, n_yaw = S.ctx, 7
    S.perlin()
    mask = random_mask(RECT[2:], n_yaw, 47, 0.97)
    src = source_of(mask, n_yaw)
    ab = moves_of(RECT[2:] + (n_yaw,))
    edited = mask.copy()
    r0 = 30 if src[0] < 22 else 5
    edited[r0:r0 + 4, 10:14] = 0
    gone = mask.copy()
    gone[src[0], src[1]] &= ~np.uint32(1 << src[2])
    gone[r0:r0 + 4, 10:14] = 0

    def refused(call, status=-1):
        with pytest.raises(_capi.ArtpError) as e:
            call()
        assert e.value.status == status, e.value

    kw = dict(rect=RECT, objective=1)
    # a plain and a learned field
    with ctx.cost_field(mask, n_yaw, [src], **kw) as p:
        before = p.dist()
        refused(lambda: p.update_clearance(edited))
        assert np.array_equal(bits(p.dist()), bits(before))
    import test_cost_field_learned as TL
    ctx.cost_load_weights(TL.blob(1, "real"))
    elev = np.zeros((N, N), np.float32)
    ctx.cost_update_map(elev, RES, N * RES, N * RES, *POS)
    with ctx.learned_cost_field(mask, n_yaw, [src], rect=RECT) as lf:
        before, w = lf.dist(), lf.edge_costs(*ab)
        refused(lambda: lf.update_clearance(edited))
        assert np.array_equal(bits(lf.dist()), bits(before)) and np.array_equal(bits(lf.edge_costs(*ab)), bits(w))
    for plain in (False, True):
        with ctx.clearance_cost_field(mask, n_yaw, [src], plain_sweeps=plain, **CLEAR, **kw) as f:
            before, d2, w = f.dist(), f.clearance(), f.edge_costs(*ab)

            def untouched(path=True):
                assert np.array_equal(bits(f.dist()), bits(before)) and np.array_equal(f.clearance(), d2)
                assert np.array_equal(bits(f.edge_costs(*ab)), bits(w))
                assert not path or f.path(src)[2] == 0.0                # (the poses of a path need the field's own map)

            for rect in [(40, 0, 10, 10), (0, -1, 5, 5), (0, 0, 0, 5), (0, 0, 46, 1), (0, 37, 1, 2)]:
                refused(lambda: f.update_clearance(edited, rect))
            untouched()
            refused(lambda: f.update_clearance(gone))                     # the source's bit removed
            untouched()
            refused(lambda: f.update(edited))                             # the other two calls still refuse it
            refused(lambda: f.update_learned(edited))
            untouched()
            device_map(ctx, np.zeros((50, 50), np.float32), RES)         # a map of another geometry
            S.key = None
            try:
                refused(lambda: f.update_clearance(edited, None, refresh_heights=True))
                untouched(path=False)
                st = f.update_clearance(edited)                           # without the heights the edit is taken
                assert st["removed_nodes"] == int(CR.planes(mask[r0:r0 + 4, 10:14], n_yaw).sum())
            finally:
                S.perlin()
            with ctx.clearance_cost_field(edited, n_yaw, [src], **CLEAR, **kw) as fresh:
                assert np.array_equal(bits(f.dist()), bits(fresh.dist())) and np.array_equal(f.clearance(), fresh.clearance())
