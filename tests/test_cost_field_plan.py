"""Blocked moves and the lazy loop on cost-to-go fields (csrc/field_plan.h, include/artp_c.h artp_field_block_moves, _unblock,
_blocked, _plan).

What a case compares, through snapshot() / same(): distances as bit patterns, reached_nodes, the blocked words, 16 paths
with their poses and costs, and the fold of the field's own edge costs along each path.  The oracles:
  * fields of another history on the same mask and the same blocked set: all moves blocked in one call on a new field,
    one call per move, the plain form against the tiled one, inner_sweeps 1 against 64.  The least fixed point is unique,
    so they must agree bit for bit;
  * tests/lattice_ref.py's Dijkstra with w[m][a] = +inf for the blocked moves (tests/field_plan_ref.py): the finite set
    exactly, the values to the relative 1e-9 that test_cost_field.py derives;
  * for artp_field_plan: the same loop written here from public calls (path, check_motions, block_moves) on a second field.
The masks are synthetic or depend on the device's map, so every condition a case needs is asserted before it is used."""
import ctypes as C
from collections import deque

import numpy as np
import pytest

import field_plan_ref as FP
import lattice_ref as LR
from art_planner_amd import _capi
from synthetic import GridMap, map_from_device, perlin_terrain
from test_cost_field import ROBOT, assert_field, device_map, lattice, spiral_mask
from test_cost_field_update import bits_of, fold, pack

FORMS = [dict(), dict(plain_sweeps=True)]


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
def tup(x):
    return tuple(int(v) for v in x)


def split(moves):
    return np.array([a for a, _ in moves], np.int32).reshape(-1, 3), np.array([b for _, b in moves], np.int32).reshape(-1, 3)


def snapshot(f, targets, reverse):
    paths = []
    for t in targets:
        p = f.path(t)
        paths.append(None if p is None else (p[0], bits_of(p[1]), np.float64(p[2]).view(np.uint64), fold(f, p[0], reverse)))
    return dict(dist=f.dist(), reached=f.stats()["reached_nodes"], words=f.blocked(), count=f.blocked_count(), paths=paths)


def same(got, want, what):
    assert np.array_equal(bits_of(got["dist"]), bits_of(want["dist"])), \
        (what, int((bits_of(got["dist"]) != bits_of(want["dist"])).sum()))
    assert got["reached"] == want["reached"] == int(np.isfinite(want["dist"]).sum()), what
    assert np.array_equal(got["words"], want["words"]) and got["count"] == want["count"], what
    for p, q in zip(got["paths"], want["paths"]):
        assert (p is None) == (q is None), what
        if p is not None:
            assert np.array_equal(p[0], q[0]) and np.array_equal(p[1], q[1]) and p[2] == q[2], what
            assert p[3].view(np.uint64) == p[2], what        # the fold of the field's own edge costs along its path


def pick_targets(dist, sources, seed, n=16):
    rng = np.random.default_rng(seed)
    fin, rest = np.argwhere(np.isfinite(dist)), np.argwhere(~np.isfinite(dist))
    t = [tup(x) for x in fin[rng.integers(0, len(fin), n - 1)]] + [tup(sources[0])]
    if len(rest):
        t += [tup(x) for x in rest[rng.integers(0, len(rest), 2)]]
    return t


def path_moves(f, targets, every=3):
    """Every `every`-th move of the field's paths to the targets, in travel order: moves that carry shortest paths."""
    out = []
    for t in targets:
        p = f.path(t)
        if p is not None:
            nodes = [tup(x) for x in p[0]]
            out += list(zip(nodes[:-1], nodes[1:]))[1::every]
    return out


def existing_moves(lat, rng, n, rotations):
    """n random moves whose edge exists in the lattice; rotations: the share taken among moves 8 and 9."""
    out = []
    for m_lo, m_hi, cnt in ((0, 8, n - rotations), (8, 10, rotations)):
        w = lat.w[m_lo:m_hi]
        e = np.argwhere(np.isfinite(w))
        for m, r, c, k in e[rng.integers(0, len(e), cnt)] if len(e) and cnt else []:
            a = (int(r), int(c), int(k))
            b = np.unravel_index(int(lat.neighbour_index(m_lo + int(m))[a]), lat.shape)
            out.append((a, tup(b)))
    return out


def spiral_gates(n_yaw, reverse):
    """On spiral_mask(48): the top side of ring 1 (rows 4..6) right of its cut is walked from column 43 down to column 25
    on the way in.  At column 36 the two upper lanes are closed in that direction (what is left is lane 6: a detour for
    what lies behind), and ring 3's top side (rows 12..14, walked the same way) is closed altogether at column 30:
    everything further in is cut off.  A reverse field travels the other way, so there the opposite moves are the gates."""
    mv = []
    for k in range(n_yaw):
        for rows, col, closed in (((4, 5, 6), 36, (4, 5)), ((12, 13, 14), 30, (12, 13, 14))):
            for r_to in closed:
                for r_from in rows:
                    if abs(r_from - r_to) <= 1:
                        a, b = (r_from, col + 1, k), (r_to, col, k)
                        mv.append((a, b) if not reverse else (b, a))
    return mv


def blocked_exactly(ctx, gm, mask, n_yaw, rect, sources, objective, moves_of, inners=(64,), seed=0):
    """For both directions: moves = moves_of(a forward-or-reverse field, its lattice) blocked (a) in one call, (b) one call
    per move in random order (all of them in the first form, 32 and then the rest in the others), in every form; all
    against one another, and (a) against Dijkstra on the blocked weights."""
    for reverse in (False, True):
        kw = dict(rect=rect, objective=objective, reverse=reverse)
        lat = lattice(ctx, gm, mask, n_yaw, rect, objective)
        with ctx.cost_field(mask, n_yaw, sources, **kw) as f0:
            moves = moves_of(f0, lat, reverse)
            before = f0.dist()
            assert f0.blocked_count() == 0 and not f0.blocked().any()
        moves = list(dict.fromkeys(moves))               # a set, in order
        a, b = split(moves)
        want_words = FP.words(lat.shape, lat, moves, reverse)
        FP.block(lat, moves)
        ref = lat.dijkstra(sources, reverse)[0]
        assert (ref[np.isfinite(before)] > before[np.isfinite(before)] * (1 + 1e-6)).any()   # the set matters
        forms = [dict(inner_sweeps=i) for i in inners] + [dict(plain_sweeps=True)]
        want = None
        for form in forms:
            with ctx.cost_field(mask, n_yaw, sources, **kw, **form) as f, \
                    ctx.cost_field(mask, n_yaw, sources, **kw, **form) as g:
                assert f.block_moves(a, b) == len(moves)
                assert f.block_moves(a[:3], b[:3]) == 0                     # again: nothing new, nothing changes
                order = np.random.default_rng(seed).permutation(len(moves))
                single = len(order) if want is None else 32                 # one call per move
                for i in order[:single]:
                    assert g.block_moves(a[i], b[i]) == 1
                if len(order) > single:
                    assert g.block_moves(a[order[single:]], b[order[single:]]) == len(order) - single
                if want is None:
                    d = f.dist()
                    assert_field(d, ref)
                    assert np.array_equal(f.blocked(), want_words) and f.blocked_count() == len(moves)
                    targets = pick_targets(d, sources, seed) + [tup(m[1] if not reverse else m[0]) for m in moves[:4]]
                    want = snapshot(f, targets, reverse)
                    assert np.isinf(f.edge_costs(a, b)).all()               # a blocked move is an absent edge
                    back = f.edge_costs(b, a)                               # the other direction is not
                    gone = {(tup(x), tup(y)) for x, y in moves}
                    keep = [i for i in range(len(moves)) if (tup(b[i]), tup(a[i])) not in gone]
                    assert np.isfinite(back[keep]).all()
                same(snapshot(f, targets, reverse), want, ("one call", form, reverse))
                same(snapshot(g, targets, reverse), want, ("move by move", form, reverse))
                # and back: every bit cleared in one call gives the field of the mask alone
                assert f.unblock() == len(moves) and f.blocked_count() == 0
                assert np.array_equal(bits_of(f.dist()), bits_of(before))


# ---- 1. blocking is exact ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n_yaw", [1, 16])
@pytest.mark.parametrize("objective", [0, 1])
def test_blocked_moves_on_a_spiral(ctx, objective, n_yaw):
    n = 48
    gm = device_map(ctx, np.zeros((n, n), np.float32), 0.04)
    mask, src = spiral_mask(n, n_yaw)

    def moves_of(f, lat, reverse):
        rng = np.random.default_rng(31 + n_yaw)
        d = f.dist()
        tg = pick_targets(d, [src], 5, 6)
        mv = path_moves(f, tg)                                           # moves that carry shortest paths
        mv += existing_moves(lat, rng, 24, 8 if n_yaw > 1 else 0)        # random ones, rotations among them
        mv += [((14, 15, 0), (14, 16, 0)), ((14, 16, 0), (14, 15, 0)),   # a two-way pair across a tile border
               ((14, 15, 0), (13, 16, 0))]                               # and a diagonal across it
        mv += spiral_gates(n_yaw, reverse)
        for a, b in mv:
            assert lat.exists(a) and lat.exists(b), (a, b)
        return mv

    blocked_exactly(ctx, gm, mask, n_yaw, None, [src], objective, moves_of, inners=(64, 1) if n_yaw == 16 else (64,))


@pytest.mark.gpu
def test_blocked_moves_on_a_random_mask_in_an_odd_rectangle(ctx):
    n_yaw = 7
    elev = np.ascontiguousarray(perlin_terrain(83, 0.05, seed=21)[:, :71]) * np.float32(0.8)
    gm = device_map(ctx, elev, 0.05, pos=(0.3, 0.7))
    rect = (7, 5, 37, 45)                            # 3 x 3 tiles, partial ones on both edges
    rng = np.random.default_rng(77)
    bits = rng.random((rect[2], rect[3], n_yaw)) < 0.8
    sources = [(2, 3, 0), (33, 40, n_yaw - 1)]
    for s in sources + [(15, 15, 2), (16, 16, 2), (15, 16, 2), (16, 15, 2)]:
        bits[s] = True
    mask = pack(bits)

    def moves_of(f, lat, reverse):
        r = np.random.default_rng(78)
        mv = path_moves(f, pick_targets(f.dist(), sources, 6, 12), every=2)
        mv += existing_moves(lat, r, 60, 20)
        mv += [((15, 15, 2), (16, 16, 2)), ((16, 16, 2), (15, 15, 2)),   # across the corner where four tiles meet
               ((15, 16, 2), (16, 15, 2))]
        return mv

    for objective in (0, 1):
        blocked_exactly(ctx, gm, mask, n_yaw, rect, sources, objective, moves_of, inners=(64, 1), seed=objective)


def random_case(ctx, n_yaw):
    """The map, the odd rectangle (3 x 3 tiles, partial ones on both edges), a random mask at density 0.8, two sources."""
    elev = np.ascontiguousarray(perlin_terrain(83, 0.05, seed=21)[:, :71]) * np.float32(0.8)
    gm = device_map(ctx, elev, 0.05, pos=(0.3, 0.7))
    rect = (7, 5, 37, 45)
    bits = np.random.default_rng(77 + n_yaw).random((rect[2], rect[3], n_yaw)) < 0.8
    sources = [(2, 3, 0), (33, 40, n_yaw - 1)]
    for s in sources:
        bits[s] = True
    bits[20, 20] = bits[20, 21] = bits[21, 20] = True              # the cells of the rotation case below
    return gm, rect, pack(bits), sources


@pytest.mark.gpu
@pytest.mark.parametrize("n_yaw", [2, 32])
def test_blocked_moves_at_2_and_32_headings(ctx, n_yaw):
    """32 headings: the largest tiles (126 KB of LDS).  2 headings: k + 1 and k - 1 are the same neighbour, so a rotation
    sits in pull slots 8 AND 9 of its owner; blocking it must close both."""
    gm, rect, mask, sources = random_case(ctx, n_yaw)

    def moves_of(f, lat, reverse):
        mv = path_moves(f, pick_targets(f.dist(), sources, 6, 12), every=2)
        mv += existing_moves(lat, np.random.default_rng(79), 40, 20)
        return mv + [((20, 20, 0), (20, 20, 1)), ((20, 20, 1), (20, 20, 0))]

    blocked_exactly(ctx, gm, mask, n_yaw, rect, sources, 1, moves_of, inners=(64, 1), seed=n_yaw)


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("reverse", [False, True])
def test_a_blocked_rotation_at_2_headings_is_on_no_path(ctx, reverse, form):
    """Objective 1 from (20, 20, 0): the way to the other heading of the same cell is the one rotation (translations keep
    the heading, so any other way holds a rotation as well, and more).  Blocked, it must be gone from dist and from the
    path, whichever of its two slots a kernel reads; plan() on the field must not come back with status 2."""
    gm, rect, mask, _ = random_case(ctx, 2)
    src, tgt = (20, 20, 0), (20, 20, 1)
    move = (src, tgt) if not reverse else (tgt, src)                # travel direction
    with ctx.cost_field(mask, 2, [src], rect=rect, objective=1, reverse=reverse, **form) as f:
        d0 = f.dist()
        nodes = f.path(tgt)[0]
        assert len(nodes) == 2 and d0[tgt] == f.edge_costs([move[0]], [move[1]])[0]
        assert f.block_moves([move[0]], [move[1]]) == 1 and f.blocked_count() == 1
        owner = move[0] if reverse else move[1]
        assert f.blocked()[owner] == 0x300 and int((f.blocked() != 0).sum()) == 1
        assert f.block_moves([move[0]], [move[1]]) == 0
        d = f.dist()
        assert np.isfinite(d[tgt]) and d[tgt] > d0[tgt] and np.isinf(f.edge_costs([move[0]], [move[1]])[0])
        nodes, _, cost = f.path(tgt)
        steps = list(zip([tup(x) for x in nodes[:-1]], [tup(x) for x in nodes[1:]]))
        assert move not in steps and len(steps) >= 3 and fold(f, nodes, reverse) == cost == d[tgt]
        lat = lattice(ctx, gm, mask, 2, rect, 1)
        FP.block(lat, [move])
        assert_field(d, lat.dijkstra([src], reverse)[0])
        res = f.plan([tgt, (20, 21, 1), (21, 20, 0)], max_rounds=16)
        assert all(r[0] in (0, 1) for r in res), [r[0] for r in res]
        assert f.plan_stats()["rounds"] < 16 and len(f.plan_stats()["round_tile_runs"]) == f.plan_stats()["rounds"]
        assert f.blocked()[owner] & 0x300 == 0x300                    # plan() may have added translations onto it
        assert f.unblock() == f.plan_stats()["moves_blocked"] + 1 and f.blocked_count() == 0
        assert np.array_equal(bits_of(f.dist()), bits_of(d0))


# ---- 2. cut off -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_blocking_the_single_entry_move_cuts_the_arm_off(ctx, form):
    """Objective 0 at 7 headings: rotations cost 0, so behind the entry the headings of a cell hold one another up by
    distance alone; only the hop rule lets them die."""
    n, n_yaw = 48, 7
    device_map(ctx, np.zeros((n, n), np.float32), 0.04)
    mask, src = spiral_mask(n, n_yaw)
    mid = n // 2
    # the way from ring 0 into ring 1 (row 3, columns mid - 3 .. mid - 1) narrowed to ONE move: one cell at one heading,
    # and that heading taken from the two cells that could step onto it diagonally
    mask[3, mid - 3] = mask[3, mid - 1] = 0
    mask[3, mid - 2] = 1 << 3
    mask[2, mid - 3] &= ~np.uint32(1 << 3)
    mask[2, mid - 1] &= ~np.uint32(1 << 3)
    entry = ((2, mid - 2, 3), (3, mid - 2, 3))
    inside = mask != 0
    inside[:4] = inside[-3:] = inside[:, :3] = inside[:, -3:] = False         # ring 1 and further in
    inside[3, mid - 2] = True
    with ctx.cost_field(mask, n_yaw, [src], objective=0, **form) as f:
        d0 = f.dist()
        snap0 = snapshot(f, pick_targets(d0, [src], 1), False)
        n_in = int(((mask[inside][:, None] >> np.arange(n_yaw, dtype=np.uint32)) & 1).sum())
        assert np.isfinite(d0[inside][(mask[inside][:, None] >> np.arange(n_yaw, dtype=np.uint32)) & 1 == 1]).all()
        assert f.block_moves([entry[1]], [entry[0]]) == 1                     # the way OUT: nothing depends on it
        assert np.array_equal(bits_of(f.dist()), bits_of(d0))
        assert f.block_moves([entry[0]], [entry[1]]) == 1
        d = f.dist()
        assert np.isinf(d[inside]).all() and f.stats()["reached_nodes"] == int(np.isfinite(d0).sum()) - n_in
        assert np.array_equal(bits_of(d[~inside]), bits_of(d0[~inside]))
        assert f.path((20, 20, 0)) is None
        words = f.blocked()
        # the way in is move 6 (+1, 0): stored at its end under the offset that leads back, 1; the way out likewise
        assert words[3, mid - 2, 3] == 1 << 1 and words[2, mid - 2, 3] == 1 << 6 and f.blocked_count() == 2
        # a rectangle that misses the owner's cell changes nothing
        assert f.unblock((4, 0, n - 4, n)) == 0 and f.unblock((3, mid - 1, 1, 5)) == 0
        assert np.array_equal(bits_of(f.dist()), bits_of(d)) and f.blocked_count() == 2
        assert f.unblock((3, mid - 2, 1, 1)) == 1                              # the owner of the way in
        same(dict(snapshot(f, pick_targets(d0, [src], 1), False), words=snap0["words"], count=0), snap0, "unblocked")
        assert f.blocked_count() == 1 and f.unblock() == 1 and not f.blocked().any()


# ---- 3. learned fields, and updates that keep the set --------------------------------------------------------------
@pytest.fixture(scope="module")
def S():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from art_planner_amd.context import Context
    from test_cost_field_learned_update import State
    c = Context(0, "yaml")
    yield State(c)
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("reverse", [False, True])
def test_blocks_on_a_learned_field_survive_a_reprice(S, reverse):
    from test_cost_field_learned import RECT, WEIGHTS, random_mask
    n_yaw = 7
    S.set(1, "real", 0)
    ctx = S.ctx
    mask = random_mask(RECT[2:], n_yaw, 51, p=0.9)
    lat = S.lattice(mask, n_yaw, RECT, **WEIGHTS)
    label, sizes = lat.components()
    comp = np.argwhere(label == int(np.argmax(sizes)))
    sources = [tup(comp[len(comp) // 2])]
    kw = dict(rect=RECT, reverse=reverse, **WEIGHTS)
    fields = [ctx.learned_cost_field(mask, n_yaw, sources, **kw, **form) for form in (dict(), dict(inner_sweeps=1),
                                                                                     dict(plain_sweeps=True))]
    try:
        f = fields[0]
        d0 = f.dist()
        targets = pick_targets(d0, sources, 3)
        moves = list(dict.fromkeys(path_moves(f, targets, every=2) + existing_moves(lat, np.random.default_rng(4), 40, 12)))
        a, b = split(moves)
        for g in fields:
            assert g.block_moves(a, b) == len(moves)
        want = snapshot(f, targets, reverse)
        assert (want["dist"][np.isfinite(d0)] > d0[np.isfinite(d0)]).any()
        assert np.isinf(f.edge_costs(a, b)).all()
        for j, g in enumerate(fields[1:]):
            same(snapshot(g, targets, reverse), want, ("forms", j))
        # against the reference: Dijkstra on the restated weights with the blocked moves at +inf
        FP.block(lat, moves)
        assert_field(want["dist"], lat.dijkstra(sources, reverse)[0])
        # the cost map moves: every slot is priced again; the blocks are an overlay, so changed_slots does not see them
        with ctx.learned_cost_field(mask, n_yaw, sources, **kw) as clean:
            S.set(1, "real", 1)
            clean_stats = clean.update_learned()
        stats = [g.update_learned() for g in fields]
        with ctx.learned_cost_field(mask, n_yaw, sources, **kw) as fresh:
            assert fresh.block_moves(a, b) == len(moves)
            want = snapshot(fresh, targets, reverse)
        for j, g in enumerate(fields):
            same(snapshot(g, targets, reverse), want, ("repriced", j))
            assert stats[j]["changed_slots"] == clean_stats["changed_slots"] > 0
            assert np.isinf(g.edge_costs(a, b)).all()
    finally:
        for g in fields:
            g.close()
        S.set(1, "real", 0)


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_a_mask_update_keeps_the_blocks(ctx, form):
    n_yaw = 7
    elev = np.ascontiguousarray(perlin_terrain(83, 0.05, seed=21)[:, :71]) * np.float32(0.8)
    gm = device_map(ctx, elev, 0.05, pos=(0.3, 0.7))
    rect, sub = (7, 5, 37, 45), (8, 10, 20, 20)
    rng = np.random.default_rng(207)
    bits = rng.random((rect[2], rect[3], n_yaw)) < 0.8
    sources = [(2, 3, 0), (33, 40, n_yaw - 1)]
    for s in sources:
        bits[s] = True
    new = bits.copy()
    new[sub[0]:sub[0] + sub[2], sub[1]:sub[1] + sub[3]] ^= rng.random((sub[2], sub[3], n_yaw)) < 0.15
    for objective, reverse in ((0, False), (1, True)):
        kw = dict(rect=rect, objective=objective, reverse=reverse, **form)
        with ctx.cost_field(pack(bits), n_yaw, sources, **kw) as f, ctx.cost_field(pack(new), n_yaw, sources, **kw) as fresh:
            moves = list(dict.fromkeys(path_moves(f, pick_targets(f.dist(), sources, 9), every=2) +
                                       path_moves(fresh, pick_targets(fresh.dist(), sources, 9), every=2)))
            a, b = split(moves)
            f.block_moves(a, b)
            f.update(pack(new), sub)
            fresh.block_moves(a, b)
            targets = pick_targets(fresh.dist(), sources, 10)
            same(snapshot(f, targets, reverse), snapshot(fresh, targets, reverse), (objective, reverse))
            lat = lattice(ctx, gm, pack(new), n_yaw, rect, objective)
            FP.block(lat, moves)
            assert_field(f.dist(), lat.dijkstra(sources, reverse)[0])


# ---- 4. the loop against its own parts ----------------------------------------------------------------------------
_worlds = {}


def world(ctx, amplitude, n_yaw):
    """The 120 x 120 Perlin map through the device's preprocessing, its reachability mask at n_yaw headings, the source
    (the middle node of the largest component) and 16 targets by hop rank over the farther half; made once."""
    key = (amplitude, n_yaw)
    n, res = 120, 0.04
    raw = GridMap(n, n, res)
    raw.add("elevation", perlin_terrain(n, res, seed=1234, amplitude=amplitude))
    raw.add("traversability", np.ones((n, n), np.float32))
    gm = map_from_device(ctx, raw, ROBOT)
    if key not in _worlds:
        mask = ctx.reachability_map(n_yaw)
        lat = lattice(ctx, gm, mask, n_yaw, None, 1)
        label, sizes = lat.components()
        comp = np.argwhere(label == int(np.argmax(sizes)))
        src = tup(comp[len(comp) // 2])
        indptr, adj, _ = lat.csr(False)
        hops = {lat.index(src): 0}
        q = deque([lat.index(src)])
        while q:
            u = q.popleft()
            for e in range(indptr[u], indptr[u + 1]):
                if adj[e] not in hops:
                    hops[adj[e]] = hops[u] + 1
                    q.append(adj[e])
        order = sorted(hops, key=lambda i: (hops[i], i))
        ranks = np.linspace(len(order) // 2, len(order) - 1, 16).astype(int)
        targets = [tup(np.unravel_index(order[r], lat.shape)) for r in ranks]
        print(f"  amplitude {amplitude}, {n_yaw} headings: component of {len(order)} nodes, targets "
              f"{hops[order[ranks[0]]]}..{hops[order[ranks[-1]]]} hops away")
        _worlds[key] = (mask, src, targets)
    return (gm,) + _worlds[key]


def loop_from_public_calls(ctx, g, targets, max_rounds):
    """artp_field_plan restated: (results, rounds, raw paths with a failing move, checked moves with their verdicts)."""
    pending = list(range(len(targets)))
    out = [(2, None, None, np.inf)] * len(targets)
    rounds, raw_bad, checked = 0, None, []
    while pending and rounds < max_rounds:
        rounds += 1
        paths = [g.path(targets[i]) for i in pending]
        s1 = [p[1][:-1] for p in paths if p is not None and len(p[0]) > 1]
        s2 = [p[1][1:] for p in paths if p is not None and len(p[0]) > 1]
        ok = ctx.check_motions(np.concatenate(s1), np.concatenate(s2)) if s1 else np.zeros(0, np.uint8)
        at, nxt, bad_a, bad_b, n_bad = 0, [], [], [], 0
        for i, p in zip(pending, paths):
            if p is None:
                out[i] = (1, None, None, np.inf)
                continue
            m = len(p[0]) - 1
            v = ok[at:at + m]
            checked += [(p[1][j], p[1][j + 1], int(v[j])) for j in range(m)]
            at += m
            if v.all():
                out[i] = (0, p[0], p[1], p[2])
            else:
                n_bad += 1
                nxt.append(i)
                bad_a += [p[0][j] for j in np.flatnonzero(v == 0)]
                bad_b += [p[0][j + 1] for j in np.flatnonzero(v == 0)]
        if raw_bad is None:
            raw_bad = n_bad
        if bad_a:
            g.block_moves(bad_a, bad_b)
        pending = nxt
    return out, rounds, raw_bad, checked


def same_results(got, want):
    assert len(got) == len(want)
    for i, (p, q) in enumerate(zip(got, want)):
        assert p[0] == q[0], (i, p[0], q[0])
        assert np.float64(p[3]).view(np.uint64) == np.float64(q[3]).view(np.uint64), i
        if p[0] == 0:
            assert np.array_equal(p[1], q[1]) and np.array_equal(bits_of(p[2]), bits_of(q[2])), i
        else:
            assert p[1] is None and p[2] is None and np.isinf(p[3])


def plan_against_loop(ctx, amplitude, n_yaw, objective, reverse, form, condition, oracle=False, max_rounds=64):
    gm, mask, src, targets = world(ctx, amplitude, n_yaw)
    kw = dict(objective=objective, reverse=reverse, **form)
    with ctx.cost_field(mask, n_yaw, [src], **kw) as f, ctx.cost_field(mask, n_yaw, [src], **kw) as g:
        got = f.plan(targets, max_rounds)
        st = f.plan_stats()
        want, rounds, raw_bad, checked = loop_from_public_calls(ctx, g, targets, max_rounds)
        print(f"  {raw_bad} of 16 raw paths held a failing move; {st}")
        same_results(got, want)
        assert st["rounds"] == rounds and np.array_equal(f.blocked(), g.blocked())
        assert st["moves_blocked"] == f.blocked_count() == g.blocked_count()
        assert st["moves_checked"] == len(checked)
        assert len(st["round_tile_runs"]) == rounds and sum(st["round_tile_runs"]) == st["update_tile_runs"]
        assert sum(r > 0 for r in st["round_tile_runs"]) == (st["updates"] if not form.get("plain_sweeps") else 0)
        assert f.plan([]) == []
        assert np.array_equal(bits_of(f.dist()), bits_of(g.dist()))
        if condition:
            assert raw_bad >= 4 and rounds >= 2, (raw_bad, rounds)
        d = f.dist()
        for t, (status, nodes, se3, cost) in zip(targets, got):
            assert status in (0, 1)                                         # max_rounds are enough
            if status == 1:
                assert np.isinf(d[t])
                continue
            assert tup(nodes[-1 if not reverse else 0]) == t and tup(nodes[0 if not reverse else -1]) == src
            assert ctx.check_motions(se3[:-1], se3[1:]).all()               # every move of the path passes
            assert fold(f, nodes, reverse).view(np.uint64) == np.float64(cost).view(np.uint64) == d[t].view(np.uint64)
        # the field is the one a new field with the same set blocked in one call holds
        with ctx.cost_field(mask, n_yaw, [src], **kw) as fresh:
            words = f.blocked()
            own = np.argwhere(words != 0)
            moves = []
            for r, c, k in own:
                for j in range(10):
                    if (words[r, c, k] >> j) & 1:
                        nb = (r + LR.MOVES[j][0], c + LR.MOVES[j][1], k) if j < 8 else (r, c, (k + (1 if j == 8 else -1)) % n_yaw)
                        moves.append(((r, c, k), nb) if reverse else (nb, (r, c, k)))
            moves = list(dict.fromkeys((tup(x), tup(y)) for x, y in moves))      # 2 headings: slots 8 and 9 are one move
            if moves:
                a, b = split(moves)
                assert fresh.block_moves(a, b) == len(moves)
            assert np.array_equal(fresh.blocked(), words)
            tg = targets[::3]
            same(snapshot(f, tg, reverse), snapshot(fresh, tg, reverse), "a new field with the same set")
        if oracle:            # the verdicts of the blocked and of the accepted moves against the CPU oracle
            import oracle_py
            om, rob = oracle_py.OracleMap(gm), oracle_py.robot(ROBOT)
            uniq = {(a.tobytes(), b.tobytes()): v for a, b, v in checked}
            s1 = np.array([np.frombuffer(k[0], np.float64) for k in uniq])
            s2 = np.array([np.frombuffer(k[1], np.float64) for k in uniq])
            ref, _ = om.check_motions(rob, s1, s2)
            dev = np.array(list(uniq.values()), np.uint8)
            print(f"  {len(uniq)} distinct moves against the oracle: {int((dev == 0).sum())} failed")
            assert np.array_equal(ref != 0, dev != 0)
        return st


@pytest.mark.gpu
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("objective", [0, 1])
@pytest.mark.parametrize("amplitude", [0.25, 0.5])
def test_plan_equals_the_loop_of_its_parts_at_8_headings(ctx, amplitude, objective, reverse):
    forms = FORMS + ([dict(inner_sweeps=1)] if objective == int(reverse) else [])      # inner_sweeps 1 in four of the eight
    stats = [plan_against_loop(ctx, amplitude, 8, objective, reverse, form, condition=True,
                               oracle=(amplitude, objective, reverse) == (0.25, 1, True) and not form) for form in forms]
    for st in stats[1:]:                                                                # the forms walk the same rounds
        assert [st[k] for k in ("rounds", "moves_checked", "moves_blocked")] == \
            [stats[0][k] for k in ("rounds", "moves_checked", "moves_blocked")]


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_plan_equals_the_loop_of_its_parts_at_16_headings(ctx, form):
    plan_against_loop(ctx, 0.25, 16, 1, True, form, condition=False)


@pytest.mark.gpu
@pytest.mark.parametrize("n_yaw,form", [(2, dict()), (2, dict(plain_sweeps=True)), (32, dict())])
def test_plan_equals_the_loop_of_its_parts_at_2_and_32_headings(ctx, n_yaw, form):
    """No condition on the raw paths.  At 2 headings a rotation is a turn by pi on the spot, which fails on most cells of
    this terrain, and every round only removes the rotations the pending paths tried: the loop needs far more rounds than
    at 8 headings (each round blocks at least one move, so at most as many as the component has moves).  The cap is that
    bound's order, 4096; plan_against_loop asserts that no target ends with status 2 -- a failing rotation that stayed
    usable through its twin slot would make every round block nothing new, and would."""
    plan_against_loop(ctx, 0.25, n_yaw, 1, n_yaw == 2, form, condition=False, max_rounds=4096 if n_yaw == 2 else 64)


# ---- 5. limits and statuses -------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_one_round_at_a_time(ctx, form):
    gm, mask, src, targets = world(ctx, 0.25, 8)
    kw = dict(objective=1, reverse=True, **form)
    with ctx.cost_field(mask, 8, [src], **kw) as f, ctx.cost_field(mask, 8, [src], **kw) as g, \
            ctx.cost_field(mask, 8, [src], **kw) as h:
        full = g.plan(targets)
        first = f.plan(targets, max_rounds=1)
        assert f.plan_stats()["rounds"] == 1
        want, _, raw_bad, _ = loop_from_public_calls(ctx, h, targets, 1)
        same_results(first, want)
        assert sum(r[0] == 2 for r in first) == raw_bad >= 4
        assert np.array_equal(f.blocked(), h.blocked()) and f.blocked_count() > 0     # the blocks stay after status 2
        second = f.plan(targets)
        assert all(r[0] in (0, 1) for r in second)
        assert f.plan_stats()["rounds"] == g.plan_stats()["rounds"] - 1
        assert np.array_equal(f.blocked(), g.blocked()) and np.array_equal(bits_of(f.dist()), bits_of(g.dist()))
        for a, b in zip(second, full):
            assert a[0] == b[0] and np.float64(a[3]).view(np.uint64) == np.float64(b[3]).view(np.uint64)


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_statuses_capacity_and_refusals(ctx, form):
    n, n_yaw = 48, 4
    elev = np.zeros((96, 96), np.float32)
    device_map(ctx, elev, 0.04)
    rect = (24, 24, n, n)                          # the middle of a flat map: the robot stands on it at every node
    full = np.uint32((1 << n_yaw) - 1)
    mask = np.zeros((n, n), np.uint32)
    mask[20, 10:40] = full                         # one corridor, one cell wide: every move is the only way on
    src = (20, 12, 0)
    with ctx.cost_field(mask, n_yaw, [src], objective=1, rect=rect, **form) as f:
        d0 = f.dist()
        wall = [((20, 29, k), (20, 30, k)) for k in range(n_yaw)]
        a, b = split(wall)
        assert f.block_moves(a, b) == n_yaw
        targets = [(20, 35, 1), src, (5, 5, 0), (20, 25, 2)]       # behind the wall, a source, no node, reachable
        res = f.plan(targets)
        assert [r[0] for r in res] == [1, 0, 1, 0]
        assert len(res[1][1]) == 1 and tup(res[1][1][0]) == src and res[1][3] == 0.0 and res[1][2].shape == (1, 7)
        assert np.isinf(res[0][3]) and np.isinf(res[2][3])
        assert tup(res[3][1][-1]) == (20, 25, 2) and res[3][3] == d0[20, 25, 2]
        st = f.plan_stats()
        assert st["rounds"] == 1 and st["moves_blocked"] == 0 and st["moves_checked"] == len(res[3][1]) - 1
        # cap_states too small: the offsets say what is needed
        t = np.array(targets, np.int32)
        stt, cost, off = np.zeros(4, np.int32), np.zeros(4), np.zeros(5, np.uint64)
        nodes, se3 = np.zeros((4, 3), np.int32), np.zeros((4, 7))
        rc = f.L.artp_field_plan(f.h, t.ctypes.data, 4, 8, stt.ctypes.data, cost.ctypes.data, off.ctypes.data,
                                 nodes.ctypes.data, se3.ctypes.data, 4)
        assert rc == -5 and list(stt) == [1, 0, 1, 0]
        assert list(off) == [0, 0, 1, 1, 1 + len(res[3][1])] and cost[3] == res[3][3]
        # costs only
        assert f.L.artp_field_plan(f.h, t.ctypes.data, 4, 8, stt.ctypes.data, cost.ctypes.data, None, None, None, 0) == 0
        # refused: max_rounds < 1, a target outside the rectangle
        assert f.L.artp_field_plan(f.h, t.ctypes.data, 4, 0, stt.ctypes.data, cost.ctypes.data, None, None, None, 0) == -1
        with pytest.raises(_capi.ArtpError):
            f.plan([(20, n, 0)])
        # non-moves: refused with the field untouched, the good pairs in front of them included
        before, words = f.dist(), f.blocked()
        for bad in ([((20, 20, 0), (20, 22, 0))], [((20, 20, 0), (20, 20, 2))], [((20, 20, 0), (21, 21, 1))],
                    [((20, 20, 0), (20, 20, 0))], [((20, 20, 0), (20, 21, 0)), ((20, 47, 0), (20, 48, 0))],
                    [((-1, 20, 0), (0, 20, 0))], [((20, 20, 0), (20, 21, n_yaw))]):
            with pytest.raises(_capi.ArtpError):
                f.block_moves(*split(bad))
            assert np.array_equal(f.blocked(), words) and np.array_equal(bits_of(f.dist()), bits_of(before))
        with pytest.raises(_capi.ArtpError):
            f.unblock((0, 0, n + 1, 1))
        # a move whose edge does not exist in the mask: the bit is set, nothing else changes
        assert f.block_moves([(5, 5, 0)], [(5, 6, 0)]) == 1 and f.blocked_count() == n_yaw + 1
        assert np.array_equal(bits_of(f.dist()), bits_of(before))
        # after a layer update the poses are gone
        ctx.update_layer_rect(0, elev[:4, :4], 0, 0)
        with pytest.raises(_capi.ArtpError):
            f.plan(targets)
        a, b = split([((20, 15, k), (20, 16, k)) for k in range(n_yaw)])
        assert f.block_moves(a, b) == n_yaw                         # the set itself needs no poses
        assert np.isinf(f.dist()[20, 16:, :]).all() and np.isfinite(f.dist()[20, 10:16, :]).all()
