"""Learned-cost fields (csrc/field.h, artp_field_compute_learned) against tests/lattice_learned_ref.py.

The weight of every move is made OUTSIDE the code under test: the EdgeMatrix rows from reachability_poses, the network's
answer from ctx.cost_query on those rows, MotionCostObjective's pricing restated in numpy float64.  The field's own table
must hold the same bits (edge_costs), so Dijkstra over the restated weights and the device differ by one rounding per hop
at the most: the finite set exactly, finite values to a relative 1e-9 (section 12's bound), the two kernel forms and every
inner_sweeps bit for bit.

The network's three outputs are clamped to >= 0 (energy, time) and [0, 1] (risk) and the call refuses negative weights,
so no parameter set reaches a NEGATIVE cost through the interface: the rule "a negative or NaN cost is no edge" is held
on the reference (tests/test_lattice_learned_ref.py) and, on the device, through the infeasible edges, which take the
same way to +inf.  Risk never exceeds 1, so risk_threshold = 1 keeps every edge."""
import os
import sys

import numpy as np
import pytest

import common

sys.path.insert(0, os.path.join(common.ROOT, "oracle"))
sys.path.insert(0, os.path.join(common.ROOT, "tools"))
import convert_weights as cw  # noqa: E402
import cost_exact_ref as R  # noqa: E402
import lattice_learned_ref as LL  # noqa: E402
import motion_cost_oracle as mo  # noqa: E402
from art_planner_amd import _capi  # noqa: E402
from synthetic import perlin_terrain  # noqa: E402
from test_cost_field import assert_field, check_paths, device_map, spiral_mask  # noqa: E402

pytestmark = pytest.mark.gpu

N, RES, POS = 96, 0.04, (0.5, -0.25)
WEIGHTS = dict(w_energy=0.5, w_time=1.0, w_risk=2.0, risk_threshold=1.0)
RECT = (7, 5, 45, 38)        # odd sizes, not at the origin, no multiple of the tile: 3 x 3 tiles, the last ones padded


def blob(net, kind):
    p = R.probe_params(net, kind) if kind != "real" else mo.random_params(0, R.shapes_of(net))
    return cw.to_blob(p)


class Setup:
    def __init__(self, ctx):
        self.ctx = ctx
        self.elev = perlin_terrain(N, RES, seed=11) * np.float32(0.2)
        self.gm = device_map(ctx, self.elev, RES, pos=POS)
        self.net = None
        self.cache = {}

    def install(self, net=1, kind="real"):
        """Load a network and run it on the map's heights (row index growing along world x, as the cost server stores it)."""
        if self.net == (net, kind):
            return
        self.ctx.cost_load_weights(blob(net, kind))
        self.ctx.cost_update_map(np.ascontiguousarray(self.elev[::-1, ::-1]), RES, N * RES, N * RES, *POS)
        self.net = (net, kind)

    def cost3(self, n_yaw, rect):
        """(the network's answer (10, nr, nc, n_yaw, 3) for every move, inside (10, nr, nc, n_yaw)) on the installed network."""
        key = (self.net, n_yaw, rect)
        if key not in self.cache:
            rows, inside = LL.edge_rows(self.ctx.reachability_poses(n_yaw, rect))
            c3 = self.ctx.cost_query(rows.reshape(-1, 6)).reshape(rows.shape[:-1] + (3,))
            self.cache[key] = (c3, inside)
        return self.cache[key]

    def lattice(self, mask, n_yaw, rect, **wts):
        c3, _ = self.cost3(n_yaw, rect)
        return LL.LearnedLattice(mask, n_yaw, LL.price(c3, **wts))


@pytest.fixture(scope="module")
def S():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from art_planner_amd.context import Context
    c = Context(0, "yaml")
    yield Setup(c)
    c.close()


def random_mask(shape, n_yaw, seed, p=0.7):
    bits = np.random.default_rng(seed).random(shape + (n_yaw,)) < p
    return (bits.astype(np.uint64) << np.arange(n_yaw, dtype=np.uint64)).sum(axis=2).astype(np.uint32)


def forms(ctx, mask, n_yaw, sources, ref, inner=(1, 3), **kw):
    """dist of the tiled form: against the reference, and bit for bit against the plain form and other inner_sweeps."""
    with ctx.learned_cost_field(mask, n_yaw, sources, **kw) as f:
        d, st = f.dist(), f.stats()
    assert_field(d, ref)
    assert st["reached_nodes"] == int(np.isfinite(ref).sum()) and st["outer_rounds"] > 0 and st["plain_sweeps"] == 0
    with ctx.learned_cost_field(mask, n_yaw, sources, plain_sweeps=True, **kw) as p:
        dp, sp = p.dist(), p.stats()
    assert np.array_equal(d.view(np.uint64), dp.view(np.uint64))
    assert sp["plain_sweeps"] > 0 and sp["outer_rounds"] == 0
    for sweeps in inner:
        with ctx.learned_cost_field(mask, n_yaw, sources, inner_sweeps=sweeps, **kw) as g:
            assert np.array_equal(d.view(np.uint64), g.dist().view(np.uint64)), sweeps
    print(f"  tiled: {st['outer_rounds']} rounds, {st['tile_launches']} tile runs; plain: {sp['plain_sweeps']} sweeps")
    return d


def all_moves(lat):
    """(a, b, m): every move of every cell and heading of the rectangle, the target's triple possibly outside."""
    nr, nc, ny = lat.shape
    idx = np.stack(np.meshgrid(np.arange(nr), np.arange(nc), np.arange(ny), indexing="ij"), -1).reshape(-1, 3)
    a, b, mm = [], [], []
    for m in range(10):
        t = idx.copy()
        if m < 8:
            t[:, 0] += LL.LR.MOVES[m][0]
            t[:, 1] += LL.LR.MOVES[m][1]
        else:
            t[:, 2] = (t[:, 2] + (1 if m == 8 else -1)) % ny
        a.append(idx)
        b.append(t)
        mm.append(np.full(len(idx), m))
    return np.concatenate(a), np.concatenate(b), np.concatenate(mm)


@pytest.mark.parametrize("net,kind", [(1, "real"), (2, "real"), (1, "positive")])
def test_edge_costs_are_the_restated_weights_bit_for_bit(S, net, kind):
    S.install(net, kind)
    ctx, n_yaw, rect = S.ctx, 7, (11, 30, 20, 23)
    mask = random_mask(rect[2:], n_yaw, 3, p=0.8)
    c3, inside = S.cost3(n_yaw, rect)
    thr = float(np.median(c3[..., 2][inside])) if kind == "real" else 1.0     # infeasible edges among them
    wts = dict(WEIGHTS, risk_threshold=thr)
    lat = LL.LearnedLattice(mask, n_yaw, LL.price(c3, **wts))
    a, b, m = all_moves(lat)
    want = lat.w[m, a[:, 0], a[:, 1], a[:, 2]]
    want[~inside[m, a[:, 0], a[:, 1], a[:, 2]]] = np.nan      # the target lies outside the rectangle: no lattice move
    assert np.isnan(want).any() and np.isinf(want).any() and np.isfinite(want).sum() > len(want) // 4
    src = tuple(int(v) for v in np.argwhere(lat.bits)[0])
    for reverse in (False, True):
        with ctx.learned_cost_field(mask, n_yaw, [src], rect=rect, reverse=reverse, **wts) as f:
            got = f.edge_costs(a, b)
            # no lattice move at all: the node itself, a cell two away, two headings away
            odd = f.edge_costs([(3, 3, 0)] * 3, [(3, 3, 0), (5, 3, 0), (3, 3, 2)])
        assert np.isnan(odd).all()
        assert np.array_equal(np.isnan(got), np.isnan(want))
        ok = ~np.isnan(want)
        bad = np.flatnonzero(got[ok].view(np.uint64) != want[ok].view(np.uint64))
        assert len(bad) == 0, (reverse, len(bad), a[ok][bad[:3]], m[ok][bad[:3]], got[ok][bad[:3]], want[ok][bad[:3]])


def test_the_weights_are_not_symmetric(S):
    S.install(1, "real")
    n_yaw = 7
    c3, inside = S.cost3(n_yaw, RECT)
    w = LL.price(c3, **WEIGHTS)
    nr, nc = RECT[2:]
    total = differ = rot = 0
    for m in range(10):
        if m < 8:
            a, b = LL.move_slices(nr, nc, m)
            wa, wb = w[m][a], w[7 - m][b]
        else:
            k2 = (np.arange(n_yaw) + (1 if m == 8 else -1)) % n_yaw
            wa, wb = w[m], w[17 - m][:, :, k2]
            rot += int((wa != wb).sum())
        total += wa.size
        differ += int((wa != wb).sum())
    print(f"  w(a -> b) != w(b -> a) on {differ} of {total} edges, {rot} of them rotations")
    assert differ * 10 > total and rot >= 1
    mask = random_mask(RECT[2:], n_yaw, 107)
    lat = LL.LearnedLattice(mask, n_yaw, w)
    label, sizes = lat.components()
    comp = np.argwhere(label == int(np.argmax(sizes)))
    src = tuple(int(v) for v in comp[len(comp) // 2])
    with S.ctx.learned_cost_field(mask, n_yaw, [src], rect=RECT, **WEIGHTS) as f, \
            S.ctx.learned_cost_field(mask, n_yaw, [src], rect=RECT, reverse=True, **WEIGHTS) as r:
        df, dr = f.dist(), r.dist()
    assert np.array_equal(np.isfinite(df), np.isfinite(dr))      # every edge has its opposite: the same component
    assert (df != dr)[np.isfinite(df)].any()


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("n_yaw", [1, 16])
def test_spiral_corridor(S, n_yaw, reverse):
    S.install(1, "real")
    mask, src = spiral_mask(N, n_yaw)
    lat = S.lattice(mask, n_yaw, None, **WEIGHTS)
    ref, hops = lat.dijkstra([src], reverse)
    assert np.isfinite(ref[..., 0][mask != 0]).all()
    far = tuple(int(v) for v in np.unravel_index(np.argmax(np.where(np.isfinite(ref), ref, -1.0)), ref.shape))
    print(f"n_yaw {n_yaw} reverse {reverse}: farthest node {far} at {hops[far]} hops, cost {ref[far]:.3f}")
    assert hops[far] >= 500
    d = forms(S.ctx, mask, n_yaw, [src], ref, reverse=reverse, **WEIGHTS)
    with S.ctx.learned_cost_field(mask, n_yaw, [src], reverse=reverse, **WEIGHTS) as f:
        assert f.stats()["outer_rounds"] > 50
        nodes = np.argwhere(np.isfinite(ref))
        pick = nodes[np.random.default_rng(5).integers(0, len(nodes), 10)]
        check_paths(S.ctx, f, lat, d, mask, n_yaw, None, [src], reverse, [far, src] + [tuple(t) for t in pick])


@pytest.mark.parametrize("n_yaw", [2, 7, 32])
def test_random_masks_two_sources_and_fifty_paths(S, n_yaw):
    S.install(2 if n_yaw == 7 else 1, "real")
    mask = random_mask(RECT[2:], n_yaw, 100 + n_yaw)
    lat = S.lattice(mask, n_yaw, RECT, **WEIGHTS)
    label, sizes = lat.components()
    comp = np.argwhere(label == int(np.argmax(sizes)))
    srcs = [tuple(int(v) for v in comp[len(comp) // 5]), tuple(int(v) for v in comp[4 * len(comp) // 5])]
    for reverse in (False, True):
        ref, _ = lat.dijkstra(srcs, reverse)
        assert np.array_equal(np.isfinite(ref), label == int(np.argmax(sizes)))
        d = forms(S.ctx, mask, n_yaw, srcs, ref, rect=RECT, reverse=reverse, **WEIGHTS)
        with S.ctx.learned_cost_field(mask, n_yaw, srcs, rect=RECT, reverse=reverse, **WEIGHTS) as f:
            rng = np.random.default_rng(7)
            reached, rest = np.argwhere(np.isfinite(ref)), np.argwhere(~np.isfinite(ref))
            targets = ([tuple(t) for t in reached[rng.integers(0, len(reached), 50)]] +
                       [tuple(t) for t in rest[rng.integers(0, len(rest), 4)]])
            check_paths(S.ctx, f, lat, d, mask, n_yaw, RECT, srcs, reverse, targets)


@pytest.mark.parametrize("reverse", [False, True])
def test_infeasible_edges_are_no_edges(S, reverse):
    S.install(1, "real")
    n_yaw = 7
    c3, inside = S.cost3(n_yaw, RECT)
    thr = float(np.float32(np.median(c3[..., 2][inside])))
    wts = dict(WEIGHTS, risk_threshold=thr)
    mask = random_mask(RECT[2:], n_yaw, 11, p=0.9)
    keep = LL.LearnedLattice(mask, n_yaw, LL.price(c3, **WEIGHTS))
    lat = LL.LearnedLattice(mask, n_yaw, LL.price(c3, **wts))
    gone = 1.0 - np.isfinite(lat.w).sum() / np.isfinite(keep.w).sum()
    print(f"  threshold {thr}: {gone:.3f} of the edges are infeasible")
    assert 0.3 <= gone <= 0.7
    src = tuple(int(v) for v in np.argwhere(lat.bits)[lat.bits.sum() // 2])
    ref, _ = lat.dijkstra([src], reverse)
    full, _ = keep.dijkstra([src], reverse)
    assert np.isfinite(ref).sum() > 1 and np.isfinite(ref).sum() < np.isfinite(full).sum()   # the pruning cuts nodes off
    d = forms(S.ctx, mask, n_yaw, [src], ref, rect=RECT, reverse=reverse, **wts)
    with S.ctx.learned_cost_field(mask, n_yaw, [src], rect=RECT, reverse=reverse, **wts) as f:
        nodes = np.argwhere(np.isfinite(full))
        pick = nodes[np.random.default_rng(3).integers(0, len(nodes), 20)]
        check_paths(S.ctx, f, lat, d, mask, n_yaw, RECT, [src], reverse, [tuple(t) for t in pick])


def test_zero_cost_edges(S):
    S.install(1, "real")
    n_yaw = 4
    zero = dict(w_energy=0.0, w_time=0.0, w_risk=0.0, risk_threshold=1.0)
    mask = random_mask(RECT[2:], n_yaw, 21, p=0.6)
    lat = S.lattice(mask, n_yaw, RECT, **zero)
    assert (lat.w[np.isfinite(lat.w)] == 0.0).all()
    label, sizes = lat.components()
    big = int(np.argmax(sizes))
    src = tuple(int(v) for v in np.argwhere(label == big)[sizes[big] // 2])
    for reverse in (False, True):
        depth = lat.bfs_depth([src], reverse)
        ref = np.where(label == big, 0.0, np.inf)
        d = forms(S.ctx, mask, n_yaw, [src], ref, rect=RECT, reverse=reverse, **zero)
        assert (d[label == big] == 0.0).all() and np.isinf(d[label != big]).all()
        with S.ctx.learned_cost_field(mask, n_yaw, [src], rect=RECT, reverse=reverse, **zero) as f:
            nodes = np.argwhere(label == big)
            deepest = tuple(int(v) for v in np.unravel_index(np.argmax(depth), depth.shape))
            pick = [deepest] + [tuple(t) for t in nodes[np.random.default_rng(9).integers(0, len(nodes), 30)]]
            for t in pick:                                  # every descent ends, after exactly the BFS depth
                assert len(f.path(t)[0]) - 1 == depth[t], t
            check_paths(S.ctx, f, lat, d, mask, n_yaw, RECT, [src], reverse, pick[:5])


def test_an_external_query_function_does_not_reach_the_field(S):
    S.install(1, "real")
    n_yaw = 4
    mask = random_mask(RECT[2:], n_yaw, 31)
    lat = S.lattice(mask, n_yaw, RECT, **WEIGHTS)
    a, b, _ = all_moves(lat)
    src = tuple(int(v) for v in np.argwhere(lat.bits)[0])
    with S.ctx.learned_cost_field(mask, n_yaw, [src], rect=RECT, **WEIGHTS) as f:
        before, d0 = f.edge_costs(a, b), f.dist()
    calls = []

    def fn(edges):
        calls.append(len(edges))
        return np.full((len(edges), 3), 0.25, np.float32)
    S.ctx.cost_set_external_query(fn)
    try:
        with S.ctx.learned_cost_field(mask, n_yaw, [src], rect=RECT, **WEIGHTS) as f:
            after, d1 = f.edge_costs(a, b), f.dist()
    finally:
        S.ctx.cost_set_external_query(None)
    assert not calls
    assert np.array_equal(before.view(np.uint64), after.view(np.uint64))
    assert np.array_equal(d0.view(np.uint64), d1.view(np.uint64))


def test_refusals_leave_the_context_usable(S):
    from art_planner_amd.context import Context
    ctx = S.ctx
    ones = np.ones((10, 10), np.uint32)
    fresh = Context(0, "yaml")
    fresh._grid = (10, 10)   # as if a map were installed: the library itself must refuse
    with pytest.raises(_capi.ArtpError) as e:
        fresh.learned_cost_field(ones, 1, [(0, 0, 0)])
    assert e.value.status == -6   # ARTP_ERR_NO_WEIGHTS
    fresh.cost_load_weights(blob(1, "real"))
    with pytest.raises(_capi.ArtpError) as e:
        fresh.learned_cost_field(ones, 1, [(0, 0, 0)])
    assert e.value.status == -4   # ARTP_ERR_NO_MAP: no feature map
    fresh.cost_update_map(np.ascontiguousarray(S.elev), RES, N * RES, N * RES)
    with pytest.raises(_capi.ArtpError) as e:
        fresh.learned_cost_field(ones, 1, [(0, 0, 0)])
    assert e.value.status == -4   # ARTP_ERR_NO_MAP: no sampler layers
    fresh.close()

    S.install(1, "real")
    mask = np.full((N, N), 0xf, np.uint32)
    mask[3, 4] = 0b0101

    def still_usable():
        with ctx.cost_field(mask, 4, [(3, 4, 2)], objective=1) as f:
            assert f.dist()[3, 4, 2] == 0.0 and f.stats()["reached_nodes"] > N * N

    bad = [dict(w_energy=-1.0), dict(w_risk=-0.0001), dict(risk_threshold=float("nan")), dict(w_time=float("inf")),
           dict(sources=[(3, 4, 1)]), dict(sources=[(N, 0, 0)]), dict(sources=[(0, 0, 4)]), dict(inner_sweeps=0)]
    for kw in bad:
        args = dict(sources=[(1, 1, 0)])
        args.update(kw)
        with pytest.raises(_capi.ArtpError) as e:
            ctx.learned_cost_field(mask, 4, args.pop("sources"), **args)
        assert e.value.status == -1, kw   # ARTP_ERR_INVALID_ARG
        still_usable()
    for n_yaw, rect in [(0, None), (33, None), (4, (0, 0, 0, 5)), (4, (90, 0, 10, 10))]:
        shape = (N, N) if rect is None else (max(rect[2], 0), max(rect[3], 0))
        with pytest.raises(_capi.ArtpError) as e:
            ctx.learned_cost_field(np.ones(shape, np.uint32), n_yaw, [(0, 0, 0)], rect=rect)
        assert e.value.status == -1, (n_yaw, rect)
    still_usable()
    with pytest.raises(_capi.ArtpError) as e:
        ctx.cost_field(mask, 4, [(1, 1, 0)], objective=2)
    assert e.value.status == -1
    still_usable()
    small = np.full((20, 20), 0xf, np.uint32)
    with ctx.learned_cost_field(small, 4, [(1, 1, 0)], rect=(0, 0, 20, 20), **WEIGHTS) as f:
        d = f.dist()
        with pytest.raises(_capi.ArtpError) as e:
            f.update(small)
        assert e.value.status == -1
        assert np.array_equal(f.dist().view(np.uint64), d.view(np.uint64))     # untouched
        ls = f.learned_stats()
        assert ls["table_bytes"] == 8 * ls["table_rows"] == 8 * 4 * 4 * 10 * 256 and ls["chunks"] == 1
    still_usable()
