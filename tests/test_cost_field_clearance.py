"""Clearance-weighted cost-to-go fields (csrc/clearance.h, artp_field_compute_clearance).

The weight of every move is made OUTSIDE the code under test: the clearance map by tests/clearance_ref.py, the factor
1 + gain max(pen(a), pen(b)) restated in numpy float64, the base cost by tests/lattice_ref.py (for Dijkstra) or by the
device's own plain field (for the table, move by move).

Tolerances.  Table: pen carries about 4 roundings (sqrt, the product with res, the quotient, the difference), the factor 2
more, the product with the base 1; relative to a factor >= 1 that stays below gain * 3e-16, so with gain <= 100 every
weight agrees with base * factor to a relative 1e-13.  dist: section 12's relative 1e-9 (a few ulp per weight, one rounding
per hop, no path of 2^22 hops) holds with one more rounding per weight; the finite set exactly; the kernel forms and every
inner_sweeps bit for bit."""
import numpy as np
import pytest

import clearance_ref as CR
import lattice_learned_ref as LL
import lattice_ref as LR
from art_planner_amd import _capi
from synthetic import perlin_terrain
from test_clearance_ref import corridor
from test_cost_field import RTOL, assert_field, check_paths, device_map, lattice

pytestmark = pytest.mark.gpu

N, RES, POS = 96, 0.04, (0.5, -0.25)
RECT = (7, 5, 45, 38)        # odd sizes, not at the origin, no multiple of the tile: 3 x 3 tiles, the last ones padded
CLEAR = dict(radius_cells=5, margin=0.15, gain=3.0)
W_RTOL = 1e-13


class Setup:
    def __init__(self, ctx):
        self.ctx = ctx
        self.key = None
        self.gm = None

    def perlin(self):
        if self.key != "perlin":
            self.gm = device_map(self.ctx, perlin_terrain(N, RES, seed=11) * np.float32(0.2), RES, pos=POS)
            self.key = "perlin"
        return self.gm

    def flat(self, n):
        if self.key != ("flat", n):
            self.gm = device_map(self.ctx, np.zeros((n, n), np.float32), RES)
            self.key = ("flat", n)
        return self.gm


@pytest.fixture(scope="module")
def S():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from art_planner_amd.context import Context
    c = Context(0, "yaml")
    yield Setup(c)
    c.close()


def random_mask(shape, n_yaw, seed, p):
    bits = np.random.default_rng(seed).random(shape + (n_yaw,)) < p
    return (bits.astype(np.uint64) << np.arange(n_yaw, dtype=np.uint64)).sum(axis=2).astype(np.uint32)


def all_moves(shape):
    """(a, b, m): every move of every cell and heading of the rectangle, the target's triple possibly outside."""
    nr, nc, ny = shape
    idx = np.stack(np.meshgrid(np.arange(nr), np.arange(nc), np.arange(ny), indexing="ij"), -1).reshape(-1, 3)
    a, b, mm = [], [], []
    for m in range(10):
        t = idx.copy()
        if m < 8:
            t[:, 0] += LR.MOVES[m][0]
            t[:, 1] += LR.MOVES[m][1]
        else:
            t[:, 2] = (t[:, 2] + (1 if m == 8 else -1)) % ny
        a.append(idx)
        b.append(t)
        mm.append(np.full(len(idx), m))
    return np.concatenate(a), np.concatenate(b), np.concatenate(mm)


def bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


_cases = {}


def case(S, objective, n_yaw):
    """mask, source, reference d2 and the restated weights of one (objective, n_yaw) on the Perlin map; made once."""
    gm = S.perlin()
    key = (objective, n_yaw)
    if key not in _cases:
        mask = random_mask(RECT[2:], n_yaw, 40 + n_yaw, 0.97)
        base = lattice(S.ctx, gm, mask, n_yaw, RECT, objective)
        d2 = CR.clearance_map(mask, n_yaw, CLEAR["radius_cells"])
        w = CR.weights(base.w, d2, RES, CLEAR["margin"], CLEAR["gain"])
        lat = LL.LearnedLattice(mask, n_yaw, w)
        nodes = np.argwhere(lat.bits)
        src = tuple(int(v) for v in nodes[len(nodes) // 3])
        assert (w[np.isfinite(w)] > base.w[np.isfinite(w)]).any()
        _cases[key] = (mask, src, d2, base, lat, {})
    return _cases[key]


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("n_yaw", [1, 2, 7, 16, 32])
@pytest.mark.parametrize("objective", [0, 1])
def test_the_table_holds_the_restated_weights(S, objective, n_yaw, reverse):
    ctx = S.ctx
    mask, src, d2, base, lat, _ = case(S, objective, n_yaw)
    a, b, m = all_moves(lat.shape)
    kw = dict(rect=RECT, reverse=reverse, objective=objective)
    with ctx.clearance_cost_field(mask, n_yaw, [src], **CLEAR, **kw) as f, ctx.cost_field(mask, n_yaw, [src], **kw) as p:
        assert np.array_equal(f.clearance(), d2)
        got, plain = f.edge_costs(a, b), p.edge_costs(a, b)
        odd = f.edge_costs([(3, 3, 0)] * 2, [(3, 3, 0), (5, 3, 0)])      # no lattice move at all
    assert np.isnan(odd).all()
    nr, nc, _ = lat.shape
    inside = (b[:, 0] >= 0) & (b[:, 0] < nr) & (b[:, 1] >= 0) & (b[:, 1] < nc) & ((m < 8) | (n_yaw > 1))
    assert np.array_equal(np.isnan(got), ~inside) and np.array_equal(np.isnan(plain), ~inside)
    bi = b[inside]
    edge = np.zeros(len(a), bool)
    edge[inside] = lat.bits[a[inside, 0], a[inside, 1], a[inside, 2]] & lat.bits[bi[:, 0], bi[:, 1], bi[:, 2]]
    assert (got[inside & ~edge] == np.inf).all() and (inside & ~edge).any()          # a move that is not an edge
    fac = CR.factors(d2, RES, CLEAR["margin"], CLEAR["gain"])[m, a[:, 0], a[:, 1], a[:, 2]]
    want = plain[edge] * fac[edge]
    err = np.abs(got[edge] - want)
    worst = float((err / np.maximum(want, 1e-300)).max())
    print(f"  {int(edge.sum())} edges, {int((fac[edge] > 1).sum())} of them inflated, largest relative error {worst:.3e}")
    assert np.isfinite(got[edge]).all() and (err <= W_RTOL * want).all(), worst
    assert (fac[edge] > 1).sum() > edge.sum() // 20 and (fac[edge] == 1).sum() > edge.sum() // 20


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("n_yaw", [1, 2, 7, 16, 32])
@pytest.mark.parametrize("objective", [0, 1])
def test_dist_against_dijkstra_over_the_restated_weights(S, objective, n_yaw, reverse):
    ctx = S.ctx
    mask, src, d2, base, lat, refs = case(S, objective, n_yaw)
    if reverse not in refs:
        refs[reverse] = lat.dijkstra([src], reverse)[0]
    ref = refs[reverse]
    kw = dict(rect=RECT, reverse=reverse, objective=objective, **CLEAR)
    with ctx.clearance_cost_field(mask, n_yaw, [src], **kw) as f:
        d, st = f.dist(), f.stats()
        assert_field(d, ref)
        assert st["reached_nodes"] == int(np.isfinite(ref).sum()) and st["outer_rounds"] > 0 and st["plain_sweeps"] == 0
        rng = np.random.default_rng(n_yaw)
        fin = np.argwhere(np.isfinite(ref))
        targets = [tuple(int(v) for v in fin[i]) for i in rng.integers(0, len(fin), 6)] + [src]
        rest = np.argwhere(~np.isfinite(ref))
        targets += [tuple(int(v) for v in rest[i]) for i in rng.integers(0, len(rest), 2)]
        longest = check_paths(ctx, f, lat, d, mask, n_yaw, RECT, [src], reverse, targets)
        assert longest > 5
    with ctx.clearance_cost_field(mask, n_yaw, [src], plain_sweeps=True, **kw) as p:
        assert np.array_equal(bits(d), bits(p.dist()))
        assert p.stats()["plain_sweeps"] > 0 and p.stats()["outer_rounds"] == 0
    for sweeps in (1, 3):
        with ctx.clearance_cost_field(mask, n_yaw, [src], inner_sweeps=sweeps, **kw) as g:
            assert np.array_equal(bits(d), bits(g.dist())), sweeps


@pytest.mark.parametrize("objective", [0, 1])
def test_gain_zero_is_the_plain_field(S, objective):
    ctx = S.ctx
    for n_yaw in (1, 7, 32):
        mask, src, *_ = case(S, objective, n_yaw)
        for reverse in (False, True):
            kw = dict(rect=RECT, reverse=reverse, objective=objective)
            with ctx.clearance_cost_field(mask, n_yaw, [src], radius_cells=5, margin=0.15, gain=0.0, **kw) as f, \
                    ctx.cost_field(mask, n_yaw, [src], **kw) as p:
                assert np.array_equal(bits(f.dist()), bits(p.dist())), (n_yaw, reverse)
                assert f.stats()["reached_nodes"] == p.stats()["reached_nodes"] > 100


@pytest.mark.parametrize("objective", [0, 1])
def test_the_path_keeps_clear_of_the_walls(S, objective):
    """The L-shaped corridor of tests/test_clearance_ref.py, 7 cells wide.  On the reference (both objectives): the unweighted
    path has 48 states and touches d2 = 1, the weighted one 53 states along the centre line, d2 = 16."""
    ctx = S.ctx
    gm = S.flat(40)
    m, src, tgt = corridor()
    d2 = CR.clearance_map(m, 1, 5)
    base = lattice(ctx, gm, m, 1, None, objective)
    lat = LL.LearnedLattice(m, 1, CR.weights(base.w, d2, RES, 4 * RES, 4.0))
    ref0, ref1 = base.dijkstra([src])[0][tgt], lat.dijkstra([src])[0][tgt]
    with ctx.cost_field(m, 1, [src], objective=objective) as p, \
            ctx.clearance_cost_field(m, 1, [src], objective=objective, radius_cells=5, margin=4 * RES, gain=4.0) as f:
        n0, _, c0 = p.path(tgt)
        n1, _, c1 = f.path(tgt)
        assert np.array_equal(f.clearance(), d2)
    assert abs(c0 - ref0) <= RTOL * ref0 and abs(c1 - ref1) <= RTOL * ref1 and c1 > c0
    low0 = min(int(d2[tuple(v)]) for v in n0[3:-3])
    low1 = min(int(d2[tuple(v)]) for v in n1[3:-3])
    print(f"  unweighted: {len(n0)} states, min d2 {low0}; weighted: {len(n1)} states, min d2 {low1}")
    assert low0 <= 2
    assert low1 > low0


def test_block_and_unblock_on_a_clearance_field(S):
    ctx, objective, n_yaw = S.ctx, 1, 7
    mask, src, d2, base, lat, _ = case(S, objective, n_yaw)
    kw = dict(rect=RECT, objective=objective, **CLEAR)
    with ctx.clearance_cost_field(mask, n_yaw, [src], **kw) as f:
        first = f.dist()
        far = tuple(int(v) for v in np.argwhere(first == first[np.isfinite(first)].max())[0])
        nodes = [tuple(int(v) for v in nd) for nd in f.path(far)[0]]
        assert len(nodes) > 8
        a, b = nodes[len(nodes) // 2], nodes[len(nodes) // 2 + 1]          # a tight move: it carries a shortest path
        mv = lat.move_between(a, b)
        assert mv is not None and np.isfinite(lat.w[mv][a])
        assert f.block_moves([a], [b]) == 1 and f.blocked_count() == 1
        w = lat.w.copy()
        w[mv][a] = np.inf
        cut = LL.LearnedLattice(mask, n_yaw, w).dijkstra([src])[0]
        blocked = f.dist()
        assert_field(blocked, cut)
        assert not np.array_equal(bits(blocked), bits(first))
        assert f.edge_costs([a], [b])[0] == np.inf
        assert f.unblock() == 1 and f.blocked_count() == 0
        assert np.array_equal(bits(f.dist()), bits(first))
        assert np.array_equal(f.clearance(), d2)


def test_plan_on_a_clearance_field(S):
    from test_cost_field_plan import split, tup, world
    ctx, n_yaw = S.ctx, 8
    S.key = None                                     # world() installs its own map
    gm, mask, src, targets = world(ctx, 0.5, n_yaw)
    kw = dict(objective=1, yaw_spread=1)         # on this map one raw path of this field holds a move check_motions rejects
    with ctx.clearance_cost_field(mask, n_yaw, [src], **kw) as f:
        got = f.plan(targets)
        st = f.plan_stats()
        print(f"  {st}")
        done = 0
        for t, (status, nodes, se3, cost) in zip(targets, got):
            if status == 0:
                done += 1
                assert tup(nodes[-1]) == t and tup(nodes[0]) == src
                assert ctx.check_motions(se3[:-1], se3[1:]).all()
        print(f"  statuses {[r[0] for r in got]}")
        assert done >= 1 and st["moves_blocked"] >= 1 and st["rounds"] >= 2
        words = f.blocked()
        moves = []
        for r, c, k in np.argwhere(words != 0):
            for j in range(10):
                if (words[r, c, k] >> j) & 1:
                    nb = (r + LR.MOVES[j][0], c + LR.MOVES[j][1], k) if j < 8 else (r, c, (k + (1 if j == 8 else -1)) % n_yaw)
                    moves.append((tup(nb), (int(r), int(c), int(k))))
        assert len(moves) == st["moves_blocked"] == f.blocked_count()
        with ctx.clearance_cost_field(mask, n_yaw, [src], **kw) as fresh:
            if moves:
                a, b = split(moves)
                assert fresh.block_moves(a, b) == len(moves)
            assert np.array_equal(fresh.blocked(), words)
            assert np.array_equal(bits(fresh.dist()), bits(f.dist()))
            assert np.array_equal(fresh.clearance(), f.clearance())


def test_refusals(S):
    ctx = S.ctx
    mask, src, d2, *_ = case(S, 1, 7)
    kw = dict(rect=RECT, objective=1)

    def refused(call, status=-1):
        with pytest.raises(_capi.ArtpError) as e:
            call()
        assert e.value.status == status, e.value

    with ctx.clearance_cost_field(mask, 7, [src], **CLEAR, **kw) as f, ctx.cost_field(mask, 7, [src], **kw) as p:
        before = f.dist()
        edited = mask.copy()
        r0 = 30 if src[0] < 22 else 5                          # away from the source
        edited[r0:r0 + 4, 10:14] = 0
        refused(lambda: f.update(edited))
        refused(lambda: f.update_learned())
        refused(lambda: f.update_learned(edited))
        assert np.array_equal(bits(f.dist()), bits(before)) and np.array_equal(f.clearance(), d2)
        assert f.path(src)[2] == 0.0
        refused(lambda: p.clearance())
        assert p.update(edited)["changed_words"] > 0          # the plain field still takes the edit
    R = CLEAR["radius_cells"]
    for bad in (dict(margin=0.0), dict(margin=-0.1), dict(margin=np.inf), dict(margin=np.nan), dict(margin=R * RES * 1.001),
                dict(gain=-1.0), dict(gain=np.inf), dict(gain=np.nan), dict(radius_cells=0, margin=0.01),
                dict(radius_cells=33), dict(yaw_spread=-1), dict(yaw_spread=4), dict(objective=2), dict(objective=3),
                dict(max_lat_vel=0.0), dict(inner_sweeps=0)):
        refused(lambda: ctx.clearance_cost_field(mask, 7, [src], **{**CLEAR, **kw, **bad}))
    refused(lambda: ctx.clearance_cost_field(mask, 33, [src], **CLEAR, **kw))
    refused(lambda: ctx.clearance_cost_field(mask, 7, [(0, 0, 9)], **CLEAR, **kw))
    # the limits themselves are allowed, and the context is still usable
    with ctx.clearance_cost_field(mask, 7, [src], radius_cells=R, margin=R * RES * 0.999, gain=100.0, yaw_spread=3, **kw) as g:
        assert g.stats()["reached_nodes"] > 100
        assert np.array_equal(g.clearance(), CR.clearance_map(mask, 7, R, 3))
