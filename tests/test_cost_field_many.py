"""Many cost-to-go fields in one batched search and pose-to-pose cost matrices (csrc/field_many.h, the many-kernel of
csrc/field.h, include/artp_c.h artp_field_compute_many / artp_field_cost_matrix).

The batch runs the tile body of the single field on a grid of (tiles, fields); the least fixed point of a field is unique,
so field b of a batch must hold the BITS of cost_field on set b alone: dist, the hop counts (seen through path()), the
edge costs and reached_nodes.  "Bit for bit" compares uint64 views.  Against tests/lattice_ref.py the tolerance is the
suite's RTOL of test_cost_field.py, for the reasons given there.

Shapes: 45 x 37 cells are 3 x 3 tiles with padded edge tiles; the 96 x 96 spiral is the smallest case where one field of
a batch is finished (after its first round) while another runs for some sixty more, so that a write into a finished field
would show; 32 headings need the many-kernel's own opt-in for more than 64 KB of LDS."""
import ctypes as C

import numpy as np
import pytest

from art_planner_amd import _capi
from synthetic import perlin_terrain
from test_cost_field import ROBOT, RTOL, assert_field, device_map, lattice

N_YAW = 7
RECT = (7, 5, 45, 37)
ISLAND = (22, 30, 4)          # a node of the random mask all of whose neighbours are missing


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def tup(x):
    return tuple(int(v) for v in x)


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
def random_mask(nrows, ncols, n_yaw, seed, island=None):
    rng = np.random.default_rng(seed)
    b = rng.random((nrows, ncols, n_yaw)) < 0.7
    mask = (b.astype(np.uint64) << np.arange(n_yaw, dtype=np.uint64)).sum(axis=2).astype(np.uint32)
    if island is not None:
        r, c, k = island
        mask[r - 1:r + 2, c - 1:c + 2] = 0
        mask[r, c] = 1 << k
    return mask


def perlin_world(ctx):
    """The map, the odd rectangle and the random mask (with its island) that most cases share."""
    elev = np.ascontiguousarray(perlin_terrain(83, 0.05, seed=21)[:, :71]) * np.float32(0.8)
    gm = device_map(ctx, elev, 0.05, pos=(0.3, 0.7))
    return gm, random_mask(RECT[2], RECT[3], N_YAW, 1234, ISLAND)


def big_component(lat, n):
    """n nodes spread over the largest component of the lattice."""
    label, sizes = lat.components()
    comp = np.argwhere(label == int(np.argmax(sizes)))
    assert len(comp) * 2 >= int((label >= 0).sum())
    return [tup(comp[(2 * i + 1) * len(comp) // (2 * n)]) for i in range(n)]


def targets_of(dist, seed, n=10):
    """n - 2 reachable nodes and two that are not."""
    rng = np.random.default_rng(seed)
    fin, rest = np.argwhere(np.isfinite(dist)), np.argwhere(~np.isfinite(dist))
    t = [tup(x) for x in fin[rng.integers(0, len(fin), n - 2)]]
    return t + [tup(x) for x in rest[rng.integers(0, len(rest), 2)]]


def same_field(got, want, targets, edge_costs=False):
    """got holds want's bits: dist, reached_nodes, and every path (so the hop counts that choose it)."""
    d, w = got.dist(), want.dist()
    assert np.array_equal(bits(d), bits(w)), int((bits(d) != bits(w)).sum())
    assert got.stats()["reached_nodes"] == want.stats()["reached_nodes"] == int(np.isfinite(w).sum())
    for t in targets:
        p, q = got.path(t), want.path(t)
        assert (p is None) == (q is None) == (not np.isfinite(w[t])), t
        if p is None:
            continue
        assert np.array_equal(p[0], q[0]) and np.array_equal(bits(p[1]), bits(q[1])), t
        assert np.float64(p[2]).view(np.uint64) == np.float64(q[2]).view(np.uint64) == w[t].view(np.uint64)
        if edge_costs and len(p[0]) > 1:
            assert np.array_equal(bits(got.edge_costs(p[0][:-1], p[0][1:])), bits(want.edge_costs(p[0][:-1], p[0][1:])))
    return w


def close_all(fields):
    for f in fields:
        f.close()


def spiral_mask(n, n_yaw):
    """test_cost_field.py's spiral: a 3-cell corridor between 1-cell walls, square rings of pitch 4, each cut once and
    opened to the next ring on alternating sides of the cut: the only way inwards runs the whole length of every ring."""
    m = np.zeros((n, n), np.uint32)
    full = np.uint32((1 << n_yaw) - 1)
    mid = n // 2
    rings = 0
    for i in range(n // 8):
        o = 4 * i
        if n - 2 * o < 14:
            break
        rings += 1
        ring = np.zeros((n, n), bool)
        ring[o:n - o, o:n - o] = True
        ring[o + 3:n - o - 3, o + 3:n - o - 3] = False
        m[ring] = full
        m[o:o + 3, mid] = 0
    for i in range(rings - 1):
        if i % 2 == 0:
            m[4 * i + 3, mid - 3:mid] = full
        else:
            m[4 * i + 3, mid + 1:mid + 4] = full
    return m, (1, mid + 2, 0)


# ---- CPU: the C ABI without a device ------------------------------------------------------------------------------
def test_many_entry_points_are_declared_exported_and_refuse_a_null_context():
    import common
    header = open(common.ROOT + "/include/artp_c.h").read()
    L = _capi.load()
    for name in ("artp_field_compute_many", "artp_field_cost_matrix"):
        assert name in _capi.SYMBOLS and "int " + name + "(" in header
        assert getattr(L, name) is not None
    p = _capi.FieldParams()
    L.artp_field_params_defaults(C.byref(p))
    mask, src = np.ones(4, np.uint32), np.zeros(3, np.int32)
    off = np.array([0, 1], np.uint64)
    handles = (C.c_void_p * 1)()
    handles[0] = 1234
    assert L.artp_field_compute_many(None, C.byref(p), 1, None, mask.ctypes.data, 0, src.ctypes.data, off.ctypes.data, 1, 0,
                                     handles) == -1
    assert not handles[0]                       # no handle is given out
    out = np.zeros(1)
    st = _capi.FieldManyStats(1, 2, 3, 4, 5, 6)
    assert L.artp_field_cost_matrix(None, C.byref(p), 1, None, mask.ctypes.data, 0, src.ctypes.data, 1, 0, out.ctypes.data,
                                    C.byref(st)) == -1
    assert (st.groups, st.fields, st.dist_rounds, st.hop_rounds, st.tile_runs, st.hop_tile_runs) == (0,) * 6


def test_many_stats_layout_matches_the_header():
    import re
    import common
    header = open(common.ROOT + "/include/artp_c.h").read()
    body = re.search(r"typedef struct artp_field_many_stats_t \{(.*?)\} artp_field_many_stats_t;", header, re.S).group(1)
    members = re.findall(r"uint64_t (\w+);", body)
    assert members == [n for n, _ in _capi.FieldManyStats._fields_]
    assert all(t is C.c_uint64 for _, t in _capi.FieldManyStats._fields_)
    assert C.sizeof(_capi.FieldManyStats) == 8 * len(members)
    assert len(re.findall(r"\w+;", body)) == len(members)        # nothing but these members


# ---- GPU -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_one_set_is_a_plain_field(ctx):
    gm, mask = perlin_world(ctx)
    lat = lattice(ctx, gm, mask, N_YAW, RECT, 1)
    src = big_component(lat, 1)
    kw = dict(rect=RECT, objective=1)
    many = ctx.cost_fields(mask, N_YAW, [src], **kw)
    assert len(many) == 1
    with ctx.cost_field(mask, N_YAW, src, **kw) as single, many[0] as f:
        d = same_field(f, single, targets_of(single.dist(), 3) + src, edge_costs=True)
        assert d[src[0]] == 0.0
        st, ss = f.stats(), single.stats()
        assert (st["nodes"], st["tiles"], st["plain_sweeps"]) == (ss["nodes"], ss["tiles"], 0) and st["tiles"] == 9
        assert st["outer_rounds"] >= 1 and st["hop_rounds"] >= 1 and st["tile_launches"] >= 1


@pytest.mark.gpu
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("objective", [0, 1])
def test_random_masks_in_an_odd_rectangle(ctx, objective, reverse):
    gm, mask = perlin_world(ctx)
    lat = lattice(ctx, gm, mask, N_YAW, RECT, objective)
    s = big_component(lat, 6)
    sets = [[s[0]], [s[1], s[2]], [s[3]], [s[3]], [s[4], s[5], s[0]]]      # unequal sizes, two sets identical
    kw = dict(rect=RECT, objective=objective, reverse=reverse)
    many = ctx.cost_fields(mask, N_YAW, sets, **kw)
    try:
        assert len(many) == len(sets)
        for b, (f, srcs) in enumerate(zip(many, sets)):
            ref, _ = lat.dijkstra(srcs, reverse)
            with ctx.cost_field(mask, N_YAW, srcs, **kw) as single:
                d = same_field(f, single, targets_of(ref, 10 + b))
            assert_field(d, ref)                                     # finite set exact, no node left out
            assert np.isinf(d[ISLAND]) and all(d[t] == 0.0 for t in srcs)
        assert np.array_equal(bits(many[2].dist()), bits(many[3].dist()))
        assert not np.array_equal(bits(many[0].dist()), bits(many[2].dist()))
    finally:
        close_all(many)


@pytest.mark.gpu
def test_fields_that_finish_far_apart(ctx):
    n, n_yaw = 96, 8
    device_map(ctx, perlin_terrain(n, 0.04, seed=11) * np.float32(0.5), 0.04, pos=(0.5, -0.25))
    mask, src = spiral_mask(n, n_yaw)
    island = (n // 2, n // 2, 3)
    assert not mask[island[0] - 1:island[0] + 2, island[1] - 1:island[1] + 2].any()      # the empty middle of the spiral
    mask[island[0], island[1]] = 1 << island[2]
    with ctx.cost_field(mask, n_yaw, [src], objective=1) as f:
        d = f.dist()
    fin = np.isfinite(d)
    far = tup(np.unravel_index(np.argmax(np.where(fin, d, -1.0)), d.shape))
    middle = tup(np.unravel_index(np.argmin(np.where(fin, np.abs(d - 0.5 * d[far]), np.inf)), d.shape))
    sets = [[far], [middle], [island]]
    many = ctx.cost_fields(mask, n_yaw, sets, objective=1)
    try:
        rounds = [f.stats()["outer_rounds"] for f in many]
        hop_rounds = [f.stats()["hop_rounds"] for f in many]
        print(f"  far {far} middle {middle}: distance rounds {rounds}, hop rounds {hop_rounds}")
        di = many[2].dist()
        assert many[2].stats()["reached_nodes"] == 1 == int(np.isfinite(di).sum()) and di[island] == 0.0
        assert rounds[2] == 1 and hop_rounds[2] == 1                  # quiet after its first round
        assert many[2].stats()["tile_launches"] >= 1
        batch_rounds = max(rounds)                                    # the loop ends with the last field
        assert all(r <= batch_rounds for r in rounds) and rounds[2] == min(rounds) and rounds[2] < min(rounds[:2])
        assert rounds[0] > 50                                         # the whole corridor, as in test_cost_field.py
        for f, srcs, seed in ((many[0], sets[0], 1), (many[1], sets[1], 2)):
            with ctx.cost_field(mask, n_yaw, srcs, objective=1) as single:
                w = same_field(f, single, targets_of(d, seed, 6) + [src, far])
            assert np.isinf(w[island]) and int(np.isfinite(w).sum()) == int(fin.sum())
    finally:
        close_all(many)


@pytest.mark.gpu
def test_32_headings_use_the_many_kernels_own_lds_opt_in(ctx):
    n_yaw, rect = 32, (3, 2, 33, 20)
    elev = np.ascontiguousarray(perlin_terrain(83, 0.05, seed=21)[:, :71]) * np.float32(0.8)
    gm = device_map(ctx, elev, 0.05, pos=(0.3, 0.7))
    mask = random_mask(rect[2], rect[3], n_yaw, 77)
    for objective in (0, 1):
        lat = lattice(ctx, gm, mask, n_yaw, rect, objective)
        s = big_component(lat, 4)
        sets = [[s[0]], [s[1], s[2]], [s[3]]]
        kw = dict(rect=rect, objective=objective)
        many = ctx.cost_fields(mask, n_yaw, sets, **kw)
        try:
            for b, (f, srcs) in enumerate(zip(many, sets)):
                with ctx.cost_field(mask, n_yaw, srcs, **kw) as single:
                    d = same_field(f, single, targets_of(single.dist(), 20 + b))
                assert int(np.isfinite(d).sum()) > mask.size * n_yaw // 3
        finally:
            close_all(many)


@pytest.mark.gpu
def test_fields_of_a_batch_are_independent_afterwards(ctx):
    gm, mask = perlin_world(ctx)
    lat = lattice(ctx, gm, mask, N_YAW, RECT, 1)
    s = big_component(lat, 3)
    kw = dict(rect=RECT, objective=1)
    many = ctx.cost_fields(mask, N_YAW, [[s[0]], [s[1]], [s[2]]], **kw)
    try:
        before = [f.dist() for f in many]
        # update() of the first on an edited mask: a new field on that mask, and the others keep their bits
        edited = mask.copy()
        edited[10:20, 8:14] = 0
        for t in s:
            edited[t[0], t[1]] = mask[t[0], t[1]]
        assert (edited != mask).sum() > 20
        many[0].update(edited)
        with ctx.cost_field(edited, N_YAW, [s[0]], **kw) as fresh:
            d0 = same_field(many[0], fresh, targets_of(fresh.dist(), 5))
        assert not np.array_equal(bits(d0), bits(before[0]))
        assert np.array_equal(bits(many[1].dist()), bits(before[1])) and np.array_equal(bits(many[2].dist()), bits(before[2]))
        # block_moves on the second, then plan() on it
        target = tup(np.unravel_index(np.argmax(np.where(np.isfinite(before[1]), before[1], -1.0)), before[1].shape))
        nodes = many[1].path(target)[0]
        assert len(nodes) > 4
        assert many[1].block_moves([nodes[1]], [nodes[2]]) == 1
        with ctx.cost_field(mask, N_YAW, [s[1]], **kw) as fresh:
            assert fresh.block_moves([nodes[1]], [nodes[2]]) == 1
            same_field(many[1], fresh, targets_of(before[1], 6) + [target])
            got, want = many[1].plan([target, s[1]]), fresh.plan([target, s[1]])
            assert [g[0] for g in got] == [w[0] for w in want]
            assert np.array_equal(bits(many[1].dist()), bits(fresh.dist()))
            assert many[1].blocked_count() == fresh.blocked_count() >= 1
        assert np.array_equal(bits(many[2].dist()), bits(before[2]))
        # close() the first: the others still answer
        many[0].close()
        assert many[0].h is None
        assert np.array_equal(bits(many[2].dist()), bits(before[2]))
        assert many[2].path(s[2])[2] == 0.0 and many[1].path(s[1])[2] == 0.0
        with ctx.cost_field(mask, N_YAW, [s[2]], **kw) as single:
            same_field(many[2], single, targets_of(before[2], 7))
    finally:
        close_all(many)


@pytest.mark.gpu
def test_refusals_leak_nothing_and_leave_the_context_usable(ctx):
    import torch
    n, n_yaw = 128, 16
    gm = device_map(ctx, perlin_terrain(n, 0.05, seed=5) * np.float32(0.4), 0.05)
    mask = np.full((n, n), (1 << n_yaw) - 1, np.uint32)
    mask[3, 4] = 0b0101
    good = (1, 1, 0)
    many = ctx.cost_fields(mask, n_yaw, [[good], [(5, 5, 1)], [(9, 9, 2)]])      # every lazy allocation made once
    close_all(many)
    torch.cuda.synchronize()
    free_before = torch.cuda.mem_get_info()[0]
    bad = [dict(sources_list=[[good], [(2, 2, 2)], [(7, 7, 0), (3, 4, 1)]]),         # a bad source in set 2 of 3
           dict(sources_list=[]),                                                      # zero sets
           dict(sources_list=[[good], [], [(2, 2, 2)]]),                               # an empty set
           dict(plain_sweeps=True), dict(objective=2)]
    for i, kw in enumerate(bad):
        args = dict(sources_list=[[good], [(2, 2, 2)]])
        args.update(kw)
        with pytest.raises(_capi.ArtpError) as e:
            ctx.cost_fields(mask, n_yaw, args.pop("sources_list"), **args)
        assert e.value.status == -1, kw                                                # ARTP_ERR_INVALID_ARG
        if i == 0:
            assert "set 2" in str(e.value), str(e.value)
    # offsets that decrease: only the C ABI can say that
    p = _capi.FieldParams()
    ctx.L.artp_field_params_defaults(C.byref(p))
    p.objective = 1
    src = np.array([good, (2, 2, 2), (5, 5, 1)], np.int32)
    keep = np.asfortranarray(mask)
    handles = (C.c_void_p * 2)()
    for off in ([0, 2, 1], [0, 3, 3], [1, 2, 3]):
        o = np.array(off, np.uint64)
        handles[0] = handles[1] = 99
        rc = ctx.L.artp_field_compute_many(ctx.h, C.byref(p), n_yaw, None, keep.ctypes.data, 0, src.ctypes.data, o.ctypes.data,
                                           2, 0, handles)
        assert rc == -1 and not handles[0] and not handles[1], off
        assert ctx.L.artp_last_error(ctx.h)
    with pytest.raises(_capi.ArtpError) as e:
        ctx.cost_matrix(mask, n_yaw, [good, (3, 4, 1), (2, 2, 2)])
    assert e.value.status == -1 and "pose 1" in str(e.value)
    # Nothing leaked.  The three fields of the first refusal hold 3 * 128 * 128 * 16 * 12 bytes = 9.4 MB of dist and hops
    # alone, one of them 3.1 MB; the runtime hands device memory out in pages of at most 2 MiB, so free memory returns to
    # within one such page of where it was.
    torch.cuda.synchronize()
    free_after = torch.cuda.mem_get_info()[0]
    print(f"  free memory before {free_before} after {free_after} ({free_after - free_before:+d} bytes)")
    assert abs(free_after - free_before) <= 2 << 20
    # a cost_field on the same context afterwards is correct
    rect = (0, 0, 45, 37)
    sub = random_mask(rect[2], rect[3], n_yaw, 9)
    lat = lattice(ctx, gm, sub, n_yaw, rect, 1)
    s = big_component(lat, 1)
    ref, _ = lat.dijkstra(s, False)
    with ctx.cost_field(sub, n_yaw, s, rect=rect, objective=1) as f:
        assert_field(f.dist(), ref)


@pytest.mark.gpu
def test_cost_matrix(ctx):
    gm, mask = perlin_world(ctx)
    lat = lattice(ctx, gm, mask, N_YAW, RECT, 1)
    poses = big_component(lat, 5)
    poses.insert(2, ISLAND)
    n = len(poses)
    kw = dict(rect=RECT, objective=1)
    m, st = ctx.cost_matrix(mask, N_YAW, poses, return_stats=True, **kw)
    assert m.shape == (n, n) and m.dtype == np.float64
    assert (st["groups"], st["fields"]) == (1, n) and st["dist_rounds"] >= 1 and st["hop_rounds"] >= 1
    assert st["tile_runs"] >= n and st["hop_tile_runs"] >= n
    want, ref = np.empty((n, n)), np.empty((n, n))
    for i, p in enumerate(poses):
        with ctx.cost_field(mask, N_YAW, [p], **kw) as f:
            d = f.dist()
        r, _ = lat.dijkstra([p], False)
        want[i] = [d[q] for q in poses]
        ref[i] = [r[q] for q in poses]
    assert np.array_equal(bits(m), bits(want))
    off = ~np.eye(n, dtype=bool)
    assert (np.diag(m) == 0.0).all()
    assert np.isposinf(m[2][off[2]]).all() and np.isposinf(m[:, 2][off[:, 2]]).all()
    rest = [i for i in range(n) if i != 2]
    assert np.isfinite(m[np.ix_(rest, rest)]).all() and (m[np.ix_(rest, rest)][~np.eye(n - 1, dtype=bool)] > 0).all()
    assert np.array_equal(np.isfinite(m), np.isfinite(ref))
    fin = np.isfinite(ref)
    assert (np.abs(m[fin] - ref[fin]) <= RTOL * np.abs(ref[fin])).all()
    # groups of 4 and 2: the same bits
    m4, st4 = ctx.cost_matrix(mask, N_YAW, poses, batch=4, return_stats=True, **kw)
    assert np.array_equal(bits(m4), bits(m)) and (st4["groups"], st4["fields"]) == (2, n)
    assert np.array_equal(bits(ctx.cost_matrix(mask, N_YAW, poses, 1, **kw)), bits(m))


@pytest.mark.gpu
def test_a_batch_on_lane_1_gives_the_bits_of_lane_0(ctx):
    gm, mask = perlin_world(ctx)
    lat = lattice(ctx, gm, mask, N_YAW, RECT, 1)
    s = big_component(lat, 6)
    sets = [[s[0]], [s[1], s[2]], [s[3]], [s[3]], [s[4], s[5], s[0]]]
    kw = dict(rect=RECT, objective=1)
    opened = []                                   # closed on every way out: a field must not outlive its context
    try:
        ctx.set_lane(2)
        live = ctx.cost_field(mask, N_YAW, [s[5]], **kw)
        opened.append(live)
        live_d = live.dist()
        ctx.set_lane(0)
        base = ctx.cost_fields(mask, N_YAW, sets, **kw)
        opened += base
        ctx.set_lane(1)
        other = ctx.cost_fields(mask, N_YAW, sets, **kw)
        opened += other
        assert ctx.lane == 1
        for b, (f, g) in enumerate(zip(other, base)):
            same_field(f, g, targets_of(live_d, 30 + b))
        m1 = ctx.cost_matrix(mask, N_YAW, s, **kw)
        ctx.set_lane(0)
        assert np.array_equal(bits(m1), bits(ctx.cost_matrix(mask, N_YAW, s, **kw)))
        close_all(other)
        close_all(base)
        ctx.set_lane(2)
        assert np.array_equal(bits(live.dist()), bits(live_d))
        with ctx.cost_field(mask, N_YAW, [s[5]], **kw) as again:
            same_field(live, again, targets_of(live_d, 40))
    finally:
        close_all(opened)
        ctx.set_lane(0)
