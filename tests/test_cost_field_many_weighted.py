"""Batched learned and clearance-weighted cost fields on one weight table, and their pose-to-pose matrices
(csrc/field_many.h, csrc/clearance.h, field_tile_many_kernel<PHASE, LEARNED> of csrc/field.h, include/artp_c.h
artp_field_compute_many_learned / _clearance and artp_field_cost_matrix_learned / _clearance).

The table of a batch is priced once, by the single field's own build, and the least fixed point of a field is unique:
field b of a batch must hold the BITS of learned_cost_field / clearance_cost_field on set b alone -- dist, the hop counts
(seen through path()), the edge costs, reached_nodes and clearance().  "Bit for bit" compares uint64 views.  Against
Dijkstra over the restated weights (tests/lattice_learned_ref.py) the bound is the suite's: the finite set exactly, values
to a relative 1e-9 (one rounding per hop).

Shapes are those of the single-field files: the 45 x 38 rectangle at 7 headings is 3 x 3 tiles with padded edge tiles,
whose lanes read the table's padding; the 96 x 96 spiral is the
smallest case where one field of a batch is finished after its first round while the others run for more than fifty; 32
headings need the new kernel's own opt-in for more than 64 KB of LDS."""
import ctypes as C
import re

import numpy as np
import pytest

from art_planner_amd import _capi
from test_cost_field import assert_field, device_map
from test_cost_field_clearance import CLEAR
from test_cost_field_clearance import RECT as C_RECT
from test_cost_field_clearance import Setup as ClearanceSetup
from test_cost_field_clearance import case
from test_cost_field_learned import LL, N, POS, RECT, RES, WEIGHTS
from test_cost_field_learned import Setup as LearnedSetup
from test_cost_field_learned import all_moves, random_mask
from test_cost_field_many import big_component, bits, same_field, spiral_mask, targets_of

NAMES = ("artp_field_compute_many_learned", "artp_field_compute_many_clearance", "artp_field_cost_matrix_learned",
         "artp_field_cost_matrix_clearance")
N_YAW = 7


def tup(x):
    return tuple(int(v) for v in x)


def close_all(fields):
    for f in fields:
        f.close()


@pytest.fixture(scope="module")
def S():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from art_planner_amd.context import Context
    c = Context(0, "yaml")
    yield LearnedSetup(c)
    c.close()


@pytest.fixture(scope="module")
def SC():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from art_planner_amd.context import Context
    c = Context(0, "yaml")
    yield ClearanceSetup(c)
    c.close()


# ---- CPU: the C ABI without a device ------------------------------------------------------------------------------
def _null_context_calls(L):
    """Every new entry point on a NULL context: (name, status, handles, stats, table stats)."""
    lp, cp = _capi.FieldLearnedParams(), _capi.FieldClearanceParams()
    L.artp_field_learned_params_defaults(C.byref(lp))
    L.artp_field_clearance_params_defaults(C.byref(cp))
    mask, src = np.ones(4, np.uint32), np.zeros(6, np.int32)
    off = np.array([0, 1, 2], np.uint64)
    out = []
    for name, p in ((NAMES[0], lp), (NAMES[1], cp)):
        handles = (C.c_void_p * 2)()
        handles[0] = handles[1] = 1234
        rc = getattr(L, name)(None, C.byref(p), 1, None, mask.ctypes.data, 0, src.ctypes.data, off.ctypes.data, 2, 0, handles)
        out.append((name, rc, [handles[0], handles[1]], None, None))
    for name, p in ((NAMES[2], lp), (NAMES[3], cp)):
        m = np.zeros(4)
        st = _capi.FieldManyStats(1, 2, 3, 4, 5, 6)
        ts = _capi.FieldManyTableStats(1, 2, 3, 4, 5.0)
        rc = getattr(L, name)(None, C.byref(p), 1, None, mask.ctypes.data, 0, src.ctypes.data, 2, 0, m.ctypes.data,
                              C.byref(st), C.byref(ts))
        out.append((name, rc, [], st, ts))
    return out


def test_weighted_entry_points_are_declared_exported_and_refuse_a_null_context():
    import common
    header = open(common.ROOT + "/include/artp_c.h").read()
    L = _capi.load()
    for name in NAMES:
        assert name in _capi.SYMBOLS and "int " + name + "(" in header
        assert getattr(L, name) is not None
    for name, rc, handles, st, ts in _null_context_calls(L):
        assert rc == -1, name


def test_a_null_context_clears_the_handles_and_zeroes_both_stats():
    for name, rc, handles, st, ts in _null_context_calls(_capi.load()):
        assert not any(handles), name
        if st is not None:
            assert [getattr(st, n) for n, _ in _capi.FieldManyStats._fields_] == [0] * 6, name
            assert [getattr(ts, n) for n, _ in _capi.FieldManyTableStats._fields_] == [0, 0, 0, 0, 0.0], name


def test_table_stats_layout_matches_the_header():
    import common
    header = open(common.ROOT + "/include/artp_c.h").read()
    body = re.search(r"typedef struct artp_field_many_table_stats_t \{(.*?)\} artp_field_many_table_stats_t;", header,
                     re.S).group(1)
    members = re.findall(r"(uint64_t|double) (\w+);", body)
    assert [n for _, n in members] == [n for n, _ in _capi.FieldManyTableStats._fields_]
    assert [n for _, n in members] == ["table_builds", "table_rows", "table_bytes", "table_copies", "build_ms"]
    for (t, _), (_, ct) in zip(members, _capi.FieldManyTableStats._fields_):
        assert ct is (C.c_uint64 if t == "uint64_t" else C.c_double)
    assert C.sizeof(_capi.FieldManyTableStats) == 8 * len(members)
    assert len(re.findall(r"\w+;", body)) == len(members)        # nothing but these members


# ---- GPU, learned ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_one_learned_set_is_a_single_learned_field(S):
    S.install(1, "real")
    mask = random_mask(RECT[2:], N_YAW, 107)
    lat = S.lattice(mask, N_YAW, RECT, **WEIGHTS)
    src = big_component(lat, 1)
    kw = dict(rect=RECT, **WEIGHTS)
    many = S.ctx.learned_cost_fields(mask, N_YAW, [src], **kw)
    assert len(many) == 1
    with S.ctx.learned_cost_field(mask, N_YAW, src, **kw) as single, many[0] as f:
        d = same_field(f, single, targets_of(single.dist(), 3) + src, edge_costs=True)     # ten paths and the source
        assert d[src[0]] == 0.0
        ls, ss = f.learned_stats(), single.learned_stats()
        assert ls["table_rows"] == ss["table_rows"] == 9 * N_YAW * 10 * 256
        assert ls["table_bytes"] == ss["table_bytes"] and ls["chunks"] == ss["chunks"] == 1
        st = f.stats()
        assert st["tiles"] == 9 and st["outer_rounds"] >= 1 and st["hop_rounds"] >= 1 and st["plain_sweeps"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("reverse", [False, True])
def test_learned_sets_in_an_odd_rectangle_with_infeasible_edges(S, reverse):
    S.install(1, "real")
    c3, inside = S.cost3(N_YAW, RECT)
    thr = float(np.float32(np.median(c3[..., 2][inside])))
    wts = dict(WEIGHTS, risk_threshold=thr)
    mask = random_mask(RECT[2:], N_YAW, 11, p=0.9)
    lat = LL.LearnedLattice(mask, N_YAW, LL.price(c3, **wts))
    label, sizes = lat.components()               # the pruning cuts the lattice up: six nodes of its largest piece
    comp = np.argwhere(label == int(np.argmax(sizes)))
    assert len(comp) > 100
    s = [tup(comp[(2 * i + 1) * len(comp) // 12]) for i in range(6)]
    sets = [[s[0]], [s[1], s[2]], [s[3]], [s[3]], [s[4], s[5], s[0]]]      # sizes 1, 2, 1, 1, 3; two sets identical
    kw = dict(rect=RECT, reverse=reverse, **wts)
    many = S.ctx.learned_cost_fields(mask, N_YAW, sets, **kw)
    try:
        assert len(many) == len(sets)
        for b, (f, srcs) in enumerate(zip(many, sets)):
            ref, _ = lat.dijkstra(srcs, reverse)
            with S.ctx.learned_cost_field(mask, N_YAW, srcs, **kw) as single:
                d = same_field(f, single, targets_of(ref, 10 + b), edge_costs=True)
                if b == 0:      # infeasible edges exist, and the batch's table holds them: the single-field test's bounds
                    a, nb, m = all_moves(lat)
                    want = lat.w[m, a[:, 0], a[:, 1], a[:, 2]]
                    want[~inside[m, a[:, 0], a[:, 1], a[:, 2]]] = np.nan      # the target lies outside the rectangle
                    assert np.isinf(want).any() and np.isfinite(want).sum() > len(want) // 4
                    got = f.edge_costs(a, nb)
                    assert np.array_equal(np.isnan(got), np.isnan(want))
                    ok = ~np.isnan(want)
                    assert np.array_equal(bits(got[ok]), bits(want[ok]))
                    assert np.array_equal(bits(got[ok]), bits(single.edge_costs(a, nb)[ok]))
                    print(f"  threshold {thr}: {int(np.isposinf(got).sum())} of {int(ok.sum())} edge costs are +inf")
            assert_field(d, ref)                                     # finite set exact, values to 1e-9
            assert all(d[t] == 0.0 for t in srcs)
        assert np.array_equal(bits(many[2].dist()), bits(many[3].dist()))
        assert not np.array_equal(bits(many[0].dist()), bits(many[2].dist()))
    finally:
        close_all(many)


@pytest.mark.gpu
def test_learned_fields_that_finish_far_apart(S):
    S.install(1, "real")
    n_yaw = 8
    mask, src = spiral_mask(N, n_yaw)
    island = (N // 2, N // 2, 3)
    assert not mask[island[0] - 1:island[0] + 2, island[1] - 1:island[1] + 2].any()      # the empty middle of the spiral
    mask[island[0], island[1]] = 1 << island[2]
    with S.ctx.learned_cost_field(mask, n_yaw, [src], **WEIGHTS) as f:
        d = f.dist()
    fin = np.isfinite(d)
    far = tup(np.unravel_index(np.argmax(np.where(fin, d, -1.0)), d.shape))
    middle = tup(np.unravel_index(np.argmin(np.where(fin, np.abs(d - 0.5 * d[far]), np.inf)), d.shape))
    sets = [[far], [middle], [island]]
    many = S.ctx.learned_cost_fields(mask, n_yaw, sets, **WEIGHTS)
    try:
        rounds = [f.stats()["outer_rounds"] for f in many]
        hop_rounds = [f.stats()["hop_rounds"] for f in many]
        print(f"  far {far} middle {middle}: distance rounds {rounds}, hop rounds {hop_rounds}")
        di = many[2].dist()
        assert many[2].stats()["reached_nodes"] == 1 == int(np.isfinite(di).sum()) and di[island] == 0.0
        assert rounds[2] == 1 and hop_rounds[2] == 1                  # quiet after its first round
        assert rounds[0] > 50 and rounds[1] > 50                      # the corridor: a write into field 2 would show
        for f, srcs, seed in ((many[0], sets[0], 1), (many[1], sets[1], 2)):
            with S.ctx.learned_cost_field(mask, n_yaw, srcs, **WEIGHTS) as single:
                w = same_field(f, single, targets_of(d, seed, 6) + [src, far])
            assert np.isinf(w[island]) and int(np.isfinite(w).sum()) == int(fin.sum())
    finally:
        close_all(many)


@pytest.mark.gpu
def test_32_headings_use_the_weighted_many_kernels_own_lds_opt_in(S):
    S.install(1, "real")
    n_yaw, rect = 32, (3, 2, 33, 20)
    mask = random_mask(rect[2:], n_yaw, 77)
    lat = S.lattice(mask, n_yaw, rect, **WEIGHTS)
    s = big_component(lat, 3)
    sets = [[s[0]], [s[1], s[2]]]
    kw = dict(rect=rect, **WEIGHTS)
    many = S.ctx.learned_cost_fields(mask, n_yaw, sets, **kw)
    try:
        for b, (f, srcs) in enumerate(zip(many, sets)):
            with S.ctx.learned_cost_field(mask, n_yaw, srcs, **kw) as single:
                d = same_field(f, single, targets_of(single.dist(), 20 + b))
            assert int(np.isfinite(d).sum()) > mask.size * n_yaw // 3
    finally:
        close_all(many)


@pytest.mark.gpu
def test_learned_fields_of_a_batch_are_independent_afterwards(S):
    S.install(1, "real")
    mask = random_mask(RECT[2:], N_YAW, 107)
    lat = S.lattice(mask, N_YAW, RECT, **WEIGHTS)
    s = big_component(lat, 3)
    kw = dict(rect=RECT, **WEIGHTS)
    many = S.ctx.learned_cost_fields(mask, N_YAW, [[s[0]], [s[1]], [s[2]]], **kw)
    try:
        before = [f.dist() for f in many]
        # update_learned of field 1 on an edited mask: a new field on that mask, and the others keep their bits
        edited = mask.copy()
        edited[10:20, 8:14] = 0
        for t in s:
            edited[t[0], t[1]] = mask[t[0], t[1]]
        assert (edited != mask).sum() > 20
        many[1].update_learned(edited)
        with S.ctx.learned_cost_field(edited, N_YAW, [s[1]], **kw) as fresh:
            d1 = same_field(many[1], fresh, targets_of(fresh.dist(), 5), edge_costs=True)
        assert not np.array_equal(bits(d1), bits(before[1]))
        assert np.array_equal(bits(many[0].dist()), bits(before[0])) and np.array_equal(bits(many[2].dist()), bits(before[2]))
        # block_moves and plan on field 2
        target = tup(np.unravel_index(np.argmax(np.where(np.isfinite(before[2]), before[2], -1.0)), before[2].shape))
        nodes = many[2].path(target)[0]
        assert len(nodes) > 4
        assert many[2].block_moves([nodes[1]], [nodes[2]]) == 1
        with S.ctx.learned_cost_field(mask, N_YAW, [s[2]], **kw) as fresh:
            assert fresh.block_moves([nodes[1]], [nodes[2]]) == 1
            same_field(many[2], fresh, targets_of(before[2], 6) + [target])
            got, want = many[2].plan([target, s[2]]), fresh.plan([target, s[2]])
            assert [g[0] for g in got] == [w[0] for w in want]
            assert np.array_equal(bits(many[2].dist()), bits(fresh.dist()))
        assert np.array_equal(bits(many[0].dist()), bits(before[0]))
        # close field 0 first: the others still answer, from tables of their own
        many[0].close()
        assert many[0].h is None
        assert many[1].path(s[1])[2] == 0.0 and many[2].path(s[2])[2] == 0.0
        with S.ctx.learned_cost_field(edited, N_YAW, [s[1]], **kw) as fresh:
            same_field(many[1], fresh, targets_of(fresh.dist(), 7), edge_costs=True)
    finally:
        close_all(many)


@pytest.mark.gpu
def test_learned_cost_matrix(S):
    S.install(1, "real")
    mask = random_mask(RECT[2:], N_YAW, 107)
    island = (22, 30, 4)
    mask[island[0] - 1:island[0] + 2, island[1] - 1:island[1] + 2] = 0
    mask[island[0], island[1]] = 1 << island[2]
    lat = S.lattice(mask, N_YAW, RECT, **WEIGHTS)
    poses = big_component(lat, 5)
    poses.insert(2, island)
    n = len(poses)
    kw = dict(rect=RECT, **WEIGHTS)
    want = np.empty((n, n))
    for i, p in enumerate(poses):
        with S.ctx.learned_cost_field(mask, N_YAW, [p], **kw) as f:
            d = f.dist()
        want[i] = [d[q] for q in poses]
    for batch, groups in ((4, 2), (1, n)):
        m, st = S.ctx.learned_cost_matrix(mask, N_YAW, poses, batch, return_stats=True, **kw)
        assert m.shape == (n, n) and m.dtype == np.float64
        assert np.array_equal(bits(m), bits(want)), batch
        assert (st["groups"], st["fields"]) == (groups, n)
        assert st["table_builds"] == 1 and st["table_copies"] == 0
        assert st["table_bytes"] == 8 * st["table_rows"] == 8 * 9 * N_YAW * 10 * 256 and st["build_ms"] > 0.0
    off = ~np.eye(n, dtype=bool)
    assert (np.diag(m) == 0.0).all()
    assert np.isposinf(m[2][off[2]]).all() and np.isposinf(m[:, 2][off[:, 2]]).all()
    rest = [i for i in range(n) if i != 2]
    sub = m[np.ix_(rest, rest)]
    assert np.isfinite(sub).all()
    asym = np.abs(sub - sub.T) / np.maximum(np.abs(sub), 1e-300)
    print(f"  largest relative asymmetry {asym.max():.3e}")
    assert (asym[~np.eye(n - 1, dtype=bool)] > 1e-6).any()           # w(a -> b) != w(b -> a): the matrix is not symmetric


# ---- GPU, clearance ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_clearance_sets_against_the_single_fields(SC):
    n_yaw = 7
    for objective in (0, 1):
        mask, src, d2, base, lat, _ = case(SC, objective, n_yaw)
        s = big_component(lat, 4)
        sets = [[src], [s[0], s[1]], [s[2]]]
        plain_kw = dict(rect=C_RECT, objective=objective)
        # gain = 0: the plain batch's bits
        zero = SC.ctx.clearance_cost_fields(mask, n_yaw, sets, **dict(CLEAR, gain=0.0), **plain_kw)
        plain = SC.ctx.cost_fields(mask, n_yaw, sets, **plain_kw)
        try:
            for f, g in zip(zero, plain):
                assert np.array_equal(bits(f.dist()), bits(g.dist()))
        finally:
            close_all(zero + plain)
        for reverse in (False, True) if objective == 1 else (False,):
            kw = dict(CLEAR, gain=2.0, reverse=reverse, **plain_kw)
            many = SC.ctx.clearance_cost_fields(mask, n_yaw, sets, **kw)
            try:
                for b, (f, srcs) in enumerate(zip(many, sets)):
                    with SC.ctx.clearance_cost_field(mask, n_yaw, srcs, **kw) as single:
                        same_field(f, single, targets_of(single.dist(), 50 + b), edge_costs=True)
                        assert np.array_equal(f.clearance(), single.clearance())
                    assert np.array_equal(f.clearance(), d2)
            finally:
                close_all(many)


@pytest.mark.gpu
def test_clearance_gain_two_update_and_matrix(SC):
    n_yaw, objective = 7, 1
    mask, src, d2, base, lat, _ = case(SC, objective, n_yaw)
    s = big_component(lat, 4)
    kw = dict(CLEAR, gain=2.0, rect=C_RECT, objective=objective)
    sets = [[s[0]], [s[1]], [s[2]]]
    many = SC.ctx.clearance_cost_fields(mask, n_yaw, sets, **kw)
    try:
        for b, (f, srcs) in enumerate(zip(many, sets)):
            with SC.ctx.clearance_cost_field(mask, n_yaw, srcs, **kw) as single:
                same_field(f, single, targets_of(single.dist(), 60 + b), edge_costs=True)
                assert np.array_equal(f.clearance(), single.clearance())
        before = [f.dist() for f in many]
        edited = mask.copy()
        edited[10:20, 8:14] = 0
        for t in s:
            edited[t[0], t[1]] = mask[t[0], t[1]]
        many[1].update_clearance(edited)
        with SC.ctx.clearance_cost_field(edited, n_yaw, [s[1]], **kw) as fresh:
            d1 = same_field(many[1], fresh, targets_of(fresh.dist(), 5), edge_costs=True)
            assert np.array_equal(many[1].clearance(), fresh.clearance())
        assert not np.array_equal(bits(d1), bits(before[1]))
        assert np.array_equal(bits(many[0].dist()), bits(before[0])) and np.array_equal(bits(many[2].dist()), bits(before[2]))
        assert np.array_equal(many[0].clearance(), d2) and np.array_equal(many[2].clearance(), d2)
    finally:
        close_all(many)
    poses = s
    want = np.empty((4, 4))
    for i, p in enumerate(poses):
        with SC.ctx.clearance_cost_field(mask, n_yaw, [p], **kw) as f:
            d = f.dist()
        want[i] = [d[q] for q in poses]
    for batch in (None, 3):
        m, st = SC.ctx.clearance_cost_matrix(mask, n_yaw, poses, batch, return_stats=True, **kw)
        assert np.array_equal(bits(m), bits(want)), batch
        assert st["table_builds"] == 1 and st["table_copies"] == 0 and st["fields"] == 4
    assert (np.diag(m) == 0.0).all()


# ---- GPU, both kinds ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_weighted_refusals_leak_nothing_and_leave_the_context_usable(S):
    import torch
    from art_planner_amd.context import Context
    ctx = S.ctx
    ones = np.ones((10, 10), np.uint32)
    fresh = Context(0, "yaml")
    fresh._grid = (10, 10)   # as if a map were installed: the library itself must refuse
    try:
        for call in (lambda: fresh.learned_cost_fields(ones, 1, [[(0, 0, 0)]]),
                     lambda: fresh.learned_cost_matrix(ones, 1, [(0, 0, 0)])):
            with pytest.raises(_capi.ArtpError) as e:
                call()
            assert e.value.status == -6   # ARTP_ERR_NO_WEIGHTS
    finally:
        fresh.close()
    S.install(1, "real")
    n_yaw = 4
    mask = np.full((N, N), 0xf, np.uint32)
    mask[3, 4] = 0b0101
    good = (1, 1, 0)
    sets = [[good], [(5, 5, 1)], [(9, 9, 2)]]
    close_all(ctx.learned_cost_fields(mask, n_yaw, sets, **WEIGHTS))          # every lazy allocation made once
    close_all(ctx.clearance_cost_fields(mask, n_yaw, sets, **CLEAR))
    ctx.learned_cost_matrix(mask, n_yaw, [good, (5, 5, 1)], **WEIGHTS)
    torch.cuda.synchronize()
    free_before = torch.cuda.mem_get_info()[0]
    bad_src = [[good], [(2, 2, 2)], [(7, 7, 0), (3, 4, 1)]]                   # a source off the mask in set 2 of 3
    for many, extra in ((ctx.learned_cost_fields, WEIGHTS), (ctx.clearance_cost_fields, CLEAR)):
        bad = [dict(sources_list=bad_src), dict(plain_sweeps=True), dict(sources_list=[[good], [], [(2, 2, 2)]])]
        bad += [dict(w_risk=-0.5)] if extra is WEIGHTS else [dict(margin=CLEAR["radius_cells"] * RES * 1.5)]
        for i, kw in enumerate(bad):
            args = dict(extra, sources_list=sets)
            args.update(kw)
            with pytest.raises(_capi.ArtpError) as e:
                many(mask, n_yaw, args.pop("sources_list"), **args)
            assert e.value.status == -1, kw                                    # ARTP_ERR_INVALID_ARG
            if i == 0:
                assert "set 2" in str(e.value), str(e.value)
    for matrix, extra in ((ctx.learned_cost_matrix, WEIGHTS), (ctx.clearance_cost_matrix, CLEAR)):
        with pytest.raises(_capi.ArtpError) as e:
            matrix(mask, n_yaw, [good, (3, 4, 1), (2, 2, 2)], **extra)
        assert e.value.status == -1 and "pose 1" in str(e.value)
    # a mask of the wrong shape never reaches the library: the text names the method that was called
    for call, label in ((lambda: ctx.learned_cost_fields(mask[:5], n_yaw, sets), "learned_cost_fields:"),
                        (lambda: ctx.clearance_cost_fields(mask[:5], n_yaw, sets), "clearance_cost_fields:"),
                        (lambda: ctx.learned_cost_matrix(mask[:5], n_yaw, [good]), "learned_cost_matrix:"),
                        (lambda: ctx.clearance_cost_matrix(mask[:5], n_yaw, [good]), "clearance_cost_matrix:")):
        with pytest.raises(_capi.ArtpError) as e:
            call()
        assert str(e.value).startswith(label), str(e.value)
    m = ctx.learned_cost_matrix(mask, n_yaw, [good, (5, 5, 1), (9, 9, 2)], 2, **WEIGHTS)   # a finished matrix frees its table
    assert np.isfinite(m).all()
    # Nothing leaked: the bound of test_cost_field_many.py, which frees what it allocates (the runtime hands device memory
    # out in pages of at most 2 MiB).  One table of this map is 96 * 96 * 4 * 80 bytes = 2.9 MB.
    torch.cuda.synchronize()
    free_after = torch.cuda.mem_get_info()[0]
    print(f"  free memory before {free_before} after {free_after} ({free_after - free_before:+d} bytes)")
    assert abs(free_after - free_before) <= 2 << 20
    # a single learned_cost_field afterwards is correct
    sub = random_mask(RECT[2:], N_YAW, 9)
    lat = S.lattice(sub, N_YAW, RECT, **WEIGHTS)
    s = big_component(lat, 1)
    ref, _ = lat.dijkstra(s, False)
    with ctx.learned_cost_field(sub, N_YAW, s, rect=RECT, **WEIGHTS) as f:
        assert_field(f.dist(), ref)


@pytest.mark.gpu
def test_a_weighted_batch_on_lane_1_gives_the_bits_of_lane_0(S):
    S.install(1, "real")
    ctx = S.ctx
    mask = random_mask(RECT[2:], N_YAW, 107)
    lat = S.lattice(mask, N_YAW, RECT, **WEIGHTS)
    s = big_component(lat, 4)
    sets = [[s[0]], [s[1], s[2]], [s[3]]]
    kw = dict(rect=RECT, **WEIGHTS)
    ckw = dict(CLEAR, rect=RECT, objective=1)
    opened = []                                   # closed on every way out: a field must not outlive its context
    try:
        ctx.set_lane(2)
        live = ctx.learned_cost_field(mask, N_YAW, [s[3]], **kw)
        opened.append(live)
        live_d = live.dist()
        ctx.set_lane(0)
        base = ctx.learned_cost_fields(mask, N_YAW, sets, **kw) + ctx.clearance_cost_fields(mask, N_YAW, sets, **ckw)
        opened += base
        m0 = ctx.learned_cost_matrix(mask, N_YAW, s, **kw)
        ctx.set_lane(1)
        other = ctx.learned_cost_fields(mask, N_YAW, sets, **kw) + ctx.clearance_cost_fields(mask, N_YAW, sets, **ckw)
        opened += other
        assert ctx.lane == 1
        for b, (f, g) in enumerate(zip(other, base)):
            same_field(f, g, targets_of(live_d, 30 + b))
        assert np.array_equal(bits(ctx.learned_cost_matrix(mask, N_YAW, s, **kw)), bits(m0))
        close_all(other)
        close_all(base)
        ctx.set_lane(2)
        assert np.array_equal(bits(live.dist()), bits(live_d))
        with ctx.learned_cost_field(mask, N_YAW, [s[3]], **kw) as again:
            same_field(live, again, targets_of(live_d, 40))
    finally:
        close_all(opened)
        ctx.set_lane(0)
