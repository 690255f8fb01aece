"""Windowed shortcut simplification of cost-field paths on the device (csrc/field_simplify.h, include/artp_c.h
artp_field_simplify_paths, CostField.simplify).

The oracles:
  * Roadmap.simplify, the host routine over all pairs of one path: with a window that covers the path the device's result
    must be its bits -- states, count and cost;
  * tests/field_simplify_ref.py's restatement of the windowed search, fed with this library's own per-pair answers:
    check_edges_interp and check_motions on the pair, Roadmap.simplify of the two-state path for its cost;
  * the call against itself: one call per path, other batch sizes;
  * check_motions and check_edges_interp on every pair of states a result keeps next to one another.
Two maps: the 120 x 120 Perlin map of test_cost_field_plan.py at 8 headings (paths from plan()), and a flat 200 x 200 map
on which paths are built by hand from the lattice poses (nothing requires the states of a path to come from a field).
Both depend on the device's preprocessing, so every condition a case needs is asserted before it is used."""
import ctypes as C

import numpy as np
import pytest

import field_simplify_ref as FS
from art_planner_amd import _capi
from test_cost_field import ROBOT, device_map
from test_cost_field_plan import tup, world
from test_cost_field_update import bits_of

pytestmark = pytest.mark.gpu

N_YAW = 8
WINDOWS = (1, 2, 7, 64)


def new_context():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from art_planner_amd.context import Context
    return Context(0, ROBOT)


def roadmap(ctx, path, objective):
    from art_planner_amd.roadmap import Roadmap
    return Roadmap(ctx, path[0], path[-1], n_milestones=8, objective=objective, max_lon_vel=0.5, max_lat_vel=0.1,
                   max_ang_vel=0.5)


def same_bits(a, b):
    return np.float64(a).view(np.uint64) == np.float64(b).view(np.uint64)


# ---- the Perlin map: paths from plan() ---------------------------------------------------------------------------
class Perlin:
    """The map, its mask and source (test_cost_field_plan.world), and per objective the checked paths of plan() to 16
    targets by hop rank and 24 random nodes: [(nodes, se3)], made once."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.gm, self.mask, self.src, self.far = world(ctx, 0.25, N_YAW)
        self._paths = {}

    def field(self, objective=1, **kw):
        return self.ctx.cost_field(self.mask, N_YAW, [self.src], objective=objective, **kw)

    def paths(self, objective):
        if objective not in self._paths:
            with self.field(objective) as f:
                fin = np.argwhere(np.isfinite(f.dist()))
                rng = np.random.default_rng(2024)
                targets = self.far + [tup(x) for x in fin[rng.integers(0, len(fin), 24)]]
                res = f.plan(targets)
            assert all(len(r) == 4 for r in res)                        # plan() without the argument: tuples of four
            self._paths[objective] = [(r[1], r[2]) for r in res if r[0] == 0]
            print(f"  objective {objective}: {len(self._paths[objective])} checked paths of "
                  f"{sorted(len(p[1]) for p in self._paths[objective])} states")
        return self._paths[objective]


@pytest.fixture(scope="module")
def perlin():
    c = new_context()
    yield Perlin(c)
    c.close()


# ---- the flat map: paths by hand ---------------------------------------------------------------------------------
class Flat:
    def __init__(self, ctx):
        self.ctx = ctx
        n = 200
        self.gm = device_map(ctx, np.zeros((n, n), np.float32), 0.04)
        self.poses = ctx.reachability_poses(N_YAW)
        self.rect = (96, 96, 8, 8)
        self.mask = np.full((8, 8), (1 << N_YAW) - 1, np.uint32)
        self._tables = None

    def field(self, objective=1):
        return self.ctx.cost_field(self.mask, N_YAW, [(0, 0, 0)], rect=self.rect, objective=objective)

    def run_turn_run(self, run1, run2):
        """States of: run1 cells towards smaller rows at heading 0 (forwards), two heading steps, run2 cells towards
        smaller columns at heading 2 (forwards again): 1 + run1 + 2 + run2 states, every one at least 40 cells inside."""
        r, c, k = 110, 175, 0
        nodes = [(r, c, k)]
        for _ in range(run1):
            r -= 1
            nodes.append((r, c, k))
        for _ in range(2):
            k += 1
            nodes.append((r, c, k))
        for _ in range(run2):
            c -= 1
            nodes.append((r, c, k))
        assert min(r, c) >= 40
        se3 = np.array([self.poses[v] for v in nodes])
        assert np.isfinite(se3).all() and self.ctx.validate_states(se3).all()
        return nodes, se3

    def tables(self):
        """The long path (130 states: 5 cells, the turn, 122 cells) and this library's own answers about every pair at most
        64 apart, under objective 1: usable = check_edges_interp and check_motions, cost = Roadmap.simplify of the pair."""
        if self._tables is None:
            _, path = self.run_turn_run(5, 122)
            n = len(path)
            assert n == 130
            pairs = np.array(FS.candidates(n, 64))
            s1, s2 = path[pairs[:, 0]], path[pairs[:, 1]]
            ok = (self.ctx.check_edges_interp(s1, s2)[0] != 0) & (self.ctx.check_motions(s1, s2) != 0)
            usable, cost = np.zeros((n, n), bool), np.full((n, n), np.nan)
            rm = roadmap(self.ctx, path, 1)
            try:
                for (i, j), v in zip(pairs, ok):
                    two, c = rm.simplify(path[[i, j]])
                    assert len(two) == 2 and np.isfinite(c) == bool(v), (i, j, c, v)
                    usable[i, j], cost[i, j] = v, c
            finally:
                rm.close()
            assert usable[np.arange(n - 1), np.arange(1, n)].all()          # the chain itself passes
            print(f"  flat map: {len(pairs)} pairs, {int(ok.sum())} usable")
            self._tables = (path, usable, cost)
        return self._tables


@pytest.fixture(scope="module")
def flat():
    c = new_context()
    yield Flat(c)
    c.close()


# ---- 1. a window that covers the path: the roadmap's routine -----------------------------------------------------------
def equals_the_roadmap(ctx, f, paths, objective):
    longest = max(len(p) for p in paths)
    all_pairs = f.simplify(paths, window=0)
    assert f.simplify_stats()["candidates"] == sum(len(p) * (len(p) - 1) // 2 for p in paths)
    covering = f.simplify(paths, window=longest - 1)
    beyond = f.simplify(paths, window=longest + 5)
    for p, a, b, c in zip(paths, all_pairs, covering, beyond):
        rm = roadmap(ctx, p, objective)
        try:
            want, cost = rm.simplify(p)
        finally:
            rm.close()
        print(f"    {len(p)} states -> {len(want)}, cost {cost!r}")
        for got in (a, b, c):
            assert got[0] == 0 and len(got[2]) == len(want) == len(got[1])
            assert np.array_equal(bits_of(got[2]), bits_of(want)) and same_bits(got[3], cost)
            assert np.array_equal(bits_of(p[got[1]]), bits_of(want))
    return all_pairs


@pytest.mark.parametrize("objective", [0, 1])
def test_a_covering_window_equals_the_roadmap_simplifier_on_the_perlin_map(perlin, objective):
    paths = [se3 for _, se3 in perlin.paths(objective) if 20 <= len(se3) <= 80][:6]
    assert len(paths) >= 3, [len(p[1]) for p in perlin.paths(objective)]
    with perlin.field(objective) as f:
        equals_the_roadmap(perlin.ctx, f, paths, objective)


@pytest.mark.parametrize("objective", [0, 1])
def test_a_covering_window_equals_the_roadmap_simplifier_where_chains_tie(flat, objective):
    """A straight run, a turn on the spot and a second run on a flat map: the pairs of a run cost what the chain between
    them costs, up to rounding, so many chains tie or nearly tie; the search's tie rule decides."""
    _, path = flat.run_turn_run(20, 20)
    with flat.field(objective) as f:
        got = equals_the_roadmap(flat.ctx, f, [path, path[:21], path[20:]], objective)
    assert len(path) == 43 and all(len(g[1]) < n for g, n in zip(got, (43, 21, 23)))


# ---- 2. windowed results against the restatement ---------------------------------------------------------------------
@pytest.mark.parametrize("window", WINDOWS)
def test_windowed_results_equal_the_restatement(flat, window):
    path, usable, cost = flat.tables()
    lengths = [1, 2, 3, window, window + 1, window + 2, 130]
    with flat.field(1) as f:
        got = f.simplify([path[:n] for n in lengths], window=window)
        st = f.simplify_stats()
    assert st["candidates"] == sum(FS.count(n, window) for n in lengths) and st["paths"] == len(lengths)
    assert st["states_in"] == sum(lengths) and st["states_kept"] == sum(len(g[1]) for g in got)
    for n, (status, kept, se3, total) in zip(lengths, got):
        want = FS.search(n, window, usable, cost)
        assert want[0] == 0
        assert (status, list(kept)) == want[:2], (n, list(kept), want[1])
        assert same_bits(total, want[2]) and np.array_equal(bits_of(se3), bits_of(path[:n][kept]))
        if window == 1:                                       # the input with the chain's cost
            assert list(kept) == list(range(n)) and same_bits(total, FS.fold(list(range(n)), cost))
    print(f"  window {window}: {[len(g[1]) for g in got]} of {lengths} states kept")


class Band:
    """table[i][j] for 0 < j - i <= w, stored as (n, w + 1): what field_simplify_ref.search reads of a long path."""

    def __init__(self, n, w, fill, dtype):
        self.a = np.full((n, w + 1), fill, dtype)

    def __getitem__(self, i):
        row = self.a[i]

        class Row:
            def __getitem__(self, j):
                return row[j - i]
        return Row()


def test_a_path_too_long_for_lds_is_searched_in_global_memory(flat):
    """4101 states (the search keeps best and from in LDS up to 4096): 41 times up and down a run of 50 cells, window 2.
    The per-pair answers are the device's own, from one call with every pair as a path of two states; the long path's
    search is then the restatement's.  The turning points make pairs of equal states: cost 0, many ties."""
    nodes, run = flat.run_turn_run(50, 0)
    up = run[:51]
    path = np.concatenate([up[:1]] + [np.concatenate([up[1:], up[-2::-1]]) for _ in range(41)])
    n, w = len(path), 2
    assert n == 4101
    pairs = FS.candidates(n, w)
    with flat.field(1) as f:
        two = f.simplify([path[[i, j]] for i, j in pairs], window=1)
        assert f.simplify_stats()["paths"] == len(pairs) == FS.count(n, w)
        status, kept, se3, total = f.simplify([path], window=w)[0]
        among = f.simplify([path[:60], path, path[:9]], window=w, max_batch_pairs=3000)      # next to paths that fit
        same_answers([among[0], among[2]], f.simplify([path[:60], path[:9]], window=w))
    usable, cost = Band(n, w, False, bool), Band(n, w, np.nan, np.float64)
    for (i, j), r in zip(pairs, two):
        assert r[0] in (0, 1) and (r[0] == 0) == np.isfinite(r[3])
        usable.a[i, j - i], cost.a[i, j - i] = r[0] == 0, r[3]
    want = FS.search(n, w, usable, cost)
    assert want[0] == 0 and len(want[1]) < n
    assert (status, list(kept)) == want[:2] and same_bits(total, want[2]) and np.array_equal(bits_of(se3), bits_of(path[kept]))
    assert among[1][0] == 0 and np.array_equal(among[1][1], kept) and same_bits(among[1][3], total)
    print(f"  {n} states -> {len(kept)}, cost {total!r}")


# ---- 3. batches ----------------------------------------------------------------------------------------------------
def mixed_paths(perlin):
    full = sorted((se3 for _, se3 in perlin.paths(1)), key=len, reverse=True)
    assert len(full) >= 6 and len(full[5]) >= 20
    cut = [7, 33, 12, 64, 3, 21, 9, 47, 18, 5, 29, 66, 15]
    paths = [full[i % len(full)][:n] for i, n in enumerate(cut)]
    paths.insert(2, np.zeros((0, 7)))
    paths.insert(5, full[1][:1])
    paths.insert(9, full[2][:2])
    assert len(paths) == 16
    return paths


def same_answers(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g[0] == w[0] and np.array_equal(g[1], w[1]) and np.array_equal(bits_of(g[2]), bits_of(w[2]))
        assert same_bits(g[3], w[3])


def test_sixteen_paths_in_one_call_equal_sixteen_calls_and_any_batch_size(perlin):
    paths = mixed_paths(perlin)
    with perlin.field(1) as f:
        together = f.simplify(paths, window=16)
        st = f.simplify_stats()
        assert st["batches"] == 1 and st["paths"] == 16 and st["candidates"] == sum(FS.count(len(p), 16) for p in paths) > 1000
        assert [r[0] for r in together] == [2 if len(p) == 0 else 0 for p in paths]
        assert [len(r[1]) for r in together][2] == 0 and list(together[5][1]) == [0] and together[5][3] == 0.0
        assert list(together[9][1]) == [0, 1]
        same_answers([f.simplify([p], window=16)[0] for p in paths], together)
        for batch in (256, 1000):                             # cut inside paths
            same_answers(f.simplify(paths, window=16, max_batch_pairs=batch), together)
            assert f.simplify_stats()["batches"] == -(-st["candidates"] // batch) > 1
        assert f.simplify_stats()["usable_candidates"] == st["usable_candidates"] <= st["candidates"]
        # entries of plan() and None pass through
        mixed = f.simplify([None, (1, None, None, np.inf), (0, None, paths[0], 1.0)], window=16)
        assert mixed[0] is None and mixed[1] is None
        same_answers([mixed[2]], [together[0]])
        assert f.simplify([]) == [] and f.simplify([None]) == [None]


# ---- 4. the results on their own terms ------------------------------------------------------------------------------
def test_every_kept_pair_passes_both_checks_and_larger_windows_cost_no_more(perlin):
    ctx = perlin.ctx
    both = perlin.paths(1)
    paths = [se3 for _, se3 in both]
    with perlin.field(1) as f:
        by_window = {w: f.simplify(paths, window=w) for w in WINDOWS}
        print(f"  window 64: {f.simplify_stats()}")
    for w, res in by_window.items():
        for p, (status, kept, se3, cost) in zip(paths, res):
            assert status == 0 and kept[0] == 0 and kept[-1] == len(p) - 1 and (np.diff(kept.astype(np.int64)) >= 1).all()
            assert (np.diff(kept.astype(np.int64)) <= w).all() and np.array_equal(bits_of(se3), bits_of(p[kept]))
            if len(se3) > 1:
                assert ctx.check_motions(se3[:-1], se3[1:]).all() and ctx.check_edges_interp(se3[:-1], se3[1:])[0].all()
        if w == 1:
            assert all(len(r[1]) == len(p) for p, r in zip(paths, res))
    for a, b in zip(WINDOWS[:-1], WINDOWS[1:]):
        assert all(rb[3] <= ra[3] for ra, rb in zip(by_window[a], by_window[b])), (a, b)
    assert all(np.isfinite(r[3]) for r in by_window[1])
    # the condition that keeps the above from passing on inputs nothing can be cut from
    long_ones = [(nodes, r) for (nodes, se3), r in zip(both, by_window[64]) if len(se3) >= 20]
    fewer = sum(len(r[1]) < len(nodes) for nodes, r in long_ones)
    diagonal = 0
    for nodes, r in long_ones:
        a, b = nodes[r[1][:-1]], nodes[r[1][1:]]
        diagonal += int((((a[:, 0] != b[:, 0]) | (a[:, 1] != b[:, 1])) & (a[:, 2] != b[:, 2])).sum())
    kept, came = sum(len(r[1]) for _, r in long_ones), sum(len(nodes) for nodes, _ in long_ones)
    print(f"  {fewer} of {len(long_ones)} paths of 20 states or more came back shorter ({kept} of {came} states); "
          f"{diagonal} kept shortcuts change cell and heading; cost at windows 1 and 64: "
          f"{sum(r[3] for r in by_window[1]):.3f} and {sum(r[3] for r in by_window[64]):.3f}")
    assert len(long_ones) >= 4 and 2 * fewer >= len(long_ones) and diagonal >= 1


# ---- 5. an input that does not pass -------------------------------------------------------------------------------------
def test_an_input_with_a_failing_move_comes_back_unchanged(perlin):
    """Status 1 is the host routine's "no chain of usable candidates reaches the last state".  At window 1 the candidates
    are the input's own moves, so one rejected move is enough.  A wider window may find a way round it, as the host
    routine does with all pairs: then the result is an ordinary one, and must pass the checks like any other."""
    ctx = perlin.ctx
    good = [se3 for _, se3 in perlin.paths(1)][:3]
    with perlin.field(1) as f:
        raw = [f.path(t)[1] for t in perlin.far if f.path(t) is not None]
        bad = [p for p in raw if len(p) > 1 and not ctx.check_motions(p[:-1], p[1:]).all()]
        assert len(bad) >= 4                                   # as test_cost_field_plan.py finds it on this map
        mixed = [good[0], bad[0], good[1], bad[1], good[2]]
        for window in (1, 7):
            alone = f.simplify(good, window=window)
            res = f.simplify(mixed, window=window)
            same_answers([res[0], res[2], res[4]], alone)      # the other paths of the call are unaffected
            for r, p in ((res[1], bad[0]), (res[3], bad[1])):
                if window == 1:
                    assert r[0] == 1
                if r[0] == 1:
                    assert list(r[1]) == list(range(len(p))) and np.array_equal(bits_of(r[2]), bits_of(p)) and r[3] == np.inf
                else:
                    assert r[0] == 0 and np.isfinite(r[3]) and np.array_equal(bits_of(r[2]), bits_of(p[r[1]]))
                    assert ctx.check_motions(r[2][:-1], r[2][1:]).all()
                    assert ctx.check_edges_interp(r[2][:-1], r[2][1:])[0].all()
            print(f"  window {window}: statuses {[r[0] for r in res]}")


# ---- 6. plan(simplify=True) -------------------------------------------------------------------------------------------
def test_plan_with_simplify_equals_plan_then_simplify(perlin):
    targets = perlin.far[::2] + [(0, 0, 0)]
    with perlin.field(1) as f, perlin.field(1) as g:
        got = f.plan(targets, simplify=True, window=16)
        plain = g.plan(targets)
        simple = g.simplify(plain, window=16)
    assert any(r[0] == 0 for r in plain) and any(r[0] != 0 for r in plain)
    for a, b, s in zip(got, plain, simple):
        assert len(b) == 4 and a[0] == b[0] and same_bits(a[3], b[3])
        if b[0] != 0:
            assert len(a) == 4 and a[1] is None and s is None
            continue
        assert len(a) == 6 and np.array_equal(a[1], b[1]) and np.array_equal(bits_of(a[2]), bits_of(b[2]))
        assert s[0] == 0 and np.array_equal(bits_of(a[4]), bits_of(s[2])) and same_bits(a[5], s[3])


# ---- 7. refusals and capacity ---------------------------------------------------------------------------------------
def raw_call(f, paths, window, cap, batch=0):
    n = len(paths)
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum([len(p) for p in paths])
    se3_in = np.concatenate(paths)
    prm = _capi.FieldSimplifyParams(window, 0, batch)
    out = dict(st=np.full(n, -7, np.int32), cost=np.full(n, -7.0), off=np.full(n + 1, 77, np.uint64),
               kept=np.full(max(cap, 1), 77, np.uint32), se3=np.full((max(cap, 1), 7), -7.0))
    rc = f.L.artp_field_simplify_paths(f.h, C.byref(prm), se3_in.ctypes.data, off.ctypes.data, n, out["st"].ctypes.data,
                                       out["cost"].ctypes.data, out["off"].ctypes.data, out["kept"].ctypes.data,
                                       out["se3"].ctypes.data, cap)
    return rc, out


def test_capacity_offsets_and_a_clearance_field(flat):
    _, path = flat.run_turn_run(12, 9)
    paths = [path, path[:10]]
    with flat.field(1) as f:
        want = f.simplify(paths, window=7)
        total = sum(len(w[1]) for w in want)
        assert total < len(path) + 10
        rc, out = raw_call(f, paths, 7, total - 1)
        assert rc == -5 and list(out["off"]) == [0, len(want[0][1]), total] and list(out["st"]) == [0, 0]
        assert same_bits(out["cost"][0], want[0][3]) and (out["kept"] == 77).all() and (out["se3"] == -7.0).all()
        assert "cap_states" in f.L.artp_last_error(flat.ctx.h).decode()
        rc, out = raw_call(f, paths, 7, int(out["off"][2]))
        assert rc == 0 and np.array_equal(out["kept"], np.concatenate([w[1] for w in want]))
        assert np.array_equal(bits_of(out["se3"]), bits_of(np.concatenate([w[2] for w in want])))
        # offsets that do not ascend: nothing is written
        n = 2
        off = np.array([0, 12, 5], np.uint64)
        prm = _capi.FieldSimplifyParams(7, 0, 0)
        st, cost, ooff = np.full(n, -7, np.int32), np.full(n, -7.0), np.full(n + 1, 77, np.uint64)
        rc = f.L.artp_field_simplify_paths(f.h, C.byref(prm), path.ctypes.data, off.ctypes.data, n, st.ctypes.data,
                                           cost.ctypes.data, ooff.ctypes.data, None, None, 0)
        assert rc == -1 and (st == -7).all() and (cost == -7.0).all() and (ooff == 77).all()
        # statuses and costs alone
        off = np.array([0, len(path)], np.uint64)
        rc = f.L.artp_field_simplify_paths(f.h, C.byref(prm), path.ctypes.data, off.ctypes.data, 1, st.ctypes.data,
                                           cost.ctypes.data, None, None, None, 0)
        assert rc == 0 and st[0] == 0 and same_bits(cost[0], want[0][3])
    # a clearance-weighted field is accepted and priced without its weights: at gain 0 and at gain 2 the plain field's bits
    for gain in (0.0, 2.0):
        with flat.ctx.clearance_cost_field(flat.mask, N_YAW, [(0, 0, 0)], rect=flat.rect, objective=1, margin=0.2,
                                           gain=gain) as g:
            same_answers(g.simplify(paths, window=7), want)


def test_refusals(flat):
    _, path = flat.run_turn_run(6, 6)
    ctx = flat.ctx
    with flat.field(1) as f:
        assert f.simplify([path], window=4)[0][0] == 0
        # without z bounds checkMotion cannot run: a second context that holds the layers and nothing else
        gm = flat.gm
        bare = new_context()
        try:
            bare.upload_layer(0, gm["elevation"], gm.len_x, gm.len_y, gm.pos_x, gm.pos_y)
            bare.upload_layer(1, gm["elevation_masked"], gm.len_x, gm.len_y, gm.pos_x, gm.pos_y)
            ls = [np.asfortranarray(gm["cum_prob"], np.float32), np.ascontiguousarray(gm["cum_prob_rowwise"], np.float32)] + \
                 [np.asfortranarray(gm[k], np.float32) for k in ("elevation", "normal_x", "normal_y", "normal_z",
                                                                 "plane_fit_std_dev")]
            bare._chk(bare.L.artp_upload_sampler_layers(bare.h, *[a.ctypes.data for a in ls], gm.rows, gm.cols,
                                                        gm.len_x, gm.len_y, gm.pos_x, gm.pos_y), "sampler layers")
            small = np.full((4, 4), 1, np.uint32)
            with bare.cost_field(small, 1, [(0, 0, 0)], rect=(100, 100, 4, 4)) as b:
                with pytest.raises(_capi.ArtpError) as e:
                    b.simplify([bare.reachability_poses(1, (100, 100, 4, 4))[0, :3, 0]], window=2)
                assert e.value.status == -4 and "artp_set_z_bounds" in str(e.value)
        finally:
            bare.close()
        # after a layer update the poses the field stands for are gone
        ctx.update_layer_rect(0, np.zeros((4, 4), np.float32), 0, 0)
        with pytest.raises(_capi.ArtpError) as e:
            f.simplify([path], window=4)
        assert e.value.status == -1 and "map changed" in str(e.value)
    with flat.field(1) as f:                                   # a new field on the new version works again
        assert f.simplify([path], window=4)[0][0] == 0


def test_a_learned_field_is_refused():
    from test_cost_field_learned import RECT, WEIGHTS, random_mask
    from test_cost_field_learned_update import State
    c = new_context()
    try:
        S = State(c)
        S.set(1, "real", 0)
        mask = random_mask(RECT[2:], 4, 51, p=0.9)
        src = tup(np.argwhere(mask & 1)[0]) + (0,)
        with c.learned_cost_field(mask, 4, [src], rect=RECT, **WEIGHTS) as f:
            poses = c.reachability_poses(4, RECT)
            with pytest.raises(_capi.ArtpError) as e:
                f.simplify([poses[src[0], src[1], :3]], window=2)
            assert e.value.status == -1 and "learned" in str(e.value)
    finally:
        c.close()
