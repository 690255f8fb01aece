"""checkMotion and the 0.5 m rule at every segment count, failure position and empty run (-m gpu).

Every probe family of tests/edge_probe.py (tests/test_edge_probe.py proves on the CPU what each one reaches, and that
the float64 restatement equals the C oracle, states to 1e-12: the GPU is tied to the oracle's states at 2e-12) through check_motions, check_motions_last_valid, check_edges_interp and
their _dev forms: verdicts and counts EXACT, lastValid.second EXACT, lastValid states to 1e-12 of the restatement; the
batch pipeline, the few-edge kernel and the resident pool equal to one another bit for bit (two NaNs count as equal: the
state of the nd == 0, t = -inf case); the slot behind the last edge of every _dev output keeps its sentinel; the map
version does not move.  Segment counts of checkMotion are not returned by the library: the probes that target them end
on an invalid state, so that lastValid.second = (j - 1) / nd shows nd."""
import numpy as np
import pytest

import edge_probe as EP

pytestmark = pytest.mark.gpu

SENT_U8, SENT_F, SENT_I = 0xA5, -7.0, -5


@pytest.fixture(scope="module")
def ctxs():
    from art_planner_amd.context import Context
    made = {}
    for name, fn in EP.MAPS.items():
        c = Context(0, "yaml")
        c.upload_map(fn(), sampler=False)          # no sampler layers: the edge kernels do not read them
        made[name] = (c, c.map_version())
    yield made
    for c, ver in made.values():
        assert c.map_version() == ver
        c.close()


@pytest.fixture
def use(ctxs):
    """ctx of a batch with its frozen extent set; everything back to the defaults afterwards, map version unchanged."""
    touched = []

    def get(b):
        c, _ = ctxs[b.map]
        c.set_r3_extent(b.frozen)
        touched.append(b.map)
        return c

    yield get
    for name in touched:
        c, ver = ctxs[name]
        c.set_r3_extent(0.0)
        c.set_edge_passes(True, 0)
        c.set_few_edges(True)
        c.set_persistent_latency(False)
        assert c.map_version() == ver
        if name == "shared":                       # the context stays usable
            assert c.validate_states(EP.se3(-2.0, -3.0, 0.0))[0] == 1


same = EP.same


def assert_ref(ref, idx, ok=None, t=None, st=None, count=None, what=""):
    if ok is not None:
        bad = np.flatnonzero(ok != ref.valid[idx])
        assert not len(bad), f"{what}: {len(bad)} verdicts differ, first at edge {bad[0]} (count {ref.count[idx][bad[0]]})"
    if count is not None:
        assert np.array_equal(count, ref.count[idx]), f"{what}: counts"
    if t is not None:
        bad = np.flatnonzero(~((t == ref.t[idx]) | (np.isnan(t) & np.isnan(ref.t[idx]))))
        assert not len(bad), f"{what}: lastValid.second differs on {len(bad)} edges, first {bad[0]}: {t[bad[0]]} != {ref.t[idx][bad[0]]}"
    if st is not None:
        assert same(st, ref.st[idx], 1e-12), f"{what}: lastValid states beyond 1e-12"


def dev_motions(ctx, s1, s2, want_last):
    """The _dev forms with one sentinel slot behind every output."""
    import torch
    n = len(s1)
    a, b = torch.from_numpy(np.ascontiguousarray(s1)).cuda(), torch.from_numpy(np.ascontiguousarray(s2)).cuda()
    v = torch.full((n + 1,), SENT_U8, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    if not want_last:
        ctx.check_motions_dev(a, b, v)
        ctx.synchronize()
        torch.cuda.synchronize()
        h = v.cpu().numpy()
        assert h[n] == SENT_U8, "check_motions_dev wrote behind the last edge"
        return h[:n]
    t = torch.full((n + 1,), SENT_F, dtype=torch.float64, device="cuda")
    st = torch.full((7 * (n + 1),), SENT_F, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    ctx.check_motions_last_valid_dev(a, b, v, t, st)
    ctx.synchronize()
    torch.cuda.synchronize()
    hv, ht, hs = v.cpu().numpy(), t.cpu().numpy(), st.cpu().numpy()
    assert hv[n] == SENT_U8 and ht[n] == SENT_F and (hs[7 * n:] == SENT_F).all(), "check_motions_last_valid_dev wrote behind the last edge"
    return hv[:n], ht[:n], hs[:7 * n].reshape(n, 7)


def dev_interp(ctx, s1, s2):
    import torch
    n = len(s1)
    a, b = torch.from_numpy(np.ascontiguousarray(s1)).cuda(), torch.from_numpy(np.ascontiguousarray(s2)).cuda()
    v = torch.full((n + 1,), SENT_U8, dtype=torch.uint8, device="cuda")
    ni = torch.full((n + 1,), SENT_I, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.check_edges_interp_dev(a, b, v, ni)
    ctx.synchronize()
    torch.cuda.synchronize()
    hv, hn = v.cpu().numpy(), ni.cpu().numpy()
    assert hv[n] == SENT_U8 and hn[n] == SENT_I, "check_edges_interp_dev wrote behind the last edge"
    return hv[:n], hn[:n].astype(np.int64)


def in_calls(ctx, b, calls):
    """The host entry points on slices of a batch: (verdicts of check_motions, then ok / t / states of lastValid) for
    mode 0, (verdicts, counts) for mode 1, concatenated."""
    out = [[] for _ in range(4)]
    for lo, hi in calls:
        if b.mode == 0:
            out[0].append(ctx.check_motions(b.s1[lo:hi], b.s2[lo:hi]))
            ok, t, st = ctx.check_motions_last_valid(b.s1[lo:hi], b.s2[lo:hi])
            out[1].append(ok), out[2].append(t), out[3].append(st)
        else:
            ok, ni = ctx.check_edges_interp(b.s1[lo:hi], b.s2[lo:hi])
            out[0].append(ok), out[1].append(ni.astype(np.int64))
    return [np.concatenate(o) for o in out if o]


def every_form(ctx, b, ref, what):
    """A small batch through the batch pipeline (host and _dev), and in calls of at most 64 edges through the few-edge
    kernel: all against the reference, the forms against one another."""
    idx = np.arange(b.n)
    calls = [(i, min(i + 64, b.n)) for i in range(0, b.n, 64)]
    if b.mode == 1:
        ctx.set_few_edges(False)
        bv, bn = ctx.check_edges_interp(b.s1, b.s2)
        ctx.set_few_edges(True)
        assert_ref(ref, idx, ok=bv, count=bn.astype(np.int64), what=f"{what} batch")
        dv, dn = dev_interp(ctx, b.s1, b.s2)
        fv, fn = in_calls(ctx, b, calls)
        assert np.array_equal(dv, bv) and np.array_equal(dn, bn) and np.array_equal(fv, bv) and np.array_equal(fn, bn), what
        return
    ctx.set_few_edges(False)
    bv = ctx.check_motions(b.s1, b.s2)
    bok, bt, bst = ctx.check_motions_last_valid(b.s1, b.s2)
    ctx.set_few_edges(True)
    assert_ref(ref, idx, ok=bv, what=f"{what} batch check_motions")
    assert_ref(ref, idx, ok=bok, t=bt, st=bst, what=f"{what} batch lastValid")
    dv = dev_motions(ctx, b.s1, b.s2, False)
    dok, dt, dst = dev_motions(ctx, b.s1, b.s2, True)
    fv, fok, ft, fst = in_calls(ctx, b, calls)
    for name, (v, ok, t, st) in {"dev": (dv, dok, dt, dst), "few": (fv, fok, ft, fst)}.items():
        assert np.array_equal(v, bv) and np.array_equal(ok, bok), f"{what}: {name} verdicts != batch"
        assert same(t, bt) and same(st, bst), f"{what}: {name} lastValid pair != batch, bit for bit"


# ---- failure position, thresholds, empty runs of pass 2: the batch forms under every split ----------------------------------
PASSES = [(False, 0)] + [(True, S) for S in EP.STRIDES]


def under_every_split(ctx, b, ref, what):
    idx = np.arange(b.n)
    for two, S in PASSES:
        ctx.set_edge_passes(two, S)
        assert_ref(ref, idx, ok=ctx.check_motions(b.s1, b.s2), what=f"{what} passes={two} S={S}")
        assert_ref(ref, idx, ok=dev_motions(ctx, b.s1, b.s2, False), what=f"{what} dev passes={two} S={S}")
    ctx.set_edge_passes(True, 0)


@pytest.mark.parametrize("bi", range(EP.BATCH_COUNTS["failure_position"]))
def test_failure_position(use, bi):
    b, ref = EP.failure_position()[bi], EP.ref_of("failure_position", bi)
    ctx = use(b)
    under_every_split(ctx, b, ref, b.name)
    ok, t, st = ctx.check_motions_last_valid(b.s1, b.s2)
    assert_ref(ref, np.arange(b.n), ok=ok, t=t, st=st, what=f"{b.name} lastValid")
    dok, dt, dst = dev_motions(ctx, b.s1, b.s2, True)
    assert np.array_equal(dok, ok) and same(dt, t) and same(dst, st)
    # the probes through the few-edge kernel, 64 per call
    p = b.meta["probe"]
    sub = EP.Batch(b.name, 0, b.s1[p], b.s2[p], b.frozen)
    fv, fok, ft, fst = in_calls(ctx, sub, [(i, min(i + 64, sub.n)) for i in range(0, sub.n, 64)])
    assert_ref(ref, p, ok=fv, what=f"{b.name} few")
    assert np.array_equal(fok, ok[p]) and same(ft, t[p]) and same(fst, st[p]), f"{b.name}: few lastValid != batch"


@pytest.mark.parametrize("bi", range(EP.BATCH_COUNTS["thresholds"]))
def test_form_thresholds(use, bi):
    b, ref = EP.thresholds()[bi], EP.ref_of("thresholds", bi)
    ctx = use(b)
    under_every_split(ctx, b, ref, b.name)
    ok, t, st = ctx.check_motions_last_valid(b.s1, b.s2)       # lastValid asked: one pass whatever the size
    assert_ref(ref, np.arange(b.n), ok=ok, t=t, st=st, what=f"{b.name} lastValid")
    dok, dt, dst = dev_motions(ctx, b.s1, b.s2, True)
    assert np.array_equal(dok, ok) and same(dt, t) and same(dst, st)


@pytest.mark.parametrize("bi", range(EP.BATCH_COUNTS["empty_runs_two_pass"]))
def test_empty_runs_in_pass_two(use, bi):
    b, ref = EP.empty_runs_two_pass()[bi], EP.ref_of("empty_runs_two_pass", bi)
    under_every_split(use(b), b, ref, b.name)


def test_empty_runs_of_the_half_metre_rule(use):
    for bi, b in enumerate(EP.empty_runs_interp()):
        ref = EP.ref_of("empty_runs_interp", bi)
        ctx = use(b)
        ok, ni = ctx.check_edges_interp(b.s1, b.s2)
        assert_ref(ref, np.arange(b.n), ok=ok, count=ni.astype(np.int64), what=b.name)
        dv, dn = dev_interp(ctx, b.s1, b.s2)
        assert np.array_equal(dv, ok) and np.array_equal(dn, ni), b.name


# ---- small families: every form ----------------------------------------------------------------------------------------------
SMALL = [(f, i) for f in ("s2_only", "count_boundaries", "quaternion_edges") for i in range(EP.BATCH_COUNTS[f])]


@pytest.mark.parametrize("fam,bi", SMALL, ids=[f"{f}-{i}" for f, i in SMALL])
def test_small_families_through_every_form(use, fam, bi):
    b, ref = EP.FAMILIES[fam]()[bi], EP.ref_of(fam, bi)
    every_form(use(b), b, ref, b.name)


# ---- few-edge team sizes -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bi", range(EP.BATCH_COUNTS["few_edges"]))
def test_few_edge_team_sizes(use, bi):
    """Each call 20 times (a word that was not re-armed shows in the next call), then once through the batch pipeline."""
    b, ref = EP.few_edges()[bi], EP.ref_of("few_edges", bi)
    ctx = use(b)
    calls = b.meta["calls"]
    idx = np.concatenate([np.arange(lo, hi) for lo, hi in calls])
    ctx.set_few_edges(False)
    want = in_calls(ctx, b, calls)
    ctx.set_few_edges(True)
    if b.mode == 0:
        assert_ref(ref, idx, ok=want[0], what=f"{b.name} batch")
        assert_ref(ref, idx, ok=want[1], t=want[2], st=want[3], what=f"{b.name} batch lastValid")
    else:
        assert_ref(ref, idx, ok=want[0], count=want[1], what=f"{b.name} batch")
    for rep in range(20):
        got = in_calls(ctx, b, calls)
        for k, (g, w) in enumerate(zip(got, want)):
            assert same(g, w), f"{b.name}: repeat {rep}, output {k} of the few-edge kernel != batch pipeline"


# ---- pool ------------------------------------------------------------------------------------------------------------------------
POOL = [("pool_subset", 0), ("quaternion_edges", 0), ("s2_only", 0), ("count_boundaries", 0), ("count_boundaries", 2)]


@pytest.mark.parametrize("fam,bi", POOL, ids=[f"{f}-{i}" for f, i in POOL])
def test_pool_one_and_two_edges_per_call(use, fam, bi):
    """Calls of one and two edges with the resident pool on, against the batch pipeline bit for bit.  Every call here is
    short enough for run_edges_host's pool condition (longest edge: 100 segments; estimate * n <= 8 * 256 workgroups), so
    the pool must have answered EVERY call: a call that fell back to the few-edge kernel is a failure of this test."""
    b, ref = EP.batch(fam, bi), EP.ref_of(fam, bi)
    ctx = use(b)
    idx = np.arange(b.n)
    calls, i, k = [], 0, 1
    while i < b.n:
        calls.append((i, min(i + k, b.n)))
        i, k = calls[-1][1], k % 2 + 1
    ctx.set_few_edges(False)
    want = in_calls(ctx, b, [(0, b.n)])
    ctx.set_few_edges(True)
    if b.mode == 0:
        assert_ref(ref, idx, ok=want[0], what=f"{b.name} batch")
        assert_ref(ref, idx, ok=want[1], t=want[2], st=want[3], what=f"{b.name} batch lastValid")
    else:
        assert_ref(ref, idx, ok=want[0], count=want[1], what=f"{b.name} batch")
    ctx.set_persistent_latency(True)
    before = ctx.persistent_latency_stats()["requests"]
    got = in_calls(ctx, b, calls)
    used = ctx.persistent_latency_stats()["requests"] - before
    ctx.set_persistent_latency(False)
    for k, (g, w) in enumerate(zip(got, want)):
        assert same(g, w), f"{b.name}: output {k} of the pool != batch pipeline, bit for bit"
    per_call = 2 if b.mode == 0 else 1            # check_motions and check_motions_last_valid / check_edges_interp
    assert used == per_call * len(calls), f"{b.name}: the pool answered {used} of {per_call * len(calls)} calls"
