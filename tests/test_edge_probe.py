"""The edge probes probe (CPU).  tests/test_edge_sweep.py compares the edge kernels with the float64 restatement of
tests/edge_probe.py on its probe families; that comparison is worth what the probes reach and what the restatement
is worth.  Here, without a GPU:

  * the restatement gives the C oracle's verdicts, counts and lastValid.second exactly and its states to 1e-12 (the bar
    of test_check_motion_last_valid_golden) on the edges of every family, so neither reference is trusted alone.  The
    oracle has no frozen-extent parameter: for batches with a frozen extent the COUNTS are compared under that extent
    (through a copy of the oracle's geometry) and the lastValid states at the restatement's own t; verdicts and
    lastValid.second are compared on the same edges under the map's own extent;
  * every family reaches what it targets (counted on the reference alone);
  * a Python copy of the arithmetic mutations (a), (b), (c), (d), (e), (f), (g), (h), (i) of the sweep's issue changes the
    restatement's answer on a probe of the family that targets it."""
import ctypes as C

import numpy as np
import pytest

import edge_probe as EP
import oracle_py as O

_same = EP.same


def test_batch_counts_are_the_families():
    assert EP.BATCH_COUNTS == {f: len(fn()) for f, fn in EP.FAMILIES.items()}
    names = [b.name for _, _, b in EP.all_batches()]
    assert len(set(names)) == len(names)


@pytest.mark.parametrize("fam,idx", EP.BATCH_IDS, ids=[f"{f}-{i}" for f, i in EP.BATCH_IDS])
def test_restatement_equals_the_c_oracle(fam, idx):
    """On the distinct edges of the batch (padding repeats a few hundred valid edges)."""
    b, ref = EP.batch(fam, idx), EP.ref_of(fam, idx)
    gm, rob = EP.MAPS[b.map](), EP.robot()
    om = O.OracleMap(gm)
    _, first = np.unique(np.concatenate([b.s1, b.s2], axis=1), axis=0, return_index=True)
    first = np.sort(first)
    s1, s2 = b.s1[first], b.s2[first]
    if b.mode == 1:
        ok, ni = om.edges_interp_valid(rob, s1, s2)
        assert np.array_equal(ni, ref.count[first]) and np.array_equal(ok, ref.valid[first])
        pick = np.flatnonzero(np.isin(ref.e, first))[:3000]
        for q in pick:
            e, k, n = ref.e[q], ref.j[q], ref.count[ref.e[q]]
            assert _same(O.interpolate(b.s1[e], b.s2[e], (k + 1) * (1.0 / (n + 1))), ref.states[q], 1e-12)
        return
    # Counts under a frozen extent: the oracle takes the extent from its map, so it is given a COPY of the geometry whose
    # own extent is that number (len_x = frozen / 2, len_y = 0, z extent 0; exact, see the test below).  Verdicts and the
    # lastValid pair need the real geometry for isValid: they are compared under the map's own extent, on the same edges.
    L = O.lib()
    m2, zext = O.Map.from_buffer_copy(om.m), om.z_extent(rob)
    if b.frozen > 0.0:
        m2.len_x, m2.len_y, zext = b.frozen / 2, 0.0, 0.0
    nd = np.array([L.artp_oracle_valid_segment_count(C.byref(m2), zext, s1[i].ctypes.data, s2[i].ctypes.data)
                   for i in range(len(s1))])
    assert np.array_equal(nd, ref.count[first]), np.flatnonzero(nd != ref.count[first])[:10]
    own = EP.reference(gm, rob, 0, s1, s2, 0.0) if b.frozen > 0.0 else None
    want_valid, want_t, want_st = (own.valid, own.t, own.st) if own else (ref.valid[first], ref.t[first], ref.st[first])
    okc, _ = om.check_motions(rob, s1, s2)
    ok, t, st = om.check_motions_last_valid(rob, s1, s2)
    assert np.array_equal(okc, want_valid) and np.array_equal(ok, want_valid)
    assert _same(t, want_t), "lastValid.second"
    assert _same(st, want_st, 1e-12), "lastValid state"
    if own:
        assert np.array_equal(om.segment_counts(rob, s1, s2), own.count)
        for i in np.flatnonzero(ref.valid[first] == 0)[:300]:       # the frozen batch's own lastValid states
            assert _same(O.interpolate(s1[i], s2[i], ref.t[first][i]), ref.st[first][i], 1e-12)
    pick = np.flatnonzero(np.isin(ref.e, first[:400]))[:3000]
    for q in pick:
        e, j, n = ref.e[q], ref.j[q], ref.count[ref.e[q]]
        want = b.s2[e] if j == n or n == 0 else O.interpolate(b.s1[e], b.s2[e], float(j) / float(n))
        assert _same(want, ref.states[q], 1e-12)


def test_frozen_extent_through_the_oracle_geometry_is_exact():
    """The trick above: (len_x, len_y, z) = (frozen / 2, 0, 0) gives the oracle exactly the segment frozen * 0.01."""
    for frozen in (12.5, 6.25, 0.3125, 100 * EP.FEW_SEG):
        ex = (0.0 + frozen / 2) - (0.0 - frozen / 2)
        assert np.sqrt(ex * ex + 0.0 + 0.0) * 0.01 == frozen * 0.01
    for frozen in (12.5, 6.25, 100 * EP.FEW_SEG):
        assert np.log2(frozen * 0.01) == np.round(np.log2(frozen * 0.01))     # a power of two


def _runs(ref, i):
    """(first j, length, js) of the invalid interior run of edge i; asserts that it is ONE run."""
    js = ref.bad_interior(i)
    assert len(js) and (np.diff(js) == 1).all(), (i, js)
    return int(js[0]), len(js), js


def test_failure_position_coverage():
    seen_nd = set()
    start_res = {S: np.zeros(S, int) for S in EP.STRIDES}
    only2 = {S: 0 for S in EP.STRIDES}
    only1 = {S: 0 for S in EP.STRIDES}
    lengths = set()
    for bi, b in enumerate(EP.failure_position()):
        ref = EP.ref_of("failure_position", bi)
        assert b.n >= 4096 and EP.plan_total(ref) >= 24 * b.n
        probe, tag = b.meta["probe"], b.meta["tag"]
        rest = np.setdiff1d(np.arange(b.n), probe)
        assert ref.valid[rest].all() and (ref.count[rest] == 48).all()       # the padding is valid
        for i, (nd, j) in zip(probe, tag):
            assert ref.count[i] == nd
            j0, ln, js = _runs(ref, i)
            assert j0 == j and 1 <= ln <= 3, (nd, j, j0, ln)
            assert ref.ok_of_task(i)[0] or j0 + ln == nd                    # s2 is valid unless the run reaches it
            seen_nd.add((int(nd), int(j)))
            lengths.add(ln)
            for S in EP.STRIDES:
                start_res[S][j0 % S] += 1
                mult = js % S == 0
                only2[S] += not mult.any()
                only1[S] += ln == 1 and bool(mult[0])
    assert seen_nd >= {(nd, j) for nd in EP.ND_LIST for j in range(1, nd)}
    assert lengths == {1, 2, 3}
    for S in EP.STRIDES:
        assert {S - 1, S, S + 1, 2 * S, 2 * S + 1} - {1} <= set(EP.ND_LIST)
        assert start_res[S].min() >= 20, (S, start_res[S])
        assert only2[S] >= 20 and only1[S] >= 20, (S, only2[S], only1[S])
    print("failure position: starts per residue", {S: v.tolist() for S, v in start_res.items()}, "only pass 2", only2,
          "only pass 1", only1)


def test_s2_only_edges():
    b, ref = EP.s2_only()[0], EP.ref_of("s2_only", 0)
    assert ref.count.tolist() == b.meta["nd"]
    assert not ref.valid.any() and np.array_equal(ref.first_bad, ref.count)      # only s2 fails
    assert ref.t[0] == -np.inf and np.isnan(ref.st[0, :3]).all() and np.array_equal(ref.st[0, 3:], b.s1[0, 3:])
    rot = np.arange(21, 41)
    assert (ref.n_r3[rot] == 0).all() and np.array_equal(ref.n_so3[rot], ref.count[rot])
    assert np.array_equal(ref.t[1:], (ref.count[1:] - 1) / ref.count[1:])


def test_count_boundaries():
    bs = EP.count_boundaries()
    for bi, b in enumerate(bs):
        ref = EP.ref_of("count_boundaries", bi)
        lo = 12 if b.name == "counts_rect" else 0       # no exact multiples of the segment on the map's own extent
        assert np.array_equal(ref.count[lo:], b.meta["want"][lo:]), (b.name, ref.count, b.meta["want"])
    b, ref = bs[0], EP.ref_of("count_boundaries", 0)
    x = np.abs(b.s1[:12, 0] - b.s2[:12, 0]) / 0.125                             # exact: the segment is 2^-3
    ks = np.repeat(EP.KS, 3)
    assert np.array_equal(x[0::3], ks[0::3])
    assert np.array_equal(x[1::3], np.nextafter(ks[1::3] * 0.125, 0) / 0.125)      # ONE ulp of the length
    assert np.array_equal(x[2::3], np.nextafter(ks[2::3] * 0.125, 99) / 0.125)
    d2 = (b.s1[:12, 0] - b.s2[:12, 0]) ** 2
    assert np.array_equal(np.sqrt(d2) / 0.125, x)                                   # and sqrt(d2) / seg keeps it
    assert not ref.valid.any() and (ref.t[ref.count > 1] > 0).all()              # lastValid.second depends on nd everywhere
    rotn = slice(12, 20)
    assert (ref.n_r3[rotn] == 0).all()
    mix = slice(20, 26)
    assert sorted((ref.n_so3[mix] - ref.n_r3[mix]).tolist()) == [-1, -1, -1, 1, 1, 1]
    gm = EP.rect_map()
    assert gm.len_x != gm.len_y and (gm.pos_x, gm.pos_y) != (0.0, 0.0)
    b2, r2 = bs[2], EP.ref_of("count_boundaries", 2)
    L = np.hypot(b2.s2[:, 0] - b2.s1[:, 0], b2.s2[:, 1] - b2.s1[:, 1])
    assert set(np.round(L[np.abs(L / 0.5 - np.round(L / 0.5)) == 0] / 0.5).astype(int)) == set(EP.KS)
    assert 0 < r2.valid.sum() < b2.n


def test_quaternion_edges_reach_the_branches():
    b, ref = EP.quaternion_edges()[0], EP.ref_of("quaternion_edges", 0)
    dot = EP.quat_dot(b.s1, b.s2)
    theta = EP.so3_arc(b.s1, b.s2)
    shows = (ref.valid == 0) & (ref.first_bad >= 2) & (ref.first_bad < ref.count)   # lastValid state is an interior slerp
    classes = {"copy, negative dot": (theta == 0) & (dot < 0), "copy, positive dot": (theta == 0) & (dot > 0),
               "slerp, negative dot": (theta > 0) & (dot < 0), "slerp, positive dot": (theta > 0) & (dot > 0),
               "half turn -": (np.abs(dot) < 1e-5) & (dot < 0), "half turn +": (np.abs(dot) < 1e-5) & (dot > 0),
               "below cut-off": (theta == 0) & (np.abs(dot) < 1 - 0.9e-9), "above cut-off": (theta > 0) & (theta < 5e-5)}
    for name, m in classes.items():
        assert (m & shows).sum() >= 2, name
    assert ((theta == 0) & (dot < 0) & (ref.count == 0) & (ref.t == -np.inf)).any()    # b = -a on an invalid state
    assert ((ref.count == 0) & (ref.valid == 1)).any()


def _zero_runs(counts):
    """(start, length) of the maximal runs of zero counts."""
    z = np.concatenate([[0], (counts == 0).astype(int), [0]])
    d = np.diff(z)
    return list(zip(np.flatnonzero(d == 1), np.flatnonzero(d == -1) - np.flatnonzero(d == 1)))


def test_empty_runs_of_the_half_metre_rule_reach_every_lane():
    seen = set()
    bs = EP.empty_runs_interp()
    for bi, b in enumerate(bs):
        ref = EP.ref_of("empty_runs_interp", bi)
        assert b.n <= 5000
        off = np.cumsum(ref.count) - ref.count
        for start, ln in _zero_runs(ref.count):
            seen.add((int(ln), int(off[start] % 64)))
            if start + ln < b.n:       # the edge behind a run is invalid (in one or two states), the one before valid
                assert ref.valid[start + ln] == 0 and (start == 0 or ref.valid[start - 1] == 1)
                lo, hi = np.searchsorted(ref.e, [start + ln, start + ln + 1])
                assert 1 <= (ref.ok[lo:hi] == 0).sum() <= 2
        assert ref.valid[ref.count == 0].all()
    assert seen >= {(R, lane) for R in EP.RUNS for lane in range(64)}
    r0, rl = EP.ref_of("empty_runs_interp", 0), EP.ref_of("empty_runs_interp", len(bs) - 3)
    assert r0.count[0] == 0 and rl.count[-1] == 0                                # a run at the start, one at the end
    assert EP.ref_of("empty_runs_interp", len(bs) - 2).count.sum() == 0
    last = EP.ref_of("empty_runs_interp", len(bs) - 1)
    assert last.count[:-1].sum() == 0 and last.count[-1] == 3 and last.valid[-1] == 0


def _pass2_counts(ref, S):
    alive = np.array([all(ref.ok_of_task(i)[k] for k in EP.pass_tasks(int(ref.count[i]), S)[0]) for i in range(len(ref.count))])
    interior = np.maximum(ref.count - 1, 0)
    return np.where(alive, interior - interior // S, 0), alive


def test_empty_runs_of_pass_two():
    bs = EP.empty_runs_two_pass()
    shifts = {S: set() for S in EP.STRIDES}
    for bi, b in enumerate(bs):
        ref = EP.ref_of("empty_runs_two_pass", bi)
        assert b.n >= 4096 and EP.plan_total(ref) >= 24 * b.n and b.n <= 5000
        if not b.meta["runs"]:
            continue
        for S in EP.STRIDES:
            c2, alive = _pass2_counts(ref, S)
            off = np.cumsum(c2) - c2
            runs = dict(_zero_runs(c2))
            for R, start in b.meta["runs"]:
                assert runs.get(start, 0) >= R, (b.name, S, R, start)     # (a probe that dies in pass 1 may lengthen it)
                if R == 1:
                    shifts[S].add(int(off[start] % 64))
            # some probe is alive after pass 1 and dies in pass 2
            assert (alive & (ref.valid == 0)).sum() >= 20
    for S in (3, 8, 16):
        assert shifts[S] >= set(EP.LANE_SHIFTS), (S, shifts[S])
    c2, _ = _pass2_counts(EP.ref_of("empty_runs_two_pass", len(bs) - 2), 8)
    assert c2.sum() == 0
    c2, _ = _pass2_counts(EP.ref_of("empty_runs_two_pass", len(bs) - 1), 8)
    assert c2[:-1].sum() == 0 and c2[-1] > 0


def test_threshold_batches_sit_on_the_thresholds():
    got = []
    for bi, b in enumerate(EP.thresholds()):
        ref = EP.ref_of("thresholds", bi)
        assert EP.plan_total(ref) == b.meta["total"]
        got.append((b.n, EP.plan_total(ref) - 24 * b.n))
        assert 0 < ref.valid.sum() < b.n
    assert got == [(4095, 0), (4096, 0), (4097, 0), (4096, -1)]


def test_few_edge_calls_mix_the_team_sizes():
    gm, rob = EP.shared_map(), EP.robot()
    zext = EP.z_extent(gm, rob)
    bs = EP.few_edges()
    for bi, b in enumerate(bs):
        ref = EP.ref_of("few_edges", bi)
        classes = set()
        for lo, hi in b.meta["calls"]:
            assert hi - lo <= EP.FEW_EDGES
            total, mx = EP.few_estimate(gm, zext, b.frozen, b.mode, b.s1[lo:hi], b.s2[lo:hi])
            assert total <= 65536.0                                   # the call takes the few-edge kernel
            chunks = EP.few_chunks(hi - lo, mx)
            tasks = ref.count[lo:hi] if b.mode else 1 + np.maximum(ref.count[lo:hi] - 1, 0)
            for t in tasks:
                classes.add("0" if t == 0 else "1" if t == 1 else "<" if t < chunks else "=" if t == chunks else ">")
        # (the 0.5 m rule: as many tasks as chunks takes an edge of 16 m and more, longer than the map)
        want = {"0", "1", "<"} if b.mode else {"1", "<", "=", ">"}
        assert classes >= want, (b.name, classes)
        assert 0 < ref.valid.sum() < b.n
        if b.mode == 0:
            # lastValid: first failures in the last task of a stride class (the last interior state, or s2 alone)
            assert ((ref.first_bad == ref.count - 1) & (ref.count > 2)).any() and (ref.first_bad == ref.count).any()
            assert ((ref.first_bad >= 1) & (ref.first_bad <= 2)).any()


def test_pool_subset():
    b, ref = EP.pool_subset()[0], EP.ref_of("pool_subset", 0)
    assert b.n <= 200 and 0 < ref.valid.sum() < b.n and (ref.t == -np.inf).any()


# ---- the CPU half of the mutation check ------------------------------------------------------------------------------------
@pytest.mark.parametrize("mut", ["a", "b"])
def test_mutated_pass_split_changes_a_failure_position_verdict(mut):
    for S in EP.STRIDES:
        wrong = 0
        for bi, b in enumerate(EP.failure_position()):
            ref = EP.ref_of("failure_position", bi)
            assert all(EP.two_pass_verdict(ref, i, S) == bool(ref.valid[i]) for i in b.meta["probe"])
            wrong += sum(EP.two_pass_verdict(ref, i, S, mut) != bool(ref.valid[i]) for i in b.meta["probe"])
        print(f"mutation ({mut}), stride {S}: {wrong} probe verdicts change")
        assert wrong >= 1


@pytest.mark.parametrize("mut,fam,idx", [("d", "s2_only", 0), ("f", "count_boundaries", 0), ("g", "count_boundaries", 0),
                                         ("g", "s2_only", 0), ("h", "empty_runs_interp", 0), ("h", "few_edges", 6),
                                         ("e", "quaternion_edges", 0), ("i", "s2_only", 0), ("i", "few_edges", 0)])
def test_mutated_arithmetic_changes_the_answer(mut, fam, idx):
    b, ref = EP.FAMILIES[fam]()[idx], EP.ref_of(fam, idx)
    m = EP.reference(EP.MAPS[b.map](), EP.robot(), b.mode, b.s1, b.s2, b.frozen, mutate=mut)
    if b.mode == 1:
        assert not np.array_equal(m.valid, ref.valid)
    else:
        assert not (_same(m.t, ref.t) and _same(m.st, ref.st, 1e-12) and np.array_equal(m.count, ref.count)
                    and np.array_equal(m.valid, ref.valid))


def test_lane_search_restated_and_its_mutation():
    """Mutation (c) on the CPU: without the follow-on search the restated lane search gives a wrong edge to tasks behind
    the runs of 64 and more empty edges (0.5 m rule, and pass 2 of checkMotion), and to none with it."""
    ref = EP.ref_of("empty_runs_interp", 1)
    true_e, _ = EP._ragged(ref.count)
    assert np.array_equal(EP.lane_edges(ref.count), true_e)
    wrong = EP.lane_edges(ref.count, "c") != true_e
    assert wrong.sum() >= 64
    r2 = EP.ref_of("empty_runs_two_pass", 0)
    c2, _ = _pass2_counts(r2, 8)
    assert np.array_equal(EP.lane_edges(c2), EP._ragged(c2)[0])
    assert (EP.lane_edges(c2, "c") != EP._ragged(c2)[0]).any()
