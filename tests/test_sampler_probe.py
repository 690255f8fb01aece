"""The sampler probes probe (CPU).  tests/test_sampler_sweep.py compares the GPU sampler with the C oracle on the maps
of tests/sampler_probe.py; that comparison is worth what the maps reach.  Here, from the oracle alone:

  * every map puts at least CLASS_MIN of its samples into every class it is meant to reach;
  * a float64 numpy restatement of "first index exceeding u, else last" gives the oracle's cells on every map (the
    oracle reports the cell of getIndexOfPosition, so this also pins that its truncation is the scanned cell -- the
    shortcut sample_one takes -- at every origin, the UTM-sized one included);
  * the tie probes answer where they were built to, on both sides of every pair."""
import numpy as np
import pytest

import oracle_py as O
import sampler_probe as SP

PROBES = SP.all_probes()


def test_uniform01_restatement_is_the_oracles():
    L = O.lib()
    for seed in SP.SEEDS:
        for first in SP.FIRST_INDICES:
            idx = SP.indices(first, 200)
            for k in (0, 1, 2, 5, 8, 11):
                got = SP.uniform01_np(seed, idx, k)
                ref = np.array([L.artp_oracle_uniform01(seed, int(i), k) for i in idx])
                assert np.array_equal(got, ref), (seed, first, k)
    assert SP.indices((1 << 64) - 2, 4).tolist() == [(1 << 64) - 2, (1 << 64) - 1, 0, 1]


def test_rd_f32_rounds_down():
    rng = np.random.default_rng(0)
    u = np.concatenate([rng.uniform(0, 1, 10000), [0.0, 0.5, 1.0 - 2.0 ** -53, 2.0 ** -40]])
    f = SP.rd_f32(u)
    up = np.nextafter(f, np.float32(np.inf)).astype(np.float64)
    assert (f.astype(np.float64) <= u).all() and (up > u).all()


def test_the_lists_of_the_sweep_are_covered():
    names = {p.name for p in PROBES}
    assert {f"cols_{c}" for c in SP.COLS} <= names and {f"rows_{r}" for r in SP.ROWS} <= names
    assert {f"origin_{o}_{s}" for o in SP.ORIGINS for s in SP.SPACINGS} <= names
    assert {f"idx_seed{s:#x}_first{f:#x}" for s in SP.SEEDS for f in SP.FIRST_INDICES} <= names
    assert set(SP.CROSS) <= names
    for p in PROBES:
        # a batch that starts just below 2^32, or below 2^61 where index * 8 wraps, straddles that boundary
        for edge in (1 << 32, 1 << 61):
            if p.name.startswith("idx_") and 0 < edge - p.first <= 100:
                assert p.first + p.n > edge + 1000, p.name
    ties = [p for p in PROBES if p.tie and not p.name.startswith("cross")]
    assert sorted((p.gm.rows, p.gm.cols) for p in ties) == [(1, 501), (1, 601), (1001, 1), (2201, 1)]
    cross = [SP.probe(n).gm for n in SP.CROSS]
    assert cross[0].cols <= 512 and cross[1].cols > 512 and cross[2].rows > 2048 and min(
        min(g.rows, g.cols) for g in cross) >= 2
    runs = SP.probe("plateaus").extra["runs"]
    assert sorted({(L, s % 16) for _, s, L in runs}) == [(L, o) for L in SP.PLATEAUS for o in range(16)]


@pytest.mark.parametrize("p", PROBES, ids=lambda p: p.name)
def test_probe_reaches_its_classes_and_numpy_scan_agrees(p):
    _, rc = SP.oracle_samples(p)
    counts = {name: int(m.sum()) for name, m in SP.class_masks(p, rc).items()}
    print(p.name, p.gm.rows, p.gm.cols, counts)
    assert all(v >= SP.CLASS_MIN for v in counts.values()), (p.name, counts)
    assert np.array_equal(SP.scan_cells_np(p.gm, p.seed, p.first, p.n), rc), p.name


@pytest.mark.parametrize("p", [q for q in PROBES if q.tie], ids=lambda p: p.name)
def test_tie_probe_answers_at_its_pairs(p):
    """Sample k sits exactly at its pair: the first entry does not exceed u_k (it is u_k rounded down to float), the
    second does.  No draw of these batches is itself a float32 value (that takes 29 zero bits), so no entry EQUALS
    its u; the pair's first entry is the closest a float can come from below, and about half of the draws round UP to
    the pair's second entry under round-to-nearest -- the case __double2float_rd exists for."""
    t = p.tie
    k, ax = t["k"], 1 - t["axis"]
    _, rc = SP.oracle_samples(p)
    line = np.asarray(p.gm["cum_prob"])[0] if t["axis"] == 0 else np.asarray(p.gm["cum_prob_rowwise"])
    u = SP.uniform01_np(p.seed, SP.indices(p.first, k), t["axis"])
    j = t["rank"]
    assert (line[2 * j].astype(np.float64) <= u).all() and (line[2 * j + 1].astype(np.float64) > u).all()
    assert np.array_equal(line[2 * j + 1], np.nextafter(line[2 * j], np.float32(np.inf)))
    assert np.array_equal(rc[:k, ax], 2 * j + 1)
    assert t["exact"] == 0, "a draw that is a float32 value: pin it as an `entry == u` tie"
    assert t["rounds_up"] >= 50 and k - t["rounds_up"] >= 50, t["rounds_up"]
    rest = rc[k:, ax]
    assert (rest % 2 == 0).mean() > 0.99          # between two pairs the next pair's first entry answers


def test_plateau_cells_are_never_sampled():
    p = SP.probe("plateaus")
    _, rc = SP.oracle_samples(p)
    for row, start, length in p.extra["runs"]:
        c = rc[rc[:, 0] == row, 1]
        assert len(c) >= 50 and not ((c >= start) & (c < start + length)).any(), (row, start, length)
        assert (c == start + length).sum() >= 20 and (c == start - 1).sum() >= 20, (row, start, length)


def test_nan_rows_of_the_oracle():
    """All-zero rows are reached through the last row only, and end at cols - 1; a row that turns NaN at column c
    answers below c where a finite entry exceeds u and at cols - 1 otherwise (NaN > u is false: the scan runs on)."""
    p = SP.probe("zero_rows")
    _, rc = SP.oracle_samples(p)
    assert set(np.unique(rc[:, 0])) == set(range(p.gm.rows)) - set(SP.ZERO_ROWS[:-1])
    last = rc[:, 0] == p.gm.rows - 1
    assert last.sum() >= SP.CLASS_MIN and (rc[last, 1] == p.gm.cols - 1).all()
    p = SP.probe("nan_partway")
    _, rc = SP.oracle_samples(p)
    cp = np.asarray(p.gm["cum_prob"], np.float64)
    u = SP.uniform01_np(p.seed, SP.indices(p.first, p.n), 0)
    for i, c in enumerate(SP.NAN_FROM):
        sel = rc[:, 0] == i
        early = sel & (u < cp[i, c - 1])
        assert early.sum() >= SP.CLASS_MIN and (rc[early, 1] < c).all()
        late = sel & ~early
        assert late.sum() >= SP.CLASS_MIN and (rc[late, 1] == p.gm.cols - 1).all()


@pytest.mark.parametrize("res", SP.SPACINGS)
def test_utm_origin_index_of_position_is_the_scanned_cell(res):
    """getIndexOfPosition of the cell centre, 5.2e6 m from the origin where one ulp is 9.3e-10 m, truncates to the
    scanned cell for every sample: sample_one may take the cell from its search."""
    p = SP.probe(f"origin_utm_{res}")
    so, rc = SP.oracle_samples(p)
    assert np.array_equal(rc, SP.scan_cells_np(p.gm, p.seed, p.first, p.n))
    # and the states really are UTM-sized (the perturbation along the normal is below a metre)
    assert np.abs(so[:, 0] - 4.6e5).max() < 5.0 and np.abs(so[:, 1] - 5.2e6).max() < 5.0
    su, rcu = SP.oracle_samples(p, sample_uniform=True)
    assert (rcu >= 0).all() and (rcu[:, 0] < p.gm.rows).all() and (rcu[:, 1] < p.gm.cols).all()
