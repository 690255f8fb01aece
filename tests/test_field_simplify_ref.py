"""The restatement of the windowed simplifier's search (tests/field_simplify_ref.py) against brute force, its tie rule and
its monotony in the window; and the new entry points in the built library.  No device is needed."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import common
import field_simplify_ref as FS
from art_planner_amd import _capi


def tables(rng, n, p_usable, kind):
    usable = rng.random((n, n)) < p_usable
    if kind == "random":
        cost = rng.random((n, n)) * 3.0
    elif kind == "coarse":                       # few distinct values: many chains tie
        cost = rng.integers(1, 4, (n, n)).astype(np.float64) * 0.25
    else:                                        # some costs are not finite: such a pair is not usable
        cost = rng.random((n, n))
        cost[rng.random((n, n)) < 0.15] = np.inf
        cost[rng.random((n, n)) < 0.05] = np.nan
    return usable, cost


@pytest.mark.parametrize("kind", ["random", "coarse", "nonfinite"])
def test_search_equals_brute_force_over_all_chains(kind):
    rng = np.random.default_rng({"random": 1, "coarse": 2, "nonfinite": 3}[kind])
    seen = {0: 0, 1: 0}
    for n in range(1, 13):
        for window in (0, 1, 2, 3, 5, 11, 64):
            for p in (0.5, 0.9):
                usable, cost = tables(rng, n, p, kind)
                status, kept, total = FS.search(n, window, usable, cost)
                want = FS.brute_force(n, window, usable, cost)
                seen[status] += 1
                if math.isinf(want):
                    assert (status, kept, total) == (1, list(range(n)), math.inf)
                    continue
                assert status == 0 and np.float64(total).view(np.uint64) == np.float64(want).view(np.uint64)
                assert kept[0] == 0 and kept[-1] == n - 1 and all(a < b for a, b in zip(kept[:-1], kept[1:]))
                w = FS.span(n, window)
                assert all(b - a <= w and usable[a][b] and math.isfinite(cost[a][b]) for a, b in zip(kept[:-1], kept[1:]))
                assert np.float64(FS.fold(kept, cost)).view(np.uint64) == np.float64(total).view(np.uint64)
    assert seen[0] > 25 and seen[1] > 25, seen           # both outcomes were exercised


def test_statuses_of_the_short_paths():
    one = [[0.0]]
    assert FS.search(0, 7, one, one) == (2, [], math.inf)
    assert FS.search(1, 7, one, one) == (0, [0], 0.0)
    assert FS.search(2, 1, [[0, 1], [0, 0]], [[0.0, 2.5], [0.0, 0.0]]) == (0, [0, 1], 2.5)
    assert FS.search(2, 1, [[0, 0], [0, 0]], [[0.0, 2.5], [0.0, 0.0]]) == (1, [0, 1], math.inf)
    assert FS.search(2, 0, [[0, 1], [0, 0]], [[0.0, math.inf], [0.0, 0.0]]) == (1, [0, 1], math.inf)


@pytest.mark.parametrize("n,window", [(12, 3), (12, 5), (30, 7), (9, 0), (130, 64)])
def test_the_smallest_i_wins_a_tie(n, window):
    """c(i, j) = j - i exactly: every chain folds to n - 1 and best[j] = j, so every candidate onto j ties.  Only the first
    one, from i = max(0, j - w), may be taken; the chain from n - 1 back is then n - 1, n - 1 - w, ..."""
    usable = np.ones((n, n), bool)
    cost = np.subtract.outer(-np.arange(n, dtype=np.float64), -np.arange(n, dtype=np.float64))   # [i][j] = j - i
    assert cost[2][5] == 3.0
    status, kept, total = FS.search(n, window, usable, cost)
    w = FS.span(n, window)
    want = []
    v = n - 1
    while v > 0:
        want.append(v)
        v = max(0, v - w)
    assert status == 0 and total == float(n - 1) and kept == [0] + want[::-1]
    # one pair made cheaper: now it alone decides, wherever the ties would have gone
    cost[1][3] = 1.5
    _, kept2, total2 = FS.search(n, window, usable, cost)
    assert total2 == total - 0.5 and 1 in kept2 and 3 in kept2


def test_the_cost_never_rises_with_the_window():
    """The chains of a smaller window are a subset of those of a larger one, and the search returns the smallest fold over
    its chains: bit for bit monotone, with no tolerance."""
    rng = np.random.default_rng(9)
    for n in (2, 3, 8, 20, 45):
        for kind in ("random", "coarse", "nonfinite"):
            usable, cost = tables(rng, n, 0.8, kind)
            for k in range(n - 1):                       # the chain itself passes: window 1 has an answer
                usable[k][k + 1] = True
                cost[k][k + 1] = 1.0 + 0.01 * k
            totals = [FS.search(n, w, usable, cost)[2] for w in (1, 2, 3, 7, 16, 64, 0)]
            assert np.float64(totals[0]).view(np.uint64) == np.float64(FS.fold(list(range(n)), cost)).view(np.uint64)
            assert all(b <= a for a, b in zip(totals[:-1], totals[1:])), totals
            assert totals[-1] == FS.search(n, n - 1, usable, cost)[2] == FS.search(n, n + 5, usable, cost)[2]


def test_candidate_count_and_order():
    for n in range(0, 40):
        for window in (0, 1, 2, 7, 38, 39, 64):
            c = FS.candidates(n, window)
            assert len(c) == FS.count(n, window)
            assert c == sorted(c) and all(1 <= j - i <= FS.span(n, window) for i, j in c)


def test_the_library_exports_the_simplifier_next_to_the_header():
    src = open(os.path.join(common.ROOT, "include", "artp_c.h")).read()
    L = _capi.load()
    for name in ("artp_field_simplify_paths", "artp_field_simplify_stats"):
        assert re.search(r"\bint %s\s*\(" % name, src), name
        assert name in _capi.SYMBOLS and hasattr(L, name)
    for field in ("window", "max_batch_pairs"):
        assert re.search(r"\b%s;" % field, src)
    assert C.sizeof(_capi.FieldSimplifyParams) == 16 and _capi.FieldSimplifyParams.max_batch_pairs.offset == 8
    assert C.sizeof(_capi.FieldSimplifyStats) == 9 * 8
    for name, _ in _capi.FieldSimplifyStats._fields_:
        assert re.search(r"\b%s;" % name, src), name
    # without a field there is nothing to simplify: refused before anything is touched
    st = _capi.FieldSimplifyStats()
    assert L.artp_field_simplify_stats(None, C.byref(st)) == -1
    p = _capi.FieldSimplifyParams(4, 0, 0)
    assert L.artp_field_simplify_paths(None, C.byref(p), None, None, 0, None, None, None, None, None, 0) == -1
