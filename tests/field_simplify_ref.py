"""artp_field_simplify_paths' search restated over given per-pair tables (include/artp_c.h): the
forward DAG search of the roadmap's simplifier with the candidates limited to a window.

usable[i][j] and cost[i][j] (j > i; (n, n) numpy arrays or nested lists, costs as float64) say what the device's two checks and its cost kernel say about the pair; nothing
outside 1 <= j - i <= window is read."""
import itertools
import math


def span(n, window):
    """The largest j - i a candidate of a path of n states may have (window 0 = all pairs)."""
    return n - 1 if window == 0 else min(window, n - 1)


def candidates(n, window):
    """The candidates in the device's order: by i, then by j."""
    w = span(n, window)
    return [(i, j) for i in range(n - 1) for j in range(i + 1, min(i + w, n - 1) + 1)]


def count(n, window):
    """The closed form the library sizes its batches with."""
    if n < 2:
        return 0
    m, w = n - 1, span(n, window)
    return w * (m - w + 1) + w * (w - 1) // 2


def search(n, window, usable, cost):
    """(status, kept indices, cost): status 0 = simplified, 1 = the input does not pass (all indices back, +inf),
    2 = empty.  best[j] takes best[i] + c(i, j) only when strictly smaller, i ascending: the smallest i wins a tie."""
    if n == 0:
        return 2, [], math.inf
    best = [math.inf] * n
    frm = [None] * n
    best[0] = 0.0
    for i, j in candidates(n, window):
        c = cost[i][j]
        if not usable[i][j] or not math.isfinite(c) or not math.isfinite(best[i]):
            continue
        if best[i] + c < best[j]:
            best[j] = best[i] + c
            frm[j] = i
    if n > 1 and not math.isfinite(best[n - 1]):
        return 1, list(range(n)), math.inf
    kept = []
    v = n - 1
    while v is not None:
        kept.append(v)
        v = frm[v]
    return 0, kept[::-1], best[n - 1]


def fold(kept, cost):
    """The left fold ((0 + c1) + c2) + ... along a chain."""
    total = 0.0
    for a, b in zip(kept[:-1], kept[1:]):
        total = total + cost[a][b]
    return total


def brute_force(n, window, usable, cost):
    """The smallest fold over ALL chains 0 = v0 < v1 < ... = n - 1 of usable candidates inside the window (+inf: none)."""
    if n == 1:
        return 0.0
    w = span(n, window)
    best = math.inf
    inner = list(range(1, n - 1))
    for r in range(len(inner) + 1):
        for mid in itertools.combinations(inner, r):
            chain = [0, *mid, n - 1]
            steps = list(zip(chain[:-1], chain[1:]))
            if all(b - a <= w and usable[a][b] and math.isfinite(cost[a][b]) for a, b in steps):
                best = min(best, fold(chain, cost))
    return best
