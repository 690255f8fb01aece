"""Numpy restatement of the clearance maps and the clearance-weighted move costs (include/artp_c.h artp_clearance_map,
artp_field_compute_clearance).

clearance_map compares shifted windows of a padded obstacle array over all offsets of the disc; brute_clearance_map is an
independent formulation (pairwise distances from every node to every obstacle cell, the obstacle test done bit by bit) for
masks small enough to afford it.  weights() restates the f64 pricing, in the order of operations the header states."""
import numpy as np

import lattice_ref as LR

NONE = 0xffff


def erode(mask, n_yaw, yaw_spread):
    """bit k of the result = bits k - s .. k + s (mod n_yaw) of the word are all set; only the low n_yaw bits count"""
    full = (1 << n_yaw) - 1
    w = np.asarray(mask).astype(np.uint64) & np.uint64(full)
    e = w.copy()
    for t in range(1, int(yaw_spread) + 1):
        rotl = ((w << np.uint64(t)) | (w >> np.uint64(n_yaw - t))) & np.uint64(full)
        rotr = ((w >> np.uint64(t)) | (w << np.uint64(n_yaw - t))) & np.uint64(full)
        e &= rotl & rotr
    return e


def planes(words, n_yaw):
    return ((np.asarray(words).astype(np.uint64)[..., None] >> np.arange(n_yaw, dtype=np.uint64)) & np.uint64(1)).astype(bool)


def clearance_map(mask, n_yaw, radius_cells, yaw_spread=0, outside_is_obstacle=False):
    """(nrows, ncols, n_yaw) uint16"""
    mask = np.asarray(mask)
    nr, nc = mask.shape
    R = int(radius_cells)
    node = planes(mask, n_yaw)
    obst = np.full((nr + 2 * R, nc + 2 * R, n_yaw), bool(outside_is_obstacle))
    obst[R:R + nr, R:R + nc] = ~planes(erode(mask, n_yaw, yaw_spread), n_yaw)
    d2 = np.full((nr, nc, n_yaw), NONE, np.int64)
    for dr in range(-R, R + 1):
        for dc in range(-R, R + 1):
            dd = dr * dr + dc * dc
            if dd > R * R:
                continue
            win = obst[R + dr:R + dr + nr, R + dc:R + dc + nc]
            d2 = np.where(win & (dd < d2), dd, d2)
    d2[~node] = 0
    return d2.astype(np.uint16)


def brute_clearance_map(mask, n_yaw, radius_cells, yaw_spread=0, outside_is_obstacle=False):
    """The same from the definition: per heading the list of obstacle cells (those of a frame of R cells around the
    rectangle included when the outside counts), then the least squared distance from every node to the list."""
    mask = np.asarray(mask)
    nr, nc = mask.shape
    R, s = int(radius_cells), int(yaw_spread)
    out = np.zeros((nr, nc, n_yaw), np.uint16)
    for k in range(n_yaw):
        cells = []
        for r in range(-R, nr + R):
            for c in range(-R, nc + R):
                if 0 <= r < nr and 0 <= c < nc:
                    word = int(mask[r, c])
                    if any(not (word >> ((k + t) % n_yaw)) & 1 for t in range(-s, s + 1)):
                        cells.append((r, c))
                elif outside_is_obstacle:
                    cells.append((r, c))
        ob = np.array(cells, np.int64).reshape(-1, 2)
        for r in range(nr):
            for c in range(nc):
                if not (int(mask[r, c]) >> k) & 1:
                    continue
                dd = (ob[:, 0] - r) ** 2 + (ob[:, 1] - c) ** 2
                dd = dd[dd <= R * R]
                out[r, c, k] = dd.min() if len(dd) else NONE
    return out


def penalty(d2, res, margin):
    """pen(v) = 0 at 0xffff, else max(0.0, 1.0 - (res sqrt(d2)) / margin), f64"""
    d2 = np.asarray(d2)
    pen = np.maximum(0.0, 1.0 - (np.float64(res) * np.sqrt(d2.astype(np.float64))) / np.float64(margin))
    return np.where(d2 == NONE, 0.0, pen)


def factors(d2, res, margin, gain):
    """f[m][r, c, k] = 1.0 + gain max(pen(a), pen(b)) for move m from a = (r, c, k) to b; NaN where b lies outside the
    rectangle (or the move does not exist: a rotation at one heading)"""
    nr, nc, n_yaw = d2.shape
    pen = penalty(d2, res, margin)
    f = np.full((10, nr, nc, n_yaw), np.nan)
    for m, (dr, dc) in enumerate(LR.MOVES):
        a = (slice(max(0, -dr), nr - max(0, dr)), slice(max(0, -dc), nc - max(0, dc)))
        b = (slice(max(0, dr), nr - max(0, -dr)), slice(max(0, dc), nc - max(0, -dc)))
        f[m][a] = 1.0 + np.float64(gain) * np.maximum(pen[a], pen[b])
    if n_yaw > 1:
        for m, step in ((8, 1), (9, -1)):
            k2 = (np.arange(n_yaw) + step) % n_yaw
            f[m] = 1.0 + np.float64(gain) * np.maximum(pen, pen[..., k2])
    return f


def weights(base, d2, res, margin, gain):
    """w[m][r, c, k] = base[m][r, c, k] (1.0 + gain max(pen(a), pen(b))): base = the plain objective's cost of move m from
    (r, c, k), (10, nrows, ncols, n_yaw), +inf (kept) where the edge does not exist"""
    base = np.asarray(base, np.float64)
    f = factors(d2, res, margin, gain)
    return np.where(np.isfinite(base), base * np.where(np.isnan(f), 1.0, f), base)
