"""The device map preprocessing (art_planner_amd/csrc/preprocess.h, artp_preprocess_map_ex) restated in numpy, in the
kernels' own float32 order, plus a float64 reference of its floating-point stages.

The library is built with -ffp-contract=off and its division and sqrt are correctly rounded, so every float32 stage
below -- one rounding per operation, the terms in the kernel's order -- must come out BIT-EQUAL to the device layers:
  * estimate_normals_kernel: cell coordinates in double cast to float (pre_cell_x / pre_cell_y, with the float-rounded
    cell size), the cross product written out, the norm as sqrtf((tx*tx + ty*ty) + tz*tz), the terms in the kernel's
    offset order (+x/+y, -x/-y, then the two diagonal loops);
  * morph_kernel: min / max over the footprint of getCircularKernel(size) (oracle/map_processors._disk, no size limit)
    with replicated borders -- exact in any order (fminf / fmaxf: a NaN loses against a number);
  * the select chain pre_threshold_kernel ... pre_masked_elevation_kernel and the sample filter;
  * vertex_histogram_kernel, the two gauss_pass_kernel passes (acc += taps[d] * x for d = -r..r, BORDER_REFLECT_101
    applied as often as needed), nonneg_max_kernel, base_distribution_kernel;
  * the unknown-mass cap: known_unknown_mass_kernel's summation order (grid-stride over 64 workgroups x 256 threads when
    n >= 8192, else one workgroup; a shuffle-xor tree per wavefront; ((w0 + w1) + w2) + w3; the workgroups in order);
  * cdf_rows_kernel / cdf_rowwise_kernel: sequential sums, then c += v / s;
  * change_kernel.

The float64 reference (reference64) takes the same float32 cell coordinates, elevations, taps and probabilities and does
all its arithmetic in float64: it is there so that the restatement and the kernels cannot share a mistake unseen."""
from __future__ import annotations

import math
import os
import sys
from types import SimpleNamespace

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import map_processors  # noqa: E402

F32 = np.float32
U = 2.0 ** -24           # unit roundoff of float32

# artp_params_yaml / artp_params_defaults (the robot numbers the preprocessing reads)
ROBOTS = {
    "yaml": SimpleNamespace(torso_length=1.31, torso_width=0.65, reach_x=0.2, reach_y=0.2, unknown_space_untraversable=1),
    "defaults": SimpleNamespace(torso_length=1.05, torso_width=0.55, reach_x=0.25, reach_y=0.1,
                                unknown_space_untraversable=1),
}
# artp_preprocess_params_yaml / artp_preprocess_params_defaults
PARAMS = {
    "yaml": dict(traversability_thres=0.15, foothold_margin=0.3, foothold_margin_max_hole_size=0.3,
                 foothold_margin_max_drop=0.3, foothold_margin_max_drop_search_radius=0.16,
                 foothold_margin_min_step=0.3, foothold_size=0.1, use_inverse_vertex_density=1,
                 use_max_prob_unknown_samples=1, max_prob_unknown_samples=0.1),
    "defaults": dict(traversability_thres=0.5, foothold_margin=0.0, foothold_margin_max_hole_size=0.0,
                     foothold_margin_max_drop=0.0, foothold_margin_max_drop_search_radius=0.0,
                     foothold_margin_min_step=0.0, foothold_size=0.0, use_inverse_vertex_density=0,
                     use_max_prob_unknown_samples=0, max_prob_unknown_samples=0.1),
}


def params(kind="yaml", **overrides):
    p = dict(PARAMS[kind])
    p.update(overrides)
    return SimpleNamespace(**p)


def robot(kind="yaml", **overrides):
    r = dict(vars(ROBOTS[kind]))
    r.update(overrides)
    return SimpleNamespace(**r)


# ---- geometry ---------------------------------------------------------------------------------------------------------
def cell_size(rows, len_x):
    """artp_preprocess_map_ex: res = len_x / rows (double); the kernels' PreGeom holds it as a float."""
    return len_x / rows


def cell_x(rows, len_x, pos_x):
    """pre_cell_x: ((pos_x + (0.5 len_x - 0.5 res_f)) - res_f * i) in double, then cast to float."""
    rf = float(F32(cell_size(rows, len_x)))
    return ((pos_x + (0.5 * len_x - 0.5 * rf)) - rf * np.arange(rows, dtype=np.float64)).astype(F32)


def cell_y(rows, cols, len_x, len_y, pos_y):
    rf = float(F32(cell_size(rows, len_x)))
    return ((pos_y + (0.5 * len_y - 0.5 * rf)) - rf * np.arange(cols, dtype=np.float64)).astype(F32)


def normal_counts(rob, res):
    """(n_r, n_d) of estimateNormals(map, (torso.length + torso.width) * 0.25)."""
    radius = (rob.torso_length + rob.torso_width) * 0.25
    return int(radius / res), int(radius * 0.70710678118 / res)


def _pairs(rows, cols, n_r, n_d):
    """The kernel's neighbour pairs in its order: (di_a, dj_a, di_b, dj_b, valid mask over (i, j))."""
    I = np.arange(rows)[:, None]
    J = np.arange(cols)[None, :]
    out = []
    for o in range(1, n_r):
        out.append((o, 0, 0, o, (I + o < rows) & (J + o < cols)))
    for o in range(1, n_r):
        out.append((-o, 0, 0, -o, (I - o >= 0) & (J - o >= 0)))
    for o in range(1, n_d):
        out.append((o, o, -o, o, (I + o < rows) & (J + o < cols) & (I - o >= 0)))
    for o in range(1, n_d):
        out.append((-o, -o, o, -o, (I - o >= 0) & (J - o >= 0) & (I + o < rows)))
    return out


def _shift(a, di, dj):
    """a[i + di, j + dj] where it exists (anything elsewhere: masked by the caller)."""
    rows, cols = a.shape
    ii = np.clip(np.arange(rows) + di, 0, rows - 1)
    jj = np.clip(np.arange(cols) + dj, 0, cols - 1)
    return a[np.ix_(ii, jj)]


def _points(elev, len_x, len_y, pos_x, pos_y):
    rows, cols = elev.shape
    X = np.broadcast_to(cell_x(rows, len_x, pos_x)[:, None], (rows, cols))
    Y = np.broadcast_to(cell_y(rows, cols, len_x, len_y, pos_y)[None, :], (rows, cols))
    return X, Y, np.asarray(elev, F32)


# ---- estimate_normals_kernel ------------------------------------------------------------------------------------------
def estimate_normals(elev, len_x, len_y, pos_x, pos_y, n_r, n_d):
    """float32, kernel order: (nx, ny, nz, plane_fit_std_dev)."""
    rows, cols = elev.shape
    X, Y, Z = _points(elev, len_x, len_y, pos_x, pos_y)
    sx = np.zeros((rows, cols), F32)
    sy = np.zeros((rows, cols), F32)
    sz = np.zeros((rows, cols), F32)
    mdz = np.zeros((rows, cols), F32)
    cnt = np.zeros((rows, cols), np.int64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for dia, dja, dib, djb, ok in _pairs(rows, cols, n_r, n_d):
            ux, uy, uz = _shift(X, dia, dja) - X, _shift(Y, dia, dja) - Y, _shift(Z, dia, dja) - Z
            vx, vy, vz = _shift(X, dib, djb) - X, _shift(Y, dib, djb) - Y, _shift(Z, dib, djb) - Z
            tx = uy * vz - uz * vy
            ty = uz * vx - ux * vz
            tz = ux * vy - uy * vx
            nrm = np.sqrt((tx * tx + ty * ty) + tz * tz)
            pos = nrm > 0
            tx = np.where(pos, tx / nrm, tx)
            ty = np.where(pos, ty / nrm, ty)
            tz = np.where(pos, tz / nrm, tz)
            sx = np.where(ok, sx + tx, sx)
            sy = np.where(ok, sy + ty, sy)
            sz = np.where(ok, sz + tz, sz)
            mdz = np.where(ok, np.fmax(mdz, np.fmax(np.abs(uz), np.abs(vz))), mdz)
            cnt += ok
        has = cnt > 0
        fn = cnt.astype(F32)
        sx = np.where(has, sx / fn, sx)
        sy = np.where(has, sy / fn, sy)
        sz = np.where(has, sz / fn, sz)
        nrm = np.sqrt((sx * sx + sy * sy) + sz * sz)
        pos = nrm > 0
        return (np.where(pos, sx / nrm, sx).astype(F32), np.where(pos, sy / nrm, sy).astype(F32),
                np.where(pos, sz / nrm, sz).astype(F32), mdz.astype(F32))


def estimate_normals64(elev, len_x, len_y, pos_x, pos_y, n_r, n_d):
    """float64 reference on the same float32 coordinates and elevations: (nx, ny, nz, std, |mean of the unit terms|,
    number of terms)."""
    rows, cols = elev.shape
    X, Y, Z = (a.astype(np.float64) for a in _points(elev, len_x, len_y, pos_x, pos_y))
    s = np.zeros((3, rows, cols))
    mdz = np.zeros((rows, cols))
    cnt = np.zeros((rows, cols), np.int64)
    for dia, dja, dib, djb, ok in _pairs(rows, cols, n_r, n_d):
        u = np.stack([_shift(X, dia, dja) - X, _shift(Y, dia, dja) - Y, _shift(Z, dia, dja) - Z])
        v = np.stack([_shift(X, dib, djb) - X, _shift(Y, dib, djb) - Y, _shift(Z, dib, djb) - Z])
        t = np.cross(u, v, axis=0)
        nrm = np.sqrt((t * t).sum(axis=0))
        t = t / np.where(nrm > 0, nrm, 1.0)
        s += np.where(ok, t, 0.0)
        mdz = np.where(ok, np.maximum(mdz, np.maximum(np.abs(u[2]), np.abs(v[2]))), mdz)
        cnt += ok
    s = s / np.maximum(cnt, 1)
    m = np.sqrt((s * s).sum(axis=0))
    n = s / np.where(m > 0, m, 1.0)
    return n[0], n[1], n[2], mdz, m, cnt


# ---- morph_kernel ----------------------------------------------------------------------------------------------------
def disk(size):
    return map_processors._disk(size)


def morph(m, size, dilate):
    """Grey dilation (max) / erosion (min) with disk(size), anchored at (n/2, n/2), replicated borders; footprint row y
    (column offset y - r) is one span of row offsets [x0 - r, x1 - r], reduced with a sparse table of 2^k-wide
    extremes."""
    k = disk(size)
    n = k.shape[0]
    r = n // 2
    R, C = m.shape
    f = np.fmax if dilate else np.fmin
    pad = np.pad(np.asarray(m, F32), ((r, n), (0, 0)), mode="edge")     # pad[i + x] = m[clamp(i + x - r)]
    table = [pad]
    while (1 << len(table)) <= n:
        p, w = table[-1], 1 << (len(table) - 1)
        table.append(f(p[:-w], p[w:]))                               # table[l][i] = extreme of pad[i : i + 2^l]
    out = np.full((R, C), -np.inf if dilate else np.inf, F32)
    for y in range(n):
        xs = np.flatnonzero(k[y])
        if xs.size == 0:
            continue
        x0, x1 = int(xs[0]), int(xs[-1])
        assert xs.size == x1 - x0 + 1, "footprint row is not one span"
        lv = (x1 - x0 + 1).bit_length() - 1
        t = table[lv]
        band = f(t[x0:x0 + R], t[x1 - (1 << lv) + 1:x1 - (1 << lv) + 1 + R])
        jj = np.clip(np.arange(C) + y - r, 0, C - 1)
        out = f(out, band[:, jj])
    return out


def erode(m, size):
    return morph(m, size, False)


def dilate(m, size):
    return morph(m, size, True)


# ---- the sampling distribution ---------------------------------------------------------------------------------------
def gauss_taps(rob, res):
    """pre_sampling_distribution's taps: (k, float32 taps); exp through the C library like std::exp."""
    blur_radius = (rob.torso_length + rob.torso_width) * 0.25
    k = int(6 * blur_radius / res)
    sigma = blur_radius / res
    if k % 2 == 0:
        k += 1
    taps = np.empty(k, F32)
    s = 0.0
    for i in range(k):
        x = i - (k - 1) * 0.5
        taps[i] = F32(math.exp(-0.5 / (sigma * sigma) * x * x))
        s += float(taps[i])
    for i in range(k):
        taps[i] = F32(float(taps[i]) * (1.0 / s))
    return k, taps


def vertex_histogram(verts, rows, cols, len_x, len_y, pos_x, pos_y):
    res_f = float(F32(cell_size(rows, len_x)))
    verts = np.asarray(verts, np.float64).reshape(-1, 7)
    tx = -((verts[:, 0] - pos_x) - 0.5 * len_x)
    ty = -((verts[:, 1] - pos_y) - 0.5 * len_y)
    ins = (tx >= 0.0) & (ty >= 0.0) & (tx < len_x) & (ty < len_y)
    i = np.minimum((tx[ins] / res_f).astype(np.int64), rows - 1)
    j = np.minimum((ty[ins] / res_f).astype(np.int64), cols - 1)
    cnt = np.zeros((rows, cols), F32)
    np.add.at(cnt, (i, j), F32(1))
    return cnt


def reflect101(p, n):
    if n == 1:
        return 0
    while p < 0 or p >= n:
        p = -p if p < 0 else 2 * (n - 1) - p
    return p


def gauss_blur(counts, taps, dtype=F32):
    """The two gauss_pass_kernel passes (along the rows index, then along the columns index) in `dtype`."""
    r = len(taps) // 2
    out = np.asarray(counts, dtype)
    tp = np.asarray(taps, F32).astype(dtype)
    for axis in (0, 1):
        n = out.shape[axis]
        acc = np.zeros_like(out)
        for d in range(-r, r + 1):
            idx = np.array([reflect101(p + d, n) for p in range(n)])
            acc = acc + tp[d + r] * np.take(out, idx, axis=axis)
        out = acc
    return out


def base_distribution(blurred, sample_filter):
    """nonneg_max_kernel + base_distribution_kernel; blurred None: no density term."""
    if blurred is None:
        return (F32(1) * sample_filter).astype(F32)
    mx = np.fmax(blurred, F32(0)).max()
    if mx == 0:
        return (F32(1) * sample_filter).astype(F32)
    return ((mx - blurred) * sample_filter).astype(F32)


def _wave_tree(v):
    """known_unknown_mass_kernel's shuffle-xor tree on one wavefront (64 doubles): lane 0's sum."""
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[lanes ^ off]
    return v[0]


def unknown_mass(prob, observed):
    """(known, unknown) in known_unknown_mass_kernel (+ _final) order."""
    p = np.asarray(prob, F32).ravel(order="F").astype(np.float64)
    o = np.asarray(observed, F32).ravel(order="F")
    n = p.size
    n_part = 64 if n >= 8192 else 1
    stride = n_part * 256
    tot = []
    for which in (o > 0, ~(o > 0)):
        q = np.where(which, p, 0.0)
        # thread g adds q[g], q[g + stride], ... in order (adding an exact 0.0 for a cell of the other kind changes
        # nothing: the thread's double sum starts at +0.0 and x + 0.0 == x)
        per_thread = np.zeros(stride)
        for t0 in range(0, n, stride):
            chunk = q[t0:t0 + stride]
            per_thread[:chunk.size] = per_thread[:chunk.size] + chunk
        parts = []
        for b in range(n_part):
            w = [_wave_tree(per_thread[b * 256 + 64 * k:b * 256 + 64 * (k + 1)]) for k in range(4)]
            parts.append(((w[0] + w[1]) + w[2]) + w[3])
        if n_part == 1:
            tot.append(parts[0])
        else:
            s = 0.0
            for x in parts:
                s += x
            tot.append(s)
    return tot[0], tot[1]


def cap_unknown(prob, observed, max_prob):
    """cap_unknown_kernel: (capped probability, the masses)."""
    known, unknown = unknown_mass(prob, observed)
    out = np.asarray(prob, F32).copy()
    if known > 0 and unknown > 0 and unknown / (known + unknown) > max_prob:
        mk, mu = F32((1 - max_prob) / known), F32(max_prob / unknown)
        out = (out * np.where(observed > F32(0), mk, mu)).astype(F32)
    return out, (known, unknown)


def cdf(prob):
    """cdf_rows_kernel + cdf_rowwise_kernel: (cum_prob, cum_prob_rowwise, total)."""
    prob = np.asarray(prob, F32)
    rows, cols = prob.shape
    s = np.zeros(rows, F32)
    for j in range(cols):
        s = s + prob[:, j]
    cum = np.empty((rows, cols), F32)
    c = np.zeros(rows, F32)
    with np.errstate(invalid="ignore", divide="ignore"):
        for j in range(cols):
            c = c + prob[:, j] / s
            cum[:, j] = c
        total = F32(0)
        for i in range(rows):
            total = F32(total + s[i])
        q = s / total
    rowwise = np.empty(rows, F32)
    c1 = F32(0)
    for i in range(rows):
        c1 = F32(c1 + q[i])
        rowwise[i] = c1
    return cum, rowwise, total


def cdf64(prob):
    """float64 reference of both CDFs from the same float32 probabilities."""
    p = np.asarray(prob, F32).astype(np.float64)
    s = p.sum(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.cumsum(p / s[:, None], axis=1), np.cumsum(s / s.sum())


# ---- the whole chain -------------------------------------------------------------------------------------------------
def sizes(prm, res):
    """The morphology sizes of artp_preprocess_map_ex and setTraversabilityFilter."""
    return dict(fh=int(math.ceil(prm.foothold_size / res)), margin=int(math.ceil(2 * prm.foothold_margin / res)),
                hole=int(math.floor(prm.foothold_margin_max_hole_size / res)),
                search=int(math.ceil(2 * prm.foothold_margin_max_drop_search_radius / res)))


def reach_sizes(rob, res):
    total_reach = math.sqrt(rob.reach_x * rob.reach_x + rob.reach_y * rob.reach_y)
    min_wall = min((rob.torso_length - rob.reach_x) * 0.5, (rob.torso_width - rob.reach_y) * 0.5)
    return int(total_reach / res), int(min_wall / res)


def sampling_distribution(L, prm, rob, geom, vertices=None):
    """pre_sampling_distribution on the layers in L (sample filter, observed): writes n_samples, sample_probability,
    cum_prob, cum_prob_rowwise (and a few intermediates under '_')."""
    rows, cols = L["elevation"].shape
    len_x, len_y, pos_x, pos_y = geom
    res = cell_size(rows, len_x)
    density = bool(prm.use_inverse_vertex_density) and vertices is not None and len(vertices) > 0
    if density:
        k, taps = gauss_taps(rob, res)
        cnt = vertex_histogram(vertices, rows, cols, len_x, len_y, pos_x, pos_y)
        L["_counts"], L["_taps"] = cnt, taps
        L["n_samples"] = gauss_blur(cnt, taps).astype(F32)
    else:
        L["n_samples"] = np.zeros((rows, cols), F32)
    prob = base_distribution(L["n_samples"] if density else None, L["traversability_sample_filter"])
    L["_mass"] = None
    if prm.use_max_prob_unknown_samples:
        prob, L["_mass"] = cap_unknown(prob, L["observed"], prm.max_prob_unknown_samples)
    L["sample_probability"] = prob
    L["cum_prob"], L["cum_prob_rowwise"], L["_total"] = cdf(prob)
    return L


def preprocess(elevation, len_x, len_y, pos_x=0.0, pos_y=0.0, traversability=None, observed=None, vertices=None,
               prm=None, rob=None):
    """artp_preprocess_map_ex restated: a dict of every layer artp_preprocessed_get_layer returns (but 'updated'),
    plus the masks of the select chain under '_hole', '_wall', '_keep'."""
    prm = prm or params("yaml")
    rob = rob or robot("yaml")
    elev = np.asarray(elevation, F32)
    rows, cols = elev.shape
    res = cell_size(rows, len_x)
    L = {"elevation": elev.copy()}
    trav = np.ones((rows, cols), F32) if traversability is None else np.asarray(traversability, F32).copy()
    obs = np.ones((rows, cols), F32) if observed is None else np.asarray(observed, F32).copy()
    if rob.unknown_space_untraversable:
        trav = np.where(obs > F32(0.5), trav, F32(0)).astype(F32)
    L["traversability"], L["observed"] = trav, obs
    n_r, n_d = normal_counts(rob, res)
    L["normal_x"], L["normal_y"], L["normal_z"], L["plane_fit_std_dev"] = estimate_normals(
        elev, len_x, len_y, pos_x, pos_y, n_r, n_d)
    # setMaskedElevationAndTraversability
    sz = sizes(prm, res)
    one, zero = F32(1), F32(0)
    tf = np.where(trav > F32(prm.traversability_thres), one, zero).astype(F32)
    closed = erode(dilate(tf, sz["hole"]), sz["hole"])
    eroded = erode(elev, sz["search"])
    dilated = dilate(elev, sz["margin"])
    with np.errstate(invalid="ignore"):
        hole = (elev - eroded) > F32(prm.foothold_margin_max_drop)
        wall = (dilated - elev) > F32(prm.foothold_margin_min_step)
    safety = np.where(wall, one, np.where(hole, tf, closed)).astype(F32)
    keep = (tf < F32(0.5)) | wall
    t1 = np.where(keep, tf, erode(safety, sz["margin"])).astype(F32)
    t1 = dilate(erode(t1, sz["fh"]), sz["fh"])
    safety = np.where(tf < F32(0.5), tf, t1).astype(F32)
    L["traversability_thresholded_no_safety"] = tf
    L["traversability_thresholded"] = safety
    L["elevation_masked"] = np.where(safety > F32(0.5), elev, F32(-np.inf)).astype(F32)
    L["_hole"], L["_wall"], L["_keep"], L["_closed"] = hole, wall, keep, closed
    # setTraversabilityFilter
    reach, min_wall = reach_sizes(rob, res)
    L["traversability_sample_filter"] = erode(erode(dilate(safety, reach), reach), min_wall)
    return sampling_distribution(L, prm, rob, (len_x, len_y, pos_x, pos_y), vertices)


def change(elev_new, trav_new, elev_old, trav_old, si, sj, thres):
    """change_kernel: (updated, (row0, col0, nrows, ncols), count) as artp_preprocessed_change reports them."""
    rows, cols = elev_new.shape
    I = np.arange(rows)[:, None] - si
    J = np.arange(cols)[None, :] - sj
    inside = (I >= 0) & (J >= 0) & (I < rows) & (J < cols)
    io, jo = np.clip(I, 0, rows - 1), np.clip(J, 0, cols - 1)
    eo, to = elev_old[io, jo], trav_old[io, jo]
    with np.errstate(invalid="ignore"):
        same = ~(np.abs(elev_new - eo) > F32(thres)) & ~((to - trav_new) > F32(0.5))
    upd = np.where(inside & same, F32(0), F32(1)).astype(F32)
    ii, jj = np.nonzero(upd)
    cnt = int(ii.size)
    rect = (int(ii.min()), int(jj.min()), int(ii.max() - ii.min() + 1), int(jj.max() - jj.min() + 1)) if cnt else (0, 0, 0, 0)
    return upd, rect, cnt


# ---- the float64 reference and its bounds ----------------------------------------------------------------------------
def reference64(L, elevation, geom, prm, rob):
    """float64 restatement of the floating-point stages, from the float32 inputs of each stage in L.
    Returns a dict with the reference values and each stage's bound (see the derivations in
    tests/test_preprocess_restated.py)."""
    len_x, len_y, pos_x, pos_y = geom
    rows, cols = L["elevation"].shape
    res = cell_size(rows, len_x)
    n_r, n_d = normal_counts(rob, res)
    nx, ny, nz, std, m, cnt = estimate_normals64(np.asarray(elevation, F32), len_x, len_y, pos_x, pos_y, n_r, n_d)
    out = dict(normal_x=nx, normal_y=ny, normal_z=nz, plane_fit_std_dev=std, mean_norm=m, n_terms=cnt)
    out["normal_tol"] = normal_bound(cnt, m)
    if "_counts" in L:
        b = gauss_blur(L["_counts"], L["_taps"], dtype=np.float64)
        out["n_samples"] = b
        out["n_samples_tol"] = blur_bound(len(L["_taps"])) * b
    cum, rw = cdf64(L["sample_probability"])
    out["cum_prob"], out["cum_prob_rowwise"] = cum, rw
    out["cum_prob_tol"] = cdf_bound(cols) * np.abs(cum)
    out["cum_prob_rowwise_tol"] = rowwise_bound(rows, cols) * np.abs(rw)
    return out


def within(x, ref, tol):
    """|x - ref| <= tol where ref is a number; NaN exactly where ref is NaN."""
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    nan = np.isnan(ref)
    with np.errstate(invalid="ignore"):
        return bool(np.array_equal(np.isnan(x), nan) and (nan | (np.abs(x - ref) <= tol)).all())


def normal_bound(n_terms, mean_norm):
    """Per cell |float32 - float64| bound on a unit-normal component (derivation: test_preprocess_restated)."""
    with np.errstate(divide="ignore"):
        b = (12 + 2 * n_terms) * U / np.where(mean_norm > 0, mean_norm, 1.0) + 2 * U
    return np.minimum(b, 1e-5)


def blur_bound(k):
    return (2 * k + 3) * U


def cdf_bound(cols):
    return (2 * cols + 3) * U


def rowwise_bound(rows, cols):
    return (2 * rows + 2 * cols + 4) * U


# ---- test maps -------------------------------------------------------------------------------------------------------
def sweep_map(rows, cols, res, seed=0):
    """(elevation, traversability) of a rows x cols map at any spacing: smooth terrain, a terraced quarter (ties for
    min and max), an exactly flat plateau, a raised block 0.6 m high (steps above min_step = 0.3 m) and a pit 0.6 m
    deep (drops below max_drop = 0.3 m), placed as fractions of the map so that every spacing and shape of at least
    8 x 8 cells has them; traversability = 1 - clamp(slope / 0.6, 0, 1)."""
    rng = np.random.default_rng(seed)
    x = (np.arange(rows) * res)[:, None]
    y = (np.arange(cols) * res)[None, :]
    h = np.zeros((rows, cols))
    for _ in range(3):
        a, b = rng.uniform(0.3, 1.5, 2)
        p, q = rng.uniform(0, 2 * np.pi, 2)
        h = h + 0.12 * np.sin(a * x + p) * np.cos(b * y + q)
    R, C = rows, cols

    def box(f0, f1, g0, g1):
        return slice(int(f0 * R), max(int(f1 * R), int(f0 * R) + 1)), slice(int(g0 * C), max(int(g1 * C), int(g0 * C) + 1))

    if min(rows, cols) >= 8:                             # tiny maps keep the smooth terrain: something to sample
        t = box(0.5, 1.0, 0.5, 1.0)
        h[t] = np.round(h[t] / 0.05) * 0.05              # terraces
        h[box(0.05, 0.3, 0.05, 0.35)] = 0.2              # plateau
        h[box(0.2, 0.45, 0.55, 0.8)] += 0.6              # block
        h[box(0.6, 0.85, 0.15, 0.4)] -= 0.6              # pit
    h = h.astype(F32)
    if min(rows, cols) >= 2:
        gx, gy = np.gradient(h.astype(np.float64), res)
    else:
        gx = gy = np.zeros((rows, cols))
    trav = (1.0 - np.clip(np.sqrt(gx * gx + gy * gy) / 0.6, 0.0, 1.0)).astype(F32)
    return np.asfortranarray(h), np.asfortranarray(trav)


def sweep_vertices(rows, cols, res, pos_x, pos_y, n=400, seed=0):
    """Roadmap vertices (n x 7) inside the map, outside it, on its edges and on cell boundaries."""
    rng = np.random.default_rng(seed)
    len_x, len_y = rows * res, cols * res
    v = np.zeros((n, 7))
    v[:, 6] = 1.0
    m = n // 4
    v[:m, 0] = pos_x + rng.uniform(-0.5, 0.5, m) * len_x                      # inside
    v[:m, 1] = pos_y + rng.uniform(-0.5, 0.5, m) * len_y
    v[m:2 * m, 0] = pos_x + rng.uniform(-1.5, 1.5, m) * len_x                # around, mostly outside
    v[m:2 * m, 1] = pos_y + rng.uniform(-1.5, 1.5, m) * len_y
    e = np.array([-0.5, 0.5])                                                 # the four edges and corners
    k = np.arange(2 * m, 3 * m)
    v[k, 0] = pos_x + np.where(k % 2 == 0, rng.choice(e, m) * len_x, rng.uniform(-0.5, 0.5, m) * len_x)
    v[k, 1] = pos_y + np.where(k % 2 == 1, rng.choice(e, m) * len_y, rng.uniform(-0.5, 0.5, m) * len_y)
    k = np.arange(3 * m, n)                                                   # on cell boundaries
    v[k, 0] = pos_x + 0.5 * len_x - res * rng.integers(0, rows + 1, k.size)
    v[k, 1] = pos_y + 0.5 * len_y - res * rng.integers(0, cols + 1, k.size)
    return v
