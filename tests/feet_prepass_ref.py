"""numpy restatement of lane_corner_probe (box_check.h), the pre-pass of feet_stream_kernel.

The pre-pass looks at ONE corner of a foot box, the lowest in the heightfield's frame, and at the two triangles of the
cell under it.  A triangle that is kept, whose own partner bit is clear in a window the partner table covers, and which
accepts one of dCollideBoxPlane's contacts settles the box ("touches"): such a triangle is a group of its own in the
reference's greedy grouping, so its contact makes dCollide non-zero whatever the rest of the window holds.  Everything
else is refused, with the reason, and left to the full corner stage.

Every function works on arrays of boxes in float32, one IEEE rounding per operation, in the order of the device code
(artp_math.h setup_box, triangle_plane, box_plane_contacts, is_on_heightfield2; box_check.h corner_pair,
corner_probe_at).  `probe` needs no GPU: the partner flags are an input, and `partner_flags` computes them from their
definition (FieldDev::partner_flags) for a CPU test."""
from __future__ import annotations

import copy
import math

import numpy as np

f32 = np.float32
EPS = f32(1.1920928955078125e-07)
MARGIN = f32(1.0e-4)

DECIDED, BORDER, NOT_KEPT, FILTERED, PARTNER, NO_CONTACT = range(6)
REASONS = ("decided", "border margin", "not kept", "filtered by height", "partner", "no accepted contact")


def _dot3(a0, a1, a2, b0, b1, b2):
    return (a0 * b0 + a1 * b1) + a2 * b2


def _safe_normalize3(a0, a1, a2):
    b0, b1, b2 = np.abs(a0), np.abs(a1), np.abs(a2)
    idx = np.where(b1 > b0, np.where(b2 > b1, 2, 1), np.where(b2 > b0, 2, 0))
    skip = (idx == 0) & ~(b0 > 0)
    big = np.where(idx == 0, a0, np.where(idx == 1, a1, a2))
    first = np.where(idx == 0, a1, a0)
    second = np.where(idx == 2, a1, a2)
    with np.errstate(all="ignore"):
        recip = f32(1.0) / np.abs(big)
        p1, p2 = first * recip, second * recip
        l = f32(1.0) / np.sqrt((f32(1.0) + p1 * p1) + p2 * p2)
    nb, n1, n2 = np.copysign(l, big), p1 * l, p2 * l
    o0 = np.where(idx == 0, nb, n1)
    o1 = np.where(idx == 1, nb, np.where(idx == 0, n1, n2))
    o2 = np.where(idx == 2, nb, n2)
    return np.where(skip, a0, o0), np.where(skip, a1, o1), np.where(skip, a2, o2)


def _orthogonalize(m0, m1, m2, m4, m5, m6, m8, m9, m10):
    """orthogonalize_R9 on arrays."""
    nz0 = (m0 != 0) | (m1 != 0) | (m2 != 0)
    n0 = (m0 * m0 + m1 * m1) + m2 * m2
    proj = _dot3(m0, m1, m2, m4, m5, m6)
    in_place = ~(proj != 0)
    with np.errstate(all="ignore"):
        pd = proj / n0
    r0 = np.where(in_place, m4, m4 - pd * m0)
    r1 = np.where(in_place, m5, m5 - pd * m1)
    r2 = np.where(in_place, m6, m6 - pd * m2)
    act = nz0 & ((r0 != 0) | (r1 != 0) | (r2 != 0))
    a0, a1, a2 = _safe_normalize3(m0, m1, m2)
    norm0 = act & (n0 != 1)
    m0, m1, m2 = np.where(norm0, a0, m0), np.where(norm0, a1, m1), np.where(norm0, a2, m2)
    n1 = (r0 * r0 + r1 * r1) + r2 * r2
    s0, s1, s2 = _safe_normalize3(r0, r1, r2)
    norm1 = n1 != 1
    r0, r1, r2 = np.where(norm1, s0, r0), np.where(norm1, s1, r1), np.where(norm1, s2, r2)
    w = act & in_place
    m4, m5, m6 = np.where(w, r0, m4), np.where(w, r1, m5), np.where(w, r2, m6)
    m8 = np.where(act, m1 * r2 - m2 * r1, m8)
    m9 = np.where(act, m2 * r0 - m0 * r2, m9)
    m10 = np.where(act, m0 * r1 - m1 * r0, m10)
    return m0, m1, m2, m4, m5, m6, m8, m9, m10


def _next_down(x):
    return np.nextafter(x, f32(-np.inf))


def _next_up(x):
    return np.nextafter(x, f32(np.inf))


def setup_boxes(field, side, poses):
    """setup_box on arrays: dict of pos (3), R (9), side (3), aabb (6), minX, maxX, minZ, maxZ, on_field.
    field: oracle_py.OracleField; side: 3 floats; poses: (n, 16) dPoses."""
    f = field.f
    fR = [f32(v) for v in f.R]
    P = np.ascontiguousarray(poses, np.float32).reshape(-1, 16)
    side = [f32(v) for v in np.asarray(side, np.float32)]
    w = _orthogonalize(P[:, 4], P[:, 5], P[:, 6], P[:, 8], P[:, 9], P[:, 10], P[:, 12], P[:, 13], P[:, 14])
    R = [_dot3(w[j], w[3 + j], w[6 + j], fR[i], fR[4 + i], fR[8 + i]) for i in range(3) for j in range(3)]
    p = [P[:, i] - f32(f.pos[i]) for i in range(3)]
    pos = [_dot3(fR[i], fR[4 + i], fR[8 + i], p[0], p[1], p[2]) for i in range(3)]
    pos[0] = pos[0] + f32(f.half_w)
    pos[2] = pos[2] + f32(f.half_d)
    ext = [f32(0.5) * ((np.abs(R[3 * r] * side[0]) + np.abs(R[3 * r + 1] * side[1])) + np.abs(R[3 * r + 2] * side[2]))
           for r in range(3)]
    aabb = [pos[0] - ext[0], pos[0] + ext[0], pos[1] - ext[1], pos[1] + ext[1], pos[2] - ext[2], pos[2] + ext[2]]
    on_field = ~((aabb[0] > f32(f.width)) | (aabb[4] > f32(f.depth))) & ~((aabb[1] < 0) | (aabb[5] < 0))
    inv_w, inv_d = f32(f.inv_w), f32(f.inv_d)
    minX = np.maximum(np.floor(_next_down(aabb[0] * inv_w)).astype(np.int64), 0)
    maxX = np.minimum(np.ceil(_next_up(aabb[1] * inv_w)).astype(np.int64), f.nW - 1)
    minZ = np.maximum(np.floor(_next_down(aabb[4] * inv_d)).astype(np.int64), 0)
    maxZ = np.minimum(np.ceil(_next_up(aabb[5] * inv_d)).astype(np.int64), f.nD - 1)
    return dict(pos=pos, R=R, side=side, aabb=aabb, minX=minX, maxX=maxX, minZ=minZ, maxZ=maxZ, on_field=on_field)


def _triangle_plane(v0, v1, v2, is_up):
    """triangle_plane on arrays; v = (x, y, z) triples; is_up a bool array.  Returns (n0, n1, n2, d)."""
    with np.errstate(all="ignore"):   # non-finite samples: their triangles are never kept
        e1 = [v2[k] - v0[k] for k in range(3)]
        e2 = [v1[k] - v0[k] for k in range(3)]
        a = [np.where(is_up, e1[k], e2[k]) for k in range(3)]
        b = [np.where(is_up, e2[k], e1[k]) for k in range(3)]
        t0 = a[1] * b[2] - a[2] * b[1]
        t1 = a[2] * b[0] - a[0] * b[2]
        t2 = a[0] * b[1] - a[1] * b[0]
        dinv = f32(1.0) / np.sqrt((t0 * t0 + t1 * t1) + t2 * t2)
        t0, t1, t2 = t0 * dinv, t1 * dinv, t2 * dinv
        return t0, t1, t2, _dot3(t0, t1, t2, v0[0], v0[1], v0[2])


def _cell_plane(f, h, cx, cz, up):
    """Plane of triangle `up` of the cells (cx, cz) (absolute indices); h = samples [z, x]."""
    hA, hB, hC, hD = h[cz, cx], h[cz, cx + 1], h[cz + 1, cx], h[cz + 1, cx + 1]
    sw, sd = f32(f.sample_w), f32(f.sample_d)
    xA, xB = cx.astype(np.float32) * sw, (cx + 1).astype(np.float32) * sw
    zA, zC = cz.astype(np.float32) * sd, (cz + 1).astype(np.float32) * sd
    v0 = (np.where(up, xA, xB), np.where(up, hA, hD), np.where(up, zA, zC))
    return _triangle_plane(v0, (xB, hB, zA), (xA, hC, zC), up)


def partner_flags(field, radius):
    """FieldDev::partner_flags from its definition: bit 0 / bit 1 of cell (x, z) = its ABC / DBC triangle has ANOTHER
    all-finite triangle with an epsilon-equal plane (planes_eps_equal) within Chebyshev distance `radius` cells.
    Returns uint8 [nD, nW] indexed [z, x] like the samples."""
    f = field.f
    nW, nD = f.nW, f.nD
    h = field.storage.reshape(nD, nW)
    cz, cx = np.meshgrid(np.arange(nD - 1), np.arange(nW - 1), indexing="ij")
    fin = np.isfinite(h)
    pl, ok = [], []
    for up in (True, False):
        pl.append(np.stack(_cell_plane(f, h, cx, cz, np.full(cx.shape, up))))          # [4, nD-1, nW-1]
        ok.append(fin[:-1, 1:] & fin[1:, :-1] & (fin[:-1, :-1] if up else fin[1:, 1:]))
    flags = np.zeros((nD, nW), np.uint8)
    nz, nx = nD - 1, nW - 1
    with np.errstate(all="ignore"):
        for dz in range(-radius, radius + 1):
            z0, z1 = max(0, -dz), min(nz, nz - dz)
            if z0 >= z1:
                continue
            for dx in range(-radius, radius + 1):
                x0, x1 = max(0, -dx), min(nx, nx - dx)
                if x0 >= x1:
                    continue
                own = (slice(z0, z1), slice(x0, x1))
                oth = (slice(z0 + dz, z1 + dz), slice(x0 + dx, x1 + dx))
                for o in range(2):
                    for p in range(2):
                        if dz == 0 and dx == 0 and o == p:
                            continue
                        a, b = pl[o][(slice(None),) + own], pl[p][(slice(None),) + oth]
                        eq = ok[o][own] & ok[p][oth] & (np.abs(a - b) < EPS).all(axis=0)
                        flags[:nz, :nx][own] |= (eq.astype(np.uint8) << o)
    return flags


def _box_plane_contacts(b, n0, n1, n2, d):
    """box_plane_contacts(b, n, d, 10, .) on arrays: (number of contacts, [(x, z)] * 4)."""
    R, side, pos = b["R"], b["side"], b["pos"]
    Q = [_dot3(n0, n1, n2, R[i], R[3 + i], R[6 + i]) for i in range(3)]
    A = [side[i] * Q[i] for i in range(3)]
    B = [np.abs(A[i]) for i in range(3)]
    depth = (d + f32(0.5) * ((B[0] + B[1]) + B[2])) - _dot3(n0, n1, n2, pos[0], pos[1], pos[2])
    p = [pos[0], pos[1], pos[2]]
    for i in range(3):
        hs = f32(0.5) * side[i]
        sg = A[i] > 0
        p = [np.where(sg, p[k] - hs * R[3 * k + i], p[k] + hs * R[3 * k + i]) for k in range(3)]
    lt01, lt20, lt12, lt21, lt02 = B[0] < B[1], B[2] < B[0], B[1] < B[2], B[2] < B[1], B[0] < B[2]
    s1 = np.where(lt01, np.where(lt20, 2, 0), np.where(lt21, 2, 1))
    s2 = np.where(lt01, np.where(lt20, np.where(lt01, 0, 1), np.where(lt12, 1, 2)),
                  np.where(lt21, np.where(lt01, 0, 1), np.where(lt02, 0, 2)))

    def pick(s, v):
        return np.where(s == 0, v[0], np.where(s == 1, v[1], v[2]))

    def neighbour(s):
        sd, As, Bs = pick(s, side), pick(s, A), pick(s, B)
        r = [pick(s, [R[3 * k], R[3 * k + 1], R[3 * k + 2]]) for k in range(3)]
        c = [np.where(As > 0, p[k] + sd * r[k], p[k] - sd * r[k]) for k in range(3)]
        return c, Bs

    c1, B1 = neighbour(s1)
    c2, B2 = neighbour(s2)
    has0 = ~(depth < 0)
    has1 = has0 & ~(depth - B1 < 0)
    has2 = has1 & ~(depth - B2 < 0)
    depth1, depth2 = depth - B1, depth - B2
    d4 = (depth1 + depth2) - depth
    has3 = has2 & (d4 > 0)
    c3 = [(c1[k] + c2[k]) - p[k] for k in range(3)]
    n = has0.astype(int) + has1 + has2 + has3
    return n, [(p[0], p[2]), (c1[0], c1[2]), (c2[0], c2[2]), (c3[0], c3[2])]


def _is_on_heightfield2(f, gx, gz, px, pz, up):
    sw, sd, asp = f32(f.sample_w), f32(f.sample_d), f32(f.zx_aspect)
    gxf, gzf = gx.astype(np.float32), gz.astype(np.float32)
    minX_u, maxX_u = gxf * sw, (gx + 1).astype(np.float32) * sw
    minZ_u, maxZ_u = gzf * sd, (gz + 1).astype(np.float32) * sd
    in_u = ~(px < minX_u) & ~(px >= maxX_u) & ~(pz < minZ_u) & ~(pz >= maxZ_u) & ((maxZ_u - pz) > (px - minX_u) * asp)
    maxX_d, minX_d = gxf * sw, (gx - 1).astype(np.float32) * sw
    maxZ_d, minZ_d = gzf * sd, (gz - 1).astype(np.float32) * sd
    in_d = ~(px >= maxX_d) & ~(px < minX_d) & ~(pz >= maxZ_d) & ~(pz < minZ_d) & ((maxZ_d - pz) <= (px - minX_d) * asp)
    return np.where(up, in_u, in_d)


def _lowest_corner(b, flip=False):
    R, pos, sd = b["R"], b["pos"], b["side"]
    lo, hi = (f32(0.5), f32(-0.5)) if flip else (f32(-0.5), f32(0.5))
    s = [np.where(R[3 + i] > 0, lo, hi) for i in range(3)]
    return tuple(((pos[k] + s[0] * sd[0] * R[3 * k]) + s[1] * sd[1] * R[3 * k + 1]) + s[2] * sd[2] * R[3 * k + 2]
                 for k in range(3))


def lowest_corner(field, side, poses):
    """(px, py, pz) of every box's lowest corner in the field's frame (x, z along the samples, y up)."""
    return _lowest_corner(setup_boxes(field, side, poses))


def field_to_world(field, dx, dy, dz):
    """A displacement in the field's frame as a displacement of the dPose's origin (the field's rotation is a signed
    axis permutation)."""
    fR = field.f.R
    return tuple(fR[4 * k] * dx + fR[4 * k + 1] * dy + fR[4 * k + 2] * dz for k in range(3))


def probe(field, side, poses, flags, radius, highest=False):
    """lane_corner_probe for both triangle kinds of every box (highest: corner_probe_at for the box's HIGHEST corner
    instead, the opposite one -- the kernel never asks for it; it reaches the height filter of the shared per-pair code,
    which the lowest corner cannot: see test_feet_prepass_ref.py).

    field: oracle_py.OracleField of the feet layer; side: the foot box's sides; poses: (n, 16) dPoses;
    flags: partner flags [nD, nW] (None: no table) and radius: the table's radius (FieldDev::partner_R).
    Returns (decided [n] bool, why [n, 2]): why[:, o] is the outcome of the lane with triangle kind o (0 = ABC,
    1 = DBC), one of DECIDED, BORDER, NOT_KEPT, FILTERED, PARTNER, NO_CONTACT; a box is decided when either lane is.
    Boxes whose AABB misses the field get NOT_KEPT (the kernel never sees them)."""
    f = field.f
    b = setup_boxes(field, side, poses)
    n = len(b["minX"])
    h = field.storage.reshape(f.nD, f.nW)
    cellsX, cellsZ = b["maxX"] - b["minX"], b["maxZ"] - b["minZ"]
    covered = (flags is not None) & (cellsX <= radius) & (cellsZ <= radius)
    px, py, pz = _lowest_corner(b, highest)
    inv_w, inv_d = f32(f.inv_w), f32(f.inv_d)
    reach = f32(2.0) * MARGIN * max(inv_w, inv_d)
    cxa, cxb = np.floor((px - MARGIN) * inv_w).astype(np.int64), np.floor((px + MARGIN) * inv_w).astype(np.int64)
    cza, czb = np.floor((pz - MARGIN) * inv_d).astype(np.int64), np.floor((pz + MARGIN) * inv_d).astype(np.int64)
    border = (cxb != cxa) | (czb != cza)
    cx, cz = cxa - b["minX"], cza - b["minZ"]
    inside = b["on_field"] & (cx >= 0) & (cz >= 0) & (cx < cellsX) & (cz < cellsZ)
    ax, az = np.where(inside, cxa, 0), np.where(inside, cza, 0)     # a valid cell for the rows that are masked out
    hA, hB, hC, hD = h[az, ax], h[az, ax + 1], h[az + 1, ax], h[az + 1, ax + 1]
    fA, fB, fC, fD = (np.isfinite(v) for v in (hA, hB, hC, hD))
    minO2 = b["aabb"][2]
    with np.errstate(invalid="ignore"):
        kA, kB, kC, kD = (fv & (hv > minO2) for fv, hv in ((fA, hA), (fB, hB), (fC, hC), (fD, hD)))
    why = np.empty((n, 2), np.int64)
    for o in range(2):
        up = np.full(n, o == 0)
        kept = ((kA | kB | kC) & (fA & fB & fC)) if o == 0 else ((kB | kC | kD) & (fB & fC & fD))
        h0 = hA if o == 0 else hD
        with np.errstate(all="ignore"):
            h4 = (hB + hC) - h0
            top = np.fmax(np.fmax(h0, h4), np.fmax(hB, hC))
            spread = np.abs(hB - h0) + np.abs(hC - h0)
            filtered = py > (top + spread * reach) + f32(1.0e-3)
            flag = ((flags[az, ax] >> o) & 1).astype(bool) if flags is not None else np.ones(n, bool)
            partner = ~covered | flag
            n0, n1, n2, d = _cell_plane(f, h, ax, az, up)
            nc, cp = _box_plane_contacts(b, n0, n1, n2, d)
            gx, gz = ax + (0 if o == 0 else 1), az + (0 if o == 0 else 1)
            hit = np.zeros(n, bool)
            for i in range(4):
                hit |= (i < nc) & _is_on_heightfield2(f, gx, gz, cp[i][0], cp[i][1], up)
        w = np.where(hit, DECIDED, NO_CONTACT)
        w = np.where(partner, PARTNER, w)
        w = np.where(filtered, FILTERED, w)
        w = np.where(kept & inside, w, NOT_KEPT)
        why[:, o] = np.where(border, BORDER, w)
    return (why == DECIDED).any(axis=1), why


def box_reason(why):
    """One reason per box out of its two lanes' outcomes: DECIDED when either lane decided, else the outcome of the lane
    that got furthest (no accepted contact > partner > filtered by height > not kept > border margin)."""
    rank = np.array([5, 0, 1, 2, 3, 4])   # indexed by outcome
    pick = np.where(rank[why[:, 0]] >= rank[why[:, 1]], why[:, 0], why[:, 1])
    return pick


# ---- what both test files need around the probe ----------------------------------------------------------------------
def foot_radius(rob, res):
    """partner_radius (artp_capi.hip) of the feet layer."""
    s = rob.foot.astype(np.float64)
    return int(math.ceil(math.sqrt(float((s * s).sum())) / res)) + 3


def terraced(gm, step=0.05):
    out = copy.deepcopy(gm)
    for name in ("elevation", "elevation_masked"):
        a = out[name].astype(np.float64)
        out.layers[name] = np.asfortranarray(np.where(np.isfinite(a), np.round(a / step) * step, a).astype(np.float32))
    return out


def foot_poses(om, rob, se3):
    poses, _ = om.state_poses(rob, se3)
    return poses[:, 1:5].reshape(-1, 16)
