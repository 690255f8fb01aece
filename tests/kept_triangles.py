"""Kept-triangle count of a box's window, in numpy: the rule of grp_compact_triangles (box_check.h), i.e. of
dCollideHeightfieldZone's triangle buffer.  The tests use it to prove that a constructed set of boxes really has
windows whose kept-triangle list is longer than the device's LDS list (4096).

Box setup follows setup_box (artp_math.h) on an oracle_py.OracleField: the box centre and rotation in the field's
frame, the AABB, and the index window from floor / ceil of the AABB over the sample spacing (one ulp outwards)."""
from __future__ import annotations

import numpy as np

LDS_LIST_CAP = 4096  # the device's kept-triangle list per box (size_scratch: 64 lanes x 64-bit mask)

f32 = np.float32


def _dot3(a, b, c, x, y, z):
    """artp_math.h dot3: a*x + (b*y + c*z) in float."""
    return f32(f32(a * x) + f32(f32(b * y) + f32(c * z)))


def box_window(field, side, pose):
    """(minX, maxX, minZ, maxZ, minO2) of a box, or None when its AABB misses the field.
    field: oracle_py.OracleField; side: 3 floats; pose: dPose of 16 floats (origin[4], rotation rows of 4)."""
    f = field.f
    fR = [f32(v) for v in f.R]
    pose = np.asarray(pose, np.float32).reshape(16)
    side = np.asarray(side, np.float32)
    p = [f32(pose[i] - f32(f.pos[i])) for i in range(3)]
    pos = [_dot3(fR[i], fR[4 + i], fR[8 + i], p[0], p[1], p[2]) for i in range(3)]
    rot = [pose[4], pose[5], pose[6], pose[8], pose[9], pose[10], pose[12], pose[13], pose[14]]
    # box_rotation_in_field: bR = fR^T * rot (the field's R is a signed axis permutation, so no rounding)
    bR = [f32(0.0)] * 9
    for r in range(3):
        for c in range(3):
            bR[3 * r + c] = f32(sum(float(fR[4 * k + r]) * float(rot[3 * k + c]) for k in range(3)))
    pos[0] = f32(pos[0] + f32(f.half_w))
    pos[2] = f32(pos[2] + f32(f.half_d))
    ext = [f32(f32(0.5) * f32(f32(f32(abs(f32(bR[3 * r] * side[0]))) + f32(abs(f32(bR[3 * r + 1] * side[1]))))
                              + f32(abs(f32(bR[3 * r + 2] * side[2]))))) for r in range(3)]
    aabb = [f32(pos[0] - ext[0]), f32(pos[0] + ext[0]), f32(pos[1] - ext[1]), f32(pos[1] + ext[1]),
            f32(pos[2] - ext[2]), f32(pos[2] + ext[2])]
    if aabb[0] > f32(f.width) or aabb[4] > f32(f.depth) or aabb[1] < 0 or aabb[5] < 0:
        return None
    lo = lambda v: int(np.floor(np.nextafter(f32(v), f32(-np.inf))))   # noqa: E731
    hi = lambda v: int(np.ceil(np.nextafter(f32(v), f32(np.inf))))     # noqa: E731
    minX = max(lo(aabb[0] * f32(f.inv_w)), 0)
    maxX = min(hi(aabb[1] * f32(f.inv_w)), f.nW - 1)
    minZ = max(lo(aabb[4] * f32(f.inv_d)), 0)
    maxZ = min(hi(aabb[5] * f32(f.inv_d)), f.nD - 1)
    return minX, maxX, minZ, maxZ, aabb[2]


def kept_triangles(field, side, pose):
    """Number of kept triangles of the box's window (0 when the box misses the field)."""
    w = box_window(field, side, pose)
    if w is None:
        return 0
    minX, maxX, minZ, maxZ, minO2 = w
    f = field.f
    h = field.storage.reshape(f.nD, f.nW)[minZ:maxZ + 1, minX:maxX + 1]   # [z, x], ODE sample layout
    fin = np.isfinite(h)
    col = fin & (h > minO2)
    A, B, C, D = (slice(None, -1), slice(None, -1)), (slice(None, -1), slice(1, None)), \
        (slice(1, None), slice(None, -1)), (slice(1, None), slice(1, None))
    up = (col[A] | col[B] | col[C]) & fin[A] & fin[B] & fin[C]
    down = (col[B] | col[C] | col[D]) & fin[B] & fin[C] & fin[D]
    return int(up.sum() + down.sum())
