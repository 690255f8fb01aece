"""Soundness of the feet pre-pass's implication, on the CPU: feet_prepass_ref.probe against the C oracle.

feet_stream_kernel settles a foot box as "touches" when a triangle under the box's lowest corner is kept, has no
partner in a covered window and accepts a contact (lane_corner_probe, restated in feet_prepass_ref.py).  The kernel
gives the probe the boxes that exits (b)-(e) left open; for those the oracle's exit code is EXIT_VERTEX, EXIT_PLANE or
EXIT_NONE, and every box the restatement decides must have one of the first two.  (A box that an exit (b)-(e) decides
never reaches the kernel, and those exits are not existence tests: the reference answers 0 for a box wholly under
the terrain, whatever its corners touch.  The counts of such boxes are printed, nothing is asserted about them.)

Inputs: the sampler's 2^15 states on make_map(100, 0.04, seed=3) and 2^15 random states on the terraced 200-cell map of
test_feet_corner_first.py, both robots (4 x 2^17 foot boxes), plus two constructed sets: a tilted plane with the lowest
corner placed within half the margin of a cell border, and a step whose lower side the lowest corner overhangs while
another corner touches the upper side.

Branches: decided and the refusals border margin, not kept, partner and no accepted contact are each reached at least
100 times.  The fifth refusal, "filtered by height", CANNOT be reached from the lowest corner: that corner's height is
py = pos_y - sum_i |side_i R[3+i]| / 2 and the window's colliding threshold is minO2 = pos_y - (sum_i |R[3+i] side_i|) / 2,
the same number up to a few roundings (< 1e-5 at these coordinates); a kept triangle has a vertex above minO2, its
`top` is at least that vertex, so py > top + spread * reach + 1e-3 would need py > minO2 + 1e-3.  The test asserts that
it never fires there, and reaches that branch of the shared per-pair code at least 100 times through the box's highest
corner instead (probe(..., highest=True), decided boxes checked against the oracle in the same way)."""
import math

import numpy as np
import pytest

import common
import feet_prepass_ref as P
import oracle_py as O
from synthetic import make_map

N = 1 << 15
MIN_EACH = 100
EXIT_VERTEX, EXIT_PLANE, EXIT_NONE = 5, 6, 8


def layer_field(layer, res):
    """An oracle heightfield over one square layer."""
    n = layer.shape[0]
    return O.OracleField(np.asfortranarray(layer, dtype=np.float32), n * res, n * res)


def tilted_plane_border_poses(field, side, n, rng, res):
    """Foot poses over a tilted plane whose lowest corner lies within half the margin of a cell border (x, z or both)."""
    nW = field.f.nW
    ext = nW * res
    x, y = rng.uniform(-0.3 * ext, 0.3 * ext, n), rng.uniform(-0.3 * ext, 0.3 * ext, n)
    P0 = common.make_dposes(x, y, np.zeros(n), rng.uniform(-0.3, 0.3, n), rng.uniform(-0.3, 0.3, n), rng.uniform(-np.pi, np.pi, n))
    px, py, pz = P.lowest_corner(field, side, P0)
    sw, sd = float(field.f.sample_w), float(field.f.sample_d)
    off = rng.uniform(-0.5, 0.5, (2, n)) * float(P.MARGIN)          # within half the margin of the border
    which = rng.integers(0, 3, n)                                     # 0: x border, 1: z border, 2: both
    dx = np.where(which != 1, np.round(px / sw) * sw + off[0] - px, 0.0)
    dz = np.where(which != 0, np.round(pz / sd) * sd + off[1] - pz, 0.0)
    # height: the corner on the plane's surface there, a little under or over
    h = field.storage.reshape(field.f.nD, field.f.nW)
    ix, iz = np.clip(np.floor((px + dx) / sw).astype(int), 0, nW - 2), np.clip(np.floor((pz + dz) / sd).astype(int), 0, field.f.nD - 2)
    dy = h[iz, ix] + rng.uniform(-0.03, 0.01, n) - py
    wx, wy, wz = P.field_to_world(field, dx, dy, dz)
    P1 = P0.copy()
    P1[:, 0] += wx.astype(np.float32)
    P1[:, 1] += wy.astype(np.float32)
    P1[:, 2] += wz.astype(np.float32)
    return P1


def step_overhang_poses(field, side, n, rng, res, step_h):
    """Foot poses across a step (low half / high half of the map): tilted so that the lowest corner hangs over the low
    side, above it, while the box's other end reaches the high side."""
    ext = field.f.nW * res
    along = rng.uniform(-0.3 * ext, 0.3 * ext, n)
    yaw = rng.choice([0.0, np.pi / 2, np.pi, -np.pi / 2], n) + rng.uniform(-0.3, 0.3, n)
    roll, pitch = rng.uniform(-0.25, 0.25, n), rng.uniform(-0.25, 0.25, n)
    across = rng.uniform(-0.6, 0.6, n) * float(max(side[0], side[1]))
    z = step_h + 0.5 * float(side[2]) + rng.uniform(-0.06, 0.04, n)
    return np.concatenate([common.make_dposes(across, along, z, roll, pitch, yaw),
                           common.make_dposes(along, across, z, roll, pitch, yaw)])


@pytest.fixture(scope="module")
def cases():
    """(name, field, side, poses, flags, radius) for every input set; built once."""
    out = []
    gm1 = make_map(100, 0.04, seed=3)
    gmt = P.terraced(make_map(200, 0.04, seed=3))
    rng = np.random.default_rng(21)
    se3_t = common.random_states(gmt, N, rng, z_off=(0.0, 0.03), tilt=0.15, spread=0.5)
    for rname in ("yaml", "defaults"):
        rob = O.robot(rname)
        R = P.foot_radius(rob, 0.04)
        for tag, gm, se3 in (("perlin", gm1, None), ("terraced", gmt, se3_t)):
            om = O.OracleMap(gm)
            if se3 is None:
                se3 = O.OracleSampler(gm).sample(rob, 42, 0, N)
                se3 = se3[0] if isinstance(se3, tuple) else se3
            out.append((f"{tag}/{rname}", om.feet, rob.foot, P.foot_poses(om, rob, se3), P.partner_flags(om.feet, R), R, om))
    rob = O.robot("yaml")
    R = P.foot_radius(rob, 0.04)
    n = 120
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    rng = np.random.default_rng(7)
    # a plane with irrational slopes: no two triangles are coplanar to an epsilon
    tilted = (0.013 * math.sqrt(2.0) * i + 0.011 * math.sqrt(3.0) * j + 0.002 * np.sin(0.37 * i * j)).astype(np.float32)
    ft = layer_field(tilted, 0.04)
    out.append(("tilted plane, corner at a cell border", ft, rob.foot, tilted_plane_border_poses(ft, rob.foot, 4096, rng, 0.04),
                P.partner_flags(ft, R), R, ft))
    step = (np.where(i < n // 2, 0.0, 0.3) + 0.001 * np.sin(0.9 * i + 1.7 * j) + 0.0007 * np.cos(0.31 * i * j)).astype(np.float32)
    fs = layer_field(step, 0.04)
    out.append(("step, lowest corner overhangs", fs, rob.foot, step_overhang_poses(fs, rob.foot, 4096, rng, 0.04, 0.3),
                P.partner_flags(fs, R), R, fs))
    return out


def _oracle(field, side, poses):
    hit, ec, _ = field.check_boxes(side, poses, want_detail=True)
    return hit, ec


def test_decided_boxes_touch_and_every_branch_is_reached(cases):
    total = np.zeros(6, np.int64)
    total_hi = np.zeros(6, np.int64)
    boxes = open_boxes = 0
    for name, field, side, poses, flags, radius, _ in cases:
        hit, ec = _oracle(field, side, poses)
        neg = np.isin(ec, (EXIT_VERTEX, EXIT_PLANE, EXIT_NONE))   # exits (b)-(e) negative: what the kernel gives the probe
        for highest, acc in ((False, total), (True, total_hi)):
            decided, why = P.probe(field, side, poses, flags, radius, highest=highest)
            reason = P.box_reason(why)
            cnt = np.bincount(reason[neg], minlength=6)
            acc += cnt
            bad = decided & neg & ~np.isin(ec, (EXIT_VERTEX, EXIT_PLANE))
            print(f"{name:42s} {'highest' if highest else 'lowest '} corner: boxes {len(ec)}, exits negative {int(neg.sum())}, "
                  + ", ".join(f"{P.REASONS[k]} {int(cnt[k])}" for k in range(6))
                  + f"; decided by oracle exit {np.bincount(ec[decided], minlength=9).tolist()}")
            assert not bad.any(), f"{name}: {int(bad.sum())} decided boxes that the oracle ends with EXIT_NONE"
        boxes += len(ec)
        open_boxes += int(neg.sum())
    print("all sets, lowest corner:", {P.REASONS[k]: int(total[k]) for k in range(6)}, "of", open_boxes, "boxes with negative exits,", boxes, "boxes")
    print("all sets, highest corner:", {P.REASONS[k]: int(total_hi[k]) for k in range(6)})
    assert open_boxes >= 100_000
    for k in (P.DECIDED, P.BORDER, P.NOT_KEPT, P.PARTNER, P.NO_CONTACT):
        assert total[k] >= MIN_EACH, (P.REASONS[k], int(total[k]))
    assert total[P.FILTERED] == 0, int(total[P.FILTERED])        # unreachable from the lowest corner, see the module docstring
    assert total_hi[P.FILTERED] >= MIN_EACH, int(total_hi[P.FILTERED])


def test_constructed_sets_are_what_they_claim(cases):
    """The tilted-plane set really has its lowest corner in the border margin (every box refused for that reason), and
    the step set holds at least 100 boxes that the oracle ends with a contact or a vertex while the probe refuses them."""
    by = {c[0]: c for c in cases}
    name, field, side, poses, flags, radius, _ = by["tilted plane, corner at a cell border"]
    _, why = P.probe(field, side, poses, flags, radius)
    assert (why == P.BORDER).all(), np.bincount(why.ravel(), minlength=6)
    hit, ec = _oracle(field, side, poses)
    print("tilted plane: oracle exits", np.bincount(ec, minlength=9).tolist())
    assert min((ec == EXIT_PLANE).sum() + (ec == EXIT_VERTEX).sum(), (ec == EXIT_NONE).sum()) >= MIN_EACH
    name, field, side, poses, flags, radius, _ = by["step, lowest corner overhangs"]
    decided, why = P.probe(field, side, poses, flags, radius)
    hit, ec = _oracle(field, side, poses)
    over = ~decided & np.isin(ec, (EXIT_VERTEX, EXIT_PLANE)) & (P.box_reason(why) == P.NOT_KEPT)
    print("step: oracle exits", np.bincount(ec, minlength=9).tolist(), "touching boxes the probe refuses as not kept", int(over.sum()))
    assert over.sum() >= MIN_EACH


def test_partner_flags_of_a_flat_and_a_generic_layer():
    """partner_flags from the definition: every triangle of a flat layer has a partner, none of a layer without two
    coplanar triangles, and a non-finite vertex takes its triangles out on both sides."""
    n = 24
    flat = np.zeros((n, n), np.float32)
    ff = layer_field(flat, 0.04)
    fl = P.partner_flags(ff, 3)
    assert (fl[:-1, :-1] == 3).all() and (fl[-1, :] == 0).all() and (fl[:, -1] == 0).all()
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    rough = (0.01 * np.sin(1.3 * i * i + 0.7 * j) + 0.013 * np.cos(0.9 * j * j + 0.3 * i)).astype(np.float32)
    assert (P.partner_flags(layer_field(rough, 0.04), 3) == 0).all()
    holed = flat.copy()
    holed[10, 10] = np.nan
    fh = layer_field(holed, 0.04)
    fl = P.partner_flags(fh, 3)
    h = fh.storage.reshape(n, n)
    z, x = np.argwhere(~np.isfinite(h))[0]
    assert fl[z, x] == 2 and fl[z - 1, x - 1] == 1      # the vertex is A of its own cell and D of the one before: the other triangle stays
    assert fl[z - 1, x] == 0 and fl[z, x - 1] == 0      # it is C resp. B there: a vertex of both triangles


def test_nothing_is_decided_without_a_covering_partner_table(cases):
    """No partner table, or a table whose radius is smaller than every window that holds a cell: the window is not covered, a kept
    triangle may have a partner the table cannot rule out, and the probe decides nothing (no robot or spacing that the
    library accepts produces such a window on the GPU: the table's radius is sized from the box diagonal)."""
    name, field, side, poses, flags, radius, _ = cases[0]
    decided, why = P.probe(field, side, poses, flags, radius)
    assert decided.sum() >= MIN_EACH
    for fl, r in ((None, radius), (flags, 0)):
        d2, w2 = P.probe(field, side, poses, fl, r)
        assert not d2.any()
        assert ((w2 == P.PARTNER) == np.isin(why, (P.DECIDED, P.PARTNER, P.NO_CONTACT))).all()
