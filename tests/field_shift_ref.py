"""Reference for carrying a cost-to-go field across a map move: artp_field_shift restated in
numpy.  The field (dist, hops) and the bits of its mask move by (si, sj) whole cells -- node (r, c, k) becomes
(r + si, c + sj, k) -- with +inf / NONE / no node in the cells that entered, and field_update_ref.update repairs the
result on the lattice of the new window.  Shares nothing with the library; tests/test_field_shift_ref.py holds it against
field_update_ref.compute on the new window.

Also the masks of the two cases that decide whether a shift looks at the right places, for that test and for the device's
(tests/test_cost_field_shift.py): a U-shaped corridor whose bend leaves, and an island that an entering strip joins."""
import numpy as np

import field_update_ref as FU
import lattice_ref as LR

# The spacing of the cell centres.  The reference's weights come from x[b] - x[a]; with a spacing such as 0.1 that
# difference depends on the row (0.1 * 7 - 0.1 * 6 != 0.1 * 6 - 0.1 * 5 in float64), so the same move costs another few
# ulp one row further on, and after a one-row shift nearly every node loses its bit-for-bit support.  The repaired field
# is still right, but the test would no longer say anything about which nodes have to die.  0.125 is exact in binary:
# every difference of two centres is exact, as the library's res * (-dr) is for any res.
SPACING = 0.125


def move(a, si, sj, fill):
    """out[r + si, c + sj] = a[r, c] where both lie inside; `fill` in the cells that entered."""
    out = np.full_like(a, fill)
    nr, nc = a.shape[:2]
    r0, r1, c0, c1 = max(0, si), min(nr, nr + si), max(0, sj), min(nc, nc + sj)
    if r0 < r1 and c0 < c1:
        out[r0:r1, c0:c1] = a[r0 - si:r1 - si, c0 - sj:c1 - sj]
    return out


def window_lattice(world_mask, world_z, top, left, nr, nc, n_yaw, objective):
    """The lattice of the nr x nc window whose cell (0, 0) is world cell (top, left)."""
    x = -SPACING * np.arange(top, top + nr, dtype=np.float64)
    y = -SPACING * np.arange(left, left + nc, dtype=np.float64)
    return LR.Lattice(world_mask[top:top + nr, left:left + nc], n_yaw, x, y, world_z[top:top + nr, left:left + nc], objective)


def shift(lat_new, old_bits, dist, hops, si, sj, reverse=False):
    """(dist, hops, stats) of the field of old_bits after the move by (si, sj), on lat_new (the new window: its mask, its
    weights).  The sources are the nodes at hops 0; they move with the rest."""
    b = move(old_bits, si, sj, False)
    d, h, st = FU.update(lat_new, b, move(dist, si, sj, np.inf), move(hops, si, sj, FU.NONE), reverse)
    nr, nc = old_bits.shape[:2]
    st.update(shift_rows=si, shift_cols=sj, left_nodes=int(old_bits.sum()) - int(b.sum()),
              kept_cells=max(0, nr - abs(si)) * max(0, nc - abs(sj)))
    return d, h, st


def u_corridor(nr, nc, n_yaw, width, si):
    """(old mask, new mask, source, far arm): two arms of `width` cells along the rows, at columns 1.. and ..nc - 2,
    joined by a bend in the rows nr - 1 - width .. nr - 2.  With si >= width + 1 the bend lies in the rows that leave,
    nothing enters (new mask = the old one moved), and the far arm -- a boolean (nr, nc) array over the NEW window -- is
    cut off from the source in the near arm."""
    assert si >= width + 1 and nc >= 2 * width + 3 and nr > si + 3
    full = np.uint32((1 << n_yaw) - 1)
    old = np.zeros((nr, nc), np.uint32)
    old[1:nr - 1, 1:1 + width] = full
    old[1:nr - 1, nc - 1 - width:nc - 1] = full
    old[nr - 1 - width:nr - 1, 1:nc - 1] = full
    new = move(old, si, 0, 0)
    far = np.zeros((nr, nc), bool)
    far[:, nc - 1 - width:nc - 1] = new[:, nc - 1 - width:nc - 1] != 0
    return old, new, (2, 1 + width // 2, 0), far


def island(nr, nc, n_yaw, si):
    """(old mask, new mask, source, island): the columns right of the wall column nc // 2 are cut off in the old window;
    the si rows that enter at the top are open across the wall and join them.  island: boolean (nr, nc) over the NEW
    window, the cells right of the wall that were there before."""
    assert 0 < si < nr - 3
    full = np.uint32((1 << n_yaw) - 1)
    wall = nc // 2
    old = np.full((nr, nc), full, np.uint32)
    old[:, wall] = 0
    new = move(old, si, 0, 0)
    new[:si] = full
    isl = np.zeros((nr, nc), bool)
    isl[si:, wall + 1:] = True
    return old, new, (nr // 2 - si, 1, 0), isl
