"""Reference for carrying a clearance-weighted cost-to-go field across a map move:
artp_field_shift_clearance restated in numpy from parts the library shares nothing with -- field_shift_ref.move for the
move, clearance_ref.clearance_map for d2 of the new window, field_update_clearance_ref.move_weights for its weights and
field_update_ref.update for the repair on the weighted lattice.  tests/test_field_shift_clearance_ref.py holds it against
the field computed on the new window.

Also the counts of the call from the slot's side (changed_slots, weight_tiles), for that test and for the device's
(tests/test_cost_field_shift_clearance.py).  The weight table holds one slot per node v and offset j: the weight of the
edge between v and its neighbour u by offset j that the search pulls along at v -- w(v -> u), move j from v, in a reverse
field; w(u -> v), the move that leads back from u, in a forward one.  The slot moves with v."""
import numpy as np

import clearance_ref as CR
import field_shift_ref as FS
import field_update_clearance_ref as UR
import lattice_learned_ref as LL
import lattice_ref as LR

T = UR.T


def weighted_window(world_mask, top, left, nr, nc, n_yaw, objective, radius_cells, margin, gain, yaw_spread=0,
                    outside_is_obstacle=False):
    """(lattice, d2) of the nr x nc window whose cell (0, 0) is world cell (top, left), on flat ground at
    field_shift_ref.SPACING: the window's own clearance map (what lies outside the window is outside the rectangle) and the
    weighted lattice over it."""
    mask = np.ascontiguousarray(world_mask[top:top + nr, left:left + nc])
    d2 = CR.clearance_map(mask, n_yaw, radius_cells, yaw_spread, outside_is_obstacle)
    w = UR.move_weights(mask, n_yaw, d2, FS.SPACING, margin, gain, objective)
    return LL.LearnedLattice(mask, n_yaw, w), d2


def slot_weights(w, reverse):
    """s[j][r, c, k] = the slot of node (r, c, k) and offset j, from w[m][r, c, k] = the cost of move m FROM (r, c, k)
    ((10, nrows, ncols, n_yaw); NaN or +inf where there is no such edge).  +inf where the slot holds no edge."""
    w = np.where(np.isnan(w), np.inf, np.asarray(w, np.float64))
    if reverse:
        return w.copy()
    _, nr, nc, ny = w.shape
    s = np.full(w.shape, np.inf)
    for j, (dr, dc) in enumerate(LR.MOVES):        # the neighbour u = v + (dr, dc); the move u -> v is 7 - j from u
        v = (slice(max(0, -dr), nr - max(0, dr)), slice(max(0, -dc), nc - max(0, dc)))
        u = (slice(max(0, dr), nr - max(0, -dr)), slice(max(0, dc), nc - max(0, -dc)))
        s[j][v] = w[7 - j][u]
    if ny > 1:
        k = np.arange(ny)
        s[8] = w[9][..., (k + 1) % ny]             # u = heading k + 1; back to k is its move 9
        s[9] = w[8][..., (k - 1) % ny]
    return s


def changed(w_before, w_after, si, sj, reverse):
    """(changed_slots, weight_tiles) of a move by (si, sj): w_before the move costs of the field before the call, w_after
    those of the field on the new window, both as slot_weights takes them.  The slots before the move go with their nodes
    (+inf in the cells that entered); a slot counts when its bit pattern differs, a tile when it holds one."""
    before = np.stack([FS.move(s, si, sj, np.inf) for s in slot_weights(w_before, reverse)])
    after = slot_weights(w_after, reverse)
    ch = np.ascontiguousarray(before).view(np.uint64) != np.ascontiguousarray(after).view(np.uint64)
    cells = np.argwhere(ch.any(axis=(0, 3)))
    tiles = {(int(r) // T, int(c) // T) for r, c in cells}
    return int(ch.sum()), len(tiles)


def shift(lat_new, lat_old, dist, hops, si, sj, reverse=False):
    """(dist, hops, stats) of the field of lat_old after the move by (si, sj), repaired on lat_new (the new window's mask,
    clearance and weights); stats as field_shift_ref.shift's, with changed_slots and weight_tiles."""
    d, h, st = FS.shift(lat_new, lat_old.bits, dist, hops, si, sj, reverse)
    st["changed_slots"], st["weight_tiles"] = changed(lat_old.w, lat_new.w, si, sj, reverse)
    return d, h, st
