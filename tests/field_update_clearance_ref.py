"""Numpy restatement of the two windows of artp_field_update_clearance (include/artp_c.h): which
16 x 16 tiles have their clearance computed again, which have their weight-table slots priced again, and what pasting the
recomputed tiles into the old clearance map gives.  The device tests compare the update's stats with these counts."""
import numpy as np

import clearance_ref as CR
import lattice_ref as LR

T = 16                       # the tile edge (csrc/field.h FIELD_T)
SLOTS_PER_TILE = 10 * T * T  # per heading: ten moves of 256 lanes, padded lanes included


def grown(shape, sub, grow):
    """(r_lo, r_hi, c_lo, c_hi), inclusive: sub = (row0, col0, nrows, ncols) grown by `grow` cells, clipped to the rectangle"""
    nr, nc = shape
    r0, c0, sr, sc = sub
    return max(r0 - grow, 0), min(r0 + sr - 1 + grow, nr - 1), max(c0 - grow, 0), min(c0 + sc - 1 + grow, nc - 1)


def inside(shape, sub, grow):
    """(nrows, ncols) bool: the cells of sub grown by `grow`"""
    r_lo, r_hi, c_lo, c_hi = grown(shape, sub, grow)
    m = np.zeros(shape, bool)
    m[r_lo:r_hi + 1, c_lo:c_hi + 1] = True
    return m


def window(shape, sub, grow):
    """(tr_lo, tr_hi, tc_lo, tc_hi), inclusive: the tiles that intersect sub grown by `grow`"""
    r_lo, r_hi, c_lo, c_hi = grown(shape, sub, grow)
    return r_lo // T, r_hi // T, c_lo // T, c_hi // T


def window_tiles(shape, sub, grow):
    a, b, c, d = window(shape, sub, grow)
    return (b - a + 1) * (d - c + 1)


def full(shape):
    return (0, 0, shape[0], shape[1])


def clearance_tiles(shape, sub, radius_cells):
    """tiles whose d2 the update computes again (sub = None: the whole rectangle)"""
    return window_tiles(shape, sub if sub is not None else full(shape), radius_cells)


def reprice_tiles(shape, sub, radius_cells):
    return window_tiles(shape, sub if sub is not None else full(shape), radius_cells + 1)


def repriced_slots(shape, sub, radius_cells, n_yaw):
    """slots of the weight table the update prices again: every slot of the tiles within radius_cells + 1 of sub"""
    return reprice_tiles(shape, sub, radius_cells) * SLOTS_PER_TILE * n_yaw


def paste_window(old_d2, merged_mask, n_yaw, sub, radius_cells, yaw_spread=0, outside_is_obstacle=False):
    """The update's step 3: d2 of the window's tiles from the merged mask, every other tile as it was.  A tile is computed
    from the merged words of its cells and a halo of radius_cells, the rectangle's outside as the full map has it."""
    shape = merged_mask.shape
    R = int(radius_cells)
    tr_lo, tr_hi, tc_lo, tc_hi = window(shape, sub, R)
    out = old_d2.copy()
    for tr in range(tr_lo, tr_hi + 1):
        for tc in range(tc_lo, tc_hi + 1):
            r0, r1 = tr * T, min((tr + 1) * T, shape[0])
            c0, c1 = tc * T, min((tc + 1) * T, shape[1])
            # the tile and its halo, padded where the halo leaves the rectangle: all headings set and the outside ignored,
            # or no heading set, which makes the cell an obstacle of every heading
            pad = np.uint32(0) if outside_is_obstacle else np.uint32((1 << n_yaw) - 1)
            blk = np.full((r1 - r0 + 2 * R, c1 - c0 + 2 * R), pad, np.uint32)
            a0, a1, b0, b1 = max(r0 - R, 0), min(r1 + R, shape[0]), max(c0 - R, 0), min(c1 + R, shape[1])
            blk[a0 - (r0 - R):a1 - (r0 - R), b0 - (c0 - R):b1 - (c0 - R)] = merged_mask[a0:a1, b0:b1]
            d2 = CR.clearance_map(blk, n_yaw, R, yaw_spread, False)
            out[r0:r1, c0:c1] = d2[R:R + r1 - r0, R:R + c1 - c0]
    return out


def move_weights(mask, n_yaw, d2, res, margin, gain, objective=1):
    """w[m][r, c, k] of the clearance-weighted field on flat ground: lattice_ref's base cost of move m from (r, c, k), +inf
    where the edge does not exist, times clearance_ref's factor"""
    nr, nc = mask.shape
    base = LR.Lattice(mask, n_yaw, -res * np.arange(nr), -res * np.arange(nc), np.zeros((nr, nc)), objective).w
    return CR.weights(base, d2, res, margin, gain)


def move_targets(shape3):
    """b[m] = (rows, cols) index arrays of the target cell of move m from every cell (rotations: the cell itself), clipped"""
    nr, nc, _ = shape3
    r, c = np.meshgrid(np.arange(nr), np.arange(nc), indexing="ij")
    out = []
    for m in range(10):
        dr, dc = LR.MOVES[m] if m < 8 else (0, 0)
        out.append((np.clip(r + dr, 0, nr - 1), np.clip(c + dc, 0, nc - 1)))
    return out
