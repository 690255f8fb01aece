"""CPU suite of artp_field_update_clearance's two windows (tests/field_update_clearance_ref.py), on
the numpy restatement of the clearance map and the weights (tests/clearance_ref.py): a mask edit inside sub_rect moves d2
only within radius_cells of it and weights only at nodes within radius_cells + 1, the first bound is tight, and pasting
the recomputed tiles into the old map gives the full map of the merged mask.  And the new names of the C ABI."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import clearance_ref as CR
import field_update_clearance_ref as UR
from art_planner_amd import _capi
from test_clearance_ref import random_words

RES = 0.04


def edit(mask, n_yaw, rng):
    """(sub, merged): random flips of the low bits confined to a random sub-rectangle"""
    nr, nc = mask.shape
    sr, sc = int(rng.integers(1, min(nr, 9) + 1)), int(rng.integers(1, min(nc, 9) + 1))
    r0, c0 = int(rng.integers(0, nr - sr + 1)), int(rng.integers(0, nc - sc + 1))
    flips = rng.random((sr, sc, n_yaw)) < 0.3
    word = (flips.astype(np.uint64) << np.arange(n_yaw, dtype=np.uint64)).sum(axis=2).astype(np.uint32)
    new = mask.copy()
    new[r0:r0 + sr, c0:c0 + sc] ^= word
    return (r0, c0, sr, sc), new


SPREADS = {1: (0,), 2: (0, 1), 7: (0, 1, 3), 16: (0, 1, 8)}


@pytest.mark.parametrize("outside", [False, True])
@pytest.mark.parametrize("R", [1, 5, 17])
@pytest.mark.parametrize("n_yaw", [1, 2, 7, 16])
def test_the_windows_are_sufficient(n_yaw, R, outside):
    rng = np.random.default_rng(1000 * n_yaw + 10 * R + outside)
    moved_d2 = moved_w = 0
    for spread in SPREADS[n_yaw]:
        for shape in ((40, 37), (23, 40)):
            mask = random_words(shape, n_yaw, int(rng.integers(1 << 30)), 0.93 ** (1.0 / (2 * spread + 1)))
            sub, new = edit(mask, n_yaw, rng)
            d_old = CR.clearance_map(mask, n_yaw, R, spread, outside)
            d_new = CR.clearance_map(new, n_yaw, R, spread, outside)
            ch = (d_old != d_new).any(axis=2)
            assert not (ch & ~UR.inside(shape, sub, R)).any(), (spread, shape, sub)
            moved_d2 += int(ch.sum())
            # the pasted window is the full map
            assert np.array_equal(UR.paste_window(d_old, new, n_yaw, sub, R, spread, outside), d_new), (spread, shape, sub)
            margin, gain = min(R, 4) * RES, 3.0
            for objective in (0, 1):
                w_old = UR.move_weights(mask, n_yaw, d_old, RES, margin, gain, objective)
                w_new = UR.move_weights(new, n_yaw, d_new, RES, margin, gain, objective)
                wch = w_old.view(np.uint64) != w_new.view(np.uint64)            # (10, nr, nc, n_yaw): existence included
                near = UR.inside(shape, sub, R + 1)
                tgt = UR.move_targets(d_old.shape)
                for m in range(10):
                    at = wch[m].any(axis=2)
                    assert not (at & ~near).any(), (m, "start")                   # the owner of a reverse field's slot
                    assert near[tgt[m][0][at], tgt[m][1][at]].all(), (m, "target")   # ... of a forward one
                    moved_w += int(at.sum())
            # the tile windows hold the cell windows
            a, b, c, d = UR.window(shape, sub, R)
            tiles = np.zeros(shape, bool)
            tiles[a * UR.T:(b + 1) * UR.T, c * UR.T:(d + 1) * UR.T] = True
            assert (tiles | ~UR.inside(shape, sub, R)).all()
            assert UR.clearance_tiles(shape, sub, R) == (b - a + 1) * (d - c + 1) <= UR.reprice_tiles(shape, sub, R)
            assert UR.repriced_slots(shape, sub, R, n_yaw) == UR.reprice_tiles(shape, sub, R) * 2560 * n_yaw
    assert moved_d2 > 0 and moved_w > 0


def test_the_tile_windows_by_hand():
    # 45 x 38 cells = 3 x 3 tiles; an edit over the common corner of four tiles
    shape, sub = (45, 38), (14, 13, 4, 5)
    assert UR.window(shape, sub, 5) == (0, 1, 0, 1) and UR.clearance_tiles(shape, sub, 5) == 4
    assert UR.window(shape, sub, 17) == (0, 2, 0, 2) and UR.clearance_tiles(shape, sub, 17) == 9
    # rows 20 .. 21 grown by 4: 16 .. 25, one tile; by 5: 15 .. 26, two tiles
    assert UR.clearance_tiles(shape, (20, 20, 2, 2), 4) == 1 and UR.reprice_tiles(shape, (20, 20, 2, 2), 4) == 4
    assert UR.repriced_slots(shape, (20, 20, 2, 2), 4, 7) == 4 * 2560 * 7
    # no rectangle: every tile; a window is clipped to the rectangle
    assert UR.clearance_tiles(shape, None, 5) == UR.reprice_tiles(shape, None, 5) == 9
    assert UR.window((96, 96), (92, 92, 4, 4), 5) == (5, 5, 5, 5) and UR.window((96, 96), (92, 92, 4, 4), 13) == (4, 5, 4, 5)


@pytest.mark.parametrize("R", [1, 5, 17])
def test_the_d2_window_is_tight(R):
    n = 2 * R + 7
    mask = np.ones((n, n), np.uint32)
    probe = (3, R + 3)
    new = mask.copy()
    new[probe[0] + R, probe[1]] = 0                     # one cell cleared at offset (R, 0) from the probe
    sub = (probe[0] + R, probe[1], 1, 1)
    d_old, d_new = CR.clearance_map(mask, 1, R), CR.clearance_map(new, 1, R)
    assert d_old[probe][0] == CR.NONE and d_new[probe][0] == R * R
    assert UR.inside((n, n), sub, R)[probe] and not UR.inside((n, n), sub, R - 1)[probe]   # a window of R - 1 would miss it


def test_the_new_names_are_bound_and_exported():
    names = ("artp_field_update_clearance", "artp_field_clearance_update_stats")
    for name in names:
        assert name in _capi.SYMBOLS, name
    assert C.sizeof(_capi.FieldClearanceUpdateStats) == 15 * 8 + 3 * 8
    assert [n for n, _ in _capi.FieldClearanceUpdateStats._fields_][:10] == [n for n, _ in _capi.FieldUpdateStats._fields_]
    subprocess.check_call(["make", "-s", "-C", os.path.dirname(_capi.LIB_PATH)])
    L = _capi.load()
    for name in names:
        assert hasattr(L, name), f"libartp.so does not export {name}"
