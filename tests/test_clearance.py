"""Clearance maps on the device (csrc/clearance.h, artp_clearance_map*) against tests/clearance_ref.py,
bit for bit: the values are exact integers.

The rectangle is 37 x 45: odd, 3 x 3 tiles of 16 x 16 cells, the last row and column of tiles padded.  Radii 17 and 32 reach
past the neighbouring tile.  Every word carries random bits above its low n_yaw ones."""
import ctypes as C

import numpy as np
import pytest

import clearance_ref as CR
from art_planner_amd import _capi
from test_clearance_ref import random_words

pytestmark = pytest.mark.gpu

NR, NC = 37, 45


@pytest.fixture(scope="module")
def ctx():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from art_planner_amd.context import Context
    c = Context(0, "yaml")
    yield c
    c.close()


def spreads(n_yaw):
    return sorted({s for s in (0, 1, n_yaw // 2) if s <= n_yaw // 2})


@pytest.mark.parametrize("R", [1, 5, 17, 32])
@pytest.mark.parametrize("n_yaw", [1, 2, 7, 16, 32])
def test_random_masks(ctx, n_yaw, R):
    for s in spreads(n_yaw):
        # p = 0.9 per eroded bit, so that distances are not all 0 or 1
        mask = random_words((NR, NC), n_yaw, 100 * n_yaw + s, 0.9 ** (1.0 / (2 * s + 1)))
        for outside in (False, True):
            want = CR.clearance_map(mask, n_yaw, R, s, outside)
            got = ctx.clearance_map(mask, n_yaw, R, yaw_spread=s, outside_is_obstacle=outside)
            assert got.shape == (NR, NC, n_yaw) and got.dtype == np.uint16
            bad = np.argwhere(got != want)
            assert len(bad) == 0, (s, outside, len(bad), bad[:4], got[tuple(bad[0])], want[tuple(bad[0])])
        vals = np.unique(want)
        print(f"  n_yaw {n_yaw} R {R} s {s}: {len(vals)} distinct values, largest finite {int(vals[vals != CR.NONE].max())}")


def test_host_and_device_forms_agree(ctx):
    import torch
    n_yaw, R = 7, 5
    mask = random_words((NR, NC), n_yaw, 9, 0.9)
    want = CR.clearance_map(mask, n_yaw, R, 1, True)
    mask_t = torch.from_numpy(np.asfortranarray(mask).T.copy().view(np.int32)).to(f"cuda:{ctx.device}").T   # column-major
    assert mask_t.shape == (NR, NC) and mask_t.stride() == (1, NR)
    d2_t = torch.zeros(NR * NC * n_yaw, dtype=torch.int16, device=f"cuda:{ctx.device}")
    ctx.use_torch_stream()
    ctx.clearance_map_dev(mask_t, n_yaw, d2_t, R, yaw_spread=1, outside_is_obstacle=True)
    torch.cuda.synchronize()
    dev = d2_t.cpu().numpy().view(np.uint16).reshape(NC, NR, n_yaw).transpose(1, 0, 2)
    assert np.array_equal(dev, want)
    assert np.array_equal(ctx.clearance_map(mask_t, n_yaw, R, yaw_spread=1, outside_is_obstacle=True), want)   # device mask, host out
    d2_t.zero_()
    ctx.clearance_map_dev(mask, n_yaw, d2_t, R, yaw_spread=1, outside_is_obstacle=True)                       # host mask, device out
    torch.cuda.synchronize()
    assert np.array_equal(d2_t.cpu().numpy().view(np.uint16).reshape(NC, NR, n_yaw).transpose(1, 0, 2), want)


@pytest.mark.parametrize("n_yaw", [1, 16, 32])
def test_all_valid_and_all_invalid(ctx, n_yaw):
    full = np.uint32((1 << n_yaw) - 1)
    m = np.full((NR, NC), full, np.uint32)
    for R in (5, 32):
        assert (ctx.clearance_map(m, n_yaw, R, yaw_spread=n_yaw // 2) == CR.NONE).all()
        r, c = np.meshgrid(np.arange(NR), np.arange(NC), indexing="ij")
        d = np.minimum(np.minimum(r + 1, NR - r), np.minimum(c + 1, NC - c))     # the nearest outside cell lies straight ahead
        want = np.where(d <= R, d * d, CR.NONE).astype(np.uint16)
        got = ctx.clearance_map(m, n_yaw, R, outside_is_obstacle=True)
        assert np.array_equal(got, np.repeat(want[..., None], n_yaw, 2))
        for outside in (False, True):
            assert (ctx.clearance_map(np.zeros((NR, NC), np.uint32), n_yaw, R, outside_is_obstacle=outside) == 0).all()
            # garbage only: still no node
            assert (ctx.clearance_map(np.full((NR, NC), ~full, np.uint32), n_yaw, R, outside_is_obstacle=outside) == 0).all()


@pytest.mark.parametrize("R", [1, 5, 17, 32])
def test_a_hole_at_the_corner_of_four_tiles(ctx, R):
    n_yaw = 2
    m = np.full((NR, NC), 3, np.uint32)
    m[16, 16] = 1                                   # heading 1 is missing at the first cell of tile (1, 1)
    got = ctx.clearance_map(m, n_yaw, R)
    r, c = np.meshgrid(np.arange(NR), np.arange(NC), indexing="ij")
    dd = (r - 16) ** 2 + (c - 16) ** 2
    want = np.where(dd <= R * R, dd, CR.NONE).astype(np.uint16)
    assert (got[..., 0] == CR.NONE).all()
    assert np.array_equal(got[..., 1], want)
    # one neighbour in each of the four tiles; the diagonal one lies outside a disc of radius 1
    assert got[15, 16, 1] == 1 and got[16, 15, 1] == 1 and got[16, 16, 1] == 0 and got[17, 17, 1] == (2 if R > 1 else CR.NONE)
    assert got[15, 15, 1] == (2 if R > 1 else CR.NONE)


def test_the_cap_is_a_disc(ctx):
    for hole, want in (((3, 4), 25), ((4, 4), CR.NONE)):
        m = np.ones((NR, NC), np.uint32)
        m[20 + hole[0], 13 + hole[1]] = 0
        got = ctx.clearance_map(m, 1, 5)
        assert got[20, 13, 0] == want
        assert np.array_equal(got, CR.clearance_map(m, 1, 5))


def test_refusals(ctx):
    L = ctx.L
    m = np.asfortranarray(np.full((NR, NC), 0x7f, np.uint32))
    out = np.full(NR * NC * 32, 0x1234, np.uint16)

    def call(n_yaw=7, nr=NR, nc=NC, **kw):
        p = _capi.ClearanceParams()
        L.artp_clearance_params_defaults(C.byref(p))
        for k, v in kw.items():
            setattr(p, k, v)
        return L.artp_clearance_map(ctx.h, C.byref(p), n_yaw, nr, nc, m.ctypes.data, 0, out.ctypes.data)

    p = _capi.ClearanceParams()
    L.artp_clearance_params_defaults(C.byref(p))
    assert (p.radius_cells, p.yaw_spread, p.outside_is_obstacle) == (12, 0, 0)
    INVALID = -1
    for kw in (dict(radius_cells=0), dict(radius_cells=33), dict(radius_cells=-3), dict(yaw_spread=-1), dict(yaw_spread=4),
               dict(n_yaw=0), dict(n_yaw=33), dict(n_yaw=1, yaw_spread=1), dict(outside_is_obstacle=2), dict(nr=0), dict(nc=-1)):
        assert call(**kw) == INVALID, kw
        assert (out == 0x1234).all()
    assert L.artp_clearance_map(ctx.h, None, 7, NR, NC, m.ctypes.data, 0, out.ctypes.data) == INVALID
    assert L.artp_clearance_map(ctx.h, C.byref(p), 7, NR, NC, None, 0, out.ctypes.data) == INVALID
    assert L.artp_clearance_map(ctx.h, C.byref(p), 7, NR, NC, m.ctypes.data, 0, None) == INVALID
    with pytest.raises(_capi.ArtpError):
        ctx.clearance_map(m, 7, 0)
    # the context is still usable, at the limits that are allowed
    assert call(radius_cells=32, yaw_spread=3) == 0 and (out[:NR * NC * 7] == CR.NONE).all()
