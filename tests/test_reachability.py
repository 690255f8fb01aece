"""Reachability maps (csrc/reach.h, include/artp_c.h artp_reachability_*): the lattice poses against a numpy restatement
of their definition, every mask bit against the CPU oracle and Context.validate_states on the device's own poses, rectangles,
chunking, the _dev form, argument checks and the incremental halo rule."""
import ctypes as C
import math

import numpy as np
import pytest

import common
import oracle_py as O
from art_planner_amd import _capi
from synthetic import GridMap, map_from_device, perlin_terrain, raw_map

ROBOT = "yaml"


# ---- the definition, restated -------------------------------------------------------------------------------------
def lattice_poses(gm, n_yaw, rect=None):
    """(nrows, ncols, n_yaw, 7): cell centre, yaw bin, Map::get3DPoseFrom2D's z / roll / pitch, setSO3FromRPY."""
    r0, c0, nr, nc = rect if rect is not None else (0, 0, gm.rows, gm.cols)
    res = gm.len_x / gm.rows
    px = (gm.pos_x + (0.5 * gm.len_x - 0.5 * res)) + res * -np.arange(r0, r0 + nr, dtype=np.float64)
    py = (gm.pos_y + (0.5 * gm.len_y - 0.5 * res)) + res * -np.arange(c0, c0 + nc, dtype=np.float64)
    sl = (slice(r0, r0 + nr), slice(c0, c0 + nc))
    h, nx, ny, nz = (gm[k][sl].astype(np.float64)[..., None] for k in ("elevation", "normal_x", "normal_y", "normal_z"))
    yaw = (2.0 * np.pi / n_yaw) * np.arange(n_yaw, dtype=np.float64)
    yaw = np.where(yaw > np.pi, yaw - 2.0 * np.pi, yaw)
    cy, sy = np.cos(yaw), np.sin(yaw)
    with np.errstate(invalid="ignore"):   # non-finite cells: NaN, overwritten below
        bx, by = cy * nx + sy * ny, -sy * nx + cy * ny     # Quaterniond(AngleAxisd(yaw, Z)).inverse() * normal_w
        roll, pitch = -np.arctan2(by, nz), np.arctan2(bx, nz)
        w, qx, qy, qz = common.rpy_to_quat(roll, pitch, np.broadcast_to(yaw, roll.shape))
    out = np.empty((nr, nc, n_yaw, 7))
    out[..., 0] = px[:, None, None]
    out[..., 1] = py[None, :, None]
    out[..., 2] = h
    out[..., 3], out[..., 4], out[..., 5], out[..., 6] = qx, qy, qz, w
    out[~cells_finite(gm, rect), :, 2:] = np.nan
    return out


def cells_finite(gm, rect=None):
    r0, c0, nr, nc = rect if rect is not None else (0, 0, gm.rows, gm.cols)
    sl = (slice(r0, r0 + nr), slice(c0, c0 + nc))
    return np.logical_and.reduce([np.isfinite(gm[k][sl]) for k in ("elevation", "normal_x", "normal_y", "normal_z")])


def mask_bits(mask, n_yaw):
    return ((mask[..., None] >> np.arange(n_yaw, dtype=np.uint32)) & 1).astype(np.uint8)


def assert_poses(gm, dev, n_yaw, rect=None):
    ref = lattice_poses(gm, n_yaw, rect)
    fin = cells_finite(gm, rect)
    assert dev.shape == ref.shape
    assert np.array_equal(dev[..., :2], ref[..., :2])
    np.testing.assert_allclose(dev[fin], ref[fin], rtol=0, atol=1e-12)
    assert np.isnan(dev[~fin][..., 2:]).all()


def check_every_label(ctx, gm, n_yaw, robot=ROBOT, rect=None):
    """Every bit of the mask of the whole map (or of rect = (row0, col0, nrows, ncols)) == the oracle's and
    validate_states' label of the device's own pose.  robot: a preset's name or the oracle's Robot of the context."""
    rob = robot if isinstance(robot, O.Robot) else O.robot(robot)
    mask = ctx.reachability_map(n_yaw, rect)
    poses = ctx.reachability_poses(n_yaw, rect)
    assert mask.shape == ((gm.rows, gm.cols) if rect is None else tuple(rect[2:])) and mask.dtype == np.uint32
    assert_poses(gm, poses, n_yaw, rect)
    assert (mask >> np.uint32(n_yaw) == 0).all()
    fin = cells_finite(gm, rect)
    assert (mask[~fin] == 0).all()
    states = poses[fin].reshape(-1, 7)
    bits = mask_bits(mask, n_yaw)[fin].reshape(-1)
    assert np.array_equal(bits, common.oracle_states_valid_threaded(gm, rob, states))
    assert np.array_equal(bits, ctx.validate_states(states))
    return mask


def halo_cells(rob, res):
    """artp_reachability_halo's definition: a box of a lattice pose lies within |offset| + its 3-D half-diagonal of the
    cell centre whatever the attitude (the feet's offset in the plane, the torso's from the feet plane); the larger of the
    two in cells, rounded up, plus the window margin of 4 samples."""
    toz = rob.torso_off_z - rob.feet_off_z
    torso = math.sqrt(rob.torso_off_x ** 2 + rob.torso_off_y ** 2 + toz ** 2) + 0.5 * math.sqrt(
        rob.torso_length ** 2 + rob.torso_width ** 2 + rob.torso_height ** 2)
    feet = math.sqrt(rob.feet_off_x ** 2 + rob.feet_off_y ** 2) + 0.5 * math.sqrt(
        rob.reach_x ** 2 + rob.reach_y ** 2 + rob.reach_z ** 2)
    return int(math.ceil(max(torso, feet) / res)) + 4


def check_halo_grown_recompute(ctx, gm, n_yaw, block, full0=None):
    """Raise block = (row0, col0, nrows, ncols) of both validity layers by 1 m, recompute the block grown by the halo
    (clipped to the map), paste it into the mask from before the edit: equal to a full recompute.  Returns (mask before,
    mask after, halo)."""
    full0 = ctx.reachability_map(n_yaw) if full0 is None else full0
    halo = ctx.reachability_halo()
    r0, c0, nr, nc = block
    sl = (slice(r0, r0 + nr), slice(c0, c0 + nc))
    # an obstacle block written to both validity layers; the sampler layers (heights, normals: the poses) stay
    ctx.update_layer_rects(0, [gm["elevation"][sl] + np.float32(1.0)], [(r0, c0)])
    ctx.update_layer_rects(1, [gm["elevation_masked"][sl] + np.float32(1.0)], [(r0, c0)])
    g0, h0 = max(0, r0 - halo), max(0, c0 - halo)
    g1, h1 = min(gm.rows, r0 + nr + halo), min(gm.cols, c0 + nc + halo)
    pasted = full0.copy()
    pasted[g0:g1, h0:h1] = ctx.reachability_map(n_yaw, (g0, h0, g1 - g0, h1 - h0))
    full1 = ctx.reachability_map(n_yaw)
    assert np.array_equal(pasted, full1)
    return full0, full1, halo


# ---- maps -------------------------------------------------------------------------------------------------------
def device_map(ctx, elev, res, pos=(0.0, 0.0), kind=ROBOT):
    """elev as the body / sampler elevation, every derived layer from the device preprocessing, installed."""
    raw = GridMap(elev.shape[0], elev.shape[1], res, *pos)
    raw.add("elevation", elev)
    raw.add("traversability", np.ones(elev.shape, np.float32))
    return map_from_device(ctx, raw, kind)


def c2_map(ctx):
    return map_from_device(ctx, raw_map(400, 0.04, seed=1234), ROBOT)


@pytest.fixture(scope="module")
def ctx():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from art_planner_amd.context import Context
    c = Context(0, ROBOT)
    yield c
    c.close()


# ---- CPU: the C ABI without a device ---------------------------------------------------------------------------
def test_reachability_entry_points_are_exported_and_refuse_a_null_context():
    L = _capi.load()
    mask = np.zeros(4, np.uint32)
    se3 = np.zeros(28)
    cells = C.c_int(0)
    assert L.artp_reachability_map(None, 16, None, mask.ctypes.data) == -1
    assert L.artp_reachability_map_dev(None, 16, None, mask.ctypes.data) == -1
    assert L.artp_reachability_poses(None, 16, None, se3.ctypes.data) == -1
    assert L.artp_reachability_halo(None, C.byref(cells)) == -1


# ---- GPU -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_poses_match_the_definition_on_the_c2_map(ctx):
    gm = c2_map(ctx)
    for n_yaw in (1, 7, 16, 32):
        assert_poses(gm, ctx.reachability_poses(n_yaw), n_yaw)
        rect = (37, 101, 53, 29)
        assert_poses(gm, ctx.reachability_poses(n_yaw, rect), n_yaw, rect)
    rect = (399, 0, 1, 1)
    assert_poses(gm, ctx.reachability_poses(16, rect), 16, rect)
    # heading 0 is bin 0 whatever n_yaw: the same pose
    assert np.array_equal(ctx.reachability_poses(1)[..., 0, :], ctx.reachability_poses(32)[..., 0, :])


@pytest.mark.gpu
def test_every_label_of_the_c2_map_at_16_headings(ctx):
    gm = c2_map(ctx)
    mask = check_every_label(ctx, gm, 16)
    bits = mask_bits(mask, 16)
    assert 0 < bits.sum() < bits.size


@pytest.mark.gpu
def test_every_label_of_a_flat_map(ctx):
    gm = device_map(ctx, np.zeros((160, 160), np.float32), 0.04, pos=(1.0, -2.0))
    mask = check_every_label(ctx, gm, 16)
    # flat ground: every heading of an interior cell is valid; the border strip where feet leave the map is not
    assert (mask[40:120, 40:120] == 0xffff).all()
    assert (mask != 0xffff).any()


@pytest.mark.gpu
def test_every_label_of_the_slab_slit_map(ctx):
    gm = common.slab_slit_map()
    pre = device_map(ctx, gm["elevation"], gm.res)
    for name in ("normal_x", "normal_y", "normal_z", "plane_fit_std_dev", "cum_prob", "cum_prob_rowwise"):
        gm.layers[name] = pre.layers[name]
    ctx.upload_map(gm)   # the map's own masked layer for the feet
    mask = check_every_label(ctx, gm, 16)
    assert (mask == 0).any() and (mask == 0xffff).any()


@pytest.mark.gpu
@pytest.mark.parametrize("res,robot", [(0.025, "defaults"), (0.1, "yaml")])
def test_every_label_of_a_non_square_odd_map(ctx, res, robot):
    # 0.025 m: the finest spacing whose box windows fit the LDS tile for the default robot (the YAML robot needs >= 0.03 m)
    from art_planner_amd.context import Context
    c = Context(0, robot)
    elev = perlin_terrain(123, res, seed=77)[:, :77] * np.float32(0.6)
    gm = device_map(c, np.ascontiguousarray(elev), res, pos=(0.3, 0.7), kind=robot)
    for n_yaw in (16, 5):
        check_every_label(c, gm, n_yaw, robot)
    c.close()


@pytest.mark.gpu
def test_non_finite_cells_are_zero_and_never_validated(ctx):
    elev = perlin_terrain(150, 0.04, seed=5) * np.float32(0.5)
    elev[60:66, 40:48] = np.nan                 # a hole in the elevation
    gm = device_map(ctx, elev, 0.04)
    gm.layers["normal_x"] = gm["normal_x"].copy(order="F")
    gm.layers["normal_y"] = gm["normal_y"].copy(order="F")
    gm.layers["normal_z"] = gm["normal_z"].copy(order="F")
    gm["normal_x"][100:104, 90:95] = np.nan     # holes in the normals only
    gm["normal_z"][20, 130] = np.inf
    gm["normal_y"][140:142, 10:12] = -np.inf
    ctx.upload_map(gm)
    fin = cells_finite(gm)
    assert not fin[60:66, 40:48].any() and not fin[100:104, 90:95].any() and not fin[20, 130]
    mask = check_every_label(ctx, gm, 16)
    assert (mask[~fin] == 0).all()
    assert mask.any()


@pytest.mark.gpu
def test_rects_are_slices_of_the_whole_map(ctx):
    import torch
    gm = c2_map(ctx)
    full = ctx.reachability_map(8)
    rects = [(0, 0, 17, 23), (383, 0, 17, 40), (0, 377, 30, 23), (390, 390, 10, 10), (200, 150, 1, 1),
             (0, 0, 400, 1), (0, 399, 400, 1), (399, 0, 1, 400), (123, 45, 67, 89), (0, 0, 400, 400)]
    for r0, c0, nr, nc in rects:
        part = ctx.reachability_map(8, (r0, c0, nr, nc))
        assert part.shape == (nr, nc)
        assert np.array_equal(part, full[r0:r0 + nr, c0:c0 + nc]), (r0, c0, nr, nc)
        # the _dev form: the same words, column-major, on the device
        t = torch.full((nr * nc,), -1, dtype=torch.int32, device="cuda:0")
        ctx.use_torch_stream()
        ctx.reachability_map_dev(t, 8, (r0, c0, nr, nc))
        torch.cuda.synchronize()
        assert np.array_equal(t.cpu().numpy().view(np.uint32).reshape(nc, nr).T, part), (r0, c0, nr, nc)
    t = torch.zeros(gm.rows * gm.cols, dtype=torch.int32, device="cuda:0")
    ctx.reachability_map_dev(t, 8)
    torch.cuda.synchronize()
    assert np.array_equal(t.cpu().numpy().view(np.uint32).reshape(gm.cols, gm.rows).T, full)


@pytest.mark.gpu
def test_800_map_at_32_headings_spans_several_chunks(ctx):
    import torch
    gm = map_from_device(ctx, raw_map(800, 0.04, seed=99), ROBOT)
    n_yaw = 32
    mask = ctx.reachability_map(n_yaw)
    assert gm.rows * gm.cols * n_yaw > 4 * (1 << 22)
    poses = ctx.reachability_poses(n_yaw)
    # cell-major, column-major order (the C layout): no copy of the 1.1 GB of poses
    flat = poses.transpose(1, 0, 2, 3).reshape(-1, 7)
    bits = mask_bits(mask.T.reshape(-1), n_yaw).reshape(-1)
    step = 1 << 22
    for lo in range(0, len(flat), step):
        assert np.array_equal(bits[lo:lo + step], ctx.validate_states(flat[lo:lo + step])), lo
    t = torch.zeros(gm.rows * gm.cols, dtype=torch.int32, device="cuda:0")
    ctx.use_torch_stream()
    ctx.reachability_map_dev(t, n_yaw)
    torch.cuda.synchronize()
    assert np.array_equal(t.cpu().numpy().view(np.uint32).reshape(gm.cols, gm.rows).T, mask)
    i = np.random.default_rng(3).integers(0, len(flat), 200000)
    assert np.array_equal(bits[i], common.oracle_states_valid_threaded(gm, O.robot(ROBOT), flat[i]))


@pytest.mark.gpu
def test_bad_arguments_raise_and_leave_the_context_usable(ctx):
    from art_planner_amd.context import Context
    fresh = Context(0, ROBOT)
    fresh._grid = (10, 10)   # as if a map were installed: the library itself must refuse
    with pytest.raises(_capi.ArtpError) as e:
        fresh.reachability_map(16)
    assert e.value.status == -4   # ARTP_ERR_NO_MAP
    with pytest.raises(_capi.ArtpError):
        fresh.reachability_halo()
    fresh.close()
    c2_map(ctx)
    v = ctx.map_version()
    good = ctx.reachability_map(4, (10, 20, 8, 9))
    for n_yaw, rect in [(0, None), (33, None), (-1, None), (16, (0, 0, 0, 5)), (16, (0, 0, 5, 0)),
                        (16, (395, 0, 10, 10)), (16, (0, 395, 10, 10)), (16, (-1, 0, 5, 5)), (16, (0, -3, 5, 5))]:
        with pytest.raises(_capi.ArtpError) as e:
            ctx.reachability_map(n_yaw, rect)
        assert e.value.status == -1, (n_yaw, rect)   # ARTP_ERR_INVALID_ARG
        with pytest.raises(_capi.ArtpError):
            ctx.reachability_poses(n_yaw, rect)
    assert np.array_equal(ctx.reachability_map(4, (10, 20, 8, 9)), good)
    assert ctx.map_version() == v
    ctx.reachability_map(16)
    ctx.reachability_poses(3, (0, 0, 4, 4))
    assert ctx.map_version() == v


@pytest.mark.gpu
def test_halo_grown_recompute_equals_a_full_recompute(ctx):
    gm = c2_map(ctx)
    n_yaw = 8
    r0, c0, nr, nc = 180, 150, 20, 25
    full0, full1, halo = check_halo_grown_recompute(ctx, gm, n_yaw, (r0, c0, nr, nc))
    assert halo > 4
    assert halo == halo_cells(O.robot(ROBOT), gm.res)
    written = np.zeros(full0.shape, bool)
    written[r0:r0 + nr, c0:c0 + nc] = True
    changed = full1 != full0
    assert (changed & ~written).any()   # the halo is not 0: cells next to the block change too
    # the same near a corner: the grown rectangle clipped to the map
    assert halo > 3 and 390 + 10 + halo >= gm.cols
    check_halo_grown_recompute(ctx, gm, n_yaw, (3, 390, 6, 10), full0=full1)
