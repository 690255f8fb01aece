"""artp_field_update (csrc/field.h): a cost-to-go field brought to the fixed point of an edited mask
in place must hold the bits of a field computed anew on that mask -- artp_field_compute, which the update does not touch,
is the exact oracle.  check() compares distances (bit patterns), reached_nodes, some twenty paths with their poses, and the
fold of the device's own edge costs along each path.  Every case runs in the tiled and in the plain form; the two must
agree bit for bit and kill the same number of nodes (the set of nodes that keep a chain of support is unique).  Cases 1-3
are also held against tests/lattice_ref.py's Dijkstra on the new mask, with the tolerance test_cost_field.py derives."""
import numpy as np
import pytest

from art_planner_amd import _capi
from synthetic import perlin_terrain
from test_cost_field import ROBOT, assert_field, device_map, lattice, spiral_mask


@pytest.fixture(scope="module")
def ctx():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from art_planner_amd.context import Context
    c = Context(0, ROBOT)
    yield c
    c.close()


# ---- helpers ----------------------------------------------------------------------------------------------------
def bits_of(d):
    return np.ascontiguousarray(d).view(np.uint64)


def pack(bits):
    n_yaw = bits.shape[2]
    return (bits.astype(np.uint64) << np.arange(n_yaw, dtype=np.uint64)).sum(axis=2).astype(np.uint32)


def merged(old, new, rect):
    if rect is None:
        return new.copy()
    r0, c0, nr, nc = rect
    m = old.copy()
    m[r0:r0 + nr, c0:c0 + nc] = new[r0:r0 + nr, c0:c0 + nc]
    return m


def fold(f, nodes, reverse):
    """The left fold of the device's own edge costs along a path, from the source end outwards."""
    if len(nodes) < 2:
        return np.float64(0.0)
    w = f.edge_costs(nodes[:-1], nodes[1:])
    acc = np.float64(0.0)
    for wi in (w if not reverse else w[::-1]):
        acc = acc + wi
    return acc


def check(ctx, f, mask_new, n_yaw, sources, seed=0, **kw):
    """f against a field computed anew on mask_new; returns dist."""
    reverse = bool(kw.get("reverse", False))
    with ctx.cost_field(mask_new, n_yaw, sources, **kw) as fresh:
        d, want = f.dist(), fresh.dist()
        assert np.array_equal(bits_of(d), bits_of(want)), int((bits_of(d) != bits_of(want)).sum())
        assert f.stats()["reached_nodes"] == fresh.stats()["reached_nodes"] == int(np.isfinite(want).sum())
        rng = np.random.default_rng(seed)
        fin, rest = np.argwhere(np.isfinite(want)), np.argwhere(~np.isfinite(want))
        targets = [tuple(t) for t in fin[rng.integers(0, len(fin), 16)]] + [tuple(int(v) for v in sources[0])]
        if len(rest):
            targets += [tuple(t) for t in rest[rng.integers(0, len(rest), 3)]]
        for t in targets:
            a, b = f.path(t), fresh.path(t)
            if not np.isfinite(want[t]):
                assert a is None and b is None, t
                continue
            assert np.array_equal(a[0], b[0]), t
            assert np.array_equal(bits_of(a[1]), bits_of(b[1])), t
            assert np.float64(a[2]).view(np.uint64) == want[t].view(np.uint64)
            assert fold(f, a[0], reverse).view(np.uint64) == want[t].view(np.uint64), t
    return d


def drive(ctx, n_yaw, sources, mask0, steps, ref=None, **kw):
    """One field per form on mask0, then every step (mask handed in, sub_rect, refresh_heights) on both; check() after each
    step.  ref(merged mask) -> the reference's dist, or None.  Returns the tiled form's stats per step and the last dist."""
    out, d = [], None
    cur = mask0.copy()
    with ctx.cost_field(mask0, n_yaw, sources, **kw) as ft, \
            ctx.cost_field(mask0, n_yaw, sources, plain_sweeps=True, **kw) as fp:
        for i, (m, rect, refresh) in enumerate(steps):
            arr = m.cpu().numpy().view(np.uint32).reshape(mask0.shape[1], mask0.shape[0]).T if hasattr(m, "data_ptr") else m
            cur = merged(cur, arr, rect)
            st, sp = ft.update(m, rect, refresh), fp.update(m, rect, refresh)
            print(f"  step {i}: tiled {st}")
            print(f"          plain {sp}")
            d = check(ctx, ft, cur, n_yaw, sources, seed=i, **kw)
            dp = check(ctx, fp, cur, n_yaw, sources, seed=i, **kw)
            assert np.array_equal(bits_of(d), bits_of(dp))
            for key in ("changed_words", "removed_nodes", "added_nodes", "dead_nodes", "hop_dead_nodes", "reached_nodes"):
                assert st[key] == sp[key], key
            assert sp["tile_launches"] == 0
            if ref is not None:
                assert_field(d, ref(cur))
            out.append(st)
    return out, d


def spiral_with_gap(n, n_yaw):
    """spiral_mask and the same with one more opening, right of the cut next to the source: it short-circuits ring 0 and,
    because it enters ring 1 on the far side of that ring's cut, ring 1 as well."""
    closed, src = spiral_mask(n, n_yaw)
    opened = closed.copy()
    assert closed[3, src[1] + 4] == 0 and closed[2, src[1] + 4] and closed[4, src[1] + 4]
    opened[3, src[1] + 4] = closed[2, src[1] + 4]
    return opened, closed, src


# ---- cases ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n_yaw", [1, 16])
@pytest.mark.parametrize("objective", [0, 1])
def test_closing_a_shortcut(ctx, objective, n_yaw):
    n = 48
    gm = device_map(ctx, perlin_terrain(n, 0.04, seed=11) * np.float32(0.5), 0.04, pos=(0.5, -0.25))
    opened, closed, src = spiral_with_gap(n, n_yaw)
    lat = {False: lattice(ctx, gm, opened, n_yaw, None, objective), True: lattice(ctx, gm, closed, n_yaw, None, objective)}
    before, after = lat[False].dijkstra([src])[0], lat[True].dijkstra([src])[0]
    inner = closed != 0
    inner[:8] = inner[-8:] = inner[:, :8] = inner[:, -8:] = False        # ring 2 and further in: everything behind the gap
    assert (after[inner] > before[inner] * 1.5).all() and np.isfinite(after[inner]).all()
    stats, d = drive(ctx, n_yaw, [src], opened, [(closed, None, False)], ref=lambda m: after, objective=objective)
    assert stats[0]["changed_words"] == 1 and stats[0]["removed_nodes"] == n_yaw and stats[0]["added_nodes"] == 0
    assert stats[0]["dead_nodes"] >= int(inner.sum()) * n_yaw > 0
    assert (d[inner] > before[inner] * 1.5).all()


@pytest.mark.gpu
@pytest.mark.parametrize("n_yaw", [1, 16])
@pytest.mark.parametrize("objective", [0, 1])
def test_opening_a_shortcut(ctx, objective, n_yaw):
    n = 48
    gm = device_map(ctx, perlin_terrain(n, 0.04, seed=11) * np.float32(0.5), 0.04, pos=(0.5, -0.25))
    opened, closed, src = spiral_with_gap(n, n_yaw)
    before = lattice(ctx, gm, closed, n_yaw, None, objective).dijkstra([src], True)[0]
    after = lattice(ctx, gm, opened, n_yaw, None, objective).dijkstra([src], True)[0]
    assert (after <= before).all() and (after[17, 30] < before[17, 30] / 1.5).all()     # (17, 30): the innermost ring
    gap = (3, 0, 1, n)                                                    # the wall row of the new opening
    stats, d = drive(ctx, n_yaw, [src], closed, [(opened, gap, False)], ref=lambda m: after, objective=objective,
                     reverse=True)
    assert stats[0]["changed_words"] == 1 and stats[0]["added_nodes"] == n_yaw and stats[0]["removed_nodes"] == 0
    assert stats[0]["dead_nodes"] == 0                                    # nothing lost its support: values only fall
    assert (d[17, 30] < before[17, 30] / 1.5).all()


@pytest.mark.gpu
def test_a_cut_off_island_with_rotations_of_cost_zero(ctx):
    n, n_yaw = 40, 7
    gm = device_map(ctx, perlin_terrain(n, 0.04, seed=5) * np.float32(0.4), 0.04)
    full = np.uint32((1 << n_yaw) - 1)
    old = np.full((n, n), full, np.uint32)
    old[:, 22] = 0                                  # columns 23.. are the island, across two tile columns
    old[17, 22] = full                              # joined by this one cell
    new = old.copy()
    new[17, 22] = 0
    src = (5, 5, 2)
    ref = lattice(ctx, gm, new, n_yaw, None, 0).dijkstra([src])[0]
    assert np.isinf(ref[:, 22:]).all() and np.isfinite(ref[:, :22]).all()
    stats, d = drive(ctx, n_yaw, [src], old, [(new, (10, 20, 15, 5), False)], ref=lambda m: ref, objective=0)
    assert np.isinf(d[:, 22:]).all()
    assert stats[0]["dead_nodes"] >= n * (n - 23) * n_yaw and stats[0]["removed_nodes"] == n_yaw
    assert stats[0]["reached_nodes"] == n * 22 * n_yaw


@pytest.mark.gpu
@pytest.mark.parametrize("n_yaw", [1, 2, 7, 16, 32])
def test_random_flips_across_tile_borders(ctx, n_yaw):
    elev = np.ascontiguousarray(perlin_terrain(83, 0.05, seed=21)[:, :71]) * np.float32(0.8)
    device_map(ctx, elev, 0.05, pos=(0.3, 0.7))
    rect = (7, 5, 37, 45)
    sub = (8, 10, 20, 20)                           # rows 8..27, columns 10..29: over the tile corner (16, 16)
    rng = np.random.default_rng(200 + n_yaw)
    bits = rng.random((rect[2], rect[3], n_yaw)) < 0.8
    sources = [(2, 3, 0), (33, 40, n_yaw - 1)]      # outside sub
    for s in sources:
        bits[s] = True
    new = bits.copy()
    flip = rng.random((sub[2], sub[3], n_yaw)) < 0.15
    new[sub[0]:sub[0] + sub[2], sub[1]:sub[1] + sub[3]] ^= flip
    for objective, reverse in ((0, False), (1, True)):
        stats, _ = drive(ctx, n_yaw, sources, pack(bits), [(pack(new), sub, False)], rect=rect, objective=objective,
                         reverse=reverse)
        assert stats[0]["removed_nodes"] + stats[0]["added_nodes"] == int(flip.sum())
        assert stats[0]["changed_words"] == int(flip.any(axis=2).sum())


FEW_RECT = (7, 5, 37, 45)                           # 3 x 3 tiles, partial ones on both edges
FEW_SUB = (8, 10, 20, 20)
FEW_SRC = (2, 3, 0)                                 # outside FEW_SUB


def few_sweeps_masks(n_yaw):
    """A random mask at density 0.8 over FEW_RECT and the same with random flips inside FEW_SUB, as bits."""
    rng = np.random.default_rng(300 + n_yaw)
    bits = rng.random((FEW_RECT[2], FEW_RECT[3], n_yaw)) < 0.8
    bits[FEW_SRC] = True
    new = bits.copy()
    r0, c0, nr, nc = FEW_SUB
    new[r0:r0 + nr, c0:c0 + nc] ^= rng.random((nr, nc, n_yaw)) < 0.15
    return bits, new


@pytest.mark.gpu
@pytest.mark.parametrize("n_yaw", [1, 32])
@pytest.mark.parametrize("inner_sweeps", [1, 3])
def test_tiles_that_run_out_of_inner_sweeps_flag_themselves(ctx, inner_sweeps, n_yaw):
    """inner_sweeps spent while a tile still changes: it flags itself and goes on in the next round (every other test runs
    the default of 64).  The bits of the plain form and lattice_ref's values, after the compute (step 0 hands the same mask
    in, so drive checks the computed fields) and after an update; with one inner sweep the search needs more outer rounds
    than with 64 -- the tiles did come back."""
    elev = np.ascontiguousarray(perlin_terrain(83, 0.05, seed=21)[:, :71]) * np.float32(0.8)
    gm = device_map(ctx, elev, 0.05, pos=(0.3, 0.7))
    bits, new = few_sweeps_masks(n_yaw)
    old_m, new_m = pack(bits), pack(new)
    for objective, reverse in ((0, False), (1, True)):
        kw = dict(rect=FEW_RECT, objective=objective, reverse=reverse)
        refs = {m.tobytes(): lattice(ctx, gm, m, n_yaw, FEW_RECT, objective).dijkstra([FEW_SRC], reverse)[0]
                for m in (old_m, new_m)}
        assert all(np.isfinite(r).sum() * 2 > bits.sum() for r in refs.values())   # the source reaches most of the nodes
        stats, _ = drive(ctx, n_yaw, [FEW_SRC], old_m, [(old_m, None, False), (new_m, FEW_SUB, False)],
                         ref=lambda m: refs[m.tobytes()], inner_sweeps=inner_sweeps, **kw)
        assert stats[0]["changed_words"] == 0 and stats[1]["changed_words"] == int((bits ^ new).any(axis=2).sum())
        if inner_sweeps == 1:
            with ctx.cost_field(old_m, n_yaw, [FEW_SRC], inner_sweeps=1, **kw) as few, \
                    ctx.cost_field(old_m, n_yaw, [FEW_SRC], **kw) as usual:
                for step in range(2):                   # the compute's own numbers, which an update leaves alone
                    print(f"  outer rounds: {few.stats()['outer_rounds']} at 1 inner sweep, {usual.stats()['outer_rounds']} at 64")
                    assert few.stats()["outer_rounds"] > usual.stats()["outer_rounds"]
                    few.update(new_m, FEW_SUB), usual.update(new_m, FEW_SUB)


@pytest.mark.gpu
def test_a_chain_of_five_updates_on_one_field(ctx):
    n, n_yaw = 50, 4
    device_map(ctx, perlin_terrain(n, 0.04, seed=8) * np.float32(0.5), 0.04)
    rng = np.random.default_rng(77)
    bits = rng.random((n, n, n_yaw)) < 0.85
    bits[25, 25, 0] = True
    steps, cur = [], bits
    for i, (r0, c0, nr, nc) in enumerate([(3, 3, 12, 12), (28, 10, 9, 14), (10, 30, 20, 8), (3, 3, 12, 12), (40, 40, 10, 10)]):
        nxt = cur.copy()
        block = nxt[r0:r0 + nr, c0:c0 + nc]
        if i % 2 == 0:
            block &= rng.random(block.shape) < 0.6   # removals
        else:
            block |= rng.random(block.shape) < 0.7   # additions
        steps.append((pack(nxt), (r0, c0, nr, nc), False))
        cur = nxt
    stats, _ = drive(ctx, n_yaw, [(25, 25, 0)], pack(bits), steps, objective=0)
    assert all(s["removed_nodes"] > 0 and s["added_nodes"] == 0 for s in stats[0::2])
    assert all(s["added_nodes"] > 0 and s["removed_nodes"] == 0 for s in stats[1::2])


@pytest.mark.gpu
def test_words_outside_sub_rect_are_ignored(ctx):
    import torch
    n, n_yaw = 40, 8
    device_map(ctx, perlin_terrain(n, 0.04, seed=2) * np.float32(0.2), 0.04)
    rng = np.random.default_rng(3)
    old = pack(rng.random((n, n, n_yaw)) < 0.85)
    old[1, 1] |= 1
    junk = pack(rng.random((n, n, n_yaw)) < 0.5)    # differs from old nearly everywhere
    sub = (12, 9, 11, 17)
    want = merged(old, junk, sub)
    assert (want != junk).sum() > n * n // 2 and (want != old).any()
    # the same words as a device tensor in the layout reachability_map_dev writes
    t = torch.from_numpy(np.ascontiguousarray(junk.T).view(np.int32).reshape(-1)).to("cuda:0")
    for m in (junk, t):
        stats, _ = drive(ctx, n_yaw, [(1, 1, 0)], old, [(m, sub, False)], objective=1)
        assert stats[0]["changed_words"] == int(((want ^ old) != 0).sum())


@pytest.mark.gpu
def test_refreshed_heights(ctx):
    n, n_yaw = 40, 4
    gm = device_map(ctx, perlin_terrain(n, 0.04, seed=6) * np.float32(0.3), 0.04)
    mask = np.full((n, n), (1 << n_yaw) - 1, np.uint32)
    mask[5:30, 12] = 0
    src = (20, 2, 1)
    z = np.asfortranarray(ctx.reachability_poses(1)[..., 0, 2], dtype=np.float32)
    bumped = z.copy(order="F")
    bumped[14:24, 20:30] += np.float32(0.3)
    patch = (13, 19, 12, 12)                        # the bumped cells grown by one

    def upload(elev):
        ls = [gm["cum_prob"], np.ascontiguousarray(gm["cum_prob_rowwise"], np.float32), elev, gm["normal_x"],
              gm["normal_y"], gm["normal_z"], gm["plane_fit_std_dev"]]
        ctx._chk(ctx.L.artp_upload_sampler_layers(ctx.h, *[a.ctypes.data for a in ls], n, n, gm.len_x, gm.len_y,
                                                  gm.pos_x, gm.pos_y), "artp_upload_sampler_layers")

    with ctx.cost_field(mask, n_yaw, [src], objective=0) as f, \
            ctx.cost_field(mask, n_yaw, [src], objective=0, plain_sweeps=True) as p:
        before = f.dist()
        upload(bumped)
        try:
            assert np.array_equal(ctx.reachability_poses(1)[..., 0, 2].astype(np.float32), bumped)
            for fld in (f, p):
                st = fld.update(mask, patch, refresh_heights=False)     # the field keeps its own heights
                assert st["changed_words"] == 0 and st["dead_nodes"] == 0 and st["unsupport_rounds"] == 0
                assert np.array_equal(bits_of(fld.dist()), bits_of(before))
            st, sp = f.update(mask, patch, refresh_heights=True), p.update(mask, patch, refresh_heights=True)
            print("  tiled", st, "\n  plain", sp)
            assert st["changed_words"] == 0 and st["dead_nodes"] == sp["dead_nodes"] > 0
            d = check(ctx, f, mask, n_yaw, [src], objective=0)           # a new field reads the new heights
            dp = check(ctx, p, mask, n_yaw, [src], objective=0)
            assert np.array_equal(bits_of(d), bits_of(dp))
            assert (d[16:22, 22:28] != before[16:22, 22:28]).all()
            assert_field(d, lattice(ctx, gm, mask, n_yaw, None, 0).dijkstra([src])[0])
        finally:
            upload(z)


@pytest.mark.gpu
def test_the_same_mask_changes_nothing(ctx):
    n, n_yaw = 40, 8
    device_map(ctx, perlin_terrain(n, 0.04, seed=2) * np.float32(0.2), 0.04)
    mask = pack(np.random.default_rng(4).random((n, n, n_yaw)) < 0.8)
    mask[20, 20] |= 1
    with ctx.cost_field(mask, n_yaw, [(20, 20, 0)]) as f:
        before, reached = f.dist(), f.stats()["reached_nodes"]
        st = f.update(mask)
        assert st["changed_words"] == 0 and st["dead_nodes"] == 0 and st["removed_nodes"] == st["added_nodes"] == 0
        assert st["tile_launches"] == 0 and st["reached_nodes"] == reached
        assert np.array_equal(bits_of(f.dist()), bits_of(before))
    stats, d = drive(ctx, n_yaw, [(20, 20, 0)], mask, [(mask, None, False), (mask, (0, 0, 5, 5), False)])
    assert all(s["changed_words"] == 0 and s["dead_nodes"] == 0 for s in stats)
    assert np.array_equal(bits_of(d), bits_of(before))


@pytest.mark.gpu
def test_a_far_corner_stays_local(ctx):
    n, n_yaw = 96, 8
    device_map(ctx, perlin_terrain(n, 0.04, seed=11) * np.float32(0.5), 0.04)
    old = np.full((n, n), (1 << n_yaw) - 1, np.uint32)
    new = old.copy()
    new[93, 93] = 0
    src = (2, 2, 0)
    with ctx.cost_field(old, n_yaw, [src]) as f:
        fresh = f.stats()
    assert fresh["tiles"] == 36 and fresh["tile_launches"] >= 36 and fresh["hop_tile_launches"] >= 36
    stats, _ = drive(ctx, n_yaw, [src], old, [(new, None, False)])
    print(f"  update: {stats[0]['tile_launches']} tile runs; a new field: "
          f"{fresh['tile_launches']} + {fresh['hop_tile_launches']}")
    assert stats[0]["dead_nodes"] > 0
    assert stats[0]["tile_launches"] < fresh["tile_launches"] + fresh["hop_tile_launches"]
    assert stats[0]["tile_launches"] <= 4 * 4       # four passes over the corner tile and at most its three neighbours


@pytest.mark.gpu
def test_refusals_leave_the_field_untouched(ctx):
    import torch
    n, n_yaw = 40, 4
    device_map(ctx, perlin_terrain(n, 0.04, seed=2) * np.float32(0.2), 0.04)
    mask = np.full((n, n), 0xf, np.uint32)
    src = (10, 10, 1)
    gone = mask.copy()
    gone[10, 10] = 0b1101
    gone[20:30, 20:30] = 0
    for plain in (False, True):
        with ctx.cost_field(mask, n_yaw, [src, (30, 5, 0)], plain_sweeps=plain) as f:
            before = f.dist()
            with pytest.raises(_capi.ArtpError) as e:
                f.update(gone)                                           # the source's bit removed
            assert e.value.status == -1
            assert np.array_equal(bits_of(f.dist()), bits_of(before))
            for rect in [(35, 0, 10, 10), (0, -1, 5, 5), (0, 0, 0, 5), (0, 0, 41, 1), (0, 39, 1, 2)]:
                with pytest.raises(_capi.ArtpError) as e:
                    f.update(gone, rect)
                assert e.value.status == -1, rect
            with pytest.raises(_capi.ArtpError) as e:
                f.update(torch.zeros(n * n - 1, dtype=torch.int32, device="cuda:0"))
            assert e.value.status is None                                # refused before the library saw it
            with pytest.raises(_capi.ArtpError):
                f.update(gone[:, :-1])
            assert np.array_equal(bits_of(f.dist()), bits_of(before))
            st = f.update(gone, (15, 15, 20, 20))                        # the source's cell lies outside: a valid update
            assert st["removed_nodes"] == 100 * n_yaw
            check(ctx, f, merged(mask, gone, (15, 15, 20, 20)), n_yaw, [src, (30, 5, 0)])
