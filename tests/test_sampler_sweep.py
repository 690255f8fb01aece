"""The state sampler and the bitmap exchange across CDF and map shapes (-m gpu).

Part 1, the sampler (sampler_pack_kernel, sample_one, sample_states_kernel, sample_states_at_kernel): every probe map
of tests/sampler_probe.py (tests/test_sampler_probe.py proves on the CPU which search forms and edge classes each one
reaches) against the C oracle's linear-scan sampler.  CELL: exact -- a state more than half a cell from the oracle's is
reported as a wrong cell, with the oracle's (row, col).  STATE: 1e-12 on all seven numbers (the bar of
test_sampler_matches_oracle); at the UTM-sized origin one ulp of a coordinate is 9.3e-10, so x and y get 2 ulp there
(both sides form the position with the same IEEE operations; a contracted multiply-add in the perturbation along the
normal could move the sum by one ulp) -- the test prints whether they were in fact bit-equal.  Every entry point that
runs sample_one is BIT-EQUAL to sample_states for the same (seed, index), and no device entry point writes past 7 n
doubles (NaN sentinels behind the buffer).  Rows whose CDF turns NaN part-way stay on the CPU (include/artp_c.h:
a CDF row is NaN-free or NaN throughout); rows that are NaN throughout are swept.

Part 2, the bitmap kernels (bits_word_offsets_kernel, materialise_from_bits_kernel, pack_valid_bits_kernel,
artp_indices_from_bits_dev) against numpy on the unpacked bits, on synthetic bitmaps of up to 64 tiles and 16 ranks."""
import numpy as np
import pytest

import sampler_probe as SP

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 255, 256, 257]
ARTP_ERR_INVALID_ARG = -1
PAD = 7 * 64 + 5          # doubles behind an output buffer: the LDS-staged stores of sample_states_kernel write rows of 64


# ---- contexts and comparisons ------------------------------------------------------------------------------------------
def _ctx(kind="yaml", from_dist=1):
    from art_planner_amd.context import Context, make_params
    return Context(0, make_params(kind, sample_from_distribution=from_dist))


def install(ctx, gm, validity):
    """validity: both height fields too (Context.upload_map; needs two rows and columns); else the sampler layers alone."""
    if validity:
        ctx.upload_map(gm)
        return
    ls = [np.asfortranarray(gm["cum_prob"], np.float32), np.ascontiguousarray(gm["cum_prob_rowwise"], np.float32)] + [
        np.asfortranarray(gm[k], np.float32) for k in ("elevation", "normal_x", "normal_y", "normal_z", "plane_fit_std_dev")]
    ctx._chk(ctx.L.artp_upload_sampler_layers(ctx.h, *[a.ctypes.data for a in ls], gm.rows, gm.cols, gm.len_x, gm.len_y,
                                              gm.pos_x, gm.pos_y), "artp_upload_sampler_layers")


def assert_states(sg, so, rc, gm, what):
    """Cell exact, then the state bar."""
    assert sg.shape == so.shape, what
    d = np.abs(sg - so)
    wrong = ~((d[:, 0] <= 0.5 * gm.res) & (d[:, 1] <= 0.5 * gm.res))
    if wrong.any():
        i = int(np.argmax(wrong))
        pytest.fail(f"{what}: WRONG CELL for {int(wrong.sum())} of {len(sg)} samples (position more than half a cell from "
                    f"the oracle's); first at sample {i}: oracle cell (row, col) = {tuple(int(v) for v in rc[i])}, oracle "
                    f"xy = {so[i, :2]}, GPU xy = {sg[i, :2]}")
    tol = np.full(so.shape, 1e-12)
    if max(abs(gm.pos_x), abs(gm.pos_y)) > 1e4:
        tol[:, :2] = 2.0 * np.spacing(np.abs(so[:, :2]))
    bad = ~(d <= tol)
    assert not bad.any(), (f"{what}: {int(bad.any(axis=1).sum())} of {len(sg)} states beyond the bar; max |diff| per number "
                           f"{d.max(axis=0)}; first at sample {int(np.argmax(bad.any(axis=1)))}")


def bit_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def _padded(n, torch):
    return torch.full((7 * n + PAD,), float("nan"), dtype=torch.float64, device="cuda")


def _take(buf, n, what):
    """The n states of a padded device buffer; the sentinels behind them must stand."""
    h = buf.cpu().numpy()
    assert np.isnan(h[7 * n:]).all(), f"{what}: wrote past 7 * n doubles"
    return h[:7 * n].reshape(n, 7)


def states_dev(ctx, seed, first, n):
    import torch
    buf = _padded(n, torch)
    ctx.sample_states_dev(seed, first, n, buf)
    torch.cuda.synchronize()
    return _take(buf, n, f"sample_states_dev n={n}")


def entry_points(ctx, seed, first, n, ref, validity):
    """Every entry point that runs sample_one, against ref = sample_states(seed, first, n): bit-equal."""
    import torch
    rng = np.random.default_rng(n)
    assert bit_equal(states_dev(ctx, seed, first, n), ref), f"sample_states_dev n={n}"
    if validity:
        se3, _ = ctx.sample_and_validate(seed, first, n)
        assert bit_equal(se3, ref), f"sample_and_validate n={n}"
        buf = _padded(n, torch)
        valid = torch.zeros(n, dtype=torch.uint8, device="cuda")
        ctx.sample_and_validate_dev(seed, first, n, buf, valid)
        torch.cuda.synchronize()
        assert bit_equal(_take(buf, n, f"sample_and_validate_dev n={n}"), ref), f"sample_and_validate_dev n={n}"
    # explicit indices: shuffled, with repeats, and the device count once below and once above the capacity
    for name, idx, count, cap in (("shuffled", rng.permutation(n), n, n),
                                  ("repeats", rng.integers(0, n, n + 3), n + 3, n + 3),
                                  ("count below cap", rng.permutation(n)[:(n + 1) // 2], (n + 1) // 2, n),
                                  ("count above cap", rng.permutation(n), n, (n + 1) // 2)):
        idx_t = torch.from_numpy(idx.astype(np.int32)).cuda()
        cnt_t = torch.tensor([count], dtype=torch.int64, device="cuda")
        buf = _padded(cap, torch)
        ctx.sample_states_at_dev(seed, first, idx_t, cnt_t, cap, buf)
        torch.cuda.synchronize()
        k = min(count, cap)
        h = buf.cpu().numpy()
        assert np.isnan(h[7 * k:]).all(), f"sample_states_at_dev {name} n={n}: wrote past min(count, cap) states"
        assert bit_equal(h[:7 * k].reshape(k, 7), ref[idx[:k]]), f"sample_states_at_dev {name} n={n}"
    # the bitmap route: every candidate accepted
    words = (n + 63) // 64
    bits = np.full(words, -1, np.int64)
    g = torch.from_numpy(bits.reshape(1, words)).cuda()
    out = torch.full((1, n + 2, 7), float("nan"), dtype=torch.float64, device="cuda")
    counts = torch.zeros(1, dtype=torch.int64, device="cuda")
    ctx.materialise_from_bits_dev(seed, g, n, [first], n + 2, out, counts)
    torch.cuda.synchronize()
    o = out.cpu().numpy()[0]
    assert int(counts.item()) == n and bit_equal(o[:n], ref) and np.isnan(o[n:]).all(), f"materialise_from_bits_dev n={n}"


# ---- part 1: every probe map through sample_states --------------------------------------------------------------------------
@pytest.mark.parametrize("p", SP.gpu_probes(), ids=lambda p: p.name)
def test_probe_map_matches_oracle(p):
    so, rc = SP.oracle_samples(p, "yaml")
    ctx = _ctx("yaml")
    try:
        install(ctx, p.gm, validity=False)
        sg = ctx.sample_states(p.seed, p.first, p.n)
        assert_states(sg, so, rc, p.gm, f"{p.name} sample_states n={p.n}")
        if max(abs(p.gm.pos_x), abs(p.gm.pos_y)) > 1e4:
            print(f"{p.name}: x, y bit-equal to the oracle: {bit_equal(sg[:, :2], so[:, :2])}; "
                  f"max |dx|, |dy| = {np.abs(sg[:, :2] - so[:, :2]).max(axis=0)}")
        assert bit_equal(states_dev(ctx, p.seed, p.first, p.n), sg)
        for n in (1, 63, 64, 65):
            s = ctx.sample_states(p.seed, p.first, n)
            assert_states(s, so[:n], rc[:n], p.gm, f"{p.name} sample_states n={n}")
            assert bit_equal(s, sg[:n]) and bit_equal(states_dev(ctx, p.seed, p.first, n), s), (p.name, n)
    finally:
        ctx.close()


# ---- the full cross on four maps: one per search form and a tie probe ----------------------------------------------------------
@pytest.mark.parametrize("kind", ["yaml", "defaults"])
@pytest.mark.parametrize("name", SP.CROSS)
def test_full_cross(name, kind):
    p = SP.probe(name)
    assert p.n >= 1 << 18
    so, rc = SP.oracle_samples(p, kind)
    ctx = _ctx(kind)
    try:
        install(ctx, p.gm, validity=True)
        ctx.use_torch_stream()
        for n in SIZES + [p.n]:
            ref = ctx.sample_states(p.seed, p.first, n)
            assert_states(ref, so[:n], rc[:n], p.gm, f"{name} {kind} sample_states n={n}")
            entry_points(ctx, p.seed, p.first, n, ref, validity=True)
    finally:
        ctx.close()


# ---- sample_from_distribution = 0: the CDFs are not read -------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["yaml", "defaults"])
@pytest.mark.parametrize("name", ["origin_zero_0.04", "origin_near_0.07", "origin_utm_0.1", "cross_cols_le_512"])
def test_uniform_position_sampling(name, kind):
    p = SP.probe(name)
    n = 1 << 16
    so, rc = SP.oracle_samples(p, kind, n=n, sample_uniform=True)
    ctx = _ctx(kind, from_dist=0)
    try:
        validity = name.startswith("cross")
        install(ctx, p.gm, validity)
        ctx.use_torch_stream()
        sg = ctx.sample_states(p.seed, p.first, n)
        assert_states(sg, so, rc, p.gm, f"{name} {kind} uniform sample_states n={n}")
        if name.startswith("origin_utm"):
            print(f"{name} uniform: x, y bit-equal to the oracle: {bit_equal(sg[:, :2], so[:, :2])}")
        for m in SIZES + [n]:
            entry_points(ctx, p.seed, p.first, m, sg[:m], validity)
    finally:
        ctx.close()


# ---- shape changes on one context ------------------------------------------------------------------------------------------------
def test_shape_changes_on_one_context():
    """The widest map, then a narrower one, then a taller one on ONE context (ensure_sampler_storage keeps or replaces its
    buffers by shape; the pivots behind npiv hold +inf only if the pack kernel wrote them), then the widest again:
    bit-equal to fresh contexts, and to the oracle's bar."""
    names = ["cross_cols_gt_512", "cross_cols_le_512", "cross_rows_gt_2048", "cross_cols_gt_512", "cross_tie_cols_501"]
    n = 1 << 16
    one = _ctx("yaml")
    try:
        for name in names:
            p = SP.probe(name)
            install(one, p.gm, validity=True)
            got = one.sample_states(p.seed, p.first, n)
            fresh = _ctx("yaml")
            try:
                install(fresh, p.gm, validity=True)
                want = fresh.sample_states(p.seed, p.first, n)
            finally:
                fresh.close()
            so, rc = SP.oracle_samples(p, "yaml", n=n)
            assert_states(got, so, rc, p.gm, f"{name} after a shape change")
            assert bit_equal(got, want), name
    finally:
        one.close()


# ---- part 2: the bitmap kernels against numpy -------------------------------------------------------------------------------------
TILE_BITS = 1024 * 64
PATTERNS = ["zero", "one", "first", "last", "per_tile", "gap", "d1e-4", "d0.3", "d0.999"]


def pattern(name, n, rng):
    """n bits (uint8 0 / 1)."""
    b = np.zeros(n, np.uint8)
    if name == "one":
        b[:] = 1
    elif name == "first":
        b[0] = 1
    elif name == "last":
        b[n - 1] = 1
    elif name == "per_tile":
        for t0 in range(0, n, TILE_BITS):
            b[t0 + rng.integers(0, min(TILE_BITS, n - t0))] = 1
    elif name == "gap":
        # tiles 3 to 40 empty (38 912 empty words between set bits); on a bitmap of fewer tiles, all but 3 words at either end
        b[:] = rng.random(n) < 0.05
        if n > 41 * TILE_BITS:
            b[3 * TILE_BITS:41 * TILE_BITS] = 0
        else:
            b[min(192, n // 3):max(n - 192, n // 3)] = 0
    elif name.startswith("d"):
        b[:] = rng.random(n) < float(name[1:])
    return b


def pack_words(b, extra_words=2):
    """Little-endian 64-bit words of the bits; the bits behind them in the last word, and extra_words more, are SET: a
    kernel must mask them."""
    n = len(b)
    words = (n + 63) // 64
    full = np.ones((words + extra_words) * 64, np.uint8)
    full[:n] = b
    return np.packbits(full, bitorder="little").view(np.int64)


@pytest.fixture(scope="module")
def bit_ctx():
    p = SP.probe("cross_cols_le_512")
    ctx = _ctx("yaml")
    install(ctx, p.gm, validity=True)
    ctx.use_torch_stream()
    yield ctx
    ctx.close()


def ref_at(ctx, seed, base, idx, torch):
    """sample_states_at_dev at base + idx (device tensor)."""
    k = len(idx)
    out = torch.empty((k, 7), dtype=torch.float64, device="cuda")
    if k:
        idx_t = torch.from_numpy(idx.astype(np.uint32).view(np.int32)).cuda()
        cnt = torch.tensor([k], dtype=torch.int64, device="cuda")
        ctx.sample_states_at_dev(seed, base, idx_t, cnt, k, out)
    return out


def ref_batch(ctx, seed, base, idx, n, torch, chunk=1 << 20):
    """The rows idx of the batch sample_states(seed, base, n), made chunk by chunk on the device (a 2^22 batch is 235 MB)."""
    out = torch.empty((len(idx), 7), dtype=torch.float64, device="cuda")
    buf = torch.empty((min(chunk, n), 7), dtype=torch.float64, device="cuda")
    for a in range(0, n, chunk):
        m = min(chunk, n - a)
        sel = np.flatnonzero((idx >= a) & (idx < a + m))
        if len(sel):
            ctx.sample_states_dev(seed, (base + a) % (1 << 64), m, buf)
            out[torch.from_numpy(sel).cuda()] = buf[torch.from_numpy(idx[sel] - a).cuda()]
    return out


def same_bits(a, b, torch):
    return a.shape == b.shape and bool(torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64)))


def materialise_case(ctx, seed, bits, bases, prefix, cap, batch_ref=False):
    """One call for all ranks; bits = per-rank uint8 arrays of one length."""
    import torch
    ranks, n = len(bits), len(bits[0])
    g = torch.from_numpy(np.stack([pack_words(b) for b in bits])).cuda()
    out = torch.full((ranks, cap, 7), float("nan"), dtype=torch.float64, device="cuda")
    counts = torch.full((ranks,), -7, dtype=torch.int64, device="cuda")
    ctx.materialise_from_bits_dev(seed, g, prefix, bases, cap, out, counts)
    torch.cuda.synchronize()
    c = counts.cpu().numpy()
    for r in range(ranks):
        acc = np.flatnonzero(bits[r][:prefix])
        what = (f"n={n} ranks={ranks} rank={r} prefix={prefix} cap={cap}", len(acc))
        assert c[r] == len(acc), what                                   # numpy's popcount of the prefix
        k = min(len(acc), cap)
        assert same_bits(out[r, :k], ref_at(ctx, seed, bases[r], acc[:k], torch), torch), what
        if batch_ref:
            assert same_bits(out[r, :k], ref_batch(ctx, seed, bases[r], acc[:k], n, torch), torch), what
        assert bool(torch.isnan(out[r, k:]).all()), what                # rows past k untouched
    return c


def prefixes_and_caps(n, count_of):
    """(prefix, cap) pairs: prefix = n with cap in {1, count - 1, count, count + 1, prefix}; and prefixes that end at 1,
    inside a word, on a word edge and on a tile edge, each with cap = prefix (capped where stated by the caller)."""
    cnt = count_of(n)
    pairs = [(n, c) for c in sorted({1, max(cnt - 1, 1), max(cnt, 1), cnt + 1, n})]
    for pre in (1, n - 27 if n % 64 == 0 else n - (n % 64) - 27, (n // 64) * 64, TILE_BITS, 2 * TILE_BITS, 64):
        if 1 <= pre <= n and pre not in [q for q, _ in pairs]:
            pairs.append((pre, pre))
    return pairs


BASES = [5_000_000, (1 << 32) + 11, (1 << 40) + 3, (1 << 32) - 1000, (1 << 61) - 17, (1 << 63) + 5, 0, 77]


@pytest.mark.parametrize("n", [100, TILE_BITS - 1, TILE_BITS, TILE_BITS + 1])
def test_materialise_three_ranks_every_pattern(bit_ctx, n):
    """3 ranks, every pattern (each rank its own draw of it), every prefix and capacity; the reference is
    sample_states_at_dev AND the sample_states batch at base[r] + flatnonzero(bits)[:k].  Bases above 2^32."""
    seed = 7
    rng = np.random.default_rng(n)
    for name in PATTERNS:
        bits = [pattern(name, n, rng) for _ in range(3)]
        bases = BASES[1:4]
        for prefix, cap in prefixes_and_caps(n, lambda m: int(bits[1][:m].sum())):
            materialise_case(bit_ctx, seed, bits, bases, prefix, cap, batch_ref=True)
    mixed = [pattern(name, n, rng) for name in ("d0.3", "last", "gap")]     # a different pattern per rank in one call
    for prefix, cap in prefixes_and_caps(n, lambda m: int(mixed[0][:m].sum())):
        materialise_case(bit_ctx, seed, mixed, BASES[3:6], prefix, cap, batch_ref=True)


CAP_MANY = 1 << 18     # many-rank cases: out is ranks x cap x 56 bytes (16 ranks at cap = 2^22 would be 3.8 GB)


@pytest.mark.parametrize("n,ranks", [(1 << 22, 1), (1 << 22, 2), (1 << 22, 8), (1 << 22, 16), ((1 << 22) + 1, 3)])
def test_materialise_64_tiles(bit_ctx, n, ranks):
    """Production size: 2^22 candidates per rank are 64 tiles of 1024 words (one more bit: 65 tiles).  Rank r takes
    pattern (r + shift) of the list, so every pattern meets the walk over tile totals; capacities stay at or below 2^18
    for the many-rank calls, except the single-rank call that accepts everything (cap = prefix = 2^22: 235 MB)."""
    seed = 7
    rng = np.random.default_rng(ranks)
    shifts = range(len(PATTERNS)) if ranks == 1 else (0, 4)
    for shift in shifts:
        names = [PATTERNS[(r + shift) % len(PATTERNS)] for r in range(ranks)]
        bits = [pattern(nm, n, rng) for nm in names]
        bases = [BASES[r % len(BASES)] + 1_000_003 * r for r in range(ranks)]
        cnt = int(bits[0].sum())
        pairs = [(n, CAP_MANY), (n, min(max(cnt - 1, 1), CAP_MANY)), (n, min(cnt + 1, CAP_MANY)), (n, 1),
                 (n - 27, CAP_MANY), (41 * TILE_BITS, CAP_MANY), (40 * TILE_BITS + 64, 4096), (1, 8)]
        for k, (prefix, cap) in enumerate(dict.fromkeys(pairs)):
            materialise_case(bit_ctx, seed, bits, bases, prefix, cap, batch_ref=(k == 0))
    if ranks == 1:
        materialise_case(bit_ctx, seed, [pattern("one", n, rng)], [BASES[1]], n, n, batch_ref=True)
        materialise_case(bit_ctx, seed, [pattern("d0.999", n, rng)], [BASES[4]], n - 27, n, batch_ref=False)


@pytest.mark.parametrize("n", [100, TILE_BITS - 1, TILE_BITS, TILE_BITS + 1, (1 << 22) + 1])
def test_pack_and_indices_every_pattern(bit_ctx, n):
    """pack_valid_bits_dev: bit i = (valid[i] != 0) -- ANY non-zero byte (1, 2, 255) is "valid", as for the consumers of
    validate_states -- bits behind n in the last word are 0, nothing is written behind the last word; n % 64 covers
    0, 1, 63.  indices_from_bits_dev gives numpy's flatnonzero of the first n (and of a prefix's) bits."""
    import torch
    assert {m % 64 for m in (TILE_BITS - 1, TILE_BITS, TILE_BITS + 1)} == {63, 0, 1}
    rng = np.random.default_rng(n + 1)
    words = (n + 63) // 64
    for name in PATTERNS:
        b = pattern(name, n, rng)
        valid = (b * rng.choice(np.array([1, 2, 255], np.uint8), n)).astype(np.uint8)
        v_t = torch.from_numpy(valid).cuda()
        bits_t = torch.full((words + 1,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
        bit_ctx.pack_valid_bits_dev(v_t, bits_t)
        torch.cuda.synchronize()
        got = bits_t.cpu().numpy()
        assert got[words] == 0x5A5A5A5A5A5A5A5A, (name, n)
        padded = np.zeros(words * 64, np.uint8)
        padded[:n] = b
        assert np.array_equal(got[:words], np.packbits(padded, bitorder="little").view(np.int64)), (name, n)
        ref = np.flatnonzero(b)
        for m in sorted({n, n - 27, (n // 64) * 64, 1}):
            if m < 1:
                continue
            want = ref[ref < m]
            idx = torch.full((max(len(want), 1) + 1,), -1, dtype=torch.int32, device="cuda")
            cnt = torch.full((1,), -1, dtype=torch.int64, device="cuda")
            bit_ctx.indices_from_bits_dev(bits_t, m, idx, cnt)
            torch.cuda.synchronize()
            assert int(cnt.item()) == len(want), (name, n, m)
            h = idx.cpu().numpy()
            assert np.array_equal(h[:len(want)], want.astype(np.int32)) and h[-1] == -1, (name, n, m)


def test_materialise_argument_errors(bit_ctx):
    import torch
    from art_planner_amd._capi import ArtpError
    g = torch.zeros((17, 4), dtype=torch.int64, device="cuda")
    out = torch.zeros((17, 8, 7), dtype=torch.float64, device="cuda")
    counts = torch.zeros(17, dtype=torch.int64, device="cuda")
    with pytest.raises(ArtpError) as e:
        bit_ctx.materialise_from_bits_dev(7, g, 64, list(range(17)), 8, out, counts)             # 17 ranks
    assert e.value.status == ARTP_ERR_INVALID_ARG
    with pytest.raises(ArtpError) as e:
        bit_ctx.materialise_from_bits_dev(7, g[:3], 4 * 64 + 1, [0, 1, 2], 8, out, counts)       # prefix > words * 64
    assert e.value.status == ARTP_ERR_INVALID_ARG
    base = np.zeros(3, np.uint64)
    # prefix_bits >= 2^32 is refused before anything is read (words_per_rank only CLAIMS room for it)
    rc = bit_ctx.L.artp_materialise_from_bits_dev(bit_ctx.h, 7, g.data_ptr(), 3, 1 << 27, 1 << 32, base.ctypes.data, 8,
                                                  out.data_ptr(), counts.data_ptr())
    assert rc == ARTP_ERR_INVALID_ARG
    bit_ctx.materialise_from_bits_dev(7, g[:3], 4 * 64, [0, 1, 2], 8, out, counts)               # the context stays usable
    torch.cuda.synchronize()
    assert counts[:3].cpu().numpy().tolist() == [0, 0, 0]
