"""CPU self-tests of the exact-arithmetic reference (tests/cost_exact_ref.py) that tests/test_cost_sweep.py holds the
device's motion-cost features to, bit for bit."""
import os
import sys

import numpy as np
import pytest

import common

sys.path.insert(0, os.path.join(common.ROOT, "oracle"))
sys.path.insert(0, os.path.join(common.ROOT, "tools"))
import convert_weights as cw  # noqa: E402
import cost_exact_ref as R  # noqa: E402
import motion_cost_oracle as mo  # noqa: E402

NETS = (1, 2)
# every probe with both branches must hit each of them in every layer at least this often (the reference asserts it)
MIN_BRANCH_RATE = 0.10


@pytest.mark.parametrize("net", NETS)
@pytest.mark.parametrize("kind", ["positive", "mixed"])
def test_fold_returns_exactly_the_probe_integers(net, kind):
    """gamma 1, mean 0 and UNIT_VAR: convert_weights.fold hands the device exactly the intended integer weights and biases
    (and the blob carries them), and motion_cost_oracle's own BatchNorm scale is exactly 1."""
    p = R.probe_params(net, kind)
    blob = np.frombuffer(cw.to_blob(p)[8:], "<f4")
    off = 0
    for name in R.CONVS:
        w, b = R.intended_weights(p, name)
        fw, fb = cw.fold(p, name)
        assert np.array_equal(fw.astype(np.float64), w) and np.array_equal(fb.astype(np.float64), b), name
        assert np.array_equal(w, np.round(w)), name
        assert np.array_equal(blob[off:off + w.size], w.ravel()) and np.array_equal(blob[off + w.size:off + w.size + b.size], b)
        off += w.size + b.size
        var = p[name + "_bn.running_var"]
        assert (np.float32(1) / np.sqrt(var + np.float32(1e-5)) == np.float32(1)).all(), name


@pytest.mark.parametrize("net", NETS)
def test_probes_reach_every_tap_and_every_input_channel(net):
    """Across the probe sets every (kh, kw) tap and every input channel of every conv layer carries a non-zero weight, and
    the 15 x 15 layer has non-zero weights at both ends of every kernel row's K run (kw 0 / cin 0, kw 14 / cin C - 1)."""
    ps = [R.probe_params(net, k) for k in ("positive", "mixed")]
    for name in R.CONVS:
        for p in ps:
            w = p[name + ".weight"]
            assert (np.abs(w).sum(axis=(0, 1)) > 0).all(), (name, "a tap without a weight")
            assert (np.abs(w).sum(axis=(0, 2, 3)) > 0).all(), (name, "an input channel without a weight")
            assert (np.abs(w).sum(axis=(1, 2, 3)) > 0).all(), (name, "an output channel without a weight")
    for p in ps:
        w = p["init_flatten.weight"]
        assert (w[:, 0, :, 0] != 0).any(axis=0).all() and (w[:, -1, :, -1] != 0).any(axis=0).all()


@pytest.mark.parametrize("net", NETS)
@pytest.mark.parametrize("mk", ["dense", "impulse"])
def test_restatement_equals_the_oracle_bit_for_bit_when_nothing_rounds(net, mk):
    """The 'positive' probe has no negative pre-activation and no value that rounds: the restatement (fp16 rounding
    points, float64) and motion_cost_oracle (float32, no rounding) must be the same numbers, non-square map included."""
    p = R.probe_params(net, "positive")
    m = R.probe_map(mk, 131, 118)
    st = {}
    f = R.restate(p, m, stats=st)
    assert all(v["neg"] == 0 for v in st.values()), st
    ref = mo.cnn_features(p, m)
    assert f.shape == ref.shape == ((64 if net == 2 else 48),) + R.feature_shape(131, 118)
    assert np.array_equal(f, ref.astype(np.float64))
    assert np.abs(f).max() <= 2048 and f.max() > 8


@pytest.mark.parametrize("net", NETS)
def test_restatement_without_rounding_agrees_with_the_oracle_on_random_params(net):
    """On the seeded random parameters (dense, real-valued) the same chain without the fp16 rounding points agrees with
    motion_cost_oracle to float32 accuracy: the layer order, the composition of conv1 o conv2, the pools and the fold."""
    p = mo.random_params(0, R.shapes_of(net))
    g = np.load(os.path.join(common.GOLDEN_DIR, "motion_cost_120.npz"))
    m = g["crop"].astype(np.float32)[:, :113]
    f = R.restate(p, m, round_half=False)
    ref = mo.cnn_features(p, m)
    assert f.shape == ref.shape
    assert np.abs(f - ref).max() <= 4e-6 * np.abs(ref).max() + 1e-6, float(np.abs(f - ref).max())
    # and it is not the rounded chain: the rounding points move these values
    with pytest.raises(ValueError):
        R.restate(p, m)


@pytest.mark.parametrize("net", NETS)
@pytest.mark.parametrize("mk", ["impulse", "signed", "dense"])
def test_mixed_probes_hit_both_branches_and_keep_their_quantum(net, mk):
    """The 'mixed' probe drives every layer through both branches of the leaky ReLU at MIN_BRANCH_RATE or more, and its
    quantum only halves per layer (pre-activations are multiples of 5 q: 0.3 y is a multiple of q / 2)."""
    p = R.probe_params(net, "mixed")
    st = {}
    f = R.restate(p, R.probe_map(mk, 140, 157), stats=st)
    for name, v in st.items():
        assert v["neg"] >= MIN_BRANCH_RATE and v["pos"] >= MIN_BRANCH_RATE, (name, v)
    assert [st[n]["q"] for n in ("conv12", "init_conv3", "init_conv4", "init_conv5", "init_flatten")] == [1, 0.5, 0.25, 0.125, 0.0625]
    assert (f < 0).any() and (f > 0).any() and np.isfinite(f).all()
    # values that round do occur (0.3 y of the 15 x 15 layer), and the result is an fp16 array
    assert np.array_equal(f.astype(np.float16).astype(np.float64), f)
    assert not np.array_equal(f, np.round(f * 16) / 16)


def test_oversized_probe_is_refused():
    """A probe that breaks a precondition raises instead of returning a number: sums past 2^24 q, an fp16 overflow, a
    non-integer weight, a subnormal input."""
    p = R.probe_params(1, "mixed")
    m = R.probe_map("signed", 80, 80)
    big = dict(p)
    big["init_flatten.weight"] = p["init_flatten.weight"] * 2048       # sum |w| |x| past 2^24 q (q = 1 / 16)
    with pytest.raises(ValueError, match="2\\^24"):
        R.restate(big, m)
    huge = dict(p)
    huge["init_conv3.weight"] = p["init_conv3.weight"] * 400          # conv4's inputs above 65504
    with pytest.raises(ValueError):
        R.restate(huge, m)
    frac = dict(p)
    frac["init_conv5.weight"] = p["init_conv5.weight"] * np.float32(0.5)
    with pytest.raises(ValueError, match="integers"):
        R.restate(frac, m)
    with pytest.raises(ValueError, match="subnormal"):
        R.restate(p, m * np.float32(2.0 ** -20))
    R.restate(p, m)                                                    # the probe itself passes


def test_grid_is_the_binary_quantum():
    assert R.grid(np.array([3.0, 0.0, -6.0])) == 1.0
    assert R.grid(np.array([1.5, 0.75])) == 0.25
    assert R.grid(np.array([0.0])) == np.inf
    assert R.grid(np.array([2.0 ** -14 * 3, 4096.0])) == 2.0 ** -14
