"""Exact-arithmetic reference for the motion-cost feature extractor (test infrastructure).

The device chain (artp_cost_update_map*: conv345_kernel + conv_ksplit_kernel, cost_kernels.h) multiplies fp16 operands and
accumulates in fp32.  The product of two fp16 values is exact in fp32, and a sum of multiples of a quantum q is exact in any
order while every partial sum stays below 2^24 q.  So on PROBE parameters -- small integer weights, small integer maps --
the device's features are a fixed function of the input that a float64 restatement computes bit for bit, rounding only where
the kernels round:

  * the f32 map to half in conv345_kernel's F12 patch phase           (cost_kernels.h:650 `(half_t)v[it]`);
  * conv1 o conv2 as ONE composed 5 x 5 layer (artp_capi.hip, artp_cost_load_weights), no rounding between conv1 and conv2;
    its 2 x 2 max pool on the fp32 accumulators, then fmaxf(y, 0.3f * y) and RNE to half (cost_kernels.h:421-422);
  * conv3, conv4, conv5: fmaxf(y, 0.3f * y) in fp32, RNE to half (cost_kernels.h:559, store_region_lds);
  * the 3 / 1 max pool between conv4 and conv5 on halves (cost_kernels.h:752): exact;
  * the 15 x 15 layer: fmaxf(y, 0.3f * y), RNE to half (cost_kernels.h:275-276).

restate() raises ValueError instead of returning a number when a precondition of that argument fails (prove_layer): a
weight or bias that is not an integer (or not an fp16 integer), an input that is subnormal in fp16 or above 65504, or a
layer whose bound sum |w| |x| + |b| reaches 2^24 q, q the quantum of the layer's non-zero inputs (grid()).  With
round_half=False it is the plain float64 network (no precondition), which must agree with motion_cost_oracle to fp32
accuracy on any parameters.

probe_params() builds the probe networks.  Weights of conv2 .. conv5 are multiples of 5 and the biases multiples of 5 q:
every pre-activation is then a multiple of 5 q and its negative branch 0.3 y = 1.5 (y / 5) a multiple of q / 2 -- the
quantum halves per layer instead of collapsing (with +-1 weights a pre-activation of -q would leave 0.3 q rounded to
11 bits: q / 4096 after one layer).  The 15 x 15 layer, the last, takes +-1.
"""
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
for _p in (os.path.join(_ROOT, "oracle"), os.path.join(_ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import convert_weights as cw  # noqa: E402

CONVS = cw.CONVS
HALF_MAX = 65504.0
HALF_MIN_NORMAL = 2.0 ** -14
# BatchNorm with gamma 1, mean 0 and this running variance folds to a scale of exactly 1.0 in float32 (motion_cost_oracle's
# _bn) and to 1 + 7e-9 in float64 (convert_weights.fold), which float32 rounds back to 1 for every weight below 2^24
UNIT_VAR = np.float32(0.99999)
LRELU_SLOPE = np.float32(0.3)


def shapes_of(net):
    return cw.SHAPES if net == 1 else cw.SHAPES_FULL


# ---- probe parameter sets ------------------------------------------------------------------------------------------------
def _entries(shape, per_out, rng, corner_rows=False, corner=False):
    """Sparse weight positions (o, c, kh, kw) for a conv of `shape`: every (kh, kw) tap and every input channel appears,
    each output gets per_out of them.  corner: every output also reads its bottom-right tap, so that the last map row and
    column reach the last feature row and column through every layer.  corner_rows: also, for every kernel row kh, the first and the last element of the
    row's K run (kw = 0, c = 0 and kw = KW - 1, c = C - 1: the ends of the 15 x 15 layer's per-row packing)."""
    O, C, KH, KW = shape
    taps = KH * KW
    n = max(O * per_out, taps, C)
    ent = []
    for e in range(n):
        t = e % taps
        c = (5 * e) % C                          # 5 is prime to every channel count: all C appear
        ent.append((e % O, c, t // KW, t % KW))
    for o in range(O if corner else 0):   # a chain of bottom / right edges through all layers
        ent.append((o, (5 * o + 1) % C, KH - 1, KW - 1))
    if corner_rows:
        for kh in range(KH):
            ent.append(((3 * kh) % O, 0, kh, 0))
            ent.append(((3 * kh + 1) % O, C - 1, kh, KW - 1))
    out = {}
    for o, c, kh, kw in ent:
        out[(o, c, kh, kw)] = 1
    return sorted(out)


def probe_params(net, kind, seed=0):
    """A probe parameter set for network version `net` (1 light, 2 full width).  kind:
      'positive': weights in {0, 1}, biases >= 0 -- no negative pre-activation, no value ever rounds; every output also
                  reads its bottom-right tap (the map's last row and column reach the features: values up to ~900);
      'mixed':    conv1 +-1, conv2 .. conv5 +-5, the 15 x 15 layer +-1, per-channel biases of both signs -- both
                  branches of the leaky ReLU in every layer (branch_rates)."""
    shapes = shapes_of(net)
    p = cw.random_params(seed, shapes)          # the FC part stays random (the features do not depend on it)
    rng = np.random.default_rng(1000 + seed + 17 * net + (0 if kind == "positive" else 1))
    for li, name in enumerate(CONVS):
        shp = shapes[name]
        O = shp[0]
        w = np.zeros(shp, np.float32)
        last = name == "init_flatten"
        for (o, c, kh, kw) in _entries(shp, 5 if last else 1, rng, corner_rows=last, corner=kind == "positive"):
            if kind == "positive":
                w[o, c, kh, kw] = 1
            elif name == "init_conv1" or last:
                w[o, c, kh, kw] = rng.choice([-1, 1])
            else:
                w[o, c, kh, kw] = rng.choice([-5, 5])
        if kind == "positive":
            b = rng.integers(0, 3, O).astype(np.float32)
        elif name == "init_conv1":
            b = rng.integers(-2, 3, O).astype(np.float32)
        else:
            # both signs in every layer: half the channels lean positive, half negative (multiples of 5 q of the layer)
            q = 2.0 ** -max(li - 1, 0)
            sign = np.where(np.arange(O) % 2 == 0, 1, -1)
            mag = rng.integers(1, 4, O) * (1 if last else 5)
            b = (sign * mag * q).astype(np.float32)
        p[name + ".weight"] = w
        p[name + "_bn.weight"] = np.ones(O, np.float32)
        p[name + "_bn.bias"] = b
        p[name + "_bn.running_mean"] = np.zeros(O, np.float32)
        p[name + "_bn.running_var"] = np.full(O, UNIT_VAR, np.float32)
    return p


def probe_map(kind, H, W, seed=0):
    """Small-integer elevation maps: 'impulse' (zeros with isolated ones, ~1 in 40 cells), 'dense' (integers 0 .. 3),
    'signed' (integers -2 .. 2)."""
    rng = np.random.default_rng(seed * 7919 + H * 31 + W)
    if kind == "impulse":
        m = (rng.random((H, W)) < 0.025).astype(np.float32)
    elif kind == "dense":
        m = rng.integers(0, 4, (H, W)).astype(np.float32)
    else:
        m = rng.integers(-2, 3, (H, W)).astype(np.float32)
    return m


def intended_weights(p, name):
    """The conv layer's weights / bias as written into the probe (gamma 1, mean 0: the fold must return exactly these)."""
    return np.asarray(p[name + ".weight"], np.float64), np.asarray(p[name + "_bn.bias"], np.float64)


# ---- the float64 restatement ---------------------------------------------------------------------------------------------
def _conv64(x, w, b):
    """Un-padded cross-correlation in float64, x [C,H,W], w [O,C,kh,kw], b [O] -> [O,H-kh+1,W-kw+1].  Sparse weights go
    one non-zero at a time (the probes), dense ones through torch's CPU conv2d in float64."""
    O, C, KH, KW = w.shape
    H, W = x.shape[1] - KH + 1, x.shape[2] - KW + 1
    out = np.empty((O, H, W), np.float64)
    out[:] = b[:, None, None]
    nz = np.argwhere(w != 0)
    if len(nz) <= 4 * O * KH * KW:
        for o, c, dy, dx in nz:
            out[o] += w[o, c, dy, dx] * x[c, dy:dy + H, dx:dx + W]
    else:
        import torch
        out += torch.nn.functional.conv2d(torch.from_numpy(np.ascontiguousarray(x))[None],
                                          torch.from_numpy(np.ascontiguousarray(w, np.float64)))[0].numpy()
    return out


def _maxpool(x, k, s):
    H, W = (x.shape[1] - k) // s + 1, (x.shape[2] - k) // s + 1
    out = np.full((x.shape[0], H, W), -np.inf)
    for dy in range(k):
        for dx in range(k):
            out = np.maximum(out, x[:, dy:dy + s * (H - 1) + 1:s, dx:dx + s * (W - 1) + 1:s])
    return out


def _lrelu_half(y, what):
    """fmaxf(y, 0.3f * y) in float32, then RNE to half -- the store of every activation.  y must already be an fp32 value
    (prove_layer's bound guarantees it for the device's accumulator)."""
    y32 = y.astype(np.float32)
    if not np.array_equal(y32.astype(np.float64), y):
        raise ValueError(f"{what}: a pre-activation is not an fp32 value")
    with np.errstate(over="ignore"):                      # past 65504: inf, which the next layer's proof refuses
        return np.maximum(y32, LRELU_SLOPE * y32).astype(np.float16).astype(np.float64)


def _lrelu64(y):
    return np.where(y > 0, y, 0.3 * y)


def grid(v):
    """The quantum of the values v: the largest power of two that divides every non-zero element (at least the smallest
    fp16 ulp among them; 1 for any set of integers with an odd one)."""
    nz = np.asarray(v, np.float64)
    nz = nz[nz != 0]
    if nz.size == 0:
        return np.inf
    m, e = np.frexp(nz)
    mi = np.abs(m * 2.0 ** 53).astype(np.int64)
    low = np.log2((mi & -mi).astype(np.float64)).astype(np.int64)
    return float(2.0 ** (e.astype(np.int64) - 53 + low).min())


def prove_layer(x, w, b, what):
    """The preconditions of exact fp32 accumulation for one layer: integer fp16 weights, fp16-normal finite inputs, and
    sum |w| |x| + |b| < 2^24 q for every output, q the quantum of the non-zero inputs and the bias (grid(): every one is a
    multiple of q, so is every partial sum, and below 2^24 q each is an fp32 value).  Returns q; raises ValueError
    otherwise."""
    if not np.array_equal(w, np.round(w)) or np.abs(w).max() > 2048:
        raise ValueError(f"{what}: weights are not fp16 integers")
    nzx = x[x != 0]
    if nzx.size == 0:
        raise ValueError(f"{what}: all inputs are zero")
    if np.abs(nzx).min() < HALF_MIN_NORMAL or np.abs(nzx).max() > HALF_MAX or not np.isfinite(nzx).all():
        raise ValueError(f"{what}: an input is subnormal in fp16, above 65504 or not finite")
    if not np.array_equal(x.astype(np.float16).astype(np.float64), x):
        raise ValueError(f"{what}: an input is not an fp16 value")
    q = min(grid(nzx), grid(b))
    # sum_k |w_ok| |x_k| + |b_o| <= (sum_k |w_ok|) max |x| + |b_o|: the coarser bound, checked for every output channel o
    bound = (np.abs(w).reshape(w.shape[0], -1).sum(1) * np.abs(nzx).max() + np.abs(b)).max()
    if not bound < 2.0 ** 24 * q:
        raise ValueError(f"{what}: sum |w| |x| + |b| = {bound} reaches 2^24 q = {2.0 ** 24 * q}")
    return q


def folded(p):
    """The weights / biases the device is given (convert_weights.fold, float32), in float64."""
    return {n: tuple(np.asarray(a, np.float64) for a in cw.fold(p, n)) for n in CONVS}


def composed12(f):
    """conv1 o conv2 (no activation between): the 5 x 5 layer artp_cost_load_weights builds, in float64."""
    w1, b1 = f["init_conv1"]
    w2, b2 = f["init_conv2"]
    C1 = w1.shape[0]
    wc = np.zeros((C1, 1, 5, 5))
    for a in range(3):
        for bb in range(3):
            wc[:, 0, a:a + 3, bb:bb + 3] += np.einsum("oc,chw->ohw", w2[:, :, a, bb], w1[:, 0])
    bc = b2 + np.einsum("ocab,c->o", w2, b1)
    return wc, bc


def restate(p, elev, round_half=True, stats=None):
    """The device's feature chain on parameters p and the map elev [H, W]: features [C, F_h, F_w] in float64 (fp16 values
    when round_half).  stats (a dict) receives per layer the fraction of negative pre-activations ('neg') and of positive
    ones ('pos'), and the quantum q of its inputs."""
    f = folded(p)
    rec = stats if stats is not None else {}

    def note(name, y, q=None):
        n = y.size
        rec[name] = {"neg": float((y < 0).sum()) / n, "pos": float((y > 0).sum()) / n, "q": q}

    x = np.asarray(elev, np.float64)[None]
    if round_half:
        x = x.astype(np.float16).astype(np.float64)       # the map -> half (cost_kernels.h:650)
    wc, bc = composed12(f)
    q = prove_layer(x, wc, bc, "conv1 o conv2") if round_half else None
    y = _maxpool(_conv64(x, wc, bc), 2, 2)                # the pool on the fp32 accumulators (cost_kernels.h:411-418)
    note("conv12", y, q)
    x = _lrelu_half(y, "conv12") if round_half else _lrelu64(y)
    for name in ("init_conv3", "init_conv4", "init_conv5", "init_flatten"):
        w, b = f[name]
        q = prove_layer(x, w, b, name) if round_half else None
        y = _conv64(x, w, b)
        note(name, y, q)
        x = _lrelu_half(y, name) if round_half else _lrelu64(y)
        if name == "init_conv4":
            x = _maxpool(x, 3, 1)                         # on halves: exact (cost_kernels.h:752)
    if round_half and (np.abs(x).max() > HALF_MAX or ((x != 0) & (np.abs(x) < HALF_MIN_NORMAL)).any()):
        raise ValueError("init_flatten: an output is subnormal in fp16 or above 65504")
    return x


def feature_shape(H, W):
    """(F_h, F_w) of an H x W map (both networks: (H - 4) // 2 - 22 and the same for W)."""
    return (H - 4) // 2 - 22, (W - 4) // 2 - 22
