"""The convolution kernels' dispatch classes, and inputs and float64 references for tests/test_conv_forms_gpu.py: every class that
conv_pick_config (csrc/conv_igemm.hip) can give a layer, launched the way the trunk launches it -- input, residual and output as
channel slices of wider buffers.

A class is (dtype, ksize, stride, form, cout tile bn, K chunk kc). CASES has at least one row per class; a row's cin is the smallest
that reaches the class with more than one K chunk (so that the chunk loop and the chunk stride of the packed weights take part; the
fp16 3x3 kernel with 32-channel chunks starts at cin = 160), and its cout is 48 for a 32-cout tile (one whole tile and a half-empty
last one) and 128 for a 64-cout tile (two tiles: the tile index takes part in the weight, bias and output addresses). A row whose
class the default dispatch gives to another kernel at that shape names the switch that reaches it.

As in tests/front_cases.py every reference works on the values the kernel's number format holds."""
from collections import namedtuple
from functools import lru_cache

import numpy as np

from front_cases import conv64, pairs

F16, F32, F32S = 0, 1, 2
DTYPE_CODE = {"f16": F16, "f32": F32, "split": F32S}

Row = namedtuple("Row", "dtype ks stride cin cout form bn kc switch", defaults=(None,))

CASES = [
    # fp16, the register-staged kernel: 1x1 with 64-, 32- and 16-channel chunks (cin % 64, % 32, % 16), 3x3 with 16 (cin <= 128) and 32
    Row("f16", 1, 1, 128, 128, "Staged", 64, 64), Row("f16", 1, 1, 128, 48, "Staged", 32, 64),
    Row("f16", 1, 1, 96, 128, "Staged", 64, 32), Row("f16", 1, 1, 96, 48, "Staged", 32, 32),
    Row("f16", 1, 1, 48, 128, "Staged", 64, 16), Row("f16", 1, 1, 48, 48, "Staged", 32, 16),
    Row("f16", 3, 1, 32, 128, "Staged", 64, 16), Row("f16", 3, 1, 32, 48, "Staged", 32, 16),
    Row("f16", 3, 1, 160, 128, "Staged", 64, 32), Row("f16", 3, 1, 160, 48, "Staged", 32, 32),
    Row("f16", 3, 2, 32, 128, "Staged", 64, 16), Row("f16", 3, 2, 32, 48, "Staged", 32, 16),
    Row("f16", 3, 2, 160, 128, "Staged", 64, 32), Row("f16", 3, 2, 160, 48, "Staged", 32, 32),
    # exact fp32, the same kernel: 1x1 with 32- and 16-channel chunks, 3x3 always 16
    Row("f32", 1, 1, 64, 128, "Staged", 64, 32), Row("f32", 1, 1, 64, 48, "Staged", 32, 32),
    Row("f32", 1, 1, 48, 128, "Staged", 64, 16), Row("f32", 1, 1, 48, 48, "Staged", 32, 16),
    Row("f32", 3, 1, 32, 128, "Staged", 64, 16), Row("f32", 3, 1, 32, 48, "Staged", 32, 16),
    Row("f32", 3, 2, 32, 128, "Staged", 64, 16), Row("f32", 3, 2, 32, 48, "Staged", 32, 16),
    # split-f16x3: the 32x32x16 kernel (1x1 with 32- and 16-channel chunks; 3x3 with 16), the 16x16x32 forms (64-cout tiles, cin % 32 == 0)
    Row("split", 1, 1, 64, 128, "Split", 64, 32), Row("split", 1, 1, 64, 48, "Split", 32, 32),
    Row("split", 1, 1, 48, 128, "Split", 64, 16), Row("split", 1, 1, 48, 48, "Split", 32, 16),
    Row("split", 3, 1, 32, 48, "Split", 32, 16), Row("split", 3, 1, 48, 128, "Split", 64, 16),
    Row("split", 3, 1, 64, 128, "Split", 64, 16, ("GTX_K32", "0")), Row("split", 3, 1, 64, 128, "K32", 64, 32),
    Row("split", 3, 2, 32, 48, "Split", 32, 16), Row("split", 3, 2, 48, 128, "Split", 64, 16),
    Row("split", 3, 2, 64, 128, "Split", 64, 16, ("GTX_K32S2", "0")), Row("split", 3, 2, 64, 128, "K32S2", 64, 32),
]
SWITCHES = ("GTX_K32", "GTX_K32S2")


def row_id(r):
    return f"{r.dtype}-{r.ks}x{r.ks}s{r.stride}-{r.cin}to{r.cout}-{r.form}-bn{r.bn}-kc{r.kc}" + (f"-{r.switch[0]}={r.switch[1]}" if r.switch else "")


def klass(r):
    return (r.dtype, r.ks, r.stride, r.form, r.bn, r.kc)


# ---------------------------------------------------------------------------------------------------- geometry
# Output maps of 9 x 17: two 8 x 16 tiles each way, the second one row and one column wide; batch 2. A stride-2 row gets there from
# 17 x 33 and from 18 x 34 (the even size, whose last window hangs over the border on one side only). "tile": one exact 8 x 16 tile.
N = 2
PAD_C = 16                        # channels of the wider buffer on each side of a slice (in_coff = out_coff = 16)
NARROW_C = 4                      # fp16, "tile": the output slice starts 4 channels in, which takes the kernel's 8-byte store path
SENTINEL = np.float32(-777.123)   # not an fp16 value, and with a lo half in the pair format
GARBAGE = np.float32(7.0)         # the input buffer's channels outside the slice


def geometries(stride):
    """name -> input (h, w)"""
    if stride == 1:
        return {"9x17": (9, 17), "tile": (8, 16)}
    return {"9x17odd": (17, 33), "9x17even": (18, 34), "tile": (16, 32)}


def out_hw(r, hw):
    pad = r.ks // 2
    return (hw[0] + 2 * pad - r.ks) // r.stride + 1, (hw[1] + 2 * pad - r.ks) // r.stride + 1


def np_dtype(r):
    return np.float16 if r.dtype == "f16" else np.float32


def held(r, a):
    """float64: what a buffer of row r's format holds of the array a (given in the buffer's numpy dtype)."""
    return pairs(a) if r.dtype == "split" else np.asarray(a).astype(np.float64)


def embed(r, vals, coff, cstride, fill):
    """vals [n, h, w, c] as channels [coff, coff + c) of a [n, h, w, cstride] buffer of row r's numpy dtype, `fill` elsewhere."""
    n, h, w, c = vals.shape
    buf = np.full((n, h, w, cstride), fill, np_dtype(r))
    buf[..., coff:coff + c] = vals
    return buf


# ---------------------------------------------------------------------------------------------------- exact data
KINDS = {"f16": (1,), "f32": (1,), "split": (1, 2, 3)}
FRAC = 2.0 ** -12


def _ints(rng, lim, shape):
    return rng.integers(-lim, lim + 1, shape).astype(np.float64)


@lru_cache(maxsize=None)
def exact_case(i, kind, geo):
    """Row CASES[i] on data whose every product and partial sum is exact in the kernel's formats. kind 1: small integers in
    activations and weights. kind 2: activations a + b 2^-12 (the split's lo halves are non-zero), integer weights: the cross
    product lo(x) hi(w) carries real bits. kind 3: integer activations, weights c + d 2^-12: hi(x) lo(w) does. No lo lo term
    exists in either. The ranges are narrower for K > 512. Returns x, w, bias, res (the residual slice, same kind of values
    as the activations) and the two float64 references, without and with the residual; exactness is asserted on the way."""
    r = CASES[i]
    rng = np.random.default_rng(1000 * i + 10 * kind + len(geo))
    h, w = geometries(r.stride)[geo]
    ho, wo = out_hw(r, (h, w))
    K = r.ks * r.ks * r.cin
    lx, lw = (3, 2) if K <= 512 else (2, 1)
    x = _ints(rng, lx, (N, h, w, r.cin))
    wt = _ints(rng, lw, (r.cout, r.ks, r.ks, r.cin))
    res = _ints(rng, lx, (N, ho, wo, r.cout))
    if kind == 2:
        x += _ints(rng, 3, x.shape) * FRAC
        res += _ints(rng, 3, res.shape) * FRAC
    if kind == 3:
        wt += _ints(rng, 3, wt.shape) * FRAC
    b = _ints(rng, 4, r.cout)
    ref = conv64(x, wt, b, stride=r.stride, act=0)
    ref_res = ref + res
    assert_exact(r, kind, x, wt, b, res, ref, ref_res)
    return x, wt.astype(np.float32), b.astype(np.float32), res, ref, ref_res


def split_weight_scale(wt):
    """The power of two pack_conv_weights_split scales a layer's weights by: max |w| lands in [2^13, 2^14)."""
    return 2.0 ** (14 - np.frexp(np.abs(wt).max())[1])


def assert_exact(r, kind, x, wt, b, res, ref, ref_res):
    """The reference side's own exactness: inputs and outputs are values of the format, and the sum of the magnitudes -- which bounds
    every partial sum in every order -- has no more than 24 bits above the data's unit."""
    unit = FRAC if kind > 1 else 1.0
    mag = conv64(np.abs(x), np.abs(wt), np.abs(b), stride=r.stride, act=0) + np.abs(res)
    assert mag.max() / unit < 2.0 ** 24
    for a in (x, wt, b, res, ref, ref_res):
        assert np.array_equal(a, np.round(a / unit) * unit)
    if r.dtype == "split":
        for a in (x, res, ref, ref_res, wt * split_weight_scale(wt)):
            assert np.array_equal(pairs(a), a)
    elif r.dtype == "f16":
        for a in (x, wt, res, ref, ref_res):
            assert np.abs(a).max() < 2048 and np.array_equal(a.astype(np.float16).astype(np.float64), a)
    else:
        for a in (x, wt, res, ref, ref_res):
            assert np.array_equal(a.astype(np.float32).astype(np.float64), a)


# ---------------------------------------------------------------------------------------------------- tap and channel map
TAP_G, TAP_M = 64, 3      # channel ids and coarse positions an input value tells apart: 1 + 8 + 9 * 63 + 576 * 2 = 1728 < 2048


def tap_select(r, rnd):
    """Launch `rnd` of the one-hot weights: output channel o reads tap j % ks^2 of input channel chunk * kc + j % kc, j = rnd * cout + o.
    Over tap_rounds(r) launches j runs through max(ks^2, kc) values or more, so every tap and every position inside a K chunk is
    read, from varying chunks."""
    taps, nch = r.ks * r.ks, r.cin // r.kc
    sel = []
    for o in range(r.cout):
        j = rnd * r.cout + o
        sel.append((j % taps, ((j // r.kc + 2 * o + rnd) % nch) * r.kc + j % r.kc))
    return sel


def tap_rounds(r):
    return -(-max(r.ks * r.ks, r.kc) // r.cout)


def tap_weights(r, sel):
    wt = np.zeros((r.cout, r.ks, r.ks, r.cin), np.float32)
    for o, (tap, c) in enumerate(sel):
        wt[o, tap // r.ks, tap % r.ks, c] = 1.0
    return wt


def tap_input(r, hw):
    """[2, h, w, cin] integers, exact in fp16: under any 3 x 3 window the nine values of a channel differ (y % 3, x % 3), windows
    three pixels apart differ (the coarse term), and the channel is told by c % 64 in image 0 and by (c + c // 64) % 64 in image 1,
    which is negated. No value is 0: that is what the padding reads as."""
    h, w = hw
    yy, xx = np.mgrid[0:h, 0:w]
    pos = ((yy % 3) * 3 + xx % 3)[..., None] + 9 * TAP_G * ((yy // 3 + xx // 3) % TAP_M)[..., None]
    c = np.arange(r.cin)
    x = np.stack([1 + pos + 9 * (c % TAP_G), -(1 + pos + 9 * ((c + c // TAP_G) % TAP_G))]).astype(np.float64)
    assert np.abs(x).max() < 2048 and np.abs(x).min() >= 1
    return x


def tap_reference(r, x, sel):
    """The selected neighbour (0 beyond the border), by indexing: no convolution involved."""
    n, h, w, _ = x.shape
    ho, wo = out_hw(r, (h, w))
    pad, s = r.ks // 2, r.stride
    padded = np.zeros((n, s * ho + r.ks, s * wo + r.ks, x.shape[3]))
    padded[:, pad:pad + h, pad:pad + w] = x
    out = np.zeros((n, ho, wo, len(sel)))
    for o, (tap, c) in enumerate(sel):
        ky, kx = divmod(tap, r.ks)
        out[..., o] = padded[:, ky:ky + s * ho:s, kx:kx + s * wo:s, c]      # padded row s oy + ky = input row s oy - pad + ky
    return out


# ---------------------------------------------------------------------------------------------------- values
# The output format's own rounding, (relative, absolute), as tests/test_yolov10_gpu.py's test_depthwise_kernels states it: the
# absolute part is the spacing fp16 keeps below its smallest normal value (2^-24; half of it for a value rounded once).
STORE = {"f16": (2.0 ** -11, 2.0 ** -25), "split": (2.0 ** -21, 2.0 ** -24), "f32": (2.0 ** -24, 0.0)}
SPLIT_F = 3 * 2.0 ** -22          # two weight-split roundings and the dropped lo x lo product, per product


@lru_cache(maxsize=None)
def value_case(i):
    """Row CASES[i] on wide-range data (test_conv2d_split_f16x3_meets_the_fp32_bar's: activations over five decades, one large tap
    that sets the layer's power-of-two scale), on the first geometry. Returns x and w as the kernel's format stores them (fp16 rounds
    both; the split path takes x as hi + lo and the fp32 weights as given), the bias, the float64 pre-activation sum and the sum of
    magnitudes S = conv(|x|, |w|) + |bias|."""
    r = CASES[i]
    rng = np.random.default_rng(5000 + i)
    h, w = next(iter(geometries(r.stride).values()))
    K = r.ks * r.ks * r.cin
    x = (rng.standard_normal((N, h, w, r.cin)) * 10.0 ** rng.uniform(-4, 1, (N, h, w, r.cin))).astype(np.float32)
    wt = (rng.standard_normal((r.cout, r.ks, r.ks, r.cin)) / np.sqrt(K)).astype(np.float32)
    wt[rng.integers(0, r.cout), :, :, rng.integers(0, r.cin)] *= 60.0
    b = (rng.standard_normal(r.cout) * 0.1).astype(np.float32)
    if r.dtype == "f16":
        x, wt = x.astype(np.float16), wt.astype(np.float16).astype(np.float32)
    xs = held(r, x)
    pre = conv64(xs, wt, b, stride=r.stride, act=0)
    mag = conv64(np.abs(xs), np.abs(wt), np.abs(b), stride=r.stride, act=0)
    return x, wt, b, pre, mag


def activate(pre, act):
    """ConvProblem::act: 0 identity, 1 SiLU, 2 ReLU"""
    return pre / (1.0 + np.exp(-pre)) if act == 1 else np.maximum(pre, 0.0) if act == 2 else pre


def value_bound(r, ref, mag, act):
    """Per element: B = (K + 4) 2^-24 S + f S + store (+ 8 2^-24 |y| under an activation). K + 4 fp32 roundings of sums that never
    exceed S (the products, the bias, the scale, the conversions); f = 3 2^-22 on the split path, 0 where the reference uses the
    operands as stored; the output format's own rounding of |ref|; v_exp_f32, v_rcp_f32 and two multiplications for the activation."""
    K = r.ks * r.ks * r.cin
    rel, absolute = STORE[r.dtype]
    B = (K + 4) * 2.0 ** -24 * mag + (SPLIT_F if r.dtype == "split" else 0.0) * mag + rel * np.abs(ref) + absolute
    return B + (8 * 2.0 ** -24 * np.abs(ref) if act else 0.0)
