"""RT-DETR's map-side kernels (csrc/rtdetr_kernels.hip: rt_stem1, rt_pool2, rt_dwconv / rt_dwconv_tile, rt_upsample2x, rt_tokens_in,
rt_mask_invalid) one launcher at a time through gtx_op_rt_*, each against a reference written here in float64 (or, where the
operation is exact, by indexing), in the three activation formats: fp16, fp32 and the pair format (`split`: fp32 host arrays, hi + lo
fp16 pairs on the device). The whole-detector tests (test_rtdetr_gpu.py) stretch every frame to a square whose levels' sides are a
few multiples of 8, so they never run a non-square level, a map smaller than a tile or a halo, a pixel count that straddles a
256-thread block at a batch boundary, a channel slice with live data beside it, or an anchor exactly on the validity threshold.

Common devices. Every input map is wider than the slice that is read and holds 1e30 (inf in fp16, the clamp 65504 in the pair
format) beside the slice and in one whole extra image behind the last one that runs; every output map holds a sentinel of random
fp16 values (which every format carries exactly) beside its slice and in that extra image, and the sentinel must come back value
for value. Pair-format comparisons are on the values hi + lo, not on the two halves: splitting a tie again may pick the other pair.

Bars.
  stem1 values: error = max-abs over the float64 reference's max-abs; e_kernel < 8 * e_fp32ref + 1e-7 (test_rtdetr_ops_gpu.py's
  rule), e_fp32ref being the same recipe in float32 on the CPU stored in the output format. The float64 reference starts from the
  table the kernel holds: float32(b) / float32(255) correctly rounded, rounded again to fp16 for the fp16 format.
  dwconv: data on test_depthwise_kernels' binary grid, on which every partial sum is exact in fp32: without activation and with ReLU
  the result is the float32 loop's (ky outer, kx inner, one fused multiply-add per tap) bit for bit; with SiLU that test's tolerance.
  Everything else (tap map, ReLU zeros, pool2, upsample2x, tokens_in, mask_invalid) is exact.
Each test prints what it measured (pytest -s)."""
import functools
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F16, F32, F64 = np.float16, np.float32, np.float64
FMTS = ["f16", "f32", "split"]
POISON = 1e30


def _seed(*parts):
    return zlib.crc32(repr(parts).encode())


def _pairs(a):
    """What the pair format keeps of an fp32 array: hi + lo, as float64 (tests/test_conv_k32s2_gpu.py)."""
    hi = a.astype(np.float16).astype(np.float32)
    return hi.astype(np.float64) + (a - hi).astype(np.float16).astype(np.float64)


def _np(fmt):
    return F16 if fmt == "f16" else F32


def _held(a, fmt):
    """The values a format holds of float data, as a host array of that format (fp32 for the pair format: hi + lo is an fp32 number)."""
    if fmt == "f16":
        return np.asarray(a).astype(F16)
    a32 = np.asarray(a).astype(F32)
    return _pairs(a32).astype(F32) if fmt == "split" else a32


def _stored(a32, fmt):
    """A float32 result stored in an output format, as float64."""
    if fmt == "f16":
        return a32.astype(F16).astype(F64)
    return _pairs(a32) if fmt == "split" else a32.astype(F64)


def _in_map(vals, fmt, cs, coff):
    """vals [n, h, w, c] (host values of the format) at coff of an [n + 1, h, w, cs] map that is 1e30 everywhere else."""
    n, h, w, c = vals.shape
    with np.errstate(over="ignore"):
        buf = np.full((n + 1, h, w, cs), POISON, F64).astype(_np(fmt))
    buf[:n, ..., coff:coff + c] = vals
    return buf


def _out_map(rng, fmt, n, h, w, cs):
    """An [n + 1, h, w, cs] output map full of sentinel values every format carries exactly (nonzero fp16 values)."""
    s = rng.standard_normal((n + 1, h, w, cs)).astype(F16)
    s[s == 0] = F16(0.5)
    return s.astype(_np(fmt))


def _assert_outside_kept(got, before, n, coff, c):
    keep = np.ones(before.shape, bool)
    keep[:n, ..., coff:coff + c] = False
    assert got.shape == before.shape and got.dtype == before.dtype
    assert np.array_equal(got[keep], before[keep]), "the launch wrote outside its slice or its images"


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint16 if a.dtype == F16 else np.uint32)


# ============================================================================ stem1
STEM_SIZES = [(1, 2, 4), (3, 6, 10), (2, 34, 46)]          # (n, H, W); 34 x 46 -> 17 x 23 = 391 pixels per image: a 256-thread block ends
                                                           # inside image 0 and the next spans the batch boundary


@functools.lru_cache(maxsize=None)
def _stem_data(n, H, W, c0):
    rng = np.random.default_rng(_seed("stem1", n, H, W, c0))
    img = rng.integers(0, 256, (n + 1, H, W, 4), dtype=np.uint8)
    img[..., 3] = 255
    w27 = (rng.standard_normal((27, c0)) / np.sqrt(27)).astype(F32)
    bias = (0.2 * rng.standard_normal(c0)).astype(F32)
    return img, w27, bias


def _stem_table(fmt):
    lut = np.arange(256, dtype=F32) / F32(255)             # one correctly rounded float32 division per entry
    return lut.astype(F16).astype(F32) if fmt == "f16" else lut


def _stem_taps(px):
    """px [n, H, W, 3] -> the 27 input planes [n, H / 2, W / 2] in the kernel's order (ky, kx, colour), zero beyond the border."""
    n, H, W, _ = px.shape
    pad = np.zeros((n, H + 1, W + 1, 3), px.dtype)
    pad[:, 1:, 1:] = px                                    # padded row 2 oy + ky = image row 2 oy - 1 + ky
    return [pad[:, ky:ky + H:2, kx:kx + W:2, col] for ky in range(3) for kx in range(3) for col in range(3)]


@functools.lru_cache(maxsize=None)
def _stem_refs(n, H, W, c0, table):
    """(float64 reference, the same recipe in float32) of the first n images; table: 'f16' or 'f32' (the pair format holds the fp32 table)."""
    img, w27, bias = _stem_data(n, H, W, c0)
    px = _stem_table(table)[img[:n, ..., :3]]
    out = []
    for dt in (F64, F32):
        acc = np.broadcast_to(bias.astype(dt), (n, H // 2, W // 2, c0)).copy()
        for k, plane in enumerate(_stem_taps(px.astype(dt))):
            acc += plane[..., None] * w27[k].astype(dt)
        assert acc.dtype == dt
        out.append(np.maximum(acc, dt(0)))
    return out[0], out[1]


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("c0", [16, 32, 48])
@pytest.mark.parametrize("n,H,W", STEM_SIZES, ids=lambda v: str(v))
def test_stem1_values(gtx_ctx, n, H, W, c0, fmt):
    """ReLU(conv 3x3 stride 2 of table[byte] + bias) against float64, written into a channel slice; the fourth byte does not matter."""
    from geotrax_amd import ops

    img, w27, bias = _stem_data(n, H, W, c0)
    cs, coff = c0 + 24, 8
    out0 = _out_map(np.random.default_rng(1), fmt, n, H // 2, W // 2, cs)
    got, sat = ops.rt_stem1(img, w27, bias, out0, n=n, out_coff=coff, split=fmt == "split", ctx=gtx_ctx)
    assert not sat
    _assert_outside_kept(got, out0, n, coff, c0)
    ref64, ref32 = _stem_refs(n, H, W, c0, "f16" if fmt == "f16" else "f32")
    scale = float(np.abs(ref64).max())
    e_k = float(np.abs(got[:n, ..., coff:coff + c0].astype(F64) - ref64).max() / scale)
    e_r = float(np.abs(_stored(ref32, fmt) - ref64).max() / scale)
    print(f"stem1 {fmt} n{n} {H}x{W} c0={c0}: e_kernel {e_k:.3e} e_fp32ref {e_r:.3e} ratio {e_k / max(e_r, 1e-30):.2f}")
    assert e_k < 8 * e_r + 1e-7, (e_k, e_r)
    img0 = img.copy()
    img0[..., 3] = 0
    again, _ = ops.rt_stem1(img0, w27, bias, out0, n=n, out_coff=coff, split=fmt == "split", ctx=gtx_ctx)
    assert again.tobytes() == got.tobytes()


@pytest.mark.parametrize("fmt", FMTS)
def test_stem1_tap_map(gtx_ctx, fmt):
    """One-hot weights (channel c reads row c of w27 and nothing else; channels 27..31 read nothing) on an image whose 27 values
    under any 3 x 3 window all differ and none is 0: channel c is exactly the table entry of that neighbour's byte, and exactly 0
    where the tap falls on the padding -- the top row and the left column, nothing on the right or at the bottom of an even image."""
    from geotrax_amd import ops

    n, H, W, c0 = 2, 10, 14, 32
    yy, xx = np.mgrid[0:H, 0:W]
    img = np.full((n + 1, H, W, 4), 255, np.uint8)
    for ch in range(3):
        img[0, ..., ch] = ((yy % 3) * 3 + xx % 3) * 27 + ch * 9 + (yy // 3 + xx // 3) % 9 + 1        # 1 .. 243
        img[1, ..., ch] = 255 - img[0, ..., ch]
    w27 = np.zeros((27, c0), F32)
    w27[np.arange(27), np.arange(27)] = 1.0
    out0 = _out_map(np.random.default_rng(2), fmt, n, H // 2, W // 2, c0 + 8)
    got, sat = ops.rt_stem1(img, w27, np.zeros(c0, F32), out0, n=n, out_coff=8, split=fmt == "split", ctx=gtx_ctx)
    assert not sat
    _assert_outside_kept(got, out0, n, 8, c0)
    got = got[:n, ..., 8:8 + c0].astype(F64)
    table = _stem_table(fmt)
    want = np.stack(_stem_taps(table[img[:n, ..., :3]]), -1)
    padded = np.stack(_stem_taps(np.ones((n, H, W, 3), F32)), -1) == 0
    oy, ox = np.mgrid[0:H // 2, 0:W // 2]
    for k in range(27):
        ky, kx = divmod(k // 3, 3)
        assert np.array_equal(padded[..., k], np.broadcast_to(((oy == 0) & (ky == 0)) | ((ox == 0) & (kx == 0)), padded.shape[:3]))
    assert np.array_equal(got[..., :27], _stored(want, fmt))
    assert np.all(got[..., :27][padded] == 0) and np.all(got[..., :27][~padded] > 0) and np.all(got[..., 27:] == 0)
    print(f"stem1 tap map {fmt}: 27 taps exact, {int(padded.sum())} padded entries of {padded.size}")


@pytest.mark.parametrize("fmt", FMTS)
def test_stem1_relu_and_saturation(gtx_ctx, fmt):
    """A bias of -100 gives zeros: all-zero bits, so neither a negative value nor -0.0 is stored. A bias of 1e5 is past fp16's range:
    the pair format clamps to 65504 and raises the flag, fp32 stores the value and leaves the flag."""
    from geotrax_amd import ops

    n, H, W, c0 = 2, 6, 10, 16
    img, w27, _ = _stem_data(n, H, W, c0)
    out0 = _out_map(np.random.default_rng(3), fmt, n, H // 2, W // 2, c0 + 8)
    got, sat = ops.rt_stem1(img, w27, np.full(c0, -100, F32), out0, n=n, out_coff=8, split=fmt == "split", ctx=gtx_ctx)
    assert not sat
    _assert_outside_kept(got, out0, n, 8, c0)
    assert not _bits(got[:n, ..., 8:8 + c0]).any()
    if fmt == "f16":
        return
    got, sat = ops.rt_stem1(img, w27, np.full(c0, 1e5, F32), out0, n=n, out_coff=8, split=fmt == "split", ctx=gtx_ctx)
    _assert_outside_kept(got, out0, n, 8, c0)
    part = got[:n, ..., 8:8 + c0]
    if fmt == "split":
        assert sat and np.all(part == 65504)
    else:
        assert not sat and np.all(np.abs(part - 1e5) < 10)
    print(f"stem1 saturation {fmt}: flag {int(sat)}, stored {float(part.min())} .. {float(part.max())}")


# ============================================================================ pool2
def _pool2_ref(x):
    import torch
    import torch.nn.functional as F

    t = torch.from_numpy(np.ascontiguousarray(x.astype(F64))).permute(0, 3, 1, 2)
    return F.max_pool2d(F.pad(t, [0, 1, 0, 1]), 2, 1).permute(0, 2, 3, 1).numpy()


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("c", [8, 24, 40])
@pytest.mark.parametrize("n,h,w", [(1, 1, 1), (2, 5, 7), (1, 9, 33)], ids=lambda v: str(v))
def test_pool2_matches_padded_max_pool(gtx_ctx, n, h, w, c, fmt):
    """max_pool2d(F.pad(x, [0, 1, 0, 1]), 2, 1) value for value: a maximum of held values and the padding's 0 is a held value."""
    from geotrax_amd import ops

    rng = np.random.default_rng(_seed("pool2", n, h, w, c))
    x = _held(rng.standard_normal((n, h, w, c)) * 3, fmt)
    xin = _in_map(x, fmt, c + 16, 8)
    out0 = _out_map(rng, fmt, n, h, w, c + 8)
    got, sat = ops.rt_pool2(xin, c, out0, n=n, in_coff=8, out_coff=0, split=fmt == "split", ctx=gtx_ctx)
    assert not sat
    _assert_outside_kept(got, out0, n, 0, c)
    want = _pool2_ref(x)
    assert np.array_equal(got[:n, ..., :c].astype(F64), want)
    print(f"pool2 {fmt} n{n} {h}x{w} c={c}: exact, {int((want == 0).sum())} values are the padding's zero")


@pytest.mark.parametrize("fmt", FMTS)
def test_pool2_batch_boundary(gtx_ctx, fmt):
    """Image 0 all negative, image 1 all large and positive: the padding's zeros win in image 0's last row and column (all-zero
    bits), its interior stays negative, and nothing of image 1 shows up in image 0."""
    from geotrax_amd import ops

    n, h, w, c = 2, 5, 7, 8
    rng = np.random.default_rng(11)
    x = np.empty((n, h, w, c), F64)
    x[0] = -rng.uniform(1, 4, (h, w, c))
    x[1] = rng.uniform(1000, 2000, (h, w, c))
    x = _held(x, fmt)
    out0 = _out_map(rng, fmt, n, h, w, c + 8)
    got, sat = ops.rt_pool2(_in_map(x, fmt, c + 8, 0), c, out0, n=n, out_coff=8, split=fmt == "split", ctx=gtx_ctx)
    assert not sat
    _assert_outside_kept(got, out0, n, 8, c)
    g = got[:n, ..., 8:]
    assert not _bits(g[0, -1]).any() and not _bits(g[0, :, -1]).any()
    assert np.all(g[0, :-1, :-1] < 0) and np.all(g[0] <= 0)
    assert np.array_equal(g.astype(F64), _pool2_ref(x))
    assert np.all(g[1] >= 1000)


# ============================================================================ depthwise convolution
DW_MAPS = [(1, 3), (2, 2), (8, 8), (9, 17), (13, 19)]      # smaller than the halo, exactly one 8 x 8 tile, a tile plus one row / column, two tiles each way
DW_FORMS = [(32, 1), (64, 1), (40, 1), (32, 2)]            # (c, stride): the LDS-tiled kernel twice (one and two channel blocks), the per-thread kernel twice
DW_N = 3                                                   # blockIdx.z of the tiled form


def _grid(v, q, lim):
    return (np.clip(np.round(v * q), -lim * q, lim * q) / q).astype(F32)


@functools.lru_cache(maxsize=None)
def _dw_data(k, c, stride, h, w):
    """Values on a binary grid (x, r: 2^-6 within +-4; w, b: 2^-8 within +-1): every product and partial sum is exact in fp32, and x and
    r are fp16 values, which every format holds exactly."""
    rng = np.random.default_rng(_seed("dw", k, c, stride, h, w))
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    x = _grid(rng.normal(0, 1, (DW_N, h, w, c)), 64, 4)
    wt = _grid(rng.normal(0, 1 / k, (c, 1, k, k)), 256, 1)
    b = _grid(rng.normal(0, 0.1, c), 256, 1)
    r = _grid(rng.normal(0, 1, (DW_N, ho, wo, c)), 64, 4)
    return x, wt, b, r


def _dw_loop(x, w, b, stride):
    """bias (or 0), then one fused multiply-add per tap in (ky, kx) order, float32: the product is exact in float64, one rounding per
    step. All output pixels at once; a tap on the padding adds an exact zero."""
    n, h, wd, c = x.shape
    k = w.shape[-1]
    r = k // 2
    ho, wo = (h - 1) // stride + 1, (wd - 1) // stride + 1
    xp = np.zeros((n, h + 2 * r, wd + 2 * r, c), F64)
    xp[:, r:r + h, r:r + wd] = x
    acc = np.zeros((n, ho, wo, c), F32) if b is None else np.broadcast_to(b, (n, ho, wo, c)).astype(F32)
    for ky in range(k):
        for kx in range(k):
            v = xp[:, ky:ky + (ho - 1) * stride + 1:stride, kx:kx + (wo - 1) * stride + 1:stride]
            acc = (v * w[:, 0, ky, kx].astype(F64) + acc.astype(F64)).astype(F32)
    return acc


@functools.lru_cache(maxsize=None)
def _dw_pre(k, c, stride, h, w, with_bias):
    x, wt, b, _ = _dw_data(k, c, stride, h, w)
    return _dw_loop(x, wt, b if with_bias else None, stride)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("h,w", DW_MAPS)
@pytest.mark.parametrize("c,stride", DW_FORMS)
@pytest.mark.parametrize("k", [5, 3, 7])
def test_dwconv_slices_small_maps_all_activations(gtx_ctx, k, c, stride, h, w, fmt):
    """Batch 3 read at channel 8 of c + 16, written at channel 16 of c + 24, the residual read at channel 8 of c + 8; activations none,
    SiLU and ReLU, with and without the residual, with and without a bias."""
    from geotrax_amd import ops

    x, wt, b, r = _dw_data(k, c, stride, h, w)
    n = DW_N
    ho, wo = r.shape[1:3]
    xin, rin = _in_map(x.astype(_np(fmt)), fmt, c + 16, 8), _in_map(r.astype(_np(fmt)), fmt, c + 8, 8)
    out0 = _out_map(np.random.default_rng(4), fmt, n, ho, wo, c + 24)
    store_rel, store_abs = {"f16": (2.0 ** -11, 2.0 ** -25), "split": (2.0 ** -21, 2.0 ** -24), "f32": (2.0 ** -24, 0.0)}[fmt]   # the format's own rounding
    worst = 0.0
    for act, use_res, use_bias in [(a, rr, True) for a in (0, 1, 2) for rr in (False, True)] + [(0, False, False), (2, True, False)]:
        got, sat = ops.rt_dwconv(xin, wt, b if use_bias else None, out0, stride=stride, act=act, residual=rin if use_res else None, n=n, in_coff=8,
                                 out_coff=16, res_coff=8, split=fmt == "split", ctx=gtx_ctx)
        assert not sat
        _assert_outside_kept(got, out0, n, 16, c)
        got = got[:n, ..., 16:16 + c].astype(F64)
        pre = _dw_pre(k, c, stride, h, w, use_bias)
        if act != 1:
            want = np.maximum(pre, F32(0)) if act == 2 else pre
            want = _stored(want + r if use_res else want, fmt)
            assert np.array_equal(got, want), (act, use_res, use_bias, float(np.abs(got - want).max()))
        else:
            pre = pre.astype(F64)
            silu = pre / (1 + np.exp(-pre))
            want = silu + (r if use_res else 0)
            tol = 8 * 2.0 ** -24 * np.abs(silu) + 2.0 ** -24 * np.abs(want) + store_rel * np.abs(want) + store_abs + 1e-45
            worst = max(worst, float((np.abs(got - want) / tol).max()))
            assert np.all(np.abs(got - want) <= tol), (use_res, worst)
    print(f"dwconv {fmt} k{k} c{c} s{stride} {h}x{w}: none / ReLU bit for bit, SiLU error at most {worst:.2f} of its tolerance")


# ============================================================================ upsample2x
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("c", [8, 24])
@pytest.mark.parametrize("n,h,w", [(1, 1, 1), (2, 3, 5)], ids=lambda v: str(v))
def test_upsample2x_is_a_raw_copy(gtx_ctx, n, h, w, c, fmt):
    """Output pixel (y, x) holds input pixel (y // 2, x // 2): bit patterns in fp16 and fp32 (-0.0, a subnormal and inf among them),
    values in the pair format."""
    from geotrax_amd import ops

    rng = np.random.default_rng(_seed("up", n, h, w, c))
    x = _held(rng.standard_normal((n, h, w, c)) * 3, fmt)
    if fmt != "split":
        special = [-0.0, 1e-40 if fmt == "f32" else 6e-8, np.inf, -np.inf]
        x.reshape(-1)[:4] = special
        x.reshape(-1)[-4:] = special[::-1]
        assert np.signbit(x.reshape(-1)[0]) and 0 < x.reshape(-1)[1] < np.finfo(x.dtype).tiny
    xin = _in_map(x, fmt, c + 8, 8)
    out0 = _out_map(rng, fmt, n, 2 * h, 2 * w, c + 16)
    got = ops.rt_upsample2x(xin, c, out0, n=n, in_coff=8, out_coff=8, split=fmt == "split", ctx=gtx_ctx)
    _assert_outside_kept(got, out0, n, 8, c)
    want = x.repeat(2, axis=1).repeat(2, axis=2)
    assert np.array_equal(_bits(got[:n, ..., 8:8 + c]), _bits(want))
    print(f"upsample2x {fmt} n{n} {h}x{w} c={c}: exact")


# ============================================================================ tokens_in
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("c", [8, 24, 256])
@pytest.mark.parametrize("h,w", [(3, 5), (1, 1)])
def test_tokens_in(gtx_ctx, h, w, c, fmt):
    """src = the values the format holds, exactly; q = float32(src + pos), one fp32 addition per element, with pos indexed by
    row % (h w): the positions' embeddings all differ, so the second image reusing the first one's rows is proved. Without pos and q,
    src alone is written. The rows of the image behind the last come back as given."""
    from geotrax_amd import ops

    n, T = 2, h * w
    rng = np.random.default_rng(_seed("tok", h, w, c))
    x = _held(rng.standard_normal((n, h, w, c)) * np.exp(rng.uniform(-2, 2, (n, h, w, 1))), fmt)
    pos = rng.standard_normal((T, c)).astype(F32)
    assert len(np.unique(pos, axis=0)) == T
    xin = _in_map(x, fmt, c + 16, 8)
    src0 = rng.standard_normal(((n + 1) * T, c)).astype(F32)
    q0 = rng.standard_normal(((n + 1) * T, c)).astype(F32)
    src, q = ops.rt_tokens_in(xin, c, pos, src0, q0, n=n, in_coff=8, split=fmt == "split", ctx=gtx_ctx)
    want = x.astype(F32).reshape(n * T, c)
    assert np.array_equal(_bits(src[:n * T]), _bits(want))
    want_q = want + np.tile(pos, (n, 1))
    assert want_q.dtype == F32 and np.array_equal(_bits(q[:n * T]), _bits(want_q))
    assert src[n * T:].tobytes() == src0[n * T:].tobytes() and q[n * T:].tobytes() == q0[n * T:].tobytes()
    alone, none = ops.rt_tokens_in(xin, c, None, src0, None, n=n, in_coff=8, split=fmt == "split", ctx=gtx_ctx)
    assert none is None and alone.tobytes() == src.tobytes()
    print(f"tokens_in {fmt} {h}x{w} C={c}: src and q exact")


# ============================================================================ mask_invalid
LEVEL_WH = {0: 0.05, 1: 0.1, 2: 0.2, 4: 0.8, 5: 1.6}
MASK_MAPS = [(50, 50), (7, 150), (100, 13), (3, 200), (1, 1)]


def _centres(size, reciprocal=False):
    g = np.arange(size, dtype=F32) + F32(0.5)
    v = g * (F32(1) / F32(size)) if reciprocal else g / F32(size)
    assert v.dtype == F32
    return v


def _valid(h, w, level, reciprocal=False):
    """RTDETRDecoder._generate_anchors' valid_mask in numpy float32: ((grid + 0.5) / [w, h], 0.05 * 2^level) all strictly inside
    (float32(0.01), float32(0.99)), with true float32 division (reciprocal: the cheaper evaluation the kernel must not use)."""
    inside = lambda v: (v > F32(0.01)) & (v < F32(0.99))
    wh = F32(0.05) * F32(2 ** level)
    assert wh == F32(LEVEL_WH[level])
    return inside(_centres(h, reciprocal))[:, None] & inside(_centres(w, reciprocal))[None, :] & bool(inside(wh))


@functools.lru_cache(maxsize=None)
def _assert_cases_contain_threshold_ties():
    """On the CPU: at w = 50 the first and the last cell sit exactly on the thresholds (invalid by a tie), and multiplying by the
    reciprocal instead of dividing moves at least one cell of the 50 x 50 case across: the case can see the difference."""
    cx = _centres(50)
    assert cx[0] == F32(0.01) and cx[49] == F32(0.99)
    v = _valid(50, 50, 0)
    assert not v[:, 0].any() and not v[:, 49].any() and not v[0].any() and not v[49].any() and v[1:49, 1:49].all()
    differ = int((v != _valid(50, 50, 0, reciprocal=True)).sum())
    assert differ >= 1
    return differ


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("level,h,w", [(lv, h, w) for lv in (0, 1, 2, 4) for h, w in MASK_MAPS] + [(5, 3, 5)])
def test_mask_invalid(gtx_ctx, level, h, w, fmt):
    """Cell by cell: an invalid anchor's slice is all zero bits, a valid one's comes back as it was; the channels beside the slice and
    the image behind the last keep their values whatever the cell."""
    from geotrax_amd import ops

    print(f"mask_invalid: {_assert_cases_contain_threshold_ties()} cells of 50 x 50 change with the reciprocal evaluation")
    n, c, cs, coff = 2, 8, 24, 8
    rng = np.random.default_rng(_seed("mask", level, h, w))
    m0 = _out_map(rng, fmt, n, h, w, cs)                   # nonzero fp16 values: every format returns them exactly
    got = ops.rt_mask_invalid(m0, c, level, n=n, coff=coff, split=fmt == "split", ctx=gtx_ctx)
    _assert_outside_kept(got, m0, n, coff, c)
    valid = _valid(h, w, level)
    if level == 5:
        assert not valid.any()
    zeroed = ~_bits(got[:n, ..., coff:coff + c]).any(-1)
    kept = (_bits(got[:n, ..., coff:coff + c]) == _bits(m0[:n, ..., coff:coff + c])).all(-1)
    assert np.array_equal(zeroed, np.broadcast_to(~valid, (n, h, w))), np.argwhere(zeroed != ~valid)[:8]
    assert np.array_equal(kept, np.broadcast_to(valid, (n, h, w)))
    print(f"mask_invalid {fmt} level {level} {h}x{w}: {int(valid.sum())} of {h * w} cells valid, decided as the float32 reference")
