"""Parity of every detector HIP kernel against oracle/ through the C ABI (gtx_op_*), on the
layer shapes YOLOv8s actually runs at sizes the oracle finishes in seconds."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _rand(rng, shape, dtype):
    return rng.standard_normal(shape).astype(np.float32).astype(dtype)


def _tol(dtype):
    # fp32: MFMA f32 is an exact fmaf chain, only the summation order differs from the oracle.
    # fp16: inputs are identical fp16 values, products accumulate in fp32, the stored output is
    # rounded to fp16 once (rel 2^-11) -- BASELINE.md §5 allows 2e-2 rel for this path.
    return (2e-4, 2e-4) if dtype == np.float32 else (4e-3, 4e-3)


# (cin, cout, k, stride, h, w): stem-adjacent, C2f inner, stride-2 downsamples, SPPF / concat 1x1s
CONV_CASES = [
    (32, 64, 3, 2, 40, 56),     # model.1
    (32, 32, 3, 1, 24, 40),     # model.2.m.0.cv1 (BN=32 path)
    (64, 64, 1, 1, 24, 40),     # model.2.cv1 (KC=64 path)
    (96, 64, 1, 1, 17, 33),     # model.2.cv2 (Cin=96 -> KC=32 1x1 path), ragged tile edges
    (64, 128, 3, 2, 33, 47),    # model.3, odd input size
    (128, 128, 3, 1, 16, 16),   # head cls conv, exactly one tile
    (256, 512, 3, 2, 14, 14),   # model.7, deep K
    (512, 256, 1, 1, 9, 20),    # model.9.cv1
    (768, 256, 1, 1, 8, 16),    # model.12.cv1
    (128, 192, 3, 1, 20, 36),   # fused Detect stage 1 at P3 (3 cout tiles)
    # widths that are multiples of 16 only (yolov8 n / m / x): a half-empty last cout tile, 16-channel K chunks
    (16, 16, 3, 1, 20, 36),     # yolov8n model.2.m.0.cv1
    (48, 48, 3, 1, 17, 33),     # yolov8m bottleneck
    (144, 96, 1, 1, 12, 20),    # yolov8m model.2.cv2: Cin = 3 * 48
    (80, 160, 3, 2, 21, 31),    # yolov8x model.1
    (400, 80, 1, 1, 9, 13),     # Cin = 400: multiple of 16 only; Cout = 80: 2.5 tiles of 32
]


@pytest.mark.parametrize("dtype", [np.float16, np.float32])
@pytest.mark.parametrize("case", CONV_CASES)
def test_conv2d_matches_oracle(gtx_ctx, dtype, case):
    from geotrax_amd import ops
    from oracle.yolov8_ref import conv2d_nhwc

    cin, cout, k, stride, h, w = case
    rng = np.random.default_rng(hash(case) % 2**32)
    x = _rand(rng, (2, h, w, cin), dtype)
    wt = (rng.standard_normal((cout, k, k, cin)) / np.sqrt(cin * k * k)).astype(np.float32)
    if dtype == np.float16:
        wt = wt.astype(np.float16).astype(np.float32)  # the kernel stores weights in fp16
    b = rng.standard_normal(cout).astype(np.float32) * 0.1
    got = ops.conv2d(x, wt, b, stride=stride, act=True, ctx=gtx_ctx)
    ref = conv2d_nhwc(x, wt, b, stride=stride, act=True)
    rtol, atol = _tol(dtype)
    np.testing.assert_allclose(got.astype(np.float32), ref, rtol=rtol, atol=atol)


@pytest.mark.parametrize("case", CONV_CASES)
def test_conv2d_split_f16x3_meets_the_fp32_bar(gtx_ctx, case):
    """The split-f16x3 convolution (fp32 arrays, operands split into hi + lo fp16 parts, three fp16 MFMAs per
    product) against the float64 oracle: its error must be of the order of the exact-fp32 kernel's own (both
    far inside BASELINE.md section 5's 1e-4 relative bar for the fp32 path), on wide-range data: activations
    over five decades including values whose lo part is an fp16 subnormal, weights up to +-8."""
    from geotrax_amd import ops
    from oracle.yolov8_ref import conv2d_nhwc

    cin, cout, k, stride, h, w = case
    rng = np.random.default_rng(hash(case) % 2**32 + 1)
    x = (rng.standard_normal((2, h, w, cin)) * 10.0 ** rng.uniform(-4, 1, (2, h, w, cin))).astype(np.float32)
    wt = (rng.standard_normal((cout, k, k, cin)) / np.sqrt(cin * k * k)).astype(np.float32)
    wt[rng.integers(0, cout), :, :, rng.integers(0, cin)] *= 60.0          # a few large taps set the layer's power-of-two scale
    b = rng.standard_normal(cout).astype(np.float32) * 0.1
    ref64 = conv2d_nhwc(x.astype(np.float64), wt.astype(np.float64), b.astype(np.float64), stride=stride, act=False)
    exact = ops.conv2d(x, wt, b, stride=stride, act=False, ctx=gtx_ctx)
    split = ops.conv2d(x, wt, b, stride=stride, act=False, split=True, ctx=gtx_ctx)
    scale = np.abs(ref64).max()
    e_exact, e_split = np.abs(exact - ref64).max() / scale, np.abs(split - ref64).max() / scale
    assert e_split < 2e-6, (e_split, e_exact)                     # 50x inside the 1e-4 bar
    assert e_split < 8 * e_exact + 1e-7, (e_split, e_exact)       # same order as the exact-fp32 MFMA's summation error
    got = ops.conv2d(x, wt, b, stride=stride, act=True, split=True, ctx=gtx_ctx)
    np.testing.assert_allclose(got, conv2d_nhwc(x, wt, b, stride=stride, act=True), rtol=2e-4, atol=2e-4)


@pytest.mark.parametrize("shape", [(1, 8, 16, 32, 64, False), (2, 20, 30, 64, 64, True), (1, 60, 60, 32, 128, False), (2, 37, 53, 128, 192, True),
                                   (1, 16, 32, 256, 64, False), (1, 9, 17, 96, 80, True)])
def test_conv2d_k32_split_meets_the_fp32_bar(gtx_ctx, monkeypatch, shape):
    """The v_mfma_f32_16x16x32_f16 form of the split-f16x3 3x3 stride-1 convolution (csrc/conv_k32_split.hip, GTX_K32=1): the
    direct kernel's bar against a float64 convolution of the values the pair format holds -- partial tiles, several cout
    tiles (a half-empty last one), residual and SiLU -- and within 2e-6 of the 32x32x16 kernel."""
    import torch
    from geotrax_amd import ops

    n, h, w, cin, cout, use_res = shape
    rng = np.random.default_rng(12)
    x = (rng.standard_normal((n, h, w, cin)) * np.exp(rng.uniform(-3, 3, (n, h, w, cin)))).astype(np.float32)
    wt = (rng.standard_normal((cout, 3, 3, cin)) / np.sqrt(9 * cin)).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32)
    res = rng.standard_normal((n, h, w, cout)).astype(np.float32) if use_res else None

    def pairs(a):
        hi = a.astype(np.float16).astype(np.float32)
        return hi.astype(np.float64) + (a - hi).astype(np.float16).astype(np.float64)

    y = torch.nn.functional.conv2d(torch.from_numpy(pairs(x)).permute(0, 3, 1, 2), torch.from_numpy(wt.astype(np.float64)).permute(0, 3, 1, 2),
                                   torch.from_numpy(b.astype(np.float64)), padding=1)
    y = torch.nn.functional.silu(y).permute(0, 2, 3, 1).numpy()
    if res is not None:
        y = y + pairs(res)
    monkeypatch.setenv("GTX_K32", "0")
    direct = ops.conv2d(x, wt, b, act=True, residual=res, split=True, ctx=gtx_ctx)
    monkeypatch.setenv("GTX_K32", "1")
    k32 = ops.conv2d(x, wt, b, act=True, residual=res, split=True, ctx=gtx_ctx)
    scale = np.abs(y).max()
    if cout % 64 == 0:
        assert not np.array_equal(k32, direct)        # the other kernel did run (cout % 64 != 0: 32-cout tiles, not eligible)
    assert np.abs(k32 - y).max() / scale < 2e-6 and np.abs(k32 - direct).max() / scale < 2e-6


def test_conv2d_split_slices_residual_and_exact_integers(gtx_ctx):
    from geotrax_amd import ops
    from oracle.yolov8_ref import conv2d_nhwc

    rng = np.random.default_rng(7)
    buf = _rand(rng, (1, 19, 27, 96), np.float32)
    wt = (rng.standard_normal((32, 3, 3, 32)) / 17).astype(np.float32)
    b = rng.standard_normal(32).astype(np.float32) * 0.1
    res = np.ascontiguousarray(buf[..., 32:64])
    got = ops.conv2d(buf, wt, b, in_coff=32, cin=32, out=buf.copy(), out_coff=64, residual=res, split=True, ctx=gtx_ctx)
    np.testing.assert_allclose(got[..., 64:96], conv2d_nhwc(buf[..., 32:64], wt, b, residual=res), rtol=2e-5, atol=2e-5)
    # The slices the convolution does not write come back as they went in: as (hi, lo) fp16 pairs, the form GTX_F32S
    # tensors have on the device (csrc/split_format.hpp) -- 22 significant bits of the fp32 host values
    hi = buf[..., :64].astype(np.float16)
    lo = (buf[..., :64] - hi.astype(np.float32)).astype(np.float16)
    np.testing.assert_array_equal(got[..., :64], hi.astype(np.float32) + lo.astype(np.float32))
    np.testing.assert_allclose(got[..., :64], buf[..., :64], rtol=3e-7, atol=6e-8)
    # small integers: hi parts carry everything, lo parts are zero, every partial sum is exact
    for (cin, cout, k, s) in [(32, 64, 3, 1), (64, 32, 3, 2), (128, 64, 1, 1), (48, 32, 1, 1)]:
        x = rng.integers(-3, 4, (1, 21, 35, cin)).astype(np.float32)
        wi = rng.integers(-2, 3, (cout, k, k, cin)).astype(np.float32)
        bi = rng.integers(-4, 5, cout).astype(np.float32)
        np.testing.assert_array_equal(ops.conv2d(x, wi, bi, stride=s, act=False, split=True, ctx=gtx_ctx),
                                      conv2d_nhwc(x, wi, bi, stride=s, act=False))
    # out-of-range activations are clamped when split, never NaN
    x = np.full((1, 8, 16, 32), 1e6, np.float32)
    y = ops.conv2d(x, np.ones((32, 1, 1, 32), np.float32), None, act=False, split=True, ctx=gtx_ctx)
    assert np.isfinite(y).all()


@pytest.mark.parametrize("dtype", [np.float16, np.float32])
def test_conv2d_slices_residual_identity(gtx_ctx, dtype):
    """Channel-slice input, channel-slice output (concat buffer untouched elsewhere), residual
    add after SiLU (Bottleneck shortcut) and the identity-activation variant."""
    from geotrax_amd import ops
    from oracle.yolov8_ref import conv2d_nhwc

    rng = np.random.default_rng(7)
    n, h, w = 1, 19, 27
    buf = _rand(rng, (n, h, w, 96), dtype)          # C2f concat buffer: 3 chunks of 32
    wt = (rng.standard_normal((32, 3, 3, 32)) / 17).astype(np.float32)
    if dtype == np.float16:
        wt = wt.astype(np.float16).astype(np.float32)
    b = rng.standard_normal(32).astype(np.float32) * 0.1
    res = np.ascontiguousarray(buf[..., 32:64])
    out = buf.copy()
    got = ops.conv2d(buf, wt, b, in_coff=32, cin=32, out=out, out_coff=64, residual=res, ctx=gtx_ctx)
    ref = conv2d_nhwc(buf[..., 32:64], wt, b, residual=res.astype(np.float32))
    rtol, atol = _tol(dtype)
    np.testing.assert_allclose(got[..., 64:96].astype(np.float32), ref, rtol=rtol, atol=atol)
    np.testing.assert_array_equal(got[..., :64], buf[..., :64])  # rest of the buffer untouched
    got2 = ops.conv2d(np.ascontiguousarray(buf[..., :32]), wt, None, act=False, ctx=gtx_ctx)
    ref2 = conv2d_nhwc(buf[..., :32], wt, None, act=False)
    np.testing.assert_allclose(got2.astype(np.float32), ref2, rtol=rtol, atol=atol)


def test_conv2d_exact_integer_data(gtx_ctx):
    """Small-integer inputs make every partial sum exact in fp32: any layout / fragment-mapping
    slip shows up as a hard mismatch rather than a tolerance question (asymmetric weights)."""
    from geotrax_amd import ops
    from oracle.yolov8_ref import conv2d_nhwc

    rng = np.random.default_rng(3)
    for dtype in (np.float16, np.float32):
        for (cin, cout, k, s) in [(32, 64, 3, 1), (64, 32, 3, 2), (128, 64, 1, 1)]:
            x = rng.integers(-3, 4, (1, 21, 35, cin)).astype(dtype)
            wt = rng.integers(-2, 3, (cout, k, k, cin)).astype(np.float32)
            b = rng.integers(-4, 5, cout).astype(np.float32)
            got = ops.conv2d(x, wt, b, stride=s, act=False, ctx=gtx_ctx)
            ref = conv2d_nhwc(x, wt, b, stride=s, act=False)
            assert np.abs(ref).max() < 2048  # exactly representable in fp16 too
            np.testing.assert_array_equal(got.astype(np.float32), ref)


@pytest.mark.parametrize("dtype", [np.float16, np.float32])
def test_sppf_pool_and_upsample(gtx_ctx, dtype):
    from geotrax_amd import ops
    from oracle.yolov8_ref import sppf_pools_nhwc, upsample2x_nhwc

    rng = np.random.default_rng(11)
    c = 64
    x = np.zeros((2, 13, 22, 4 * c), dtype=dtype)
    x[..., :c] = _rand(rng, (2, 13, 22, c), dtype)
    got = ops.sppf_pool(x, c, ctx=gtx_ctx)
    np.testing.assert_array_equal(got.astype(np.float32), sppf_pools_nhwc(x[..., :c]))

    src = _rand(rng, (2, 7, 9, 48), dtype)
    dst = _rand(rng, (2, 14, 18, 80), dtype)
    got = ops.upsample2x(src, 32, 16, dst, 40, ctx=gtx_ctx)
    np.testing.assert_array_equal(got[..., 40:72], upsample2x_nhwc(src[..., 16:48]))
    np.testing.assert_array_equal(got[..., :40], dst[..., :40])
    np.testing.assert_array_equal(got[..., 72:], dst[..., 72:])


@pytest.mark.parametrize("hw", [(13, 22), (60, 60), (5, 3), (64, 64), (68, 68), (70, 72)])
def test_sppf_pool_pair_format(gtx_ctx, hw):
    """The pools of the default fp32 path work on (hi, lo) pairs: maxima are taken on hi + lo and the winner's two halves are
    carried along, so the result is exactly the oracle's pools of the 22-bit rounded input. Maps up to 64 x 64 go through the
    whole-map kernel (one workgroup per image and 8-channel unit, 60 x 60 at the 1920 input), larger ones through the tiled one."""
    from geotrax_amd import ops
    from oracle.yolov8_ref import sppf_pools_nhwc

    rng = np.random.default_rng(3)
    c = 32
    h, w = hw
    x = np.zeros((2, h, w, 4 * c), np.float32)
    x[..., :c] = (rng.standard_normal((2, h, w, c)) * 3).astype(np.float32)
    hi = x.astype(np.float16).astype(np.float32)
    x22 = hi + (x - hi).astype(np.float16).astype(np.float32)               # what the pair format holds
    got = ops.sppf_pool(x, c, ctx=gtx_ctx, split=True)
    np.testing.assert_array_equal(got, sppf_pools_nhwc(x22[..., :c]))


@pytest.mark.parametrize("dtype", [np.float16, np.float32])
@pytest.mark.parametrize("shape,imgsz,rect", [((216, 384), 192, False), ((216, 384), 192, True), ((200, 300), 256, False), ((384, 216), 192, False),
                                              ((432, 768), 384, False)])     # exact 2x: 4 pixels per thread when the letterbox offsets allow, else 1
def test_preprocess_matches_oracle(gtx_ctx, dtype, shape, imgsz, rect):
    from geotrax_amd import ops
    from oracle.yolov8_ref import bgr2gray_half, letterbox

    rng = np.random.default_rng(5)
    frame = rng.integers(0, 256, (*shape, 3), dtype=np.uint8)
    ref, g = letterbox(frame, imgsz, rect, half=(dtype == np.float16))
    img, gray = ops.preprocess(frame, g["net_h"], g["net_w"], dtype=dtype, ctx=gtx_ctx)
    ref_nhwc = ref[0].permute(1, 2, 0).numpy()
    # integer pixel pipeline is exact; the /255 is one correctly rounded fp32 (or fp16) division
    np.testing.assert_array_equal(img[..., :3].astype(np.float32), ref_nhwc.astype(dtype).astype(np.float32))
    assert not img[..., 3].any()
    np.testing.assert_array_equal(gray, bgr2gray_half(frame))
