"""The v_mfma_f32_16x16x32_f16 form of the split-f16x3 3x3 stride-2 convolution (csrc/conv_k32s2_split.hip, ConvForm::K32S2,
GTX_K32S2=0 falls back to the 32x32x16 kernel), on the smallest shapes that reach each of its paths.

Bars. Between the two kernel forms: 1e-5 of the layer's largest value, the project's bar for a re-ordered sum
(test_fused_stem_matches_the_stem_launch). Against the oracle: 2e-4 of the layer's largest value (test_ops_gpu.py). Against a
float64 convolution of the values the pair format holds (hi + lo, 22 bits): 2e-6 of the largest value, the bar of the other
split-f16x3 forms (test_conv2d_k32_split_meets_the_fp32_bar) -- what is left is the weights' own 22-bit split, the dropped
lo x lo term (2^-22 per product) and an fp32 sum over at most 9 x 96 products."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FORMS_BAR, ORACLE_BAR, F64_BAR = 1e-5, 2e-4, 2e-6


def _pairs(a):
    """What the pair format keeps of an fp32 array: hi + lo, as float64."""
    hi = a.astype(np.float16).astype(np.float32)
    return hi.astype(np.float64) + (a - hi).astype(np.float16).astype(np.float64)


def _data(seed, n, h, w, cin, cout):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, h, w, cin)) * np.exp(rng.uniform(-3, 3, (n, h, w, cin)))).astype(np.float32)
    wt = (rng.standard_normal((cout, 3, 3, cin)) / np.sqrt(9 * cin)).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32)
    return x, wt, b


def _ref64(x, wt, b):
    """SiLU(conv 3x3 / stride 2 / pad 1 + bias) in float64 on the pair format's values of x."""
    import torch

    y = torch.nn.functional.conv2d(torch.from_numpy(_pairs(x)).permute(0, 3, 1, 2), torch.from_numpy(wt.astype(np.float64)).permute(0, 3, 1, 2),
                                   torch.from_numpy(b.astype(np.float64)), stride=2, padding=1)
    return torch.nn.functional.silu(y).permute(0, 2, 3, 1).numpy()


def _exact_pairs(rng, shape):
    """Values the pair format carries bit for bit (fp16 values: lo = 0): what a buffer holds before a launch."""
    return rng.standard_normal(shape).astype(np.float16).astype(np.float32)


def _rel(a, b, scale):
    return float(np.abs(a - b).max() / scale)


@pytest.mark.parametrize("cin,cout", [(32, 64), (64, 64), (32, 128), (64, 128)])
def test_partial_tiles_three_ways(gtx_ctx, monkeypatch, cin, cout):
    """19 x 37 in -> 10 x 19 out (two tile rows and two tile columns, both partial), batch 2; one and two K chunks, one and
    two cout tiles; bias and SiLU."""
    from geotrax_amd import ops
    from oracle.yolov8_ref import conv2d_nhwc

    x, wt, b = _data(21, 2, 19, 37, cin, cout)
    monkeypatch.setenv("GTX_K32S2", "0")
    old = ops.conv2d(x, wt, b, stride=2, act=True, split=True, ctx=gtx_ctx)
    monkeypatch.setenv("GTX_K32S2", "1")
    new = ops.conv2d(x, wt, b, stride=2, act=True, split=True, ctx=gtx_ctx)
    assert new.shape == (2, 10, 19, cout)
    assert not np.array_equal(new, old)               # the other kernel did run
    y = _ref64(x, wt, b)
    scale = np.abs(y).max()
    oracle = conv2d_nhwc(x, wt, b, stride=2, act=True)
    e_forms, e_f64, e_oracle = _rel(new, old, scale), _rel(new, y, scale), _rel(new, oracle, np.abs(oracle).max())
    print(f"cin={cin} cout={cout}: forms {e_forms:.2e} float64 {e_f64:.2e} oracle {e_oracle:.2e}")
    assert e_forms < FORMS_BAR and e_f64 < F64_BAR and e_oracle < ORACLE_BAR


@pytest.mark.parametrize("cin,cout", [(32, 64), (64, 128)])
def test_pad_skip_rows(gtx_ctx, monkeypatch, cin, cout):
    """34 x 34 in -> 17 x 17 out = three tile rows; ty_first = 1, ty_count = 1 computes output rows 8..15 only and the others
    keep what the buffer held, bit for bit."""
    from geotrax_amd import ops
    from oracle.yolov8_ref import conv2d_nhwc

    x, wt, b = _data(22, 2, 34, 34, cin, cout)
    held = _exact_pairs(np.random.default_rng(1), (2, 17, 17, cout))
    monkeypatch.setenv("GTX_K32S2", "1")
    full = ops.conv2d(x, wt, b, stride=2, act=True, split=True, ctx=gtx_ctx)
    part, = ops.conv2d_group([dict(x=x, w=wt, bias=b, out=held, ty_first=1, ty_count=1)], stride=2, act=True, split=True, ctx=gtx_ctx)
    np.testing.assert_array_equal(part[:, :8], held[:, :8])
    np.testing.assert_array_equal(part[:, 16:], held[:, 16:])
    np.testing.assert_array_equal(part[:, 8:16], full[:, 8:16])       # the same workgroups' sums
    monkeypatch.setenv("GTX_K32S2", "0")
    old, = ops.conv2d_group([dict(x=x, w=wt, bias=b, out=held, ty_first=1, ty_count=1)], stride=2, act=True, split=True, ctx=gtx_ctx)
    y = _ref64(x, wt, b)
    scale = np.abs(y).max()
    np.testing.assert_array_equal(old[:, :8], held[:, :8])
    assert not np.array_equal(part[:, 8:16], old[:, 8:16])
    assert _rel(part[:, 8:16], old[:, 8:16], scale) < FORMS_BAR and _rel(part[:, 8:16], y[:, 8:16], scale) < F64_BAR
    oracle = conv2d_nhwc(x, wt, b, stride=2, act=True)
    assert _rel(part[:, 8:16], oracle[:, 8:16], np.abs(oracle).max()) < ORACLE_BAR


def test_grouped_launch(gtx_ctx, monkeypatch):
    """Two members of different Cin (32 and 96: one and three K chunks), Cout and map size in one launch: block_begin and the
    XCD ranges of equal work. Every member equals its own single launch bit for bit."""
    from geotrax_amd import ops
    from oracle.yolov8_ref import conv2d_nhwc

    a = _data(23, 1, 19, 37, 32, 64)
    c = _data(24, 2, 35, 21, 96, 128)
    members = [dict(x=a[0], w=a[1], bias=a[2]), dict(x=c[0], w=c[1], bias=c[2])]
    monkeypatch.setenv("GTX_K32S2", "1")
    new = ops.conv2d_group(members, stride=2, act=True, split=True, ctx=gtx_ctx)
    singles = [ops.conv2d(x, wt, b, stride=2, act=True, split=True, ctx=gtx_ctx) for x, wt, b in (a, c)]
    monkeypatch.setenv("GTX_K32S2", "0")
    old = ops.conv2d_group(members, stride=2, act=True, split=True, ctx=gtx_ctx)
    for (x, wt, b), got, single, prev in zip((a, c), new, singles, old):
        np.testing.assert_array_equal(got, single)
        assert not np.array_equal(got, prev)
        y = _ref64(x, wt, b)
        scale = np.abs(y).max()
        oracle = conv2d_nhwc(x, wt, b, stride=2, act=True)
        assert _rel(got, prev, scale) < FORMS_BAR and _rel(got, y, scale) < F64_BAR and _rel(got, oracle, np.abs(oracle).max()) < ORACLE_BAR


def test_concat_slices(gtx_ctx, monkeypatch):
    """Input read from channels [32, 96) of a 128-channel buffer, output written to channels [64, 128) of a 160-channel one: in_coff,
    out_coff != 0 and both strides larger than C. The rest of the output buffer is untouched."""
    from geotrax_amd import ops
    from oracle.yolov8_ref import conv2d_nhwc

    rng = np.random.default_rng(25)
    xs, wt, b = _data(25, 2, 19, 37, 128, 64)
    wt = wt[:, :, :, :64].copy()
    held = _exact_pairs(rng, (2, 10, 19, 160))
    outs = {}
    for form in ("0", "1"):
        monkeypatch.setenv("GTX_K32S2", form)
        outs[form] = ops.conv2d(xs, wt, b, stride=2, act=True, in_coff=32, cin=64, out=held.copy(), out_coff=64, split=True, ctx=gtx_ctx)
    new, old = outs["1"], outs["0"]
    np.testing.assert_array_equal(new[..., :64], held[..., :64])
    np.testing.assert_array_equal(new[..., 128:], held[..., 128:])
    y = _ref64(xs[..., 32:96], wt, b)
    scale = np.abs(y).max()
    assert not np.array_equal(new, old)
    assert _rel(new[..., 64:128], old[..., 64:128], scale) < FORMS_BAR and _rel(new[..., 64:128], y, scale) < F64_BAR
    oracle = conv2d_nhwc(np.ascontiguousarray(xs[..., 32:96]), wt, b, stride=2, act=True)
    assert _rel(new[..., 64:128], oracle, np.abs(oracle).max()) < ORACLE_BAR


FRAME_HW = (432, 768)


def _frame(seed, hw=FRAME_HW):
    """A textured frame with bright rectangles (test_detector_gpu.py's)."""
    rng = np.random.default_rng(seed)
    h, w = hw
    yy, xx = np.mgrid[0:h, 0:w]
    base = 110 + 50 * np.sin(xx / 37.0) * np.cos(yy / 23.0)
    f = np.stack([base + 20 * rng.standard_normal((h, w)) for _ in range(3)], -1)
    for _ in range(25):
        x, y = rng.integers(0, w - 40), rng.integers(0, h - 20)
        f[y:y + rng.integers(8, 20), x:x + rng.integers(15, 40)] = rng.integers(150, 255, 3)
    return np.clip(f, 0, 255).astype(np.uint8)


LAYERS = ["model.0.conv", "model.1.conv", "model.2", "model.3.conv", "model.4", "model.5.conv", "model.6", "model.7.conv", "model.8", "model.9",
          "model.12", "model.15", "model.16.conv", "model.18", "model.19.conv", "model.21", "model.22.feat0", "model.22.feat1", "model.22.feat2"]


def test_detector_with_the_switch_on_and_off(gtx_ctx, monkeypatch):
    """One YOLOv8s detector at imgsz 384 built with the stride-2 layers on the new kernel and on the 32x32x16 one: every probed
    layer within the re-ordered-sum bar, detections identical in order and count; and with the new kernel a batch of two
    equals two single frames (test_detector_batch_equals_single's property on the split path)."""
    from geotrax_amd.detector import Detector
    from geotrax_amd.weights import synthetic_yolov8

    weights = synthetic_yolov8(seed=1, nc=4, scale="s", cls_bias=-3.0)
    frames = np.stack([_frame(0), _frame(1)])
    kw = dict(imgsz=384, half=False, rect=False, fp32_split=True, conf=0.25, iou=0.7, max_det=300, classes=[0, 1, 2, 3], agnostic_nms=True,
              max_batch=2, ctx=gtx_ctx)
    res = {}
    for form in ("0", "1"):
        monkeypatch.setenv("GTX_K32S2", form)
        det = Detector(weights, FRAME_HW, **kw)
        names = {r["kernel"] for r in det.profile(1, 1)}
        assert ("conv_k32s2_split_kernel" in names) == (form == "1"), names
        got = det.detect(frames[0])
        res[form] = (got, {name: det.layer_output(name) for name in LAYERS})
        if form == "1":
            singles = [got, det.detect(frames[1])]
            dptr = gtx_ctx.dev_alloc(frames.nbytes)
            try:
                gtx_ctx.dev_upload(dptr, frames)
                batch = det.detect_dev(dptr, 2)
            finally:
                gtx_ctx.dev_free(dptr)
            for s, bt in zip(singles, batch):
                np.testing.assert_array_equal(s.xyxy, bt.xyxy)
                np.testing.assert_array_equal(s.conf, bt.conf)
                np.testing.assert_array_equal(s.cls, bt.cls)
        det.close()
    (d0, l0), (d1, l1) = res["0"], res["1"]
    for name in LAYERS:
        err = _rel(l1[name], l0[name], np.abs(l0[name]).max() + 1e-6)
        assert err < FORMS_BAR, f"{name}: {err:.3e}"
    assert len(d1) == len(d0) > 0
    np.testing.assert_array_equal(d1.cls, d0.cls)
    np.testing.assert_allclose(d1.conf, d0.conf, atol=1e-5)
    np.testing.assert_allclose(d1.xyxy, d0.xyxy, atol=1e-2)
