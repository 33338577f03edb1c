"""YOLOv5u detectors on the HIP path (yolov5.yaml with the anchor-free Detect = model.24: a 6x6 stride-2 stem, C3 blocks, 1x1 Convs in
the neck): the stem launch alone against float64 (ops.stem6), the whole network at scales n and m against tests/yolov5u_ref.py, and
the extract chain.

Bars. The launch alone: tests/front_cases.py's, as for the 3x3 stem (tests/test_front_ops_gpu.py) -- the split-f16x3 form F64_BAR = 2e-6
of the layer's largest value against float64 on the pair format's values, the exact-fp32 form TOL_F32, the fp16 form TOL_F16 on
fp16-rounded pixels and weights. The whole network: tests/test_yolo11_gpu.py::_check_against_oracle's numbers (layers 2e-4 of the
layer's largest value, scores 1e-4, boxes rtol 2e-5 + 2e-3, kept confidences 1e-5, frame boxes 1e-2; `half: true`: 3e-2, 2e-2,
rtol 5e-3 + 0.5). The seeded weights of the whole-network cases are chosen on the restatement alone by
tests/test_yolo11_gpu.py::parity_weights' rule, which every case asserts on the CPU before it runs the GPU: fp32 and float64 runs of
the restatement keep the same anchors, their kept confidences lie within 2e-6 of each other and no class score is closer to `conf`
than 5e-6.

The stem kernels' workgroup tiles are 4 x 32 output pixels (matrix-core forms) and 8 x 32 (exact fp32): 38 x 140 (19 x 70 outputs)
crosses both by a partial tile in both axes."""
import argparse
import functools
import logging
from pathlib import Path

import numpy as np
import pytest

import front_cases as fc
from front_cases import F64_BAR, pairs, rel

pytestmark = pytest.mark.gpu

logger = logging.getLogger("test_yolov5u")
KW = dict(conf=0.25, iou=0.7, max_det=300, classes=[0, 1, 2, 3], agnostic_nms=True)
F16, F32, F32S = 0, 1, 2
# kernel form -> (dtype, the format its values live in, (rtol, atol) or None for the split bar)
FORMS = {"mfma_f16": (F16, "f16", fc.TOL_F16), "exact_f32": (F32, "f32", fc.TOL_F32), "split": (F32S, "split", None)}
TILE_ROWS, TILE_ROWS_F32, TILE_COLS = 4, 8, 32      # csrc/yolo_tables.hpp kStem6Rows / kStem6RowsF32 / kStem6Cols
SIZES = [(2, 2), (4, 64), (7, 67), (20, 200), (21, 193), (38, 140)]
_HO, _WO = (SIZES[-1][0] - 2) // 2 + 1, (SIZES[-1][1] - 2) // 2 + 1
assert _HO > TILE_ROWS_F32 and _HO % TILE_ROWS and _HO % TILE_ROWS_F32 and _WO > TILE_COLS and _WO % TILE_COLS


# ============================================================================ the stem launch alone
def _stem6_weights(seed, c0):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((108, c0)) / np.sqrt(108)).astype(np.float32), (rng.standard_normal(c0) * 0.1).astype(np.float32)


def _conv6_64(px, w108, bias):
    """SiLU(conv 6x6 / 2 / pad 2 + bias) in float64 on NHWC pixel values [n, h, w, 3]; w108 [108, c0] tap-major"""
    import torch
    from yolov5u_ref import oihw_of

    y = torch.nn.functional.conv2d(torch.from_numpy(np.ascontiguousarray(px, dtype=np.float64)).permute(0, 3, 1, 2),
                                   torch.from_numpy(oihw_of(np.asarray(w108, np.float64))), torch.from_numpy(np.asarray(bias, np.float64)),
                                   stride=2, padding=2)
    return fc.silu(y.permute(0, 2, 3, 1).numpy())


@functools.lru_cache(maxsize=None)
def _stem6_case(h, w, c0, fmt):
    """Two frames (fc.images), weights, and the float64 reference on the values the form holds: fc.px_values for the pixels, fp16-rounded
    weights for the packed fp16 form, fp32 weights otherwise (the split kernel's 22-bit hi + lo split of them is what its bar covers)."""
    img = fc.images(7 * h + w, h, w)
    w108, bias = _stem6_weights(100 + c0, c0)
    wr = w108.astype(np.float16).astype(np.float32) if fmt == "f16" else w108
    ref = _conv6_64(fc.px_values(img, fmt), wr, bias)
    for a in (img, w108, bias, ref):
        a.setflags(write=False)
    return img, w108, bias, ref


@pytest.mark.parametrize("c0", [16, 48, 80])
@pytest.mark.parametrize("form", list(FORMS))
def test_stem6_forms_against_float64(gtx_ctx, form, c0):
    """Batch 2 (random bytes; a frame inside a 255 and a 0 ring, right where the 2-pixel padding bites) on a single output pixel, one
    exact tile row, odd sides, several tiles per row, and a map that crosses the workgroup tile by a partial tile in both axes. The
    split form's output is legal pair format; a batch of two equals two single launches bit for bit."""
    from geotrax_amd import ops

    dtype, fmt, tol = FORMS[form]
    for h, w in SIZES:
        img, w108, bias, ref = _stem6_case(h, w, c0, fmt)
        got = ops.stem6(img, w108, bias, dtype=dtype, ctx=gtx_ctx)
        assert got.shape == ref.shape == (2, (h - 2) // 2 + 1, (w - 2) // 2 + 1, c0)
        err = rel(got, ref, np.abs(ref).max())
        if tol is None:
            print(f"stem6 {form} c0={c0} {h}x{w}: float64 {err:.2e} (bar {F64_BAR:.0e})")
            assert err < F64_BAR
            np.testing.assert_array_equal(pairs(got), got.astype(np.float64))
        else:
            print(f"stem6 {form} c0={c0} {h}x{w}: float64 {err:.2e} of max, {fc.tol_ratio(got, ref, tol):.3f} of rtol/atol {tol[0]:.0e}")
            np.testing.assert_allclose(got.astype(np.float64), ref, rtol=tol[0], atol=tol[1])
        for i in range(2):
            np.testing.assert_array_equal(ops.stem6(img[i:i + 1], w108, bias, dtype=dtype, ctx=gtx_ctx)[0], got[i])


def _tap_map_case(h, w):
    """An image whose 108 values under any 6 x 6 window all differ (2 * ((y % 6) * 6 + x % 6) * 3 + 2 * colour, + a bit that changes from
    6 x 6 cell to cell: at most 215; the second frame is 255 minus the first), and one-hot weights: channel k of 108 reads row k of the
    weight layout -- tap (ky, kx) = divmod(k // 3, 6) of colour k % 3 -- and nothing else."""
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.zeros((2, h, w, 4), np.uint8)
    for ch in range(3):
        img[0, ..., ch] = 2 * (((yy % 6) * 6 + xx % 6) * 3 + ch) + (yy // 6 + xx // 6) % 2
        img[1, ..., ch] = 255 - img[0, ..., ch]
    win = np.lib.stride_tricks.sliding_window_view(img[0, ..., :3], (6, 6), axis=(0, 1))
    assert all(len(np.unique(win[y, x])) == 108 for y in range(0, h - 5, 5) for x in range(0, w - 5, 7))
    return img, np.eye(108, dtype=np.float32)


def _tap_map64(img, fmt):
    """SiLU of the selected neighbour (0 beyond the border), by indexing: no convolution involved. [n, ho, wo, 108]"""
    px = fc.px_values(img, fmt)
    n, h, w, _ = px.shape
    ho, wo = (h - 2) // 2 + 1, (w - 2) // 2 + 1
    padded = np.zeros((n, 2 * ho + 4, 2 * wo + 4, 3))
    padded[:, 2:h + 2, 2:w + 2] = px
    out = np.zeros((n, ho, wo, 108))
    for k in range(108):
        ky, kx = divmod(k // 3, 6)
        out[..., k] = padded[:, ky:ky + 2 * ho:2, kx:kx + 2 * wo:2, k % 3]       # padded row 2 oy + ky = image row 2 oy - 2 + ky
    return fc.silu(out)


@pytest.mark.parametrize("form", list(FORMS))
def test_stem6_tap_map(gtx_ctx, form):
    """One-hot weights, 108 channels in chunks of 48 (the last chunk's spare channels read nothing): every output must be SiLU of
    exactly its neighbour, or of 0 beyond the border -- a transposed tap, a swapped colour or an off-by-one in the asymmetric footprint
    (two rows above, three below) cannot pass. 21 x 193: border, interior and partial tiles, odd sides."""
    from geotrax_amd import ops

    dtype, fmt, tol = FORMS[form]
    img, eye = _tap_map_case(21, 193)
    ref = _tap_map64(img, fmt)
    got = []
    for k0 in range(0, 108, 48):
        w108 = np.zeros((108, 48), np.float32)
        w108[:, :min(48, 108 - k0)] = eye[:, k0:k0 + 48]
        y = ops.stem6(img, w108, np.zeros(48, np.float32), dtype=dtype, ctx=gtx_ctx)
        assert not y[..., 108 - k0:].any()
        got.append(y[..., :108 - k0])
    got = np.concatenate(got, -1)
    assert got.shape == ref.shape
    err = rel(got, ref, np.abs(ref).max())
    print(f"stem6 tap map {form}: float64 {err:.2e}")
    if tol is None:
        assert err < F64_BAR
    else:
        np.testing.assert_allclose(got.astype(np.float64), ref, rtol=tol[0], atol=tol[1])
    border = ref[0, 0, :, 0:6] == 0                                         # first output row, taps of window rows 0 / 1: beyond the border
    assert border.all() and not got[0, 0, :, 0:6].any()


def test_stem6_refuses_what_it_cannot_run(gtx_ctx):
    from geotrax_amd import ops
    from geotrax_amd._lib import GtxError

    w108, bias = _stem6_weights(0, 16)
    for img, wt, b in ((np.zeros((1, 1, 8, 4), np.uint8), w108, bias), (np.zeros((1, 8, 1, 4), np.uint8), w108, bias),
                       (np.zeros((1, 8, 8, 4), np.uint8), np.zeros((108, 24), np.float32), np.zeros(24, np.float32)),
                       (np.zeros((1, 8, 8, 4), np.uint8), np.zeros((108, 112), np.float32), np.zeros(112, np.float32))):
        with pytest.raises(GtxError, match="stem6"):
            ops.stem6(img, wt, b, dtype=F32S, ctx=gtx_ctx)
    with pytest.raises(GtxError, match="dtype"):
        ops.stem6(np.zeros((1, 8, 8, 4), np.uint8), w108, bias, dtype=7, ctx=gtx_ctx)
    assert ops.stem6(np.zeros((1, 8, 8, 4), np.uint8), w108, bias, dtype=F32, ctx=gtx_ctx).shape == (1, 4, 4, 16)   # the context still works


# ============================================================================ the whole network
LAYERS = ["model.0.conv", "model.1.conv", "model.2.cv1.conv", "model.2.cv2.conv", "model.2", "model.4", "model.6", "model.8", "model.9", "model.10.conv",
          "model.13", "model.14.conv", "model.17", "model.18.conv", "model.20", "model.23", "model.24.feat0", "model.24.feat1", "model.24.feat2"]
SHAPES = {"64": ((64, 64), 64, False), "96x160": ((90, 160), 160, True)}      # frame size, imgsz, rect: 96 x 160 has 3 padding rows above and below
# (seed, gain) per (scale, shape): chosen on the restatement alone by the parity rule in the module docstring (seeds 1-6; scale n at the
# generator's gain 1.7, scale m -- 2 / 4 / 6 / 2 residual bottlenecks per C3 -- at 1.3: at 1.7 its activations reach 8e4 to 4e5, beyond fp16.
# The chosen ones stay below 130 / 11 / 3 / 3 with kept-confidence spreads of 1.2e-6 / 9.3e-7 / 2.5e-8 / 1.3e-7, threshold margins of
# 5.0e-3 / 4.5e-4 / 2.1e-5 / 9.5e-6 and fp16-emulation spreads of 2.9e-3 / 4.4e-3 / 1.2e-3 / 1.3e-3)
SEEDS = {("n", "64"): (2, 1.7), ("n", "96x160"): (3, 1.7), ("m", "64"): (1, 1.3), ("m", "96x160"): (5, 1.3)}
# anchors per level calibrated to clear conf (of 64 / 16 / 4 and 240 / 60 / 15)
KEEP = {("n", "64"): (8, 3, 1), ("m", "64"): (8, 3, 1), ("n", "96x160"): (20, 8, 2), ("m", "96x160"): (20, 8, 2)}
# `half: true` adds one figure to the rule, the restatement's own (tests/test_yolo12_gpu.py): its fp16 emulation against its fp32 run, per
# probed layer and relative to the layer's largest value, must stay below a third of the 3e-2 bar
HALF_SPREAD = 1e-2


def _frame(hw, seed=0):
    rng = np.random.default_rng(seed)
    h, w = hw
    yy, xx = np.mgrid[0:h, 0:w]
    f = np.stack([110 + 50 * np.sin(xx / 7.0) * np.cos(yy / 5.0) + 20 * rng.standard_normal((h, w)) for _ in range(3)], -1)
    for _ in range(6):
        x, y = rng.integers(0, w - 20), rng.integers(0, h - 10)
        f[y:y + rng.integers(4, 10), x:x + rng.integers(8, 20)] = rng.integers(150, 255, 3)
    return np.clip(f, 0, 255).astype(np.uint8)


def _pair(got, ref_xyxy, ref_conf):
    """For every kept box the index of the restatement's box it pairs with, one to one, at the least total distance (coordinates in
    pixels + confidence differences in units of 1e-5), as in tests/test_yolo12_gpu.py"""
    from scipy.optimize import linear_sum_assignment

    assert len(got) == len(ref_conf) > 0
    d = np.abs(got.xyxy[:, None, :] - ref_xyxy[None, :, :]).max(-1) + 1e5 * np.abs(got.conf[:, None] - ref_conf[None, :])
    i, j = linear_sum_assignment(d)
    assert i.tolist() == list(range(len(got)))
    return j


def _ref64(weights, x):
    from yolov5u_ref import Yolov5uRef

    r = Yolov5uRef(weights)
    r.t = {k: v.double() for k, v in r.t.items()}
    return r, r.forward(x.double())[0].numpy()


@functools.lru_cache(maxsize=None)
def _case(scale, shape):
    """Weights (the last class convs calibrated on the restatement's own float64 logits so that KEEP anchors per level clear conf), frame,
    network input and the parity rule's three figures, computed once on the CPU and shared."""
    from geotrax_amd.weights import synthetic_yolov5u
    from oracle.yolov8_ref import letterbox, non_max_suppression
    from yolov5u_ref import Yolov5uRef

    hw, imgsz, rect = SHAPES[shape]
    seed, gain = SEEDS[scale, shape]
    frame = _frame(hw)
    x, _ = letterbox(frame, imgsz, rect)
    w = synthetic_yolov5u(seed=seed, nc=4, scale=scale, box_weight_scale=0.1, gain=gain)
    r64, _ = _ref64(w, x)
    for l, k in enumerate(KEEP[scale, shape]):          # tests/test_yolo11_gpu.py::_calibrated on the restatement's float64 logits: each level's last class
        lv = np.sort(r64.acts[f"model.24.cls{l}"][0].amax(0).flatten().numpy())[::-1]   # conv scaled down to logits of at most 3 and shifted
        f = min(1.0, 3.0 / max(np.abs(lv).max(), 1e-6))
        delta = np.log(KW["conf"] / (1 - KW["conf"])) - f * 0.5 * (lv[k - 1] + lv[k])
        name = f"model.24.cv3.{l}.2"
        w[name + ".weight"] = (w[name + ".weight"] * np.float32(f)).astype(np.float32)
        w[name + ".bias"] = (w[name + ".bias"] * np.float32(f) + np.float32(delta)).astype(np.float32)
    a, b = Yolov5uRef(w).forward(x)[0].numpy(), _ref64(w, x)[1]
    nms = lambda q: non_max_suppression(q.astype(np.float32), KW["conf"], KW["iou"], KW["classes"], True, KW["max_det"], return_idx=True)[1]
    ia, ib = nms(a), nms(b)
    same = np.array_equal(np.sort(ia), np.sort(ib))
    spread = float(np.abs(a[ia, 4:].max(1) - b[ia, 4:].max(1)).max()) if same and len(ia) else np.inf
    return w, frame, x, (same, spread, float(np.abs(a[:, 4:] - KW["conf"]).min()), len(ia))


@functools.lru_cache(maxsize=None)
def _reference(scale, shape, half):
    """The restatement's pass (fp32, or with the fp16 emulation), shared by the paths that compare with it and left unchanged"""
    from oracle.yolov8_ref import detect, letterbox
    from yolov5u_ref import Yolov5uRef

    w, frame, _, _ = _case(scale, shape)
    hw, imgsz, rect = SHAPES[shape]
    ref = Yolov5uRef(w, emulate_half=half)
    x, g = letterbox(frame, imgsz, rect, half=half)
    raw = ref.forward(x)[0].numpy()
    acts = {k: ref.acts[k][0].permute(1, 2, 0).numpy() for k in LAYERS}
    rows = detect(ref, frame, imgsz, rect, KW["conf"], KW["iou"], KW["classes"], True, KW["max_det"])
    return raw, acts, rows, (g["net_h"], g["net_w"])


@pytest.mark.parametrize("path", ["split", "exact", "half"])
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("scale", ["n", "m"])
def test_yolov5u_matches_restatement(gtx_ctx, scale, shape, path):
    from geotrax_amd.detector import Detector

    w, frame, _, (same, spread, margin, kept) = _case(scale, shape)
    print(f"restatement fp32 vs float64: {kept} kept, confidences {spread:.1e}, threshold margin {margin:.1e}")
    assert same and kept >= 3 and spread < 2e-6 and margin > 5e-6           # the case is what the parity rule asks for
    half = path == "half"
    hw, imgsz, rect = SHAPES[shape]
    ref_raw, acts, (xyxy, conf, cls), net_hw = _reference(scale, shape, half)
    if half:
        a32 = _reference(scale, shape, False)[1]
        own = max(float(np.abs(acts[k] - a32[k]).max() / (np.abs(a32[k]).max() + 1e-6)) for k in acts)
        print(f"restatement fp16 emulation vs fp32, layers: {own:.1e}")
        assert own < HALF_SPREAD
    det = Detector(w, hw, imgsz=imgsz, rect=rect, half=half, fp32_split=path == "split", ctx=gtx_ctx, **KW)
    assert det.graph == "yolov5u" and det.net_hw == net_hw and det.net_hw == ((64, 64) if shape == "64" else (96, 160))
    got = det.detect(frame)
    assert not det.fell_back()
    rel_bar = 3e-2 if half else 2e-4
    for name in LAYERS:
        a, r = det.layer_output(name), acts[name]
        assert a.shape == r.shape, name
        err = np.abs(a - r).max() / (np.abs(r).max() + 1e-6)
        print(f"{name}: rel-to-max error {err:.3e}")
        assert err < rel_bar, f"{name}: rel-to-max error {err:.3e}"
    raw = det.raw_output()
    assert raw.shape == ref_raw.shape
    print("scores", np.abs(raw[:, 4:] - ref_raw[:, 4:]).max(), "boxes", np.abs(raw[:, :4] - ref_raw[:, :4]).max())
    np.testing.assert_allclose(raw[:, 4:], ref_raw[:, 4:], atol=2e-2 if half else 1e-4)
    np.testing.assert_allclose(raw[:, :4], ref_raw[:, :4], rtol=5e-3 if half else 2e-5, atol=0.5 if half else 2e-3)
    if not half:                                                                # the final rows equal the restatement's after NMS
        j = _pair(got, xyxy, conf)
        np.testing.assert_array_equal(got.cls, cls[j])
        np.testing.assert_allclose(got.conf, conf[j], atol=1e-5)
        np.testing.assert_allclose(got.xyxy, xyxy[j], atol=1e-2)
    else:
        assert abs(len(got) - len(conf)) <= max(3, len(conf) // 10)
    det.close()


@pytest.mark.parametrize("scale", ["n", "m"])
def test_pad_skip_on_and_off_are_bit_identical(gtx_ctx, monkeypatch, scale):
    """A 90 x 160 frame letterboxed into 160 x 160 (35 constant rows above and below), default path: the row plan goes through the 6x6
    stem's footprint (two rows above, three below) and leaves tile rows out of the backbone's launches; a detector with the plan
    switched off gives the same outputs bit for bit. (At 96 x 160, 3 padding rows, no 8-row tile is constant and nothing is skipped.)"""
    from geotrax_amd.detector import Detector

    w, frame, _, _ = _case(scale, "96x160")
    hw, imgsz = SHAPES["96x160"][0], 160
    det = Detector(w, hw, imgsz=imgsz, rect=False, ctx=gtx_ctx, **KW)
    with monkeypatch.context() as mp:
        mp.setenv("GTX_PAD_SKIP", "0")
        plain = Detector(w, hw, imgsz=imgsz, rect=False, ctx=gtx_ctx, **KW)
    on, skipped, total = det.pad_skip()
    print("pad skip:", det.pad_skip())
    assert det.net_hw == (160, 160) and on is True and 0 < skipped < total and plain.pad_skip()[0] is False
    for f in (frame, _frame(hw, 5)):
        a, b = det.detect(f), plain.detect(f)
        assert a.xyxy.tobytes() == b.xyxy.tobytes() and a.conf.tobytes() == b.conf.tobytes()
        assert det.raw_output().tobytes() == plain.raw_output().tobytes()
        for name in ("model.0.conv", "model.1.conv", "model.2", "model.4", "model.6"):
            assert det.layer_output(name).tobytes() == plain.layer_output(name).tobytes(), name
    det.close(); plain.close()


def test_object_features_read_detects_inputs(gtx_ctx):
    """`with_reid: true, model: auto`: Detect's inputs (model.17 / 20 / 23) are ordinary maps, the vectors are obj_feats_table()'s"""
    from geotrax_amd.detector import Detector
    from oracle.yolov8_ref import detect
    from yolov5u_ref import Yolov5uRef

    w, frame, _, _ = _case("n", "96x160")
    hw, imgsz, rect = SHAPES["96x160"]
    det = Detector(w, hw, imgsz=imgsz, rect=rect, obj_feats=True, ctx=gtx_ctx, **KW)
    d = det.detect(frame)
    xyxy, conf, cls, feats = detect(Yolov5uRef(w), frame, imgsz, rect, KW["conf"], KW["iou"], KW["classes"], True, KW["max_det"], return_feats=True)
    assert d.feats.shape == feats.shape == (len(conf), 64) and len(conf) > 0
    np.testing.assert_allclose(d.feats, feats[_pair(d, xyxy, conf)], atol=2e-4 * max(1.0, float(np.abs(feats).max())))
    det.close()


SAT_GAIN = 2.0          # the restatement's largest activation: 1.1e10


def test_saturation_falls_back_to_exact(gtx_ctx):
    """Scale m at gain SAT_GAIN leaves fp16's range somewhere in the stack: the split-f16x3 detector re-runs the pass on its exact-fp32
    twin (the same YOLOv5u graph, the exact-fp32 stem kernel included) and from then on equals the exact detector bit for bit."""
    from geotrax_amd.detector import Detector
    from geotrax_amd.weights import synthetic_yolov5u
    from oracle.yolov8_ref import letterbox
    from yolov5u_ref import Yolov5uRef

    hw, imgsz, rect = SHAPES["96x160"]
    w = synthetic_yolov5u(seed=1, nc=4, scale="m", cls_bias=-3.0, gain=SAT_GAIN)
    frame = _frame(hw)
    ref = Yolov5uRef(w)
    ref.forward(letterbox(frame, imgsz, rect)[0])
    peak = max(float(v.abs().max()) for v in ref.acts.values())
    print("largest activation", peak)
    assert 65504.0 < peak < 1e30                                     # the case is what it claims to be
    kw = dict(imgsz=imgsz, rect=rect, ctx=gtx_ctx, **KW)
    det = Detector(w, hw, fp32_split=True, **kw)
    first = det.detect(frame)
    assert det.saturated() and det.fell_back()
    exact = Detector(w, hw, fp32_split=False, **kw)
    assert first.conf.tobytes() == exact.detect(frame).conf.tobytes()
    assert det.detect(frame).xyxy.tobytes() == exact.detect(frame).xyxy.tobytes()
    assert det.raw_output().tobytes() == exact.raw_output().tobytes()
    det.close(); exact.close()


def test_end2end_true_is_refused(gtx_ctx):
    """`end2end: true` asks for a one-to-one head; yolov5.yaml's Detect has none, as every family but YOLOv10 / YOLO26"""
    from geotrax_amd.detector import Detector

    w, _, _, _ = _case("n", "64")
    with pytest.raises(ValueError, match="end2end"):
        Detector(w, (64, 64), imgsz=64, end2end=True, ctx=gtx_ctx, **KW)
    Detector(w, (64, 64), imgsz=64, end2end=False, ctx=gtx_ctx, **KW).close()


# ============================================================================ through the product
N_CLIP, CLIP_HW, CLIP_IMGSZ = 6, (96, 160), 160


def _clip_and_cfg(tmp_path, gtx_ctx):
    import test_extract_gpu as te
    import yaml
    from geotrax_amd.detector import Detector
    from geotrax_amd.synth import make_scene
    from geotrax_amd.weights import calibrate_cls_bias, save_weights, synthetic_yolov5u

    scene = make_scene(seed=2, h=CLIP_HW[0], w=CLIP_HW[1])
    frames = np.stack([scene.render(t, 150) for t in range(0, N_CLIP * 12, 12)])
    clip = tmp_path / "clip.npy"
    np.save(clip, frames)
    w = synthetic_yolov5u(seed=1, nc=4, scale="n", gain=1.7, box_weight_scale=0.002)
    det = Detector(w, CLIP_HW, imgsz=CLIP_IMGSZ, rect=True, ctx=gtx_ctx)
    det.detect(frames[0])
    w = calibrate_cls_bias(w, det.raw_output(logits=True)[:, 4:], 0.25, 12)
    det.close()
    path = tmp_path / "yolov5nu.safetensors"
    save_weights(w, path)
    path.with_suffix(".names.yaml").write_text("{0: car, 1: bus, 2: truck, 3: motorcycle}\n")
    cfg_path, cfg = te._cfg_file(tmp_path, path, tracker="bytetrack")
    cfg["ultralytics"]["imgsz"] = CLIP_IMGSZ
    cfg["stabilo"].update(downsample_ratio=1.0, mask_use=False)
    cfg_path.write_text(yaml.safe_dump(cfg))
    return clip, cfg_path


def _setup(clip, cfg_path):
    from geotrax_amd import extract as ex
    from geotrax_amd.config_utils import load_config_all

    args = argparse.Namespace(source=str(clip), cfg=Path(cfg_path), output_folder=None, log_path=None, verbose=False, model=None,
                              class_names=None, conf=None, classes=None, cut_frame_left=None, cut_frame_right=None, interpolate=None)
    model = ex.load_detector(args, logger)
    config = load_config_all(args, logger, model_names=model.names)
    args.cut_frame_left, args.cut_frame_right = 0, None
    return model, config


def test_extract_engine_equals_the_frame_at_a_time_loop(gtx_ctx, tmp_path):
    """The extract chain on a YOLOv5u file (ExtractEngine: batched, pipelined detector streams, ByteTrack + stabilizer) gives the
    tables of the blocking loop, which is YOLO(file).track frame by frame, byte for byte."""
    from geotrax_amd import extract as ex

    clip, cfg_path = _clip_and_cfg(tmp_path, gtx_ctx)
    model, config = _setup(clip, cfg_path)
    assert model.model.yaml_file == "yolov5n.yaml"
    t1, h1 = ex.track_with_model(model, config, logger)
    model, config = _setup(clip, cfg_path)
    config["main"].setdefault("engine", {})["pipelined"] = False
    t2, h2 = ex.track_with_model_blocking(model, config, logger)
    assert len(t1) > 0
    assert t1.dtype == t2.dtype and t1.tobytes() == t2.tobytes() and h1.tobytes() == h2.tobytes()
