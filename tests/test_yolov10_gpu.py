"""YOLOv10 detectors on the HIP path (SCDown, PSA = model.10, C2fCIB with the fused RepVGGDW 7x7, v10Detect's one-to-one head and the
NMS-free tail of csrc/v10_select.hip) against tests/yolov10_ref.py: the depthwise kernels (bit for bit without activation), every probed layer, the raw
one-to-one output and the final rows on the split-f16x3, exact-fp32 and half paths, both heads, batches, the asynchronous pair, the
saturation fallback, the ultralytics-shaped wrapper, the extract chain (ExtractEngine) and the frame-sharded run. The bars are tests/test_yolo11_gpu.py::_check_against_oracle's (themselves
tests/test_p2_gpu.py's). Smallest shapes: scale n, nc = 4, imgsz 128 on a 96 x 160 frame (a 4 x 4 P5 map, PSA with c = 128 and 2
heads, the small-map attention kernel); imgsz 256 for the tiled attention kernel; scale s for the large-kernel CIB at model.8.

Run as a script (`python -m torch.distributed.run ... tests/test_yolov10_gpu.py clip cfg out`) this file is one rank of the frame-sharded run."""
import argparse
import logging
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from test_yolo11_gpu import _frame

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
logger = logging.getLogger("test_yolov10")

FRAME_HW = (96, 160)
KW = dict(conf=0.25, iou=0.7, max_det=300, classes=[0, 1, 2, 3], agnostic_nms=True)
LAYERS = ["model.2", "model.5", "model.6", "model.8", "model.9", "model.10.attn.qkv.conv", "model.10.attn.out", "model.10", "model.13", "model.16",
          "model.19", "model.20", "model.22", "model.23.feat0", "model.23.feat1", "model.23.feat2"]
# the bars of tests/test_yolo11_gpu.py::_check_against_oracle: (fp32 grade, half)
LAYER_REL = (2e-4, 3e-2)
SCORE_ATOL = (1e-4, 2e-2)
BOX_RTOL, BOX_ATOL = (2e-5, 5e-3), (2e-3, 0.5)
CONF_ATOL, XYXY_ATOL = 1e-5, 1e-2

# Seeded cases, picked on the CPU by the rule of tests/test_yolo11_gpu.py::parity_weights (asserted by _rule below before anything is
# compared): a seeded YOLOv10 stack either amplifies (activations of 1e3-1e4, saturated scores that tie) or stays near 2 with class
# logits within +-0.2 of their bias; the calm ones are taken and the bias decides how many of the A x 4 scores clear conf = 0.25.
#              scale imgsz seed gain  cls_bias   scores above conf (restatement)
CASES = {
    "n128_many": ("n", 128, 7, 1.7, -1.2),     # 312 of 1344: the 300-cut bites
    "n128_few": ("n", 128, 7, 1.7, -1.25),     # 211: the gate decides alone
    "n256": ("n", 256, 2, 1.6, -1.0),          # 5156 of 5376; an 8 x 8 P5 map: the tiled attention kernel
    "s128": ("s", 128, 2, 1.6, -1.2),          # 49; C2fCIB with the 7x7 at model.8 as well
}


def _case(name):
    from geotrax_amd.weights import synthetic_yolov10

    scale, imgsz, seed, gain, bias = CASES[name]
    return synthetic_yolov10(seed=seed, nc=4, scale=scale, cls_bias=bias, gain=gain, box_weight_scale=0.1), imgsz


_REF = {}


def _ref(name):
    """(weights, imgsz, fp32 restatement after its forward pass, its raw output, the letterboxed input): computed once per case"""
    if name not in _REF:
        from oracle.yolov8_ref import letterbox
        from yolov10_ref import Yolov10Ref

        w, imgsz = _case(name)
        x, _ = letterbox(_frame(0, FRAME_HW), imgsz, False)
        ref = Yolov10Ref(w)
        _REF[name] = (w, imgsz, ref, ref.forward(x)[0].numpy(), x)
    return _REF[name]


def _rule(name):
    """The written rule: the restatement's own fp32-vs-float64 spread is at most a fifth of every bar, no score within 5e-6 of conf,
    no two scores within 5e-6 of each other at the 300-cut. Returns the number of scores above conf."""
    from yolov10_ref import Yolov10Ref, postprocess

    w, imgsz, r32, a, x = _ref(name)
    r64 = Yolov10Ref(w).double()
    b = r64.forward(x.double())[0].numpy()
    lay = max(float((r32.acts[n].double() - r64.acts[n]).abs().max() / (r64.acts[n].abs().max() + 1e-6)) for n in LAYERS)
    sc = float(np.abs(a[:, 4:] - b[:, 4:]).max())
    bx = float((np.abs(a[:, :4] - b[:, :4]) / (BOX_RTOL[0] * np.abs(b[:, :4]) + BOX_ATOL[0])).max())
    ra, ia = postprocess(a, KW["conf"], None, 300, return_idx=True)
    rb, ib = postprocess(b.astype(np.float32), KW["conf"], None, 300, return_idx=True)
    flat = np.sort(a[:, 4:].reshape(-1))[::-1]
    margin, gap = float(np.abs(flat - KW["conf"]).min()), float(flat[299] - flat[300])
    print(f"{name}: restatement fp32 vs float64: layers {lay:.1e}, scores {sc:.1e}, boxes {bx:.2f} of the bar, threshold margin {margin:.1e}, gap at the cut {gap:.1e}")
    assert lay <= LAYER_REL[0] / 5 and sc <= SCORE_ATOL[0] / 5 and bx <= 0.2
    assert len(ra) == len(rb) and np.array_equal(np.sort(ia), np.sort(ib)) and len(ra) > 0
    assert float(np.abs(np.sort(ra[:, 4]) - np.sort(rb[:, 4])).max()) <= CONF_ATOL / 5
    assert margin > 5e-6 and gap > 5e-6
    return int((flat > KW["conf"]).sum())


def _by_position(xyxy, conf, cls):
    o = np.lexsort((xyxy[:, 3], xyxy[:, 2], xyxy[:, 1], xyxy[:, 0], cls))
    return xyxy[o], conf[o], cls[o]


def _check(det, name, half=False):
    """Layers, raw one-to-one output and final rows of det on the case's frame against the restatement"""
    from oracle.yolov8_ref import letterbox
    from yolov10_ref import Yolov10Ref, detect

    w, imgsz, ref, ref_raw, _ = _ref(name)
    frame = _frame(0, FRAME_HW)
    if half:
        ref = Yolov10Ref(w, emulate_half=True)
        ref_raw = ref.forward(letterbox(frame, imgsz, False, half=True)[0])[0].numpy()
    h = int(half)
    got = det.detect(frame)
    for lname in LAYERS:
        a, r = det.layer_output(lname), ref.acts[lname][0].permute(1, 2, 0).numpy()
        assert a.shape == r.shape, lname
        err = np.abs(a - r).max() / (np.abs(r).max() + 1e-6)
        print(f"{lname}: rel-to-max error {err:.3e}")
        assert err < LAYER_REL[h], f"{lname}: rel-to-max error {err:.3e}"
    raw = det.raw_output()
    assert raw.shape == ref_raw.shape
    print("scores", np.abs(raw[:, 4:] - ref_raw[:, 4:]).max(), "boxes", np.abs(raw[:, :4] - ref_raw[:, :4]).max())
    np.testing.assert_allclose(raw[:, 4:], ref_raw[:, 4:], atol=SCORE_ATOL[h])
    np.testing.assert_allclose(raw[:, :4], ref_raw[:, :4], rtol=BOX_RTOL[h], atol=BOX_ATOL[h])
    xyxy, conf, cls = detect(ref, frame, imgsz, False, KW["conf"], KW["classes"], KW["max_det"])
    print(f"{name}: {len(got)} rows, restatement {len(conf)}")
    if half:                                        # fp16 scores move across conf and the cut: test_yolo11_gpu's half branch, restated
        assert abs(len(got) - len(conf)) <= max(3, len(conf) // 10)
        area = (xyxy[:, 2] - xyxy[:, 0]) * (xyxy[:, 3] - xyxy[:, 1])
        xyxy = xyxy[area > 1]
        matched = 0
        for b in xyxy:
            ix1, iy1 = np.maximum(got.xyxy[:, 0], b[0]), np.maximum(got.xyxy[:, 1], b[1])
            ix2, iy2 = np.minimum(got.xyxy[:, 2], b[2]), np.minimum(got.xyxy[:, 3], b[3])
            inter = np.clip(ix2 - ix1, 0, None) * np.clip(iy2 - iy1, 0, None)
            a = (got.xyxy[:, 2] - got.xyxy[:, 0]) * (got.xyxy[:, 3] - got.xyxy[:, 1])
            matched += (inter / (a + (b[2] - b[0]) * (b[3] - b[1]) - inter + 1e-9)).max() > 0.7
        print(f"{name}: half path, {matched} of {len(xyxy)} restatement boxes matched at IoU > 0.7")
        assert len(xyxy) > 0 and matched >= 0.9 * len(xyxy)
        return got
    assert len(got) == len(conf) > 0
    assert np.all(np.diff(got.conf) <= 0)           # sorted by score
    # scores of neighbouring rows lie within fp32 summation noise of each other: rows are paired by position, not by rank
    gx, gc, gk = _by_position(got.xyxy, got.conf, got.cls)
    rx, rc, rk = _by_position(xyxy, conf, cls)
    np.testing.assert_array_equal(gk, rk)
    np.testing.assert_allclose(gc, rc, atol=CONF_ATOL)
    np.testing.assert_allclose(gx, rx, atol=XYXY_ATOL)
    return got


# ---------------------------------------------------------------------------- the depthwise kernels, bit for bit
def _pairs(x):
    """fp32 -> what the split path's pair format holds: hi = fp16(x), lo = fp16(x - hi); hi + lo in fp32"""
    hi = x.astype(np.float16)
    lo = (x - hi.astype(np.float32)).astype(np.float16)
    return hi.astype(np.float32) + lo.astype(np.float32)


def _dw_loop(x, w, b, stride, res=None):
    """bias, then one fused multiply-add per tap in (ky, kx) order, fp32 (the product is exact in float64; one rounding per step)"""
    n, h, wd, c = x.shape
    k = w.shape[-1]
    ho, wo = (h - 1) // stride + 1, (wd - 1) // stride + 1
    out = np.zeros((n, ho, wo, c), np.float32)
    for oy in range(ho):
        for ox in range(wo):
            acc = np.broadcast_to(b, (n, c)).astype(np.float32)
            for ky in range(k):
                for kx in range(k):
                    iy, ix = oy * stride - k // 2 + ky, ox * stride - k // 2 + kx
                    if 0 <= iy < h and 0 <= ix < wd:
                        acc = (x[:, iy, ix].astype(np.float64) * w[:, 0, ky, kx].astype(np.float64) + acc.astype(np.float64)).astype(np.float32)
            out[:, oy, ox] = acc
    return out if res is None else out + res


@pytest.mark.parametrize("fmt", ["split", "f32", "f16"])
@pytest.mark.parametrize("k,stride,c", [(7, 1, 48), (7, 1, 64), (3, 2, 48), (3, 1, 64), (3, 1, 40)])
def test_depthwise_kernels(gtx_ctx, fmt, k, stride, c):
    """13 x 19 maps (odd sizes, two tiles each way, every border): the 7x7 on 48 channels (the per-thread kernel) and 64 (the LDS-tiled
    one), the stride-2 form without activation, and the residual epilogue. Without activation the output is the numpy loop's bit for
    bit in every format; with SiLU it is within the activation's own error: v_exp_f32 and v_rcp_f32 are 1-ulp approximations and two
    multiplications follow, 8 * 2^-24 relative (fp16 output: half an ulp of fp16 on top)."""
    from geotrax_amd import ops

    rng = np.random.default_rng(k * 100 + c + stride)
    # values on a binary grid (x, r: 2^-6 within +-4; w, b: 2^-8): every partial sum is exact in fp32, so the float64 emulation of
    # the fused multiply-add below cannot round twice
    grid = lambda v, q, lim: (np.clip(np.round(v * q), -lim * q, lim * q) / q).astype(np.float32)
    x = grid(rng.normal(0, 1, (2, 13, 19, c)), 64, 4)
    w = grid(rng.normal(0, 1 / k, (c, 1, k, k)), 256, 1)
    b = grid(rng.normal(0, 0.1, c), 256, 1)
    ho, wo = (13 - 1) // stride + 1, (19 - 1) // stride + 1
    r = grid(rng.normal(0, 1, (2, ho, wo, c)), 64, 4)
    if fmt == "split":
        x, r = _pairs(x), _pairs(r)
    elif fmt == "f16":
        x, r = x.astype(np.float16), r.astype(np.float16)
    store = {"split": _pairs, "f32": lambda v: v, "f16": lambda v: v.astype(np.float16)}[fmt]
    xf, rf = x.astype(np.float32), r.astype(np.float32)
    for res in (None, r):
        got, sat = ops.dwconv(x, w, b, stride=stride, act=0, residual=res, split=fmt == "split", ctx=gtx_ctx)
        want = store(_dw_loop(xf, w, b, stride, None if res is None else rf))
        assert not sat and got.shape == want.shape
        np.testing.assert_array_equal(got.astype(np.float32), want.astype(np.float32))
        got, _ = ops.dwconv(x, w, b, stride=stride, act=1, residual=res, split=fmt == "split", ctx=gtx_ctx)
        pre = _dw_loop(xf, w, b, stride).astype(np.float64)
        silu = pre / (1 + np.exp(-pre))
        want = silu + (0 if res is None else rf)
        store_rel, store_abs = {"f16": (2.0 ** -11, 2.0 ** -25), "split": (2.0 ** -21, 2.0 ** -24), "f32": (2.0 ** -24, 0.0)}[fmt]   # the format's own rounding
        tol = 8 * 2.0 ** -24 * np.abs(silu) + 2.0 ** -24 * np.abs(want) + store_rel * np.abs(want) + store_abs + 1e-45
        assert np.all(np.abs(got.astype(np.float64) - want) <= tol)


# ---------------------------------------------------------------------------- the whole network
@pytest.mark.parametrize("path", ["split", "exact", "half"])
def test_yolov10n_matches_restatement(gtx_ctx, path):
    from geotrax_amd.detector import Detector

    above = _rule("n128_many")
    assert above > 300                                           # the 300-cut bites
    w, imgsz = _case("n128_many")
    det = Detector(w, FRAME_HW, imgsz=imgsz, half=path == "half", fp32_split=path == "split", ctx=gtx_ctx, **KW)
    assert det.graph == "yolov10" and det.end2end and det.sparse_box()[0] == (path == "split")
    got = _check(det, "n128_many", half=path == "half")
    if path != "half":
        assert len(got) == 300                                   # 312 scores clear conf: the cut, not the gate, decides
    det.close()


@pytest.mark.parametrize("name", ["n128_few", "n256", "s128"])
@pytest.mark.parametrize("split", [True, False])
def test_yolov10_cases_match_restatement(gtx_ctx, name, split):
    from geotrax_amd.detector import Detector

    above = _rule(name)
    assert (above > 300) == (name == "n256")
    w, imgsz = _case(name)
    if name == "s128":
        assert w["model.8.m.0.cv1.2.conv.weight"].shape == (512, 1, 7, 7)
    det = Detector(w, FRAME_HW, imgsz=imgsz, fp32_split=split, ctx=gtx_ctx, **KW)
    got = _check(det, name)
    assert len(got) == min(above, 300)
    det.close()


def test_both_heads(gtx_ctx):
    """end2end: false on the same file is the restatement's one-to-many branch + NMS; the two heads detect different things."""
    from geotrax_amd.detector import Detector
    from oracle.yolov8_ref import non_max_suppression, scale_boxes

    w, imgsz, ref, _, x = _ref("n128_many")
    frame = _frame(0, FRAME_HW)
    e2e = Detector(w, FRAME_HW, imgsz=imgsz, ctx=gtx_ctx, **KW)
    nms = Detector(w, FRAME_HW, imgsz=imgsz, end2end=False, ctx=gtx_ctx, **KW)
    assert e2e.end2end and not nms.end2end
    a, b = e2e.detect(frame), nms.detect(frame)
    many = ref.forward(x, one2one=False)[0].numpy()
    ref.forward(x)                                               # the shared restatement keeps the one-to-one pass's activations
    np.testing.assert_allclose(nms.raw_output()[:, 4:], many[:, 4:], atol=SCORE_ATOL[0])
    rows = non_max_suppression(many, KW["conf"], KW["iou"], KW["classes"], True, KW["max_det"])
    xyxy = scale_boxes(rows[:, :4], nms.net_hw, FRAME_HW)
    assert len(b) == len(rows) > 0
    gx, gc, gk = _by_position(b.xyxy, b.conf, b.cls)
    rx, rc, rk = _by_position(xyxy, rows[:, 4], rows[:, 5].astype(np.int32))
    np.testing.assert_array_equal(gk, rk)
    np.testing.assert_allclose(gc, rc, atol=CONF_ATOL)
    np.testing.assert_allclose(gx, rx, atol=XYXY_ATOL)
    assert len(a) != len(b) or not np.allclose(a.conf, b.conf, atol=1e-3)
    fused = {k: v for k, v in w.items() if not k.startswith(("model.23.cv2.", "model.23.cv3."))}
    with pytest.raises(ValueError, match="cv2 / cv3"):
        Detector(fused, FRAME_HW, imgsz=imgsz, end2end=False, ctx=gtx_ctx, **KW)
    only = Detector(fused, FRAME_HW, imgsz=imgsz, ctx=gtx_ctx, **KW)   # a fused export runs with its one-to-one head
    c = only.detect(frame)
    np.testing.assert_array_equal(a.xyxy, c.xyxy)
    np.testing.assert_array_equal(a.conf, c.conf)
    from geotrax_amd.weights import synthetic_yolo11

    with pytest.raises(ValueError, match="end2end"):
        Detector(synthetic_yolo11(0, 4, "n"), FRAME_HW, imgsz=imgsz, end2end=True, ctx=gtx_ctx, **KW)
    with pytest.raises(NotImplementedError, match="cls"):
        Detector(w, FRAME_HW, imgsz=imgsz, obj_feats=True, ctx=gtx_ctx, **KW)
    for d in (e2e, nms, only):
        d.close()


def test_self_consistency(gtx_ctx, monkeypatch):
    """On a letterboxed frame (the 96 x 160 frame fills 77 of the 128 input rows): detectors built with
    GTX_SPARSE_BOX=0 and with GTX_PAD_SKIP=0 give the default's rows bit for bit; a batch of 2 equals two single passes; submit /
    collect equals the blocking call; `classes` and max_det act on the rows the cut keeps."""
    from geotrax_amd.detector import Detector

    w, imgsz = _case("n128_many")
    frames = np.stack([_frame(s, FRAME_HW) for s in range(2)])
    kw = dict(imgsz=imgsz, max_batch=2, ctx=gtx_ctx, **KW)
    det = Detector(w, FRAME_HW, **kw)
    assert det.sparse_box()[0]
    others = []
    for var in ("GTX_PAD_SKIP", "GTX_SPARSE_BOX"):
        with monkeypatch.context() as mp:
            mp.setenv(var, "0")
            others.append(Detector(w, FRAME_HW, **kw))
    assert others[0].pad_skip()[0] is False and others[1].sparse_box() == (False, 0)
    singles = [det.detect(f) for f in frames]
    assert len(singles[0]) > 0
    for o in others:
        for f, s in zip(frames, singles):
            b = o.detect(f)
            np.testing.assert_array_equal(s.xyxy, b.xyxy)
            np.testing.assert_array_equal(s.conf, b.conf)
            np.testing.assert_array_equal(s.cls, b.cls)
    dptr = gtx_ctx.dev_alloc(frames.nbytes)
    try:
        gtx_ctx.dev_upload(dptr, frames)
        batch = det.detect_dev(dptr, 2)
        det.submit_dev(dptr, 2)
        late = det.collect()
    finally:
        gtx_ctx.dev_free(dptr)
    for s, b, c in zip(singles, batch, late):
        for other in (b, c):
            np.testing.assert_array_equal(s.xyxy, other.xyxy)
            np.testing.assert_array_equal(s.conf, other.conf)
            np.testing.assert_array_equal(s.cls, other.cls)
    assert det.sparse_box() == (True, 0)
    # `classes` drops rows of the 300 kept (it does not make room for others), max_det cuts what is left
    sub = Detector(w, FRAME_HW, imgsz=imgsz, ctx=gtx_ctx, **{**KW, "classes": [1, 3], "max_det": 20})
    s0, d = singles[0], sub.detect(frames[0])
    keep = np.isin(s0.cls, [1, 3])
    assert 20 < keep.sum() < len(s0)
    np.testing.assert_array_equal(d.conf, s0.conf[keep][:20])
    np.testing.assert_array_equal(d.xyxy, s0.xyxy[keep][:20])
    for o in others + [det, sub]:
        o.close()


def test_every_anchor_a_candidate(gtx_ctx):
    """The case that overflowed the other families' sparse buffer cannot here: the gate's buffer holds every anchor and the box branch
    sees the 300 entries kept. With conf at 0.01 every anchor is a candidate (1344 scores above it); the sparse and the dense box
    branch give the same rows, and no overflow is counted."""
    from geotrax_amd.detector import Detector

    w, imgsz = _case("n128_many")
    frame = _frame(0, FRAME_HW)
    kw = dict(imgsz=imgsz, ctx=gtx_ctx, **{**KW, "conf": 0.01})
    sparse, exact = Detector(w, FRAME_HW, fp32_split=True, **kw), Detector(w, FRAME_HW, fp32_split=False, **kw)
    a, b = sparse.detect(frame), exact.detect(frame)
    assert len(a) == len(b) == 300 and sparse.sparse_box() == (True, 0)
    ax, ac, ak = _by_position(a.xyxy, a.conf, a.cls)
    bx, bc, bk = _by_position(b.xyxy, b.conf, b.cls)
    np.testing.assert_array_equal(ak, bk)
    np.testing.assert_allclose(ac, bc, atol=CONF_ATOL)
    np.testing.assert_allclose(ax, bx, atol=XYXY_ATOL)
    sparse.close(); exact.close()


def test_saturation_falls_back_to_exact(gtx_ctx):
    """Gain-amplified seeded weights (activations beyond fp16's range, as in test_yolo11_gpu's case): the split-f16x3 detector re-runs
    the pass on its exact-fp32 twin -- the same YOLOv10 graph and tail -- and from then on equals the exact detector bit for bit."""
    from geotrax_amd.detector import Detector
    from geotrax_amd.weights import synthetic_yolov10
    from oracle.yolov8_ref import letterbox
    from yolov10_ref import Yolov10Ref

    w = synthetic_yolov10(seed=3, nc=4, scale="n", cls_bias=-3.0, gain=2.0)
    frames = [_frame(0, FRAME_HW), _frame(1, FRAME_HW)]
    ref = Yolov10Ref(w)
    ref.forward(letterbox(frames[0], 128, False)[0])
    peak = max(float(v.abs().max()) for v in ref.acts.values())
    assert peak > 65504.0                                        # the case is what it claims to be
    kw = dict(imgsz=128, ctx=gtx_ctx, **KW)
    det = Detector(w, FRAME_HW, fp32_split=True, **kw)
    first = det.detect(frames[0])
    assert det.saturated() and det.fell_back()
    exact = Detector(w, FRAME_HW, fp32_split=False, **kw)
    np.testing.assert_array_equal(first.conf, exact.detect(frames[0]).conf)
    for f in frames:
        a, b = det.detect(f), exact.detect(f)
        assert len(a) == len(b) > 0
        np.testing.assert_array_equal(a.xyxy, b.xyxy)
        np.testing.assert_array_equal(a.conf, b.conf)
        np.testing.assert_array_equal(det.raw_output(), exact.raw_output())
    det.close(); exact.close()


def test_through_the_wrapper(gtx_ctx, tmp_path):
    """YOLO(file).track with ByteTrack on a short clip gives the tracks of the interface-level detector + tracker on the same frames;
    the wrapper names the yaml by its scale; `with_reid: true, model: auto` points to the cls-checkpoint route."""
    from geotrax_amd.detector import Detector
    from geotrax_amd.model import YOLO
    from geotrax_amd.tracker import Tracker
    from geotrax_amd.weights import save_weights

    w, imgsz = _case("n128_few")
    path = tmp_path / "yolov10n.safetensors"
    save_weights(w, path)
    model = YOLO(str(path), ctx=gtx_ctx)
    assert model.yaml_file == "yolov10n.yaml" and model.names == {0: "0", 1: "1", 2: "2", 3: "3"}
    spec = dict(tracker_type="bytetrack", track_high_thresh=0.25, track_low_thresh=0.1, new_track_thresh=0.25, track_buffer=30, match_thresh=0.8,
                fuse_score=True)
    det = Detector(w, FRAME_HW, imgsz=imgsz, conf=0.25, max_det=300, ctx=gtx_ctx)
    trk = Tracker("bytetrack", **{k: v for k, v in spec.items() if k != "tracker_type"})
    total = 0
    for t in range(4):
        frame = _frame(t, FRAME_HW)
        res = model.track(frame, persist=True, tracker=spec, imgsz=imgsz, conf=0.25, max_det=300, end2end=None)[0]
        d = det.detect(frame)
        xyxy, ids, score, cls, _ = trk.update(d.xyxy, d.conf, d.cls)
        assert model.detector.end2end
        if len(ids):
            np.testing.assert_array_equal(res.boxes._xyxy, xyxy)
            np.testing.assert_array_equal(np.asarray(res.boxes._conf), score)
            total += len(ids)
    assert total > 0
    with pytest.raises(NotImplementedError, match="cls"):
        model.track(_frame(0, FRAME_HW), tracker=dict(tracker_type="botsort", with_reid=True, model="auto", gmc_method="none"), imgsz=imgsz)
    with pytest.raises(ValueError, match="end2end"):
        YOLO(__import__("geotrax_amd.weights", fromlist=["x"]).synthetic_yolov8(0, 4, "n"), ctx=gtx_ctx).predict(_frame(0, FRAME_HW), imgsz=imgsz, end2end=True)
    det.close()


# ---------------------------------------------------------------------------- through the product: extract, ExtractEngine, shards
N_CLIP = 8


def _v10_file(tmp_path, gtx_ctx, probe):
    """Seeded YOLOv10-n weights (the calm seed of the parity cases; boxes of ~46 network pixels so that the stabilizer keeps
    background), both heads' class biases shifted so that ~60 anchors of the probe frame clear conf, as a .safetensors file + names."""
    import test_extract_gpu as te
    from geotrax_amd.detector import Detector
    from geotrax_amd.weights import save_weights, synthetic_yolov10

    w = synthetic_yolov10(seed=7, nc=4, scale="n", gain=1.7, box_weight_scale=0.002)
    for pair, e2e in (("one2one_cv3", True), ("cv3", False)):
        det = Detector(w, (te.H, te.W), imgsz=te.IMGSZ, rect=True, end2end=e2e, ctx=gtx_ctx)
        det.detect(probe)
        lg = np.sort(det.raw_output(logits=True)[:, 4:].max(1).astype(np.float64))[::-1]
        det.close()
        delta = np.float32(np.log(0.25 / 0.75) - 0.5 * (lg[59] + lg[60]))
        w = {k: (v + delta).astype(np.float32) if f".{pair}." in k and k.endswith(".2.bias") else v for k, v in w.items()}
    path = tmp_path / "yolov10n.safetensors"
    save_weights(w, path)
    path.with_suffix(".names.yaml").write_text("{0: car, 1: bus, 2: truck, 3: motorcycle}\n")
    return path


def _clip_and_cfg(tmp_path, gtx_ctx, engine=None, end2end=None):
    import test_extract_gpu as te
    import yaml
    from geotrax_amd.synth import make_scene

    scene = make_scene(seed=2, h=te.H, w=te.W)
    frames = np.stack([scene.render(t, 150) for t in range(0, N_CLIP * 12, 12)])
    clip = tmp_path / "clip.npy"
    np.save(clip, frames)
    cfg_path, cfg = te._cfg_file(tmp_path, _v10_file(tmp_path, gtx_ctx, frames[0]), tracker="bytetrack")
    cfg["ultralytics"]["end2end"] = end2end
    cfg["stabilo"]["mask_use"] = False                       # shard ranks mask with the raw detections, the single run with the tracker's boxes
    if engine:
        cfg["engine"] = engine
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
    """The extract chain on a YOLOv10 file (ExtractEngine: batched, pipelined detector streams, ByteTrack + stabilizer; `end2end` null
    through _engine_kwargs) gives the tables of the blocking loop, which is YOLO(file).track -- the interface-level detector +
    tracker -- frame by frame. `end2end: false` in the config reaches the engine's detectors and gives other tracks."""
    import yaml
    from geotrax_amd import extract as ex

    clip, cfg_path = _clip_and_cfg(tmp_path, gtx_ctx)
    model, config = _setup(clip, cfg_path)
    assert model.model.yaml_file == "yolov10n.yaml" and ex._engine_kwargs(config)[0].get("end2end") is None
    t1, h1 = ex.track_with_model(model, config, logger)
    model, config = _setup(clip, cfg_path)
    config["main"].setdefault("engine", {})["pipelined"] = False
    t2, h2 = ex.track_with_model_blocking(model, config, logger)
    assert model.detector.end2end
    assert len(t1) > 20 and len(h1) > 0
    assert t1.dtype == t2.dtype and t1.tobytes() == t2.tobytes() and h1.tobytes() == h2.tobytes()
    cfg = yaml.safe_load(Path(cfg_path).read_text())
    cfg["ultralytics"]["end2end"] = False
    Path(cfg_path).write_text(yaml.safe_dump(cfg))
    model, config = _setup(clip, cfg_path)
    assert ex._engine_kwargs(config)[0]["end2end"] is False
    t3, _ = ex.track_with_model(model, config, logger)
    model, config = _setup(clip, cfg_path)
    config["main"].setdefault("engine", {})["pipelined"] = False
    t4, _ = ex.track_with_model_blocking(model, config, logger)
    assert not model.detector.end2end
    assert len(t3) > 0 and t3.tobytes() == t4.tobytes() and t3.tobytes() != t1.tobytes()


def _rank_main(clip, cfg_path, out):
    from geotrax_amd import distributed as D
    from geotrax_amd import extract as ex

    model, config = _setup(clip, cfg_path)
    res = ex.track_with_model_sharded(model, config, logger)
    if res is not None:
        np.savez(out, tracks=res[0], transforms=res[1])
    D.shutdown_process_group()


def test_two_ranks_equal_the_single_process_run(gtx_ctx, tmp_path):
    """One world-2 gloo frame-sharded run on the one GPU (tests/test_sharded_gmc_gpu.py's pattern), two runs of one batch per rank:
    rank 0's tables are the single-process run's byte for byte."""
    from geotrax_amd import extract as ex

    clip, cfg_path = _clip_and_cfg(tmp_path, gtx_ctx, engine={"shard_run_frames": 2})
    model, config = _setup(clip, cfg_path)
    tracks, transforms = ex.track_with_model(model, config, logger)
    assert len(tracks) > 20
    out = tmp_path / "rank0.npz"
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", GTX_DIST_BACKEND="gloo", OMP_NUM_THREADS="1",
               PYTHONPATH=os.pathsep.join([str(ROOT / "geo-trax_amd"), str(ROOT), str(ROOT / "tests"), os.environ.get("PYTHONPATH", "")]))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29571", str(Path(__file__).resolve()), str(clip), str(cfg_path), str(out)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=tmp_path, env=env)      # one attempt, its own time limit
    assert p.returncode == 0 and out.exists(), (p.stdout + p.stderr)[-3000:]
    got = np.load(out)
    assert got["tracks"].dtype == tracks.dtype and got["tracks"].tobytes() == tracks.tobytes()
    assert got["transforms"].dtype == transforms.dtype and got["transforms"].tobytes() == transforms.tobytes()


if __name__ == "__main__":
    _rank_main(*sys.argv[1:4])
