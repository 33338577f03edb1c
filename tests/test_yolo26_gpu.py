"""YOLO26 detectors on the HIP path (SPPF with a linear cv1 and a residual, the C3k2 with attention at model.22, Detect with reg_max = 1
and the one-to-one head in front of csrc/v10_select.hip's tail) against tests/yolo26_ref.py: the dense reg_max = 1 box kernel against
float64, the sparse box form against the dense one bit for bit, every probed layer, the raw one-to-one output and the final rows on
the split-f16x3, exact-fp32 and half paths, both heads, the saturation fallback, the ultralytics-shaped wrapper, the extract chain
(ExtractEngine) and the frame-sharded run. The bars are tests/test_yolov10_gpu.py's, which are tests/test_yolo11_gpu.py's and
tests/test_p2_gpu.py's. Smallest shapes: scale n, nc = 4, imgsz 128 on a 96 x 160 frame (a 4 x 4 P5 map: the small-map attention
kernel at model.10 and model.22, 2 heads at c = 128); imgsz 256 for the tiled attention kernel; scale s once for 4 heads."""
import logging
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from test_yolo11_gpu import _frame
from test_yolov10_gpu import BOX_ATOL, BOX_RTOL, CONF_ATOL, LAYER_REL, SCORE_ATOL, XYXY_ATOL, _by_position, _setup

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
logger = logging.getLogger("test_yolo26")

FRAME_HW = (96, 160)
KW = dict(conf=0.25, iou=0.7, max_det=300, classes=[0, 1, 2, 3], agnostic_nms=True)
LAYERS = ["model.2", "model.6", "model.8", "model.9.cv1.conv", "model.9", "model.10", "model.13", "model.16", "model.19", "model.22.m.0.0.cv2.conv",
          "model.22.m.0.1.attn.qkv.conv", "model.22.m.0.1.attn.out", "model.22.m.0.1.ffn.1.conv", "model.22", "model.23.feat0", "model.23.feat1",
          "model.23.feat2"]

# Seeded cases, picked on the CPU by the written rule of DESIGN 7d (asserted by _rule below before anything is compared): a seeded
# stack of this family either amplifies (activations of 1e3-1e7, saturated scores that tie) or stays near 2 with class logits within
# a few tenths of their bias; the calm ones are taken and the bias decides how many of the A x 4 scores clear conf = 0.25.
#              scale imgsz seed gain  cls_bias
CASES = {
    "n128_many": ("n", 128, 7, 1.7, -1.14),    # more than 300 of 1344 scores above conf: the 300-cut bites
    "n128_few": ("n", 128, 7, 1.7, -1.25),     # fewer than 300: the gate decides alone
    "n256": ("n", 256, 2, 1.7, -1.25),         # an 8 x 8 P5 map: the tiled attention kernel; fewer than 300 (its 5376 scores lie too close
                                               # together at rank 300 for a case where the cut decides)
    "s128": ("s", 128, 1, 1.6, -1.21),         # 4 heads of attention at model.10 and model.22
}


def _case(name):
    from geotrax_amd.weights import synthetic_yolo26

    scale, imgsz, seed, gain, bias = CASES[name]
    return synthetic_yolo26(seed=seed, nc=4, scale=scale, cls_bias=bias, gain=gain), imgsz


_REF = {}


def _ref(name):
    """(weights, imgsz, fp32 restatement after its forward pass, its raw output, the letterboxed input): computed once per case"""
    if name not in _REF:
        from oracle.yolov8_ref import letterbox
        from yolo26_ref import Yolo26Ref

        w, imgsz = _case(name)
        x, _ = letterbox(_frame(0, FRAME_HW), imgsz, False)
        ref = Yolo26Ref(w)
        _REF[name] = (w, imgsz, ref, ref.forward(x)[0].numpy(), x)
    return _REF[name]


_RULE = {}


def _rule(name):
    """The written rule: the restatement's own fp32-vs-float64 spread is at most a fifth of every bar, no score within 5e-6 of conf
    and, where the 300-cut decides, no two scores within 5e-6 of each other at the cut. Returns the number of scores above conf. CPU only; once per case."""
    if name in _RULE:
        return _RULE[name]
    from yolo26_ref import Yolo26Ref, postprocess

    w, imgsz, r32, a, x = _ref(name)
    r64 = Yolo26Ref(w).double()
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
    above = int((flat > KW["conf"]).sum())
    assert margin > 5e-6 and (gap > 5e-6 or above < 300)         # with fewer than 300 above conf the gate drops everything near rank 300
    assert float(a[:, 2:4].min()) > 0                            # one distance is negative at every anchor, the boxes keep a positive size
    _RULE[name] = int((flat > KW["conf"]).sum())
    return _RULE[name]


def _check(det, name, half=False):
    """Layers, raw one-to-one output and final rows of det on the case's frame against the restatement"""
    from oracle.yolov8_ref import letterbox
    from yolo26_ref import Yolo26Ref, detect

    w, imgsz, ref, ref_raw, _ = _ref(name)
    frame = _frame(0, FRAME_HW)
    if half:
        ref = Yolo26Ref(w, emulate_half=True)
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
    if half:                                        # fp16 scores move across conf and the cut: test_yolov10_gpu's half branch
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
    gx, gc, gk = _by_position(got.xyxy, got.conf, got.cls)
    rx, rc, rk = _by_position(xyxy, conf, cls)
    np.testing.assert_array_equal(gk, rk)
    np.testing.assert_allclose(gc, rc, atol=CONF_ATOL)
    np.testing.assert_allclose(gx, rx, atol=XYXY_ATOL)
    return got


# ---------------------------------------------------------------------------- the dense reg_max = 1 box kernel against float64
MAPS = ((1, 3), (5, 7), (13, 19))
STRIDES = (8.0, 16.0, 32.0)


@pytest.mark.parametrize("fmt", ["f32", "f16"])
def test_dense_box_form_against_float64(gtx_ctx, fmt):
    """head_boxes_r1_kernel on three levels of 1 x 3, 5 x 7 and 13 x 19 cells with 64 box channels, two images, every anchor a candidate
    (every map corner among them) in a shuffled order, and a buffer longer than the count. Distances of both signs. The class half
    of every map row holds 1e30 (a read past the 64 box channels would show); entries past the count keep their sentinel. fp32 maps
    are also what the split-f16x3 path hands this kernel (the head's maps are plain fp32 there: Detector's ConvProblem::out_plain), so
    the two formats are the kernel's two instantiations. Bound, from the arithmetic: a distance is one 64-step fmaf chain from the
    bias, |error| <= 65 u S with S = |bias| + sum |f w| and u = 2^-24; a side is (centre -/+ d) * stride, two more roundings."""
    from geotrax_amd import ops

    rng = np.random.default_rng(26)
    dt = np.float16 if fmt == "f16" else np.float32
    n, cb, cc = 2, 64, 16
    levels, truth = [], []
    for (h, w), stride in zip(MAPS, STRIDES):
        feat = np.full((n, h, w, cb + cc), 1e30 if fmt == "f32" else 6e4, dt)
        feat[..., :cb] = rng.normal(0, 1, (n, h, w, cb)).astype(dt)
        wb = rng.normal(0, 0.3, (cb, 4)).astype(np.float32)
        bb = np.asarray([2.0, 0.5, 2.0, -0.5], np.float32)
        levels.append(dict(feat=feat, cb=cb, cc=cc, stride=stride, wb=wb, bb=bb))
        f64 = feat[..., :cb].astype(np.float64)
        d = f64 @ wb.astype(np.float64) + bb.astype(np.float64)                         # [n, h, w, 4]
        S = np.abs(f64) @ np.abs(wb.astype(np.float64)) + np.abs(bb.astype(np.float64))
        ys, xs = np.meshgrid(np.arange(h) + 0.5, np.arange(w) + 0.5, indexing="ij")
        box = np.stack([xs - d[..., 0], ys - d[..., 1], xs + d[..., 2], ys + d[..., 3]], -1) * stride
        tol = stride * 65 * 2.0 ** -24 * S + 3 * 2.0 ** -24 * np.abs(box) + 1e-30
        truth.append((box.reshape(n, h * w, 4), tol.reshape(n, h * w, 4), d.reshape(n, h * w, 4)))
    box64, tol64, dist = (np.concatenate([t[i] for t in truth], 1) for i in range(3))
    A = box64.shape[1]
    assert A == 3 + 35 + 247 and (dist < 0).mean() > 0.1 and (dist > 0).mean() > 0.5     # signed distances, both kinds plenty
    cap = A + 7
    anchors = np.full((n, cap), -1, np.int32)
    count = np.asarray([A, 5], np.int32)
    anchors[0, :A] = rng.permutation(A)
    anchors[1, :5] = [0, 2, 3, 3 + 34, A - 1]                                           # corners of each map; the second image's short list
    got = ops.head_boxes_r1(levels, count, anchors, ctx=gtx_ctx)
    assert got.shape == (n, cap, 4)
    for b in range(n):
        c = int(count[b])
        assert np.isnan(got[b, c:]).all()                                               # the sentinels beside the outputs are untouched
        want, tol = box64[b, anchors[b, :c]], tol64[b, anchors[b, :c]]
        err = np.abs(got[b, :c].astype(np.float64) - want)
        print(f"{fmt} image {b}: {c} boxes, largest error {err.max():.2e}, largest error / bound {(err / tol).max():.3f}")
        assert np.isfinite(got[b, :c]).all() and bool((err <= tol).all())
    none = ops.head_boxes_r1(levels, np.zeros(n, np.int32), anchors, ctx=gtx_ctx)        # no candidate: nothing is written
    assert np.isnan(none).all()


# ---------------------------------------------------------------------------- the sparse box form against the dense one
@pytest.mark.parametrize("how", ["every_anchor", "none", "one", "gate"])
def test_sparse_box_form_equals_the_dense_one(gtx_ctx, monkeypatch, how):
    """The split-f16x3 detector with the sparse reg_max = 1 form (head_sparse_box_kernel<true>: cv2[l][0] / cv2[l][1] at the entries
    kept, then the 4-output 1x1) against the same detector built with GTX_SPARSE_BOX=0 (the dense layers + head_boxes_r1_kernel): the
    rows bit for bit. every_anchor: conf 0.01, all 336 anchors candidates, 300 entries kept (the map corners have a test of their
    own below); none: conf above every score, 0 candidates; one: conf between the two best scores of the restatement; gate: conf 0.25."""
    from geotrax_amd.detector import Detector

    w, imgsz, _, raw, _ = _ref("n128_many")
    flat = np.sort(raw[:, 4:].reshape(-1))[::-1]
    assert flat[0] - flat[1] > 2e-4                                                     # the restatement's two best are far enough apart
    conf = {"every_anchor": 0.01, "none": min(0.999, float(flat[0]) + 0.05), "one": float(flat[0] + flat[1]) / 2, "gate": 0.25}[how]
    want_rows = {"every_anchor": 300, "none": 0, "one": 1, "gate": 300}[how]
    frame = _frame(0, FRAME_HW)
    kw = dict(imgsz=imgsz, fp32_split=True, ctx=gtx_ctx, **{**KW, "conf": conf})
    sparse = Detector(w, FRAME_HW, **kw)
    with monkeypatch.context() as mp:
        mp.setenv("GTX_SPARSE_BOX", "0")
        dense = Detector(w, FRAME_HW, **kw)
    assert sparse.sparse_box()[0] and dense.sparse_box() == (False, 0)
    a, b = sparse.detect(frame), dense.detect(frame)
    print(f"{how}: conf {conf:.4f}, {len(a)} rows")
    assert len(a) == len(b) == want_rows and sparse.sparse_box() == (True, 0)
    np.testing.assert_array_equal(a.xyxy, b.xyxy)
    np.testing.assert_array_equal(a.conf, b.conf)
    np.testing.assert_array_equal(a.cls, b.cls)
    sparse.close(); dense.close()


CORNER_LEVELS = (((16, 16), 0), ((8, 8), 256), ((4, 4), 320))      # imgsz 128: (cells, first anchor) of P3 / P4 / P5


@pytest.mark.parametrize("boost", [(0,), (1, 2)])
def test_sparse_box_form_on_every_map_corner(gtx_ctx, monkeypatch, boost):
    """All four corners of all three maps as candidates of the sparse form, in two runs. A one-class stack (336 scores, one per
    anchor) whose class bias is +3 on the boosted levels and -3 on the others, conf 0.01: every anchor is a candidate, the cut keeps
    300 anchors, and the boosted levels' -- P3's 256, or P4's 64 + P5's 16 -- are all among them, their scores being above 0.9 and
    the others' below 0.1 (asserted on the restatement, then on the rows). A 128 x 128 frame (no letterbox padding, gain 1) and boxes
    of 0.3 / 0.4 / 0.3 / -0.1 strides keep every corner box inside the frame, so no coordinate of a corner row is clipped: the rows
    with a corner's centre are found by position and all four coordinates compared bit for bit with the dense form's."""
    from geotrax_amd.detector import Detector
    from geotrax_amd.weights import synthetic_yolo26
    from oracle.yolov8_ref import letterbox
    from yolo26_ref import Yolo26Ref, postprocess

    hw = (128, 128)
    w = synthetic_yolo26(seed=7, nc=1, scale="n", cls_bias=0.0, gain=1.7, box_weight_scale=0.02)
    for l in range(3):
        for pair in ("cv", "one2one_cv"):
            w[f"model.23.{pair}3.{l}.2.bias"] = w[f"model.23.{pair}3.{l}.2.bias"] + np.float32(3.0 if l in boost else -3.0)
            w[f"model.23.{pair}2.{l}.2.bias"] = np.asarray([0.3, 0.4, 0.3, -0.1], np.float32)
    frame = _frame(0, hw)
    raw = Yolo26Ref(w).forward(letterbox(frame, 128, False)[0])[0].numpy()
    level = np.repeat([0, 1, 2], [256, 64, 16])
    hot = np.isin(level, boost)
    assert raw.shape == (336, 5) and raw[hot, 4].min() > 0.9 and 0.01 < raw[~hot, 4].min() and raw[~hot, 4].max() < 0.1
    rows, kept = postprocess(raw, 0.01, None, 300, return_idx=True)
    corners = [base + o for l, ((h, wd), base) in enumerate(CORNER_LEVELS) if l in boost for o in (0, wd - 1, (h - 1) * wd, h * wd - 1)]
    assert len(rows) == 300 and set(corners) <= set(int(k) for k in kept) and len(corners) == 4 * len(boost)
    kw = dict(imgsz=128, fp32_split=True, ctx=gtx_ctx, **{**KW, "conf": 0.01, "classes": [0]})
    sparse = Detector(w, hw, **kw)
    with monkeypatch.context() as mp:
        mp.setenv("GTX_SPARSE_BOX", "0")
        dense = Detector(w, hw, **kw)
    assert sparse.sparse_box()[0] and dense.sparse_box() == (False, 0) and sparse.net_hw == hw
    a, b = sparse.detect(frame), dense.detect(frame)
    assert len(a) == len(b) == 300 and int((a.conf > 0.5).sum()) == int(hot.sum()) and sparse.sparse_box() == (True, 0)
    np.testing.assert_array_equal(a.xyxy, b.xyxy)
    np.testing.assert_array_equal(a.conf, b.conf)
    found = 0
    for k in corners:                                            # the corner's row: the boosted row whose box holds the corner cell's centre
        r = rows[list(kept).index(k)]
        cx, cy = (r[0] + r[2]) / 2, (r[1] + r[3]) / 2
        i = np.flatnonzero((a.conf > 0.5) & (np.abs((a.xyxy[:, 0] + a.xyxy[:, 2]) / 2 - cx) < 0.5) & (np.abs((a.xyxy[:, 1] + a.xyxy[:, 3]) / 2 - cy) < 0.5))
        assert len(i) == 1, (k, i)
        box = a.xyxy[i[0]]
        assert 0 < box[0] < box[2] < 128 and 0 < box[1] < box[3] < 128, (k, box)       # nothing clipped
        np.testing.assert_allclose(box, r[:4], atol=XYXY_ATOL)
        np.testing.assert_array_equal(box, b.xyxy[i[0]])
        found += 1
    print(f"levels {boost}: {found} corner rows compared bit for bit, anchors {corners}")
    assert found == 4 * len(boost)
    sparse.close(); dense.close()


# ---------------------------------------------------------------------------- the whole network
@pytest.mark.parametrize("path", ["split", "exact", "half"])
def test_yolo26n_matches_restatement(gtx_ctx, path):
    from geotrax_amd.detector import Detector

    above = _rule("n128_many")
    assert above > 300                                           # the 300-cut bites
    w, imgsz = _case("n128_many")
    det = Detector(w, FRAME_HW, imgsz=imgsz, half=path == "half", fp32_split=path == "split", ctx=gtx_ctx, **KW)
    assert det.graph == "yolo26" and det.end2end and det.sparse_box()[0] == (path == "split")
    got = _check(det, "n128_many", half=path == "half")
    if path != "half":
        assert len(got) == 300
    det.close()


@pytest.mark.parametrize("name", ["n128_few", "n256", "s128"])
@pytest.mark.parametrize("split", [True, False])
def test_yolo26_cases_match_restatement(gtx_ctx, name, split):
    from geotrax_amd.detector import Detector

    above = _rule(name)
    assert 0 < above < 300                                       # the gate decides alone
    w, imgsz = _case(name)
    if name == "s128":
        assert w["model.22.m.0.1.attn.qkv.conv.weight"].shape == (512, 256, 1, 1)       # 4 heads
    det = Detector(w, FRAME_HW, imgsz=imgsz, fp32_split=split, ctx=gtx_ctx, **KW)
    got = _check(det, name)
    assert len(got) == min(above, 300)
    det.close()


def test_both_heads(gtx_ctx):
    """end2end: false on the same file is the restatement's one-to-many branch + NMS through the reg_max = 1 box forms; a fused export
    runs with its one-to-one head and refuses false; end2end: true on YOLO11 raises; obj_feats points to the cls-checkpoint route."""
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
    raw = nms.raw_output()
    np.testing.assert_allclose(raw[:, 4:], many[:, 4:], atol=SCORE_ATOL[0])
    np.testing.assert_allclose(raw[:, :4], many[:, :4], rtol=BOX_RTOL[0], atol=BOX_ATOL[0])
    rows = non_max_suppression(many, KW["conf"], KW["iou"], KW["classes"], True, KW["max_det"])
    xyxy = scale_boxes(rows[:, :4], nms.net_hw, FRAME_HW)
    print(f"end2end: {len(a)} rows; Detect + NMS: {len(b)} rows, restatement {len(rows)}")
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
    only = Detector(fused, FRAME_HW, imgsz=imgsz, ctx=gtx_ctx, **KW)
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
    """Detectors built with GTX_PAD_SKIP=0 and GTX_SPARSE_BOX=0 give the default's rows bit for bit; a batch of 2 equals two single
    passes; `classes` and max_det act on the rows the cut keeps."""
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
    finally:
        gtx_ctx.dev_free(dptr)
    for s, b in zip(singles, batch):
        np.testing.assert_array_equal(s.xyxy, b.xyxy)
        np.testing.assert_array_equal(s.conf, b.conf)
        np.testing.assert_array_equal(s.cls, b.cls)
    assert det.sparse_box() == (True, 0)
    sub = Detector(w, FRAME_HW, imgsz=imgsz, ctx=gtx_ctx, **{**KW, "classes": [1, 3], "max_det": 20})
    s0, d = singles[0], sub.detect(frames[0])
    keep = np.isin(s0.cls, [1, 3])
    assert 20 < keep.sum() < len(s0)
    np.testing.assert_array_equal(d.conf, s0.conf[keep][:20])
    np.testing.assert_array_equal(d.xyxy, s0.xyxy[keep][:20])
    for o in others + [det, sub]:
        o.close()


def test_saturation_falls_back_to_exact(gtx_ctx):
    """Gain-amplified seeded weights (activations beyond fp16's range): the split-f16x3 detector re-runs the pass on its exact-fp32
    twin -- the same YOLO26 graph and tail, make_exact() -- and from then on equals the exact detector bit for bit."""
    from geotrax_amd.detector import Detector
    from geotrax_amd.weights import synthetic_yolo26
    from oracle.yolov8_ref import letterbox
    from yolo26_ref import Yolo26Ref

    w = synthetic_yolo26(seed=3, nc=4, scale="n", cls_bias=-3.0, gain=2.0)
    frames = [_frame(0, FRAME_HW), _frame(1, FRAME_HW)]
    ref = Yolo26Ref(w)
    ref.forward(letterbox(frames[0], 128, False)[0])
    assert max(float(v.abs().max()) for v in ref.acts.values()) > 65504.0   # the case is what it claims to be
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
    path = tmp_path / "yolo26n.safetensors"
    save_weights(w, path)
    model = YOLO(str(path), ctx=gtx_ctx)
    assert model.yaml_file == "yolo26n.yaml"
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
    det.close()


# ---------------------------------------------------------------------------- through the product: extract, ExtractEngine, shards
N_CLIP = 8


def _y26_file(tmp_path, gtx_ctx, probe):
    """Seeded YOLO26-n weights (the calm seed of the parity cases), both heads' class biases shifted so that ~60 anchors of the probe
    frame clear conf, as a .safetensors file + names."""
    import test_extract_gpu as te
    from geotrax_amd.detector import Detector
    from geotrax_amd.weights import save_weights, synthetic_yolo26

    w = synthetic_yolo26(seed=7, nc=4, scale="n", gain=1.7, box_weight_scale=0.002)
    for pair, e2e in (("one2one_cv3", True), ("cv3", False)):
        det = Detector(w, (te.H, te.W), imgsz=te.IMGSZ, rect=True, end2end=e2e, ctx=gtx_ctx)
        det.detect(probe)
        lg = np.sort(det.raw_output(logits=True)[:, 4:].max(1).astype(np.float64))[::-1]
        det.close()
        delta = np.float32(np.log(0.25 / 0.75) - 0.5 * (lg[59] + lg[60]))
        w = {k: (v + delta).astype(np.float32) if f".{pair}." in k and k.endswith(".2.bias") else v for k, v in w.items()}
    path = tmp_path / "yolo26n.safetensors"
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
    cfg_path, cfg = te._cfg_file(tmp_path, _y26_file(tmp_path, gtx_ctx, frames[0]), tracker="bytetrack")
    cfg["ultralytics"]["end2end"] = end2end
    cfg["stabilo"]["mask_use"] = False                       # shard ranks mask with the raw detections, the single run with the tracker's boxes
    if engine:
        cfg["engine"] = engine
    cfg_path.write_text(yaml.safe_dump(cfg))
    return clip, cfg_path


def test_extract_engine_equals_the_frame_at_a_time_loop(gtx_ctx, tmp_path):
    """The extract chain on a YOLO26 file (ExtractEngine; `end2end` null through _engine_kwargs) gives the tables of the blocking
    loop, which is YOLO(file).track frame by frame. `end2end: false` in the config reaches the engine's detectors and gives other tracks."""
    import yaml
    from geotrax_amd import extract as ex

    clip, cfg_path = _clip_and_cfg(tmp_path, gtx_ctx)
    model, config = _setup(clip, cfg_path)
    assert model.model.yaml_file == "yolo26n.yaml" and ex._engine_kwargs(config)[0].get("end2end") is None
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


def test_two_ranks_equal_the_single_process_run(gtx_ctx, tmp_path):
    """One world-2 gloo frame-sharded run on the one GPU (tests/test_yolov10_gpu.py's pattern and its rank script, which loads whatever
    detector the config names): rank 0's tables are the single-process run's byte for byte."""
    from geotrax_amd import extract as ex

    clip, cfg_path = _clip_and_cfg(tmp_path, gtx_ctx, engine={"shard_run_frames": 2})
    model, config = _setup(clip, cfg_path)
    tracks, transforms = ex.track_with_model(model, config, logger)
    assert len(tracks) > 20
    out = tmp_path / "rank0.npz"
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", GTX_DIST_BACKEND="gloo", OMP_NUM_THREADS="1",
               PYTHONPATH=os.pathsep.join([str(ROOT / "geo-trax_amd"), str(ROOT), str(ROOT / "tests"), os.environ.get("PYTHONPATH", "")]))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29573", str(ROOT / "tests" / "test_yolov10_gpu.py"), str(clip), str(cfg_path), str(out)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=tmp_path, env=env)      # one attempt, its own time limit
    assert p.returncode == 0 and out.exists(), (p.stdout + p.stderr)[-3000:]
    got = np.load(out)
    assert got["tracks"].dtype == tracks.dtype and got["tracks"].tobytes() == tracks.tobytes()
    assert got["transforms"].dtype == transforms.dtype and got["transforms"].tobytes() == transforms.tobytes()
