"""YOLOv9 detectors on the HIP path (ELAN1 / RepNCSPELAN4, AConv / ADown behind csrc/pool_down.hip, SPPELAN, YOLOv8's Detect) against
tests/yolov9_ref.py: AConv and ADown as blocks through the detector's op emitter, every probed layer, the raw output and the final rows
on the split-f16x3, exact-fp32 and half paths, batches, the asynchronous pair, the saturation fallback and the ultralytics-shaped
wrapper. The bars are tests/test_yolov10_gpu.py's (themselves tests/test_yolo11_gpu.py::_check_against_oracle's). Smallest shapes:
scales t (AConv, ELAN1, the 24-channel RepCSP maps carried zero-padded) and c (ADown), nc = 4, imgsz 64 on a 48 x 80 frame
(letterboxed: 38 of 64 rows) and imgsz 96 on a 96 x 96 frame; scale m at imgsz 64: the widths that are no power of two (240 / 360 /
480 / 184; the 360-, 184- and 180-channel maps run zero-padded to multiples of 16 and are read back through their real channels)."""
import numpy as np
import pytest

from test_yolo11_gpu import _frame
from test_yolov10_gpu import BOX_ATOL, BOX_RTOL, CONF_ATOL, LAYER_REL, SCORE_ATOL, XYXY_ATOL, _by_position

pytestmark = pytest.mark.gpu

KW = dict(conf=0.25, iou=0.7, max_det=300, classes=[0, 1, 2, 3], agnostic_nms=True)
LAYERS = ["model.2", "model.3.pool", "model.3", "model.4", "model.5", "model.6", "model.7", "model.8", "model.9", "model.12", "model.15", "model.16.pool",
          "model.16", "model.18", "model.19", "model.21", "model.22.feat0", "model.22.feat1", "model.22.feat2"]
# Seeded cases, picked on the CPU by test_yolov10_gpu's rule (asserted by _rule before anything is compared): a seeded stack either
# amplifies (activations of 1e3-1e8, saturated scores that tie) or stays near 2 with class logits within +-0.4 of their bias; the calm
# ones are taken and the bias decides how many anchors clear conf = 0.25.
#            scale imgsz frame     seed gain cls_bias   rows of the restatement after NMS
CASES = {
    "t64": ("t", 64, (48, 80), 5, 1.6, -1.32),
    "t96": ("t", 96, (96, 96), 5, 1.6, -1.38),
    "c64": ("c", 64, (48, 80), 2, 1.6, -1.23),
    "c96": ("c", 96, (96, 96), 2, 1.6, -1.26),
    "m64": ("m", 64, (48, 80), 5, 1.6, -1.39),
}


def _case(name):
    from geotrax_amd.weights import synthetic_yolov9

    scale, imgsz, hw, seed, gain, bias = CASES[name]
    return synthetic_yolov9(seed=seed, nc=4, scale=scale, cls_bias=bias, gain=gain, box_weight_scale=0.1), imgsz, hw


_REF = {}


def _ref(name):
    """(weights, imgsz, frame size, fp32 restatement after its forward pass, its raw output, the letterboxed input): once per case"""
    if name not in _REF:
        from oracle.yolov8_ref import letterbox
        from yolov9_ref import Yolov9Ref

        w, imgsz, hw = _case(name)
        x, _ = letterbox(_frame(0, hw), imgsz, False)
        ref = Yolov9Ref(w)
        _REF[name] = (w, imgsz, hw, ref, ref.forward(x)[0].numpy(), x)
    return _REF[name]


def _rule(name):
    """The written rule: the restatement's own fp32-vs-float64 spread is at most a fifth of every bar, no score within 5e-6 of conf,
    and the restatement alone yields between 5 and 60 rows. Returns that number."""
    from oracle.yolov8_ref import non_max_suppression
    from yolov9_ref import Yolov9Ref

    w, imgsz, hw, r32, a, x = _ref(name)
    r64 = Yolov9Ref(w).double()
    b = r64.forward(x.double())[0].numpy()
    lay = max(float((r32.acts[n].double() - r64.acts[n]).abs().max() / (r64.acts[n].abs().max() + 1e-6)) for n in LAYERS if n in r32.acts)
    sc = float(np.abs(a[:, 4:] - b[:, 4:]).max())
    bx = float((np.abs(a[:, :4] - b[:, :4]) / (BOX_RTOL[0] * np.abs(b[:, :4]) + BOX_ATOL[0])).max())
    margin = float(np.abs(a[:, 4:] - KW["conf"]).min())
    rows = non_max_suppression(a, KW["conf"], KW["iou"], KW["classes"], True, KW["max_det"])
    rows64 = non_max_suppression(b.astype(np.float32), KW["conf"], KW["iou"], KW["classes"], True, KW["max_det"])
    print(f"{name}: restatement fp32 vs float64: layers {lay:.1e}, scores {sc:.1e}, boxes {bx:.2f} of the bar, threshold margin {margin:.1e}, rows {len(rows)}")
    assert lay <= LAYER_REL[0] / 5 and sc <= SCORE_ATOL[0] / 5 and bx <= 0.2
    assert margin > 5e-6 and len(rows) == len(rows64)
    assert 5 <= len(rows) <= 60
    return len(rows)


def _layers(name):
    return [n for n in LAYERS + (["model.3.maxpool", "model.16.maxpool"] if name[0] == "c" else [])]


def _check(det, name, half=False):
    """Layers, raw output and final rows of det on the case's frame against the restatement"""
    from oracle.yolov8_ref import detect, letterbox
    from yolov9_ref import Yolov9Ref

    w, imgsz, hw, ref, ref_raw, _ = _ref(name)
    frame = _frame(0, hw)
    if half:
        ref = Yolov9Ref(w, emulate_half=True)
        ref_raw = ref.forward(letterbox(frame, imgsz, False, half=True)[0])[0].numpy()
    h = int(half)
    got = det.detect(frame)
    for lname in _layers(name):
        a, r = det.layer_output(lname), ref.acts[lname][0].permute(1, 2, 0).numpy()
        assert a.shape == r.shape, lname
        err = np.abs(a - r).max() / (np.abs(r).max() + 1e-6)
        print(f"{lname}: rel-to-max error {err:.3e}")
        assert err < LAYER_REL[h], f"{lname}: rel-to-max error {err:.3e}"
        if lname.endswith(".pool"):                      # the zero border the stride-2 convolution reads as its pad: bit-zero
            assert not a[-1].any() and not a[:, -1].any(), lname
    raw = det.raw_output()
    assert raw.shape == ref_raw.shape
    print("scores", np.abs(raw[:, 4:] - ref_raw[:, 4:]).max(), "boxes", np.abs(raw[:, :4] - ref_raw[:, :4]).max())
    np.testing.assert_allclose(raw[:, 4:], ref_raw[:, 4:], atol=SCORE_ATOL[h])
    np.testing.assert_allclose(raw[:, :4], ref_raw[:, :4], rtol=BOX_RTOL[h], atol=BOX_ATOL[h])
    xyxy, conf, cls = detect(ref, frame, imgsz, False, KW["conf"], KW["iou"], KW["classes"], True, KW["max_det"])
    print(f"{name}: {len(got)} rows, restatement {len(conf)}")
    if half:                                            # fp16 scores move across conf: test_yolov10_gpu's half branch
        assert len(conf) > 0 and abs(len(got) - len(conf)) <= max(3, len(conf) // 10)
        return got
    assert 5 <= len(got) == len(conf) <= 60
    assert np.all(np.diff(got.conf) <= 0)
    gx, gc, gk = _by_position(got.xyxy, got.conf, got.cls)
    rx, rc, rk = _by_position(xyxy, conf, cls)
    np.testing.assert_array_equal(gk, rk)
    np.testing.assert_allclose(gc, rc, atol=CONF_ATOL)
    np.testing.assert_allclose(gx, rx, atol=XYXY_ATOL)
    return got


# ---------------------------------------------------------------------------- AConv and ADown as blocks, through the op emitter
@pytest.mark.parametrize("path", ["split", "exact", "half"])
@pytest.mark.parametrize("scale", ["t", "c"])
def test_down_blocks_through_the_emitter(gtx_ctx, path, scale):
    """model.3 inside a built detector (the op emitter is reached through a whole graph only): the pool launch and the convolution(s)
    behind it on the detector's own 16 x 16 model.2 output (imgsz 64; 32 channels in scale t, AConv; 256 in scale c, ADown -- not the
    16 channels the issue names, which no scale has at a downsampling row), against the restatement's block fed that same map, so an
    error upstream does not enter. The restatement's convolution runs stride 2, pad 1 on the 15 x 15 average; the HIP path's on the
    zero-bordered 16 x 16 one. The kernel on its own, 16 x 16 x 16 included: tests/test_pool_down_ops_gpu.py."""
    import torch
    from geotrax_amd.detector import Detector
    from yolov9_ref import Yolov9Ref

    name = scale + "64"
    w, imgsz, hw = _case(name)
    half = path == "half"
    det = Detector(w, hw, imgsz=imgsz, half=half, fp32_split=path == "split", ctx=gtx_ctx, **KW)
    det.detect(_frame(0, hw))
    x = det.layer_output("model.2")
    assert x.shape[:2] == (16, 16)
    ref = Yolov9Ref(w, emulate_half=half)
    want = ref._down("model.3", torch.from_numpy(np.ascontiguousarray(x.transpose(2, 0, 1)))[None])[0].permute(1, 2, 0).numpy()
    got = det.layer_output("model.3")
    for lname, r in [("model.3.pool", ref.acts["model.3.pool"][0].permute(1, 2, 0).numpy()), ("model.3", want)] + \
                    ([("model.3.maxpool", ref.acts["model.3.maxpool"][0].permute(1, 2, 0).numpy())] if scale == "c" else []):
        a = det.layer_output(lname)
        assert a.shape == r.shape, lname
        err = np.abs(a - r).max() / (np.abs(r).max() + 1e-6)
        print(f"{lname}: rel-to-max error {err:.3e}")
        assert err < LAYER_REL[int(half)], f"{lname}: {err:.3e}"
    assert got.shape == (8, 8, 64 if scale == "t" else 256)
    det.close()


# ---------------------------------------------------------------------------- the whole network
@pytest.mark.parametrize("path", ["split", "exact", "half"])
@pytest.mark.parametrize("name", ["t64", "t96", "c64", "c96", "m64"])
def test_yolov9_matches_restatement(gtx_ctx, name, path):
    from geotrax_amd.detector import Detector

    _rule(name)
    w, imgsz, hw = _case(name)
    det = Detector(w, hw, imgsz=imgsz, half=path == "half", fp32_split=path == "split", ctx=gtx_ctx, **KW)
    # the sparse box branch needs Detect inputs of whole 32-channel chunks: yolov9m's padded 368 is not, its box layers run dense
    assert det.graph == "yolov9" and not det.end2end and det.sparse_box()[0] == (path == "split" and name != "m64")
    _check(det, name, half=path == "half")
    det.close()


def test_self_consistency(gtx_ctx, monkeypatch):
    """On the letterboxed frame: detectors built with GTX_SPARSE_BOX=0 and with GTX_PAD_SKIP=0 give the default's rows bit for bit; a
    batch of 2 equals two single passes; submit / collect equals the blocking call."""
    from geotrax_amd.detector import Detector

    w, imgsz, hw = _case("t64")
    frames = np.stack([_frame(s, hw) for s in range(2)])
    kw = dict(imgsz=imgsz, max_batch=2, ctx=gtx_ctx, **KW)
    det = Detector(w, hw, **kw)
    others = []
    for var in ("GTX_PAD_SKIP", "GTX_SPARSE_BOX"):
        with monkeypatch.context() as mp:
            mp.setenv(var, "0")
            others.append(Detector(w, hw, **kw))
    assert others[0].pad_skip()[0] is False and others[1].sparse_box() == (False, 0)
    singles = [det.detect(f) for f in frames]
    assert 5 <= len(singles[0]) <= 60
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
    for o in others + [det]:
        o.close()


def test_saturation_falls_back_to_exact(gtx_ctx):
    """An amplifying seed (activations beyond fp16's range): the split-f16x3 detector re-runs the pass on its exact-fp32 twin -- the
    same YOLOv9 graph, pooling launches included -- and from then on equals the exact detector bit for bit."""
    from geotrax_amd.detector import Detector
    from geotrax_amd.weights import synthetic_yolov9
    from oracle.yolov8_ref import letterbox
    from yolov9_ref import Yolov9Ref

    hw = (48, 80)
    w = synthetic_yolov9(seed=3, nc=4, scale="t", cls_bias=-3.0, gain=1.6)
    frames = [_frame(0, hw), _frame(1, hw)]
    ref = Yolov9Ref(w)
    ref.forward(letterbox(frames[0], 64, False)[0])
    assert max(float(v.abs().max()) for v in ref.acts.values()) > 65504.0     # the case is what it claims to be
    kw = dict(imgsz=64, ctx=gtx_ctx, **KW)
    det = Detector(w, hw, fp32_split=True, **kw)
    first = det.detect(frames[0])
    assert det.saturated() and det.fell_back()
    exact = Detector(w, hw, fp32_split=False, **kw)
    np.testing.assert_array_equal(first.conf, exact.detect(frames[0]).conf)
    for f in frames:
        a, b = det.detect(f), exact.detect(f)
        np.testing.assert_array_equal(a.xyxy, b.xyxy)
        np.testing.assert_array_equal(a.conf, b.conf)
        np.testing.assert_array_equal(det.raw_output(), exact.raw_output())
    det.close(); exact.close()


def test_obj_feats(gtx_ctx):
    """`with_reid: true, model: auto`: the head is YOLOv8's Detect, so the appearance vectors of the kept rows are the restatement's
    table at the kept anchors (the bar of the layers). Scale c: its Detect inputs (256 / 512 / 512 channels) are multiples of the
    narrowest, which ultralytics' own reshape needs; the other scales' are not and are refused by name (tests/test_yolov9.py)."""
    from geotrax_amd.detector import Detector
    from oracle.yolov8_ref import detect

    w, imgsz, hw, ref, _, _ = _ref("c64")
    det = Detector(w, hw, imgsz=imgsz, obj_feats=True, ctx=gtx_ctx, **KW)
    got = det.detect(_frame(0, hw))
    xyxy, conf, cls, feats = detect(ref, _frame(0, hw), imgsz, False, KW["conf"], KW["iou"], KW["classes"], True, KW["max_det"], return_feats=True)
    assert 5 <= len(got) == len(conf) and got.feats.shape == feats.shape
    o, r = np.argsort(-got.conf, kind="stable"), np.argsort(-conf, kind="stable")
    assert np.abs(got.feats[o] - feats[r]).max() <= LAYER_REL[0] * np.abs(feats).max()
    det.close()


def test_through_the_wrapper(gtx_ctx, tmp_path):
    """YOLO(<yolov9t file>).track with ByteTrack over 3 small frames returns ids, and its boxes are the interface-level detector's
    + tracker's on the same frames; the wrapper names the yaml by its scale."""
    from geotrax_amd.detector import Detector
    from geotrax_amd.model import YOLO
    from geotrax_amd.tracker import Tracker
    from geotrax_amd.weights import save_weights

    w, imgsz, hw = _case("t64")
    path = tmp_path / "yolov9t.safetensors"
    save_weights(w, path)
    model = YOLO(str(path), ctx=gtx_ctx)
    assert model.yaml_file == "yolov9t.yaml" and model.names == {0: "0", 1: "1", 2: "2", 3: "3"}
    spec = dict(tracker_type="bytetrack", track_high_thresh=0.25, track_low_thresh=0.1, new_track_thresh=0.25, track_buffer=30, match_thresh=0.8,
                fuse_score=True)
    det = Detector(w, hw, imgsz=imgsz, conf=0.25, iou=0.7, max_det=300, agnostic_nms=False, ctx=gtx_ctx)
    trk = Tracker("bytetrack", **{k: v for k, v in spec.items() if k != "tracker_type"})
    total = 0
    for t in range(3):
        frame = _frame(t, hw)
        res = model.track(frame, persist=True, tracker=spec, imgsz=imgsz, conf=0.25, max_det=300)[0]
        d = det.detect(frame)
        xyxy, ids, score, cls, _ = trk.update(d.xyxy, d.conf, d.cls)
        if len(ids):
            np.testing.assert_array_equal(res.boxes._xyxy, xyxy)
            np.testing.assert_array_equal(np.asarray(res.boxes.id).ravel().astype(np.int64), np.asarray(ids).astype(np.int64))
            total += len(ids)
    assert total > 0
    det.close()
