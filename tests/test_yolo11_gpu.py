"""YOLO11 detectors on the HIP path (C3k2 / C3k blocks, C2PSA attention at model.10, Detect = model.23 with a depthwise class
branch) against tests/yolo11_ref.py: per-layer activations, the raw head output and the detections at four scales, the 4K default
path (padding rows, sparse box branch), batches, the asynchronous pair, the saturation fallback, the appearance vectors of
`with_reid: true, model: auto`, `half: true`, and the extract chain. The bars are tests/test_p2_gpu.py::_check_against_oracle's."""
import argparse
import logging
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
FRAME_HW = (432, 768)
KW = dict(conf=0.25, iou=0.7, max_det=300, classes=[0, 1, 2, 3], agnostic_nms=True)
LAYERS = ["model.2", "model.6", "model.9", "model.10.m.0.attn.qkv.conv", "model.10.m.0.attn.out", "model.10", "model.13", "model.16",
          "model.19", "model.22", "model.23.feat0", "model.23.feat1", "model.23.feat2"]


def _frame(seed=0, hw=FRAME_HW):
    rng = np.random.default_rng(seed)
    h, w = hw
    yy, xx = np.mgrid[0:h, 0:w]
    base = 110 + 50 * np.sin(xx / 37.0) * np.cos(yy / 23.0)
    f = np.stack([base + 20 * rng.standard_normal((h, w)) for _ in range(3)], -1)
    for _ in range(25 * max(1, (h * w) // (432 * 768))):
        x, y = rng.integers(0, w - 40), rng.integers(0, h - 20)
        f[y:y + rng.integers(8, 20), x:x + rng.integers(15, 40)] = rng.integers(150, 255, 3)
    return np.clip(f, 0, 255).astype(np.uint8)


def _level_sizes(net_hw):
    return [(net_hw[0] // s) * (net_hw[1] // s) for s in (8, 16, 32)]


def _calibrated(weights, det, frame, per_level, conf=0.25):
    """tests/test_p2_gpu.py::_calibrated for Detect = model.23: each level's final class conv is scaled down to logits of at most 3
    and shifted so that about per_level[l] anchors of level l clear conf on `frame`."""
    det.detect(frame)
    logits = det.raw_output(logits=True)[:, 4:].max(1).astype(np.float64)
    edges = np.cumsum([0] + _level_sizes(det.net_hw))
    out = dict(weights)
    for l, k in enumerate(per_level):
        lv = np.sort(logits[edges[l]:edges[l + 1]])[::-1]
        if k <= 0:
            continue
        k = min(int(k), len(lv) - 1)
        f = min(1.0, 3.0 / max(np.abs(lv).max(), 1e-6))
        delta = np.log(conf / (1 - conf)) - f * 0.5 * (lv[k - 1] + lv[k])
        name = f"model.23.cv3.{l}.2"
        out[name + ".weight"] = (weights[name + ".weight"] * np.float32(f)).astype(np.float32)
        out[name + ".bias"] = (weights[name + ".bias"] * np.float32(f) + np.float32(delta)).astype(np.float32)
    return out


GAIN = {"n": 1.7, "s": 1.7, "m": 1.5, "l": 1.5, "x": 1.5}


def _weights(gtx_ctx, scale, seed=1, hw=FRAME_HW, imgsz=640, per_level=(60, 40, 20), frame=None, gain=None, **kw):
    """Seeded weights, calibrated per level. The weight gain decides how well a seeded case is conditioned: the YOLO11 stack
    (residual PSA blocks, more layers than YOLOv8) amplifies with depth. Measured on the restatement itself, fp32 against float64,
    on the 640-pixel parity frame: scale m at the generator's default 1.7 has attention scores of 1e5 and an fp32-vs-float64 spread
    of 1.1e-3 on the attention output (bar 2e-4), so m / l / x are drawn at 1.5 (activations below 3, spread 7e-7), as
    test_detector_gpu lowers the gain of the larger YOLOv8 scales. n and s stay at 1.7: at 1.5 and below the class logits of s
    are so flat over neighbouring anchors that fp32 and float64 runs of the restatement already keep different boxes.
    At 1.7 (seed 1) scale s reaches activations of 176 and the restatement's own fp32-vs-float64 spread of the kept confidences is
    9.2e-6, right at the 1e-5 bar: the comparison with the restatement takes the `parity_weights` case instead. box_weight_scale 0.1: DFL logits of O(1) like a trained
    head's (tests/test_p2_gpu.py)."""
    from geotrax_amd.detector import Detector
    from geotrax_amd.weights import synthetic_yolo11

    w = synthetic_yolo11(seed=seed, nc=4, scale=scale, box_weight_scale=0.1, gain=gain or GAIN[scale])
    det = Detector(w, hw, imgsz=imgsz, fp32_split=False, ctx=gtx_ctx, **{**KW, **kw})
    w = _calibrated(w, det, _frame(0, hw) if frame is None else frame, per_level)
    det.close()
    return w


@pytest.fixture(scope="module")
def weights(gtx_ctx):
    """YOLO11-s, every level calibrated for a few dozen candidates on the 640-pixel frame: the amplifying seed (activations up to 176),
    for the tests that hold the library against itself or at looser bars (batches, the asynchronous pair, half, appearance vectors)."""
    return _weights(gtx_ctx, "s")


def _level_of(anchors, net_hw):
    return np.searchsorted(np.cumsum(_level_sizes(net_hw)), anchors, side="right")


def _check_against_oracle(det, frame, weights, imgsz, rect, half, layers=LAYERS, ordered=True):
    from oracle.yolov8_ref import detect, letterbox, non_max_suppression
    from yolo11_ref import Yolo11Ref

    got = det.detect(frame)
    ref = Yolo11Ref(weights, emulate_half=half)
    x, g = letterbox(frame, imgsz, rect, half=half)
    assert det.net_hw == (g["net_h"], g["net_w"])
    ref_raw = ref.forward(x)[0].numpy()
    rel = 2e-4 if not half else 3e-2
    for name in layers:
        a = det.layer_output(name)
        r = ref.acts[name][0].permute(1, 2, 0).numpy()
        assert a.shape == r.shape, name
        err = np.abs(a - r).max() / (np.abs(r).max() + 1e-6)
        print(f"{name}: rel-to-max error {err:.3e}")
        assert err < rel, f"{name}: rel-to-max error {err:.3e}"
    raw = det.raw_output()
    assert raw.shape == ref_raw.shape == (sum(_level_sizes(det.net_hw)), 8)
    print("scores", np.abs(raw[:, 4:] - ref_raw[:, 4:]).max(), "boxes", np.abs(raw[:, :4] - ref_raw[:, :4]).max())
    np.testing.assert_allclose(raw[:, 4:], ref_raw[:, 4:], atol=1e-4 if not half else 2e-2)
    np.testing.assert_allclose(raw[:, :4], ref_raw[:, :4], rtol=2e-5 if not half else 5e-3, atol=2e-3 if not half else 0.5)
    xyxy, conf, cls = detect(ref, frame, imgsz, rect, KW["conf"], KW["iou"], KW["classes"], True, KW["max_det"])
    assert len(conf) > 0
    if not half:
        assert len(got) == len(conf)
        g_cls, g_conf, g_xyxy = got.cls, got.conf, got.xyxy
        if not ordered:                      # hundreds of boxes: two whose scores tie within fp32 summation noise may swap places
            a, b = np.lexsort((g_xyxy[:, 1], g_xyxy[:, 0])), np.lexsort((xyxy[:, 1], xyxy[:, 0]))
            g_cls, g_conf, g_xyxy, cls, conf, xyxy = g_cls[a], g_conf[a], g_xyxy[a], cls[b], conf[b], xyxy[b]
        np.testing.assert_array_equal(g_cls, cls)
        np.testing.assert_allclose(g_conf, conf, atol=1e-5)
        np.testing.assert_allclose(g_xyxy, xyxy, atol=1e-2)
    else:
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
        assert matched >= 0.9 * len(xyxy)
    _, idx = non_max_suppression(ref_raw, KW["conf"], KW["iou"], KW["classes"], True, KW["max_det"], return_idx=True)
    return got, _level_of(idx, det.net_hw)


@pytest.fixture(scope="module")
def parity_weights(gtx_ctx):
    """The scale-s case of the oracle comparison: seed 5 at gain 1.65. Chosen on the restatement alone (fp32 against float64 on the
    CPU, seeds 1-6 at gains 1.7 / 1.65 / 1.6, both `rect` settings), by the rule that its own rounding must sit well below every
    bar it is used with: same kept anchors in both precisions, kept confidences within 2e-6 of each other (a fifth of the 1e-5 bar)
    and no class score closer to `conf` than 5e-6. A seeded YOLO11-s stack either amplifies (activations of 150 to 9 000: seeds 1 at
    1.7, 3, 4, 6; confidences of the two precisions 4e-6 to 1.7e-5 apart, some keep different boxes) or stays near 3 (seeds 1, 2, 5
    at 1.65 and below); of the calm ones most have a score within 1e-6 of the threshold for one `rect` setting. Seed 5 at 1.65 gives
    2e-7 on the kept confidences, 3e-7 on all scores, 1.5e-6 on the layers and threshold margins of 1.1e-5 / 3.1e-5. (Seed 1 at 1.7,
    the `weights` fixture, was the first choice: its restatement spread of 9.2e-6 leaves the 1e-5 bar no room, and both
    arithmetics, the exact-fp32 kernels included, differed from it by 1.7e-5 on 2 of 88 boxes.)"""
    return _weights(gtx_ctx, "s", seed=5, gain=1.65)


def _restatement_spread(weights, frame, imgsz, rect):
    """(kept anchors equal, largest difference of the kept confidences, smallest |score - conf|) of Yolo11Ref in fp32 and float64"""
    from oracle.yolov8_ref import letterbox, non_max_suppression
    from yolo11_ref import Yolo11Ref

    x, _ = letterbox(frame, imgsz, rect)
    a = Yolo11Ref(weights).forward(x)[0].numpy()
    r64 = Yolo11Ref(weights)
    r64.t = {k: v.double() for k, v in r64.t.items()}
    b = r64.forward(x.double())[0].numpy()
    nms = lambda p: non_max_suppression(p.astype(np.float32), KW["conf"], KW["iou"], KW["classes"], True, KW["max_det"], return_idx=True)[1]
    ia, ib = nms(a), nms(b)
    same = np.array_equal(np.sort(ia), np.sort(ib))
    spread = float(np.abs(a[ia, 4:].max(1) - b[ia, 4:].max(1)).max()) if same else np.inf
    return same, spread, float(np.abs(a[:, 4:].max(1) - KW["conf"]).min())


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("rect", [False, True])
def test_yolo11s_detector_matches_oracle(gtx_ctx, parity_weights, split, rect):
    """Every layer, the raw head output and the detections at the project's bars. The 100-odd kept boxes of this case are not
    suppressed by one another and some confidences lie 1e-7 apart, so boxes are paired by position, not by rank (`ordered=False`,
    as tests/test_p2_gpu.py does for its 4K case)."""
    from geotrax_amd.detector import Detector

    weights = parity_weights
    same, spread, margin = _restatement_spread(weights, _frame(0), 640, rect)
    print(f"restatement fp32 vs float64: kept confidences {spread:.1e}, threshold margin {margin:.1e}")
    assert same and spread < 2e-6 and margin > 5e-6                  # the case is what its fixture claims
    det = Detector(weights, FRAME_HW, imgsz=640, rect=rect, fp32_split=split, ctx=gtx_ctx, **KW)
    assert det.graph == "yolo11" and det.fp32_split == split and det.sparse_box()[0] == split
    _, levels = _check_against_oracle(det, _frame(0), weights, 640, rect, False, ordered=False)
    assert set(levels) == {0, 1, 2}                                  # every Detect level contributes kept boxes
    det.close()


@pytest.mark.parametrize("scale", ["n", "m"])
def test_yolo11_scales_match_oracle(gtx_ctx, scale):
    """n: 2 attention heads, c3k only at 6 / 8 / 22, an 8-channel bottleneck hidden layer; m: c3k everywhere, the 512-channel cap."""
    from geotrax_amd.detector import Detector

    w = _weights(gtx_ctx, scale)
    det = Detector(w, FRAME_HW, imgsz=640, fp32_split=True, ctx=gtx_ctx, **KW)
    _, levels = _check_against_oracle(det, _frame(0), w, 640, False, False)
    assert set(levels) == {0, 1, 2}
    det.close()


def test_yolo11x_builds_and_agrees(gtx_ctx):
    """x at imgsz 320: 2 repeats per block, 6 attention heads."""
    from geotrax_amd.detector import Detector

    w = _weights(gtx_ctx, "x", imgsz=320, per_level=(30, 20, 10))
    assert w["model.10.m.1.attn.qkv.conv.weight"].shape[0] == 6 * 128
    det = Detector(w, FRAME_HW, imgsz=320, fp32_split=True, ctx=gtx_ctx, **KW)
    _, levels = _check_against_oracle(det, _frame(0), w, 320, False, False)
    assert set(levels) == {0, 1, 2}
    det.close()


def test_yolo11_half_matches_oracle(gtx_ctx, weights):
    from geotrax_amd.detector import Detector

    det = Detector(weights, FRAME_HW, imgsz=640, half=True, ctx=gtx_ctx, **KW)
    _check_against_oracle(det, _frame(0), weights, 640, False, True)
    det.close()


def test_yolo11_4k_default_path(gtx_ctx, monkeypatch):
    """3840 x 2160 -> 1920 x 1920, rect off (420 + 420 padding rows), default path. The attention makes every row of model.10 and
    of everything behind it depend on the frame: rows may be skipped in model.0-9 only. Against the oracle, and bit-identical to a
    detector built with the row skipping off and to one with the sparse box branch off."""
    from geotrax_amd.detector import Detector

    hw = (2160, 3840)
    frame = _frame(3, hw)
    kw = dict(imgsz=1920, ctx=gtx_ctx, **KW)
    w = _weights(gtx_ctx, "s", seed=0, hw=hw, imgsz=1920, per_level=(200, 80, 40), frame=frame)
    det = Detector(w, hw, **kw)
    on, skipped, total = det.pad_skip()
    assert on and 0 < skipped < total and det.sparse_box()[0]
    got, levels = _check_against_oracle(det, frame, w, 1920, False, False, ordered=False,
                                         layers=["model.2", "model.9", "model.10.m.0.attn.out", "model.10", "model.16", "model.22",
                                                 "model.23.feat0", "model.23.feat2"])
    assert len(got) > 30 and set(levels) == {0, 1, 2}
    others = []
    for var in ("GTX_PAD_SKIP", "GTX_SPARSE_BOX"):
        with monkeypatch.context() as mp:
            mp.setenv(var, "0")
            others.append(Detector(w, hw, **kw))
    assert others[0].pad_skip()[0] is False and others[0].sparse_box()[0]
    assert others[1].pad_skip()[0] and others[1].sparse_box() == (False, 0)
    for f in (frame, _frame(4, hw)):
        a = det.detect(f)
        assert len(a) > 0
        for o in others:
            b = o.detect(f)
            np.testing.assert_array_equal(a.xyxy, b.xyxy)
            np.testing.assert_array_equal(a.conf, b.conf)
            np.testing.assert_array_equal(a.cls, b.cls)
    assert det.sparse_box() == (True, 0)
    det.close()
    for o in others:
        o.close()


@pytest.mark.parametrize("nb", [2, 4])
def test_yolo11_batch_equals_singles(gtx_ctx, weights, nb):
    from geotrax_amd.detector import Detector

    frames = np.stack([_frame(s) for s in range(nb)])
    det = Detector(weights, FRAME_HW, imgsz=640, max_batch=nb, ctx=gtx_ctx, **KW)
    singles = [det.detect(f) for f in frames]
    dptr = gtx_ctx.dev_alloc(frames.nbytes)
    try:
        gtx_ctx.dev_upload(dptr, frames)
        batch = det.detect_dev(dptr, nb)
        det.submit_dev(dptr, nb)                                     # the asynchronous pair gives what the blocking call gives
        late = det.collect()
    finally:
        gtx_ctx.dev_free(dptr)
    assert len(singles[0]) > 0
    for s, b, c in zip(singles, batch, late):
        for other in (b, c):
            np.testing.assert_array_equal(s.xyxy, other.xyxy)
            np.testing.assert_array_equal(s.conf, other.conf)
            np.testing.assert_array_equal(s.cls, other.cls)
    det.close()


def test_yolo11_saturation_falls_back_to_exact(gtx_ctx):
    """A checkpoint whose activations leave fp16's range (the seeded l stack at gain 1.7, as in
    test_detector_gpu.test_saturation_falls_back_to_the_exact_fp32_convolutions): the split-f16x3 detector re-runs the pass on its
    exact-fp32 twin -- the same YOLO11 graph -- and from then on equals the exact detector bit for bit."""
    from geotrax_amd.detector import Detector
    from geotrax_amd.weights import synthetic_yolo11
    from oracle.yolov8_ref import letterbox
    from yolo11_ref import Yolo11Ref

    w = synthetic_yolo11(seed=1, nc=4, scale="l", cls_bias=-3.0, gain=1.7)
    frames = [_frame(0), _frame(1)]
    kw = dict(imgsz=384, half=False, rect=False, ctx=gtx_ctx, **KW)
    ref = Yolo11Ref(w)
    ref.forward(letterbox(frames[0], 384, False)[0])
    peak = max(float(v.abs().max()) for v in ref.acts.values())
    print("largest activation", peak)
    assert peak > 65504.0                                            # the case is what it claims to be
    det = Detector(w, FRAME_HW, fp32_split=True, **kw)
    assert det.fp32_split and not det.fell_back()
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


@pytest.mark.parametrize("split", [True, False])
def test_yolo11_object_features(gtx_ctx, weights, split):
    """`with_reid: true, model: auto`: the vector of a kept box is obj_feats_table() at its anchor; the hook reads Detect's inputs
    (model.16 / 19 / 22), dim = the narrowest (128 for s)."""
    from geotrax_amd.detector import Detector
    from oracle.yolov8_ref import detect
    from yolo11_ref import Yolo11Ref

    frame = _frame(0)
    det = Detector(weights, FRAME_HW, imgsz=640, fp32_split=split, obj_feats=True, ctx=gtx_ctx, **KW)
    d = det.detect(frame)
    ref = Yolo11Ref(weights)
    xyxy, conf, cls, feats = detect(ref, frame, 640, False, KW["conf"], KW["iou"], KW["classes"], True, KW["max_det"], return_feats=True)
    assert d.feats.shape == feats.shape == (len(conf), 128) and len(conf) > 20
    np.testing.assert_array_equal(d.cls, cls)
    np.testing.assert_allclose(d.feats, feats, atol=2e-4 * max(1.0, float(np.abs(feats).max())))
    det.close()


def test_yolo11_extract_path_matches_oracle_chain(gtx_ctx, tmp_path, monkeypatch):
    """The extract chain (ExtractEngine: batched, pipelined detector, ByteTrack + stabilizer) on a YOLO11 weight file equals
    test_extract_gpu's oracle chain fed by the blocking per-frame Detector.detect."""
    import test_extract_gpu as te
    from geotrax_amd import extract as ex
    from geotrax_amd.config_utils import load_config_all
    from geotrax_amd.detector import Detector
    from geotrax_amd.synth import make_scene
    from geotrax_amd.weights import save_weights, synthetic_yolo11
    from oracle import yolov8_ref

    H, W, NF = te.H, te.W, te.NF
    scene = make_scene(seed=2, h=H, w=W)
    frames = np.stack([scene.render(t, 150) for t in range(0, NF * 12, 12)])
    src = tmp_path / "clip.npy"
    np.save(src, frames)
    w = synthetic_yolo11(seed=1, nc=4, scale="s", box_weight_scale=0.002, gain=GAIN["s"])   # boxes of ~46 network pixels: the stabilizer keeps background to match
    det = Detector(w, (H, W), imgsz=te.IMGSZ, rect=True, ctx=gtx_ctx)
    w = _calibrated(w, det, frames[0], (40, 20, 10))
    det.close()
    wpath = tmp_path / "yolo11s.safetensors"
    save_weights(w, wpath)
    wpath.with_suffix(".names.yaml").write_text("{0: car, 1: bus, 2: truck, 3: motorcycle}\n")
    cfg_path, cfg = te._cfg_file(tmp_path, wpath, tracker="bytetrack", with_reid=False)
    args = argparse.Namespace(source=str(src), cfg=cfg_path, output_folder=None, log_path=None, verbose=False, model=None,
                              class_names=None, conf=None, classes=None, cut_frame_left=None, cut_frame_right=None, interpolate=None)
    logger = logging.getLogger("test_yolo11")
    model = ex.load_detector(args, logger)
    assert model.model.yaml_file == "yolo11.yaml"
    config = load_config_all(args, logger, model_names=model.names)
    args.cut_frame_left, args.cut_frame_right = 0, None
    tracks, transforms = ex.track_with_model(model, config, logger)
    # the oracle chain (ByteTrack and stabilizer restatements) fed frame by frame by the blocking Detector.detect
    dets = {}

    def per_frame(_model, frame, imgsz, rect, conf, iou, classes, agnostic, max_det, **_kw):
        key = (imgsz, rect, conf, iou, tuple(classes) if classes is not None else None, agnostic, max_det)
        if key not in dets:
            dets[key] = Detector(w, (H, W), imgsz=imgsz, rect=rect, conf=conf, iou=iou, classes=classes, agnostic_nms=agnostic,
                                 max_det=max_det, ctx=gtx_ctx)
        d = dets[key].detect(frame)
        return d.xyxy, d.conf, d.cls

    monkeypatch.setattr(yolov8_ref, "YoloV8Ref", lambda *a, **k: None)
    monkeypatch.setattr(yolov8_ref, "detect", per_frame)
    ref_tracks, ref_transforms = te._oracle_chain(frames, w, cfg)

    assert tracks.shape == ref_tracks.shape and len(tracks) > 20
    np.testing.assert_array_equal(tracks[:, 0], ref_tracks[:, 0])
    id_map = {}
    for f in np.unique(tracks[:, 0]):
        a, b = tracks[tracks[:, 0] == f], ref_tracks[ref_tracks[:, 0] == f]
        a, b = a[np.lexsort((a[:, 3], a[:, 2]))], b[np.lexsort((b[:, 3], b[:, 2]))]
        np.testing.assert_allclose(a[:, 2:6], b[:, 2:6], atol=2e-2)
        np.testing.assert_allclose(a[:, 6:10], b[:, 6:10], atol=2e-2)
        np.testing.assert_array_equal(a[:, 10], b[:, 10])
        np.testing.assert_allclose(a[:, 11], b[:, 11], atol=1e-5)
        for ia, ib in zip(a[:, 1], b[:, 1]):
            assert id_map.setdefault(int(ia), int(ib)) == int(ib)
    assert len(set(id_map.values())) == len(id_map)
    assert sum(k != v for k, v in id_map.items()) <= 4
    ref_transforms = np.asarray(ref_transforms).reshape(-1, 10)
    assert transforms.shape == ref_transforms.shape
    for a, b in zip(transforms, ref_transforms):
        Ha, Hb = a[1:].reshape(3, 3), b[1:].reshape(3, 3)
        g = np.array([[0, 0, 1], [W, 0, 1], [0, H, 1], [W, H, 1.0]]).T
        pa, pb = Ha @ g, Hb @ g
        assert np.abs(pa[:2] / pa[2] - pb[:2] / pb[2]).max() < 1e-3
