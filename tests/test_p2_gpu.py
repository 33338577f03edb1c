"""YOLOv8-P2 detectors on the HIP path (a fourth Detect level at stride 4, Detect = model.28) against tests/yolov8p2_ref.py:
per-layer activations, the raw head output, the detections, the 4K default path (padding rows, sparse box branch), batches, the
appearance vectors of `with_reid: true, model: auto`, and the extract chain."""
import argparse
import logging
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
FRAME_HW = (432, 768)
KW = dict(conf=0.25, iou=0.7, max_det=300, classes=[0, 1, 2, 3], agnostic_nms=True)
LAYERS = ["model.2", "model.15", "model.18", "model.19.conv", "model.21", "model.24", "model.27",
          "model.28.feat0", "model.28.feat1", "model.28.feat2", "model.28.feat3"]


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
    return [(net_hw[0] // s) * (net_hw[1] // s) for s in (4, 8, 16, 32)]


def _calibrated(weights, det, frame, per_level, conf=0.25):
    """A copy of `weights` whose class heads are rescaled and shifted per Detect level so that about per_level[l] anchors of level l
    clear conf on `frame`. Seeded weights have very different logit ranges per level (up to ~80): each level's final class conv
    (weights and bias) is first scaled down to logits of at most 3, so that the shifted logits are as well conditioned as a trained
    head's, not a small difference of two large numbers."""
    det.detect(frame)
    logits = det.raw_output(logits=True)[:, 4:].max(1).astype(np.float64)
    edges = np.cumsum([0] + _level_sizes(det.net_hw))
    out = dict(weights)
    for l, k in enumerate(per_level):
        lv = np.sort(logits[edges[l]:edges[l + 1]])[::-1]
        if k <= 0:
            continue                                                  # left as it is (silenced by the seeded level_bias)
        k = min(int(k), len(lv) - 1)
        f = min(1.0, 3.0 / max(np.abs(lv).max(), 1e-6))
        delta = np.log(conf / (1 - conf)) - f * 0.5 * (lv[k - 1] + lv[k])
        name = f"model.28.cv3.{l}.2"
        out[name + ".weight"] = (weights[name + ".weight"] * np.float32(f)).astype(np.float32)
        out[name + ".bias"] = (weights[name + ".bias"] * np.float32(f) + np.float32(delta)).astype(np.float32)
    return out


@pytest.fixture(scope="module")
def weights(gtx_ctx):
    """P2-s, every level calibrated for a few dozen candidates on the 640-pixel parity frame."""
    from geotrax_amd.detector import Detector
    from geotrax_amd.weights import synthetic_yolov8_p2

    # box_weight_scale 0.1: DFL logits of O(1) like a trained head's (0.3 gives stride-32 boxes of ~600 px whose sides move by
    # 3e-5 relative under another fp32 summation order, past the raw-output bar)
    w = synthetic_yolov8_p2(seed=1, nc=4, scale="s", level_bias=(0.0, 0.0, 0.0, 0.0), box_weight_scale=0.1)
    det = Detector(w, FRAME_HW, imgsz=640, fp32_split=False, ctx=gtx_ctx, **KW)
    w = _calibrated(w, det, _frame(0), (60, 40, 30, 20))
    det.close()
    return w


def _level_of(anchors, net_hw):
    return np.searchsorted(np.cumsum(_level_sizes(net_hw)), anchors, side="right")


def _check_against_oracle(det, frame, weights, imgsz, rect, half, layers=LAYERS, ordered=True):
    from oracle.yolov8_ref import detect, letterbox, non_max_suppression
    from yolov8p2_ref import YoloV8P2Ref

    got = det.detect(frame)
    ref = YoloV8P2Ref(weights, emulate_half=half)
    x, g = letterbox(frame, imgsz, rect, half=half)
    assert det.net_hw == (g["net_h"], g["net_w"])
    ref_raw = ref.forward(x)[0].numpy()
    rel = 2e-4 if not half else 3e-2
    for name in layers:
        a = det.layer_output(name)
        r = ref.acts[name][0].permute(1, 2, 0).numpy()
        assert a.shape == r.shape, name
        err = np.abs(a - r).max() / (np.abs(r).max() + 1e-6)
        assert err < rel, f"{name}: rel-to-max error {err:.3e}"
    raw = det.raw_output()
    assert raw.shape == ref_raw.shape == (sum(_level_sizes(det.net_hw)), 8)
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


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("rect", [False, True])
def test_p2_detector_matches_oracle(gtx_ctx, weights, split, rect):
    from geotrax_amd.detector import Detector

    det = Detector(weights, FRAME_HW, imgsz=640, rect=rect, fp32_split=split, ctx=gtx_ctx, **KW)
    assert det.p2 and det.fp32_split == split
    _, levels = _check_against_oracle(det, _frame(0), weights, 640, rect, False)
    assert set(levels) == {0, 1, 2, 3}                               # every Detect level contributes kept boxes
    det.close()


def test_p2_half_matches_oracle(gtx_ctx, weights):
    from geotrax_amd.detector import Detector

    det = Detector(weights, FRAME_HW, imgsz=640, half=True, ctx=gtx_ctx, **KW)
    _check_against_oracle(det, _frame(0), weights, 640, False, True)
    det.close()


def test_p2_4k_default_path(gtx_ctx, monkeypatch):
    """3840 x 2160 -> 1920 x 1920 on the default path: padding rows skipped and the sparse box branch on (at the 480 x 480 level
    too), against the oracle, and bit-identical to the same detector with both off."""
    from geotrax_amd.detector import Detector
    from geotrax_amd.weights import synthetic_yolov8_p2

    hw = (2160, 3840)
    frame = _frame(3, hw)
    kw = dict(imgsz=1920, ctx=gtx_ctx, **KW)
    w = synthetic_yolov8_p2(seed=0, nc=4, scale="s", box_weight_scale=0.1)   # default level_bias: the stride-4 and stride-8 heads fire
    probe = Detector(w, hw, **kw)
    w = _calibrated(w, probe, frame, (300, 100, 0, 0))
    probe.close()
    det = Detector(w, hw, **kw)
    assert det.pad_skip()[0] and det.sparse_box()[0]
    got, levels = _check_against_oracle(det, frame, w, 1920, False, False, layers=["model.2", "model.18", "model.28.feat0", "model.28.feat1"],
                                         ordered=False)
    assert len(got) > 30 and {0, 1} <= set(levels)
    monkeypatch.setenv("GTX_PAD_SKIP", "0")
    monkeypatch.setenv("GTX_SPARSE_BOX", "0")
    plain = Detector(w, hw, **kw)
    assert plain.pad_skip()[0] is False and plain.sparse_box() == (False, 0)
    for f in (frame, _frame(4, hw)):
        a, b = det.detect(f), plain.detect(f)
        np.testing.assert_array_equal(a.xyxy, b.xyxy)
        np.testing.assert_array_equal(a.conf, b.conf)
        np.testing.assert_array_equal(a.cls, b.cls)
    assert det.sparse_box() == (True, 0)
    det.close(); plain.close()


def test_p2_batch_equals_singles(gtx_ctx, weights):
    from geotrax_amd.detector import Detector

    frames = np.stack([_frame(s) for s in (0, 1)])
    det = Detector(weights, FRAME_HW, imgsz=640, max_batch=2, ctx=gtx_ctx, **KW)
    singles = [det.detect(f) for f in frames]
    dptr = gtx_ctx.dev_alloc(frames.nbytes)
    try:
        gtx_ctx.dev_upload(dptr, frames)
        batch = det.detect_dev(dptr, 2)
    finally:
        gtx_ctx.dev_free(dptr)
    assert len(singles[0]) > 0
    for s, b in zip(singles, batch):
        np.testing.assert_array_equal(s.xyxy, b.xyxy)
        np.testing.assert_array_equal(s.conf, b.conf)
        np.testing.assert_array_equal(s.cls, b.cls)
    det.close()


@pytest.mark.parametrize("split", [True, False])
def test_p2_object_features_over_four_levels(gtx_ctx, weights, split):
    """`with_reid: true, model: auto`: the vector of a kept box is obj_feats_table() at its anchor, whichever of the four levels it
    came from; dim = the P2 level's width (64 for s)."""
    from geotrax_amd.detector import Detector
    from oracle.yolov8_ref import detect
    from yolov8p2_ref import YoloV8P2Ref

    frame = _frame(0)
    det = Detector(weights, FRAME_HW, imgsz=640, fp32_split=split, obj_feats=True, ctx=gtx_ctx, **KW)
    d = det.detect(frame)
    ref = YoloV8P2Ref(weights)
    xyxy, conf, cls, feats = detect(ref, frame, 640, False, KW["conf"], KW["iou"], KW["classes"], True, KW["max_det"], return_feats=True)
    assert d.feats.shape == feats.shape == (len(conf), 64) and len(conf) > 20
    np.testing.assert_array_equal(d.cls, cls)
    np.testing.assert_allclose(d.feats, feats, atol=2e-4 * max(1.0, float(np.abs(feats).max())))
    det.close()


def _p2_weights_file(tmp_path, gtx_ctx, probe_frame, H, W, imgsz):
    from geotrax_amd.detector import Detector
    from geotrax_amd.weights import save_weights, synthetic_yolov8_p2

    w = synthetic_yolov8_p2(seed=1, nc=4, scale="s", box_weight_scale=0.1)
    det = Detector(w, (H, W), imgsz=imgsz, rect=True, ctx=gtx_ctx)
    w = _calibrated(w, det, probe_frame, (40, 20, 0, 0))
    det.close()
    path = tmp_path / "yolov8s-p2.safetensors"
    save_weights(w, path)
    path.with_suffix(".names.yaml").write_text("{0: car, 1: bus, 2: truck, 3: motorcycle}\n")
    return path, w


@pytest.mark.parametrize("tracker", ["bytetrack", "botsort+reid"])
def test_p2_extract_path_matches_oracle_chain(gtx_ctx, tmp_path, monkeypatch, tracker):
    """test_extract_gpu.test_extract_path_matches_oracle_chain with a P2 weight file: the oracle chain runs YoloV8P2Ref."""
    import test_extract_gpu as te
    from geotrax_amd import extract as ex
    from geotrax_amd.config_utils import load_config_all
    from geotrax_amd.synth import make_scene
    from oracle import yolov8_ref
    from yolov8p2_ref import YoloV8P2Ref

    H, W, NF = te.H, te.W, te.NF
    reid = tracker.endswith("+reid")
    tracker = tracker.split("+")[0]
    scene = make_scene(seed=2, h=H, w=W)
    frames = np.stack([scene.render(t, 150) for t in range(0, NF * 12, 12)])
    src = tmp_path / "clip.npy"
    np.save(src, frames)
    wpath, w = _p2_weights_file(tmp_path, gtx_ctx, frames[0], H, W, te.IMGSZ)
    cfg_path, cfg = te._cfg_file(tmp_path, wpath, tracker=tracker, with_reid=reid)
    args = argparse.Namespace(source=str(src), cfg=cfg_path, output_folder=None, log_path=None, verbose=False, model=None,
                              class_names=None, conf=None, classes=None, cut_frame_left=None, cut_frame_right=None, interpolate=None)
    logger = logging.getLogger("test_p2")
    model = ex.load_detector(args, logger)
    assert model.model.yaml_file == "yolov8-p2.yaml"
    config = load_config_all(args, logger, model_names=model.names)
    args.cut_frame_left, args.cut_frame_right = 0, None
    tracks, transforms = ex.track_with_model(model, config, logger)
    monkeypatch.setattr(yolov8_ref, "YoloV8Ref", YoloV8P2Ref)       # the oracle chain's detector is the P2 graph
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
    assert transforms.shape == ref_transforms.shape == (NF - 1, 10)
    for a, b in zip(transforms, ref_transforms):
        Ha, Hb = a[1:].reshape(3, 3), b[1:].reshape(3, 3)
        g = np.array([[0, 0, 1], [W, 0, 1], [0, H, 1], [W, H, 1.0]]).T
        pa, pb = Ha @ g, Hb @ g
        assert np.abs(pa[:2] / pa[2] - pb[:2] / pb[2]).max() < 1e-3


def test_p2_extract_cli(gtx_ctx, tmp_path):
    """python -m geotrax_amd.extract on a short .npy clip with --model pointing at a P2 file."""
    import test_extract_gpu as te
    from geotrax_amd.synth import make_scene

    scene = make_scene(seed=4, h=te.H, w=te.W)
    frames = np.stack([scene.render(t, 150) for t in range(0, 48, 12)])
    src = tmp_path / "clip.npy"
    np.save(src, frames)
    wpath, _ = _p2_weights_file(tmp_path, gtx_ctx, frames[0], te.H, te.W, te.IMGSZ)
    other, _ = te._weights_file(tmp_path, gtx_ctx, frames[0])     # the config names a yolov8 file: --model overrides it
    cfg_path, _ = te._cfg_file(tmp_path, other, tracker="bytetrack")
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, "-m", "geotrax_amd.extract", str(src), "--cfg", str(cfg_path), "--model", str(wpath),
                        "--output-folder", str(out)], cwd=tmp_path, env={**os.environ, "PYTHONPATH": str(ROOT / "geo-trax_amd")},
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    rows = np.loadtxt(out / "clip.txt", delimiter=",", ndmin=2)
    assert rows.shape[1] == 14 and len(rows) > 0 and set(np.unique(rows[:, 0])) <= {0, 1, 2, 3}
    import yaml

    assert "yolov8s-p2" in str(yaml.safe_load((tmp_path / "clip.yaml").read_text())["model"])
