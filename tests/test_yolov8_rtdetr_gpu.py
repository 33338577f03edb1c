"""YOLOv8-RTDETR on the GPU (csrc/yolo_trunk.cpp + csrc/rtdetr.cpp: the YOLOv8 detector's trunk feeding the RT-DETR decoder at
model.22) against tests/yolov8_rtdetr_ref.py through the C ABI. Bars: test_rtdetr_gpu.py's (each probed layer <= 2e-4 of the layer
maximum on both fp32-grade paths, the same 300 queries up to near-ties, raw boxes / scores <= 1e-4, the same detections), the
trunk bit-identical to a YOLOv8 Detector's where letterbox and stretch agree, and the extract chain against the oracle chain."""
import argparse
import logging
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from test_rtdetr_gpu import _frame, _rel

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
FRAME_HW = (432, 768)
D = "model.22"
TRUNK = ["model.0.conv", "model.2", "model.4", "model.6", "model.8", "model.9", "model.12", "model.15", "model.18", "model.21"]


@pytest.fixture(scope="module")
def weights():
    from geotrax_amd.weights import synthetic_yolov8_rtdetr

    return synthetic_yolov8_rtdetr(seed=3, nc=4, scale="s")


def _check(det, ref, frame, imgsz, conf, classes, bar=2e-4, layers=TRUNK):
    from oracle.rtdetr_ref import postprocess, stretch

    got = det.detect(frame)
    pred = ref.forward(stretch(frame, imgsz))[0].numpy()
    worst = {}
    for name in layers:
        a = det.layer_output(name)
        r = ref.acts[name][0].permute(1, 2, 0).numpy()
        assert a.shape == r.shape, (name, a.shape, r.shape)
        worst[name] = _rel(a, r)
        assert worst[name] <= bar, (name, worst[name])
    shapes = [(imgsz // s, imgsz // s) for s in (8, 16, 32)]
    _, valid = ref._anchors(shapes)
    feats = (ref.acts[D + ".feats"] * valid)[0].numpy()
    enc, scores = ref.acts[D + ".enc_output"][0].numpy(), ref.acts[D + ".enc_scores"][0].numpy()
    o = 0
    for l, (h, w) in enumerate(shapes):
        for name, r in (("feats", feats), ("enc_output", enc), ("enc_scores", scores)):
            a = det.layer_output(f"{D}.{name}.{l}").reshape(h * w, -1)[:, :r.shape[1]]
            e = _rel(a, r[o:o + h * w])
            worst[f"{D}.{name}.{l}"] = e
            assert e <= bar, (name, l, e)
        o += h * w
    # the same queries up to swaps of near-ties (test_rtdetr_gpu._check_against_oracle explains the rule)
    idx = det.layer_output_int(D + ".topk").ravel()
    want_idx = ref.topk[0].numpy()
    inval = ~valid[0, :, 0].numpy()
    key = ref.acts[D + ".enc_scores"][0].max(-1).values.numpy()
    assert sorted(idx[~inval[idx]]) == sorted(want_idx[~inval[want_idx]]) and inval[idx].sum() == inval[want_idx].sum()
    moved = idx != want_idx
    assert np.abs(key[idx[moved]] - key[want_idx[moved]]).max(initial=0) <= 1e-5 * np.abs(key).max(), "queries out of order beyond a near-tie"
    pos = {int(a): j for j, a in enumerate(want_idx) if not inval[a]}
    spare = [j for j, a in enumerate(want_idx) if inval[a]]
    to_ref = np.array([pos[int(a)] if not inval[a] else spare.pop() for a in idx])
    for i in range(ref.ndl):
        a = det.layer_output(f"{D}.decoder.layers.{i}")[0]
        r = ref.acts[f"{D}.decoder.layers.{i}"][0].numpy()[to_ref]
        e = _rel(a, r)
        worst[f"decoder.{i}"] = e
        assert e <= bar, (i, e)
    raw = det.raw_output()
    assert raw.shape == pred.shape
    np.testing.assert_allclose(raw[:, :4], pred[to_ref, :4], atol=1e-4)
    np.testing.assert_allclose(raw[:, 4:], pred[to_ref, 4:], atol=1e-4)
    xyxy, score, cls, _ = postprocess(pred, frame.shape[:2], conf, classes, det.max_det)
    assert len(got) == len(score) > 0
    np.testing.assert_allclose(got.conf, score, atol=1e-4)
    tol = 0.05 * max(frame.shape[:2]) / 640
    for k in range(len(score)):
        near = np.flatnonzero(np.abs(score - got.conf[k]) <= 1e-4)
        d = np.abs(xyxy[near] - got.xyxy[k]).max(1)
        assert d.min() <= tol and cls[near[d.argmin()]] == got.cls[k], (k, d.min())
    return got, pred, worst


@pytest.mark.parametrize("split", [False, True])
def test_hybrid_matches_oracle(gtx_ctx, weights, split):
    from geotrax_amd.detector import Detector
    from yolov8_rtdetr_ref import YoloV8RtDetrRef

    det = Detector(weights, FRAME_HW, imgsz=640, conf=0.3, max_det=300, classes=[0, 1, 3], fp32_split=split, ctx=gtx_ctx)
    assert det.rtdetr and det.graph == "yolov8-rtdetr" and det.net_hw == (640, 640) and det.n_queries == 300
    assert det.pad_skip() == (False, 0, 0) and det.sparse_box() == (False, 0)   # stretched input, no Detect head
    got, _, worst = _check(det, YoloV8RtDetrRef(weights), _frame(0), 640, 0.3, [0, 1, 3])
    print({k: f"{v:.1e}" for k, v in worst.items()})
    assert 0 < len(got) < 300 and not det.saturated()
    det.close()


@pytest.mark.parametrize("split", [True, False])
def test_hybrid_4k_matches_oracle(gtx_ctx, weights, split):
    """The reference configuration: 3840 x 2160 stretched to 1920 x 1920 (75 600 anchors) on both fp32-grade paths."""
    from geotrax_amd.detector import Detector
    from yolov8_rtdetr_ref import YoloV8RtDetrRef

    hw = (2160, 3840)
    det = Detector(weights, hw, imgsz=1920, conf=0.25, max_det=300, fp32_split=split, ctx=gtx_ctx)
    assert det.net_hw == (1920, 1920)
    got, _, worst = _check(det, YoloV8RtDetrRef(weights), _frame(0, hw), 1920, 0.25, None,
                           layers=["model.0.conv", "model.2", "model.9", "model.15", "model.18", "model.21"])
    print({k: f"{v:.1e}" for k, v in worst.items()})
    assert len(got) > 0 and not det.saturated()
    det.close()


@pytest.mark.parametrize("split", [True, False])
def test_hybrid_trunk_is_the_yolov8_detector_trunk(gtx_ctx, split):
    """A square frame at its own size: letterbox and stretch give the same image, so the hybrid's model.15 / 18 / 21 are those of a
    YOLOv8 Detector built from synthetic_yolov8 with the same seed -- bit for bit, the same trunk code under the same conventions."""
    from geotrax_amd.detector import Detector
    from geotrax_amd.weights import synthetic_yolov8, synthetic_yolov8_rtdetr

    frame = _frame(5, (640, 640))
    hy = Detector(synthetic_yolov8_rtdetr(seed=9, nc=4, scale="s"), (640, 640), imgsz=640, fp32_split=split, ctx=gtx_ctx)
    v8 = Detector(synthetic_yolov8(seed=9, nc=4, scale="s"), (640, 640), imgsz=640, fp32_split=split, ctx=gtx_ctx)
    assert hy.net_hw == v8.net_hw == (640, 640)
    hy.detect(frame)
    v8.detect(frame)
    for name in ("model.9", "model.15", "model.18", "model.21"):
        a, b = hy.layer_output(name), v8.layer_output(name)
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), name
    hy.close()
    v8.close()


@pytest.mark.parametrize("scale", ["n", "m"])
def test_hybrid_other_scales_match_oracle(gtx_ctx, scale):
    """input_proj on 64 / 128 / 256 (n) and 192 / 384 / 576 (m) channels."""
    from geotrax_amd.detector import Detector
    from geotrax_amd.weights import synthetic_yolov8_rtdetr
    from yolov8_rtdetr_ref import YoloV8RtDetrRef

    w = synthetic_yolov8_rtdetr(seed=4, nc=4, scale=scale)
    det = Detector(w, FRAME_HW, imgsz=640, conf=0.25, max_det=300, ctx=gtx_ctx)
    _check(det, YoloV8RtDetrRef(w), _frame(1), 640, 0.25, None, layers=["model.0.conv", "model.9", "model.15", "model.18", "model.21"])
    det.close()


def test_hybrid_batch_of_two_equals_two_single_passes(gtx_ctx, weights):
    from geotrax_amd.detector import Detector

    f0, f1 = _frame(1), _frame(2)
    det = Detector(weights, FRAME_HW, imgsz=480, conf=0.25, max_det=100, max_batch=2, ctx=gtx_ctx)
    a0, a1 = det.detect(f0), det.detect(f1)
    both = np.ascontiguousarray(np.stack([f0, f1]))
    dptr = gtx_ctx.dev_alloc(both.nbytes)
    try:
        gtx_ctx.dev_upload(dptr, both)
        b0, b1 = det.detect_dev(dptr, 2)
    finally:
        gtx_ctx.dev_free(dptr)
    for a, b in ((a0, b0), (a1, b1)):
        assert len(a) == len(b) > 0
        assert a.xyxy.tobytes() == b.xyxy.tobytes() and a.conf.tobytes() == b.conf.tobytes() and (a.cls == b.cls).all()
    det.close()


def test_hybrid_half_precision_maps(gtx_ctx, weights):
    """half=True: the trunk on the YOLOv8 detector's fp16 maps, the decoder's input projections reading them; held against the fp32
    oracle as loosely as test_rtdetr_half_precision_maps."""
    from geotrax_amd.detector import Detector
    from oracle.rtdetr_ref import stretch
    from yolov8_rtdetr_ref import YoloV8RtDetrRef

    frame = _frame(0)
    det = Detector(weights, FRAME_HW, imgsz=640, conf=0.3, max_det=300, half=True, ctx=gtx_ctx)
    assert det.rtdetr and not det.fp32_split
    got = det.detect(frame)
    ref = YoloV8RtDetrRef(weights)
    pred = ref.forward(stretch(frame, 640))[0].numpy()
    for name in ["model.0.conv", "model.2", "model.9", "model.15", "model.18", "model.21"]:
        a = det.layer_output(name)
        r = ref.acts[name][0].permute(1, 2, 0).numpy()
        assert a.shape == r.shape and _rel(a, r) <= 3e-2, (name, _rel(a, r))
    idx = set(det.layer_output_int(D + ".topk").ravel().tolist())
    assert len(idx & set(ref.topk[0].numpy().tolist())) >= 240
    raw = det.raw_output()
    assert raw.shape == pred.shape and np.isfinite(raw).all() and (raw[:, :4] >= 0).all() and (raw[:, :4] <= 1).all()
    n_ref = int((pred[:, 4:].max(1) > 0.3).sum())
    assert abs(len(got) - n_ref) <= max(5, n_ref // 4)
    det.close()


def test_hybrid_saturating_checkpoint_falls_back_to_the_exact_kernels(gtx_ctx, weights, caplog):
    """Stem weights x 3e4 put the stem's output beyond fp16's range: the split pass is re-run on the exact-fp32 twin (make_exact
    builds the same hybrid) and stays there -- the boxes, scores and queries of a detector built with fp32_split=False, bit for bit."""
    from geotrax_amd.detector import Detector

    w = dict(weights)
    w["model.0.conv.weight"] = (weights["model.0.conv.weight"] * np.float32(3e4)).astype(np.float32)
    frame = _frame(0)
    kw = dict(imgsz=320, conf=0.25, max_det=300, ctx=gtx_ctx)
    exact = Detector(w, FRAME_HW, fp32_split=False, **kw)
    want = exact.detect(frame)
    assert np.abs(exact.layer_output("model.0.conv")).max() > 65504.0
    det = Detector(w, FRAME_HW, fp32_split=True, **kw)
    assert not det.fell_back()
    with caplog.at_level(logging.WARNING, logger="geotrax_amd.detector"):
        got = det.detect(frame)
    assert det.saturated() and det.fell_back() and "exact-fp32" in caplog.text
    assert len(got) == len(want)
    np.testing.assert_array_equal(got.xyxy, want.xyxy)
    np.testing.assert_array_equal(got.conf, want.conf)
    np.testing.assert_array_equal(det.raw_output(), exact.raw_output())
    np.testing.assert_array_equal(det.layer_output_int(D + ".topk"), exact.layer_output_int(D + ".topk"))
    again = det.detect(_frame(1))
    np.testing.assert_array_equal(again.conf, exact.detect(_frame(1)).conf)
    det.close()
    exact.close()


def _hybrid_weights_file(tmp_path, gtx_ctx, probe_frame, H, W, imgsz):
    """Seeded YOLOv8s-RTDETR weights whose last score head is shifted so that ~40 of the 300 queries clear conf on the probe frame."""
    from geotrax_amd.detector import Detector
    from geotrax_amd.weights import calibrate_rtdetr_scores, save_weights, synthetic_yolov8_rtdetr

    w = synthetic_yolov8_rtdetr(seed=3, nc=4, scale="s")
    det = Detector(w, (H, W), imgsz=imgsz, ctx=gtx_ctx)
    det.detect(probe_frame)
    w = calibrate_rtdetr_scores(w, det.raw_output(logits=True)[:, 4:], 0.25, 40)
    det.close()
    path = tmp_path / "yolov8s-rtdetr.safetensors"
    save_weights(w, path)
    path.with_suffix(".names.yaml").write_text("{0: car, 1: bus, 2: truck, 3: motorcycle}\n")
    return path, w


@pytest.mark.parametrize("tracker", ["bytetrack", "botsort+cls"])
def test_hybrid_extract_path_matches_oracle_chain(gtx_ctx, tmp_path, monkeypatch, tracker):
    """test_extract_gpu.test_extract_path_matches_oracle_chain with a YOLOv8-RTDETR file; the oracle chain runs the hybrid oracle in
    RtDetrRef's place. botsort+cls: BoT-SORT with `with_reid: true, model: <YOLOv8-cls file>` (the ReID network's vectors)."""
    import test_extract_gpu as te
    import yaml
    from geotrax_amd import extract as ex
    from geotrax_amd.config_utils import load_config_all
    from geotrax_amd.synth import make_scene
    from geotrax_amd.weights import save_weights, synthetic_yolov8_cls
    from oracle import rtdetr_ref
    from yolov8_rtdetr_ref import YoloV8RtDetrRef

    H, W, NF = te.H, te.W, te.NF
    cls = tracker.endswith("+cls")
    tracker = tracker.split("+")[0]
    scene = make_scene(seed=2, h=H, w=W)
    frames = np.stack([scene.render(t, 150) for t in range(0, NF * 12, 12)])
    src = tmp_path / "clip.npy"
    np.save(src, frames)
    wpath, w = _hybrid_weights_file(tmp_path, gtx_ctx, frames[0], H, W, te.IMGSZ)
    cfg_path, cfg = te._cfg_file(tmp_path, wpath, tracker=tracker)
    if cls:
        tcls = synthetic_yolov8_cls(seed=8, scale="n")
        save_weights(tcls, tmp_path / "cls.safetensors")
        cfg["tracker"]["botsort"].update(with_reid=True, model=str(tmp_path / "cls.safetensors"))
        cfg_path.write_text(yaml.safe_dump(cfg))
    args = argparse.Namespace(source=str(src), cfg=cfg_path, output_folder=None, log_path=None, verbose=False, model=None,
                              class_names=None, conf=None, classes=None, cut_frame_left=None, cut_frame_right=None, interpolate=None)
    model = ex.load_detector(args, logging.getLogger("test_yolov8_rtdetr"))
    assert model.model.yaml_file == "yolov8-rtdetr.yaml"
    config = load_config_all(args, logging.getLogger("test_yolov8_rtdetr"), model_names=model.names)
    args.cut_frame_left, args.cut_frame_right = 0, None
    tracks, transforms = ex.track_with_model(model, config, logging.getLogger("test_yolov8_rtdetr"))
    ref_cfg = cfg
    if cls:
        import copy

        import reid_ref
        from oracle import bytetrack_ref

        class ClsReidRef(bytetrack_ref.ByteTrackRef):     # the oracle BoT-SORT fed with the ReID network's vectors of the oracle's boxes
            def __init__(self, **kw):
                super().__init__(**{**kw, "with_reid": True})
                self.frame = 0

            def update(self, xyxy, conf, cls_, gmc=None, feats=None):
                f = frames[self.frame]
                self.frame += 1
                feats = reid_ref.embed(tcls, f, np.asarray(xyxy, np.float32))[1] if len(xyxy) else None
                return super().update(xyxy, conf, cls_, gmc=gmc, feats=feats)

        monkeypatch.setattr(bytetrack_ref, "ByteTrackRef", ClsReidRef)
        ref_cfg = copy.deepcopy(cfg)
        ref_cfg["tracker"]["botsort"]["with_reid"] = False  # the chain's own `model: auto` vectors are off; ClsReidRef brings the cls ones
    monkeypatch.setattr(rtdetr_ref, "RtDetrRef", YoloV8RtDetrRef)
    ref_tracks, ref_transforms = te._oracle_chain(frames, w, ref_cfg)

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


def test_hybrid_extract_cli(gtx_ctx, tmp_path):
    """python -m geotrax_amd.extract on a short .npy clip with --model pointing at a YOLOv8-RTDETR file."""
    import test_extract_gpu as te
    import yaml
    from geotrax_amd.synth import make_scene

    scene = make_scene(seed=4, h=te.H, w=te.W)
    frames = np.stack([scene.render(t, 150) for t in range(0, 48, 12)])
    src = tmp_path / "clip.npy"
    np.save(src, frames)
    wpath, _ = _hybrid_weights_file(tmp_path, gtx_ctx, frames[0], te.H, te.W, te.IMGSZ)
    other, _ = te._weights_file(tmp_path, gtx_ctx, frames[0])     # the config names a yolov8 file: --model overrides it
    cfg_path, _ = te._cfg_file(tmp_path, other, tracker="bytetrack")
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, "-m", "geotrax_amd.extract", str(src), "--cfg", str(cfg_path), "--model", str(wpath),
                        "--output-folder", str(out)], cwd=tmp_path, env={**os.environ, "PYTHONPATH": str(ROOT / "geo-trax_amd")},
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    rows = np.loadtxt(out / "clip.txt", delimiter=",", ndmin=2)
    assert rows.shape[1] == 14 and len(rows) > 0 and set(np.unique(rows[:, 0])) <= {0, 1, 2, 3}
    assert "yolov8s-rtdetr" in str(yaml.safe_load((tmp_path / "clip.yaml").read_text())["model"])


def test_hybrid_tracks_with_cls_model_and_refuses_auto(gtx_ctx, tmp_path, weights):
    from geotrax_amd.model import YOLO
    from geotrax_amd.synth import make_scene
    from geotrax_amd.weights import save_weights, synthetic_yolov8_cls

    scene = make_scene(seed=3, h=FRAME_HW[0], w=FRAME_HW[1])
    frames = [scene.render(t, 150) for t in range(0, 36, 12)]
    w, _ = _hybrid_weights_file(tmp_path, gtx_ctx, frames[0], FRAME_HW[0], FRAME_HW[1], 384)
    save_weights(synthetic_yolov8_cls(seed=8, scale="n"), tmp_path / "cls.safetensors")
    model = YOLO(str(w), ctx=gtx_ctx)
    spec = {"tracker_type": "botsort", "with_reid": True, "model": str(tmp_path / "cls.safetensors"), "gmc_method": "none"}
    n = 0
    for f in frames:
        r = model.track(f, imgsz=384, conf=0.25, tracker=spec, persist=True)[0]
        n += len(r.boxes)
    assert n > 0 and model._reid is not None
    with pytest.raises(NotImplementedError):
        YOLO(str(w), ctx=gtx_ctx).track(frames[0], imgsz=384, tracker=dict(spec, model="auto"))


def test_hybrid_per_launch_profile_has_every_launch(gtx_ctx, weights, monkeypatch):
    """Detector.profile per launch (GTX_PROFILE_PER_OP) returns one row for each launch of the pass -- the hybrid has far more than
    64 -- and its totals are the per-family table's: the decoder's query side (rt_linear, rt_mha32, rt_deform, ...) is in both."""
    from geotrax_amd.detector import Detector

    det = Detector(weights, FRAME_HW, imgsz=640, max_batch=2, ctx=gtx_ctx)
    det.detect(_frame(0))
    fam = det.profile(2, 2)
    monkeypatch.setenv("GTX_PROFILE_PER_OP", "1")
    ops = det.profile(2, 2)
    monkeypatch.delenv("GTX_PROFILE_PER_OP")
    n = sum(r["launches"] for r in fam) // 2
    assert n > 64 and len(ops) == n and all(r["launches"] == 2 for r in ops)
    names = [r["kernel"].split(" ", 1)[1] for r in ops]
    assert names[-1] == D + ".dec_score_head.5" and f"{D}.decoder.layers.5.cross_attn" in names
    assert abs(sum(r["flops"] for r in ops) - sum(r["flops"] for r in fam)) <= 1e-9 * sum(r["flops"] for r in fam)
    assert {"rt_linear_kernel", "rt_deform_kernel", "rt_mha32_kernel"} <= {r["kernel"] for r in fam}
    det.close()
