"""The separate ReID network on the GPU (`with_reid: true, model: <cls checkpoint>`): crops against PIL byte for byte, vectors
against tests/reid_ref.py, the saturation fallback, tracking through YOLO.track and the threaded engine."""
import numpy as np
import pytest

import reid_ref

pytestmark = pytest.mark.gpu

FH, FW = 2160, 3840


def _frame(seed=0, h=FH, w=FW):
    rng = np.random.default_rng(seed)
    small = rng.integers(0, 256, (h // 8 + 1, w // 8 + 1, 3)).astype(np.float32)
    big = np.repeat(np.repeat(small, 8, 0), 8, 1)[:h, :w]                     # blocky texture + noise: resampling errors show
    return np.clip(big + rng.normal(0, 25, (h, w, 3)), 0, 255).astype(np.uint8)


def _boxes(n, seed=1, h=FH, w=FW):
    """Seeded boxes: small (upscaled) and large (downscaled with the widened support), portrait and landscape, at the frame edges."""
    rng = np.random.default_rng(seed)
    size = np.exp(rng.uniform(np.log(2), np.log(1400), (n, 2)))
    size[::7, 0] *= 4                                                          # very wide
    size[3::7, 1] *= 3                                                         # very tall
    x1 = rng.uniform(-30, w - 5, n)
    y1 = rng.uniform(-30, h - 5, n)
    b = np.stack([x1, y1, x1 + size[:, 0], y1 + size[:, 1]], 1)
    b[::5, 0] = 0.0
    b[1::5, 2] = w
    b[2::5, 1] = 0.0
    b[3::5, 3] = h
    b[:, [0, 2]] = b[:, [0, 2]].clip(0, w)
    b[:, [1, 3]] = b[:, [1, 3]].clip(0, h)
    return b.astype(np.float32)


def test_crops_equal_pil_bytes(gtx_ctx):
    pytest.importorskip("PIL")
    from geotrax_amd.reid import ReIDEncoder
    from geotrax_amd.weights import synthetic_yolov8_cls

    frame, boxes = _frame(), _boxes(240)
    enc = ReIDEncoder(synthetic_yolov8_cls(seed=0, scale="n"), ctx=gtx_ctx, max_crops=240)
    v = enc(frame, boxes)
    assert v.shape == (240, enc.dim) and np.isfinite(v).all()
    cb = reid_ref.crop_box(boxes, FH, FW)
    scales = []
    for i in range(len(boxes)):
        want = reid_ref.crop_image(frame, cb[i])
        np.testing.assert_array_equal(enc.crop(i), want, err_msg=f"crop {i} box {cb[i].tolist()}")
        scales.append(min(cb[i][2] - cb[i][0], cb[i][3] - cb[i][1]) / 224)
    assert min(scales) < 0.5 and max(scales) > 3                                 # upscale and antialiased downscale both covered
    enc.close()


_REF = {}


def _reference(scale, n):
    key = scale
    if key not in _REF:
        from geotrax_amd.weights import synthetic_yolov8_cls

        t = synthetic_yolov8_cls(seed=4, scale=scale)
        frame, boxes = _frame(2), _boxes(300, seed=3)
        crops, emb, ref = reid_ref.embed(t, frame, boxes)
        _REF[key] = (t, frame, boxes, emb, {k: v[0].permute(1, 2, 0).numpy() for k, v in ref.acts.items()})
    t, frame, boxes, emb, acts0 = _REF[key]
    return t, frame, boxes[:n], emb[:n], acts0


@pytest.mark.parametrize("scale", ["n", "s"])
@pytest.mark.parametrize("split", [True, False], ids=["split", "exact"])
@pytest.mark.parametrize("n", [1, 37, 300])
def test_embeddings_match_reference(gtx_ctx, scale, split, n):
    from geotrax_amd.reid import ReIDEncoder

    t, frame, boxes, want, acts0 = _reference(scale, n)
    enc = ReIDEncoder(t, ctx=gtx_ctx, fp32_split=split, max_crops=300)
    got = enc(frame, boxes)
    assert got.shape == want.shape == (n, {"n": 256, "s": 512}[scale])
    for layer in ("model.1.conv", "model.2", "model.4", "model.6", "model.7.conv", "model.8"):
        a, b = enc.layer_output(0, layer), acts0[layer]
        assert a.shape == b.shape, layer
        err = float(np.abs(a - b).max() / np.abs(b).max())
        assert err <= 2e-4, (layer, err)
    err = float(np.abs(got - want).max() / np.abs(want).max())
    assert err <= 2e-4, err
    assert not enc.fell_back()
    z = enc(frame, np.zeros((0, 4), np.float32))
    assert z.shape == (0, enc.dim)
    enc.close()


def test_embeddings_in_chunks_match_reference(gtx_ctx):
    """More crops than the buffers hold (max_crops 16, 37 crops): three chunks through the same activations."""
    from geotrax_amd.reid import ReIDEncoder

    t, frame, boxes, want, _ = _reference("n", 37)
    enc = ReIDEncoder(t, ctx=gtx_ctx, max_crops=16)
    got = enc(frame, boxes)
    assert got.shape == want.shape
    err = float(np.abs(got - want).max() / np.abs(want).max())
    assert err <= 2e-4, err
    for i in (0, 15, 16, 31):                                                  # rows of the first chunks were not overwritten
        assert float(np.abs(got[i] - want[i]).max() / np.abs(want).max()) <= 2e-4, i
    cb = reid_ref.crop_box(boxes, frame.shape[0], frame.shape[1])
    np.testing.assert_array_equal(enc.crop(36), reid_ref.crop_image(frame, cb[36]))   # the last chunk holds crops 32..36
    with pytest.raises(Exception):
        enc.crop(5)
    enc.close()


def test_zero_crops_launch_nothing(gtx_ctx):
    from geotrax_amd.reid import ReIDEncoder
    from geotrax_amd.weights import synthetic_yolov8_cls

    enc = ReIDEncoder(synthetic_yolov8_cls(seed=0, scale="n"), ctx=gtx_ctx)
    frame = _frame(0, 64, 96)
    p = gtx_ctx.dev_alloc(frame.nbytes)
    gtx_ctx.dev_upload(p, frame)
    enc.submit_dev(p, 64, 96, [np.zeros((0, 4), np.float32), np.zeros((0, 4), np.float32)])
    out = enc.collect()
    assert [o.shape for o in out] == [(0, enc.dim), (0, enc.dim)]
    enc.submit_dev(p, 64, 96, [np.array([[10, 10, 40, 50]], np.float32)])       # and a pass after it works
    assert enc.collect()[0].shape == (1, enc.dim)
    gtx_ctx.dev_free(p)
    enc.close()


def test_saturating_pass_falls_back_to_exact(gtx_ctx):
    from geotrax_amd.reid import ReIDEncoder
    from geotrax_amd.weights import synthetic_yolov8_cls

    t = synthetic_yolov8_cls(seed=6, scale="n")
    t["model.3.conv.bias"] = t["model.3.conv.bias"] + np.float32(1e5)           # model.3's output lies beyond fp16's range
    frame, boxes = _frame(3, 540, 960), _boxes(20, seed=7, h=540, w=960)
    split = ReIDEncoder(t, ctx=gtx_ctx, fp32_split=True)
    exact = ReIDEncoder(t, ctx=gtx_ctx, fp32_split=False)
    a, b = split(frame, boxes), exact(frame, boxes)
    assert split.fell_back() and split.saturated() and not exact.fell_back()
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(split(frame, boxes[:5]), exact(frame, boxes[:5]))   # and it stays there
    split.close()
    exact.close()


TH, TW, TIMGSZ = 432, 768, 384


def _det_weights(gtx_ctx, frame):
    from geotrax_amd.detector import Detector
    from geotrax_amd.weights import calibrate_cls_bias, synthetic_yolov8

    w = synthetic_yolov8(seed=1, nc=4)
    det = Detector(w, (TH, TW), imgsz=TIMGSZ, rect=True, ctx=gtx_ctx)
    det.detect(frame)
    w = calibrate_cls_bias(w, det.raw_output(logits=True)[:, 4:], 0.25, 60)
    det.close()
    return w


def _clip(nf):
    from geotrax_amd.synth import make_scene

    scene = make_scene(seed=2, h=TH, w=TW)
    return [scene.render(t, 150) for t in range(0, nf * 12, 12)]


@pytest.mark.parametrize("ttype", ["botsort", "deepocsort", "tracktrack"])
def test_track_with_cls_model_matches_reference_chain(gtx_ctx, tmp_path, ttype):
    from geotrax_amd.model import YOLO
    from geotrax_amd.tracker import Tracker
    from geotrax_amd.weights import save_weights, synthetic_yolov8_cls

    frames = _clip(6)
    wdet = _det_weights(gtx_ctx, frames[0])
    tcls = synthetic_yolov8_cls(seed=8, scale="n")
    save_weights(tcls, tmp_path / "cls.safetensors")
    spec = {"tracker_type": ttype, "with_reid": True, "model": str(tmp_path / "cls.safetensors"), "gmc_method": "none",
            "track_high_thresh": 0.25, "new_track_thresh": 0.25}
    kw = dict(imgsz=TIMGSZ, conf=0.25, rect=True, tracker=spec, persist=True)
    model = YOLO(wdet, ctx=gtx_ctx)
    ref_model = YOLO(wdet, ctx=gtx_ctx)
    ref_trk = ref_model._make_tracker(spec)
    n_ids = 0
    for f in frames:
        r = model.track(f, **kw)[0].boxes
        d = ref_model.predict(f, **{k: v for k, v in kw.items() if k not in ("tracker", "persist")})[0].boxes
        feats = reid_ref.embed(tcls, f, d._xyxy)[1] if len(d) else None
        xyxy, ids, *_ = ref_trk.update(d._xyxy, d._conf, d._cls.astype(np.int32), gmc=None, feats=feats)
        got = [] if r.id is None else list(r.id.astype(int))
        assert got == list(np.asarray(ids).astype(int))
        if len(ids):
            np.testing.assert_allclose(r.xyxy, xyxy, atol=1e-3)
        n_ids += len(got)
    assert n_ids > 20
    assert model._reid is not None and model._reid.dim == 256


def test_rtdetr_tracks_with_cls_model_and_refuses_auto(gtx_ctx, tmp_path):
    from geotrax_amd.detector import Detector
    from geotrax_amd.model import YOLO
    from geotrax_amd.weights import calibrate_rtdetr_scores, save_weights, synthetic_rtdetr, synthetic_yolov8_cls

    frames = _clip(3)
    w = synthetic_rtdetr(seed=3, nc=4)
    det = Detector(w, (TH, TW), imgsz=TIMGSZ, ctx=gtx_ctx)
    det.detect(frames[0])
    w = calibrate_rtdetr_scores(w, det.raw_output(logits=True)[:, 4:], 0.25, 40)
    det.close()
    save_weights(synthetic_yolov8_cls(seed=8, scale="n"), tmp_path / "cls.safetensors")
    model = YOLO(w, ctx=gtx_ctx)
    spec = {"tracker_type": "botsort", "with_reid": True, "model": str(tmp_path / "cls.safetensors"), "gmc_method": "none"}
    n = 0
    for f in frames:
        r = model.track(f, imgsz=TIMGSZ, conf=0.25, tracker=spec, persist=True)[0]
        n += len(r.boxes)
    assert n > 0 and model._reid is not None
    with pytest.raises(NotImplementedError):
        YOLO(w, ctx=gtx_ctx).track(frames[0], imgsz=TIMGSZ, tracker=dict(spec, model="auto"))


def _record_feats(monkeypatch):
    """Every tracker.update call's appearance vectors, in call order (the engine's tracker stage and YOLO.track alike)."""
    from geotrax_amd.tracker import Tracker

    seen = []
    orig = Tracker.update

    def update(self, *a, **kw):
        f = kw.get("feats")
        seen.append(None if f is None else np.array(f, copy=True))
        return orig(self, *a, **kw)

    monkeypatch.setattr(Tracker, "update", update)
    return seen


def _assert_same_feats(a, b):
    assert len(a) == len(b) and len(a) > 0
    n = 0
    for x, y in zip(a, b):
        if x is None or y is None:
            assert (x is None or len(x) == 0) and (y is None or len(y) == 0)
            continue
        np.testing.assert_array_equal(x, y)
        n += len(x)
    assert n > 40


@pytest.mark.parametrize("fp32_split", [None, False], ids=["default", "exact"])
def test_engine_with_reid_equals_per_frame_track(gtx_ctx, tmp_path, monkeypatch, fp32_split):
    """2 detectors, B = 2, a clip several times longer than the frames the detectors hold (host frames through the staging
    buffers): the vectors handed to the tracker are compared, so a crop cut from a refilled frame buffer fails the test. The
    engine's encoders take the precision the detectors are given (`engine: {fp32_split: false}`), as YOLO.track does."""
    from geotrax_amd.engine import ExtractEngine
    from geotrax_amd.model import YOLO
    from geotrax_amd.weights import save_weights, synthetic_yolov8_cls

    frames = _clip(16)
    wdet = _det_weights(gtx_ctx, frames[0])
    save_weights(synthetic_yolov8_cls(seed=9, scale="n"), tmp_path / "cls.safetensors")
    spec = {"tracker_type": "botsort", "with_reid": True, "model": str(tmp_path / "cls.safetensors"), "gmc_method": "none",
            "track_high_thresh": 0.25, "new_track_thresh": 0.25}
    det_kw = dict(imgsz=TIMGSZ, conf=0.25, iou=0.7, max_det=300, rect=True, agnostic_nms=False, classes=None, half=False)
    seen = _record_feats(monkeypatch)
    model = YOLO(wdet, ctx=gtx_ctx)
    model.fp32_split = fp32_split
    want = []
    for f in frames:
        b = model.track(f, tracker=spec, persist=True, **det_kw)[0].boxes
        want.append((None if b.id is None else b.id.astype(int).tolist(), np.asarray(b.xyxy)))
    assert model._reid.fp32_split == (fp32_split is not False)
    want_feats = list(seen)
    seen.clear()
    tracker = YOLO(wdet, ctx=gtx_ctx)._make_tracker(spec)
    eng_kw = det_kw if fp32_split is None else dict(det_kw, fp32_split=fp32_split)
    eng = ExtractEngine(wdet, (TH, TW), eng_kw, tracker, None, batch=2, det_streams=2)
    assert len(eng.encoders) == 2
    assert all(e.fp32_split == (fp32_split is not False) for e in eng.encoders.values())
    assert all(d.fp32_split == (fp32_split is not False) for d in eng.dets)
    got = list(eng.run([frames[i:i + 2] for i in range(0, len(frames), 2)]))
    eng.close()
    _assert_same_feats(list(seen), want_feats)
    assert len(got) == len(want)
    for r, (ids, xyxy) in zip(got, want):
        assert (None if r.ids is None else np.asarray(r.ids).astype(int).tolist()) == ids
        np.testing.assert_array_equal(np.asarray(r.xyxy, np.float32), xyxy.astype(np.float32))


@pytest.mark.parametrize("fp32_split", [None, False], ids=["default", "exact"])
def test_cli_with_reid_y4m_feeder_equals_blocking_loop(gtx_ctx, tmp_path, monkeypatch, fp32_split):
    """`python -m geotrax_amd.extract clip.y4m --cfg cfg.yaml` with the tracker yaml pointing at a cls file: the pipelined engine
    fed by the read-ahead feeder (2 detectors, B = 2, a clip several times the feeder's ring) writes the reference's file set, and
    its tables and the vectors handed to the tracker equal the frame-at-a-time loop's (YOLO.track per frame, over the same frames
    decoded on the host)."""
    import os

    import yaml
    from geotrax_amd import extract as ex
    from geotrax_amd.config_utils import DEFAULT_CFG
    from geotrax_amd.frames import write_y4m
    from geotrax_amd.weights import save_weights, synthetic_yolov8_cls

    frames = _clip(30)
    src = tmp_path / "clip.y4m"
    write_y4m(src, frames)
    decoded = []
    from geotrax_amd.frames import open_source

    rd = open_source(str(src))
    while True:
        ok, f = rd.read()
        if not ok:
            break
        decoded.append(f.bgr() if hasattr(f, "bgr") else f)
    npy = tmp_path / "npy"
    npy.mkdir()
    np.save(npy / "clip.npy", np.stack(decoded))                               # the frame-at-a-time loop reads the decoded frames
    wdet = _det_weights(gtx_ctx, decoded[0])
    from geotrax_amd.weights import save_weights as _sw
    _sw(wdet, tmp_path / "det.safetensors")
    (tmp_path / "det.names.yaml").write_text("{0: car, 1: bus, 2: truck, 3: motorcycle}\n")
    save_weights(synthetic_yolov8_cls(seed=10, scale="n"), tmp_path / "reid-cls.safetensors")
    cfg = yaml.safe_load(DEFAULT_CFG.read_text())
    cfg["ultralytics"].update(imgsz=TIMGSZ, half=False, max_det=300, rect=True)
    cfg["stabilo"].update(downsample_ratio=0.5, max_features=500)
    cfg["tracker"]["active"] = "botsort"
    cfg["tracker"]["botsort"].update(with_reid=True, model="reid-cls.safetensors", gmc_method="none", track_high_thresh=0.25,
                                     new_track_thresh=0.25)
    cfg["extraction"]["model"] = str(tmp_path / "det.safetensors")
    cfg["extraction"]["min_track_length"] = 2
    if fp32_split is not None:
        cfg["engine"] = {"fp32_split": fp32_split}
    routes = []
    orig = ex._read_ahead_batches

    def read_ahead(*a, **kw):
        r = orig(*a, **kw)
        routes.append(r[1] is not None)
        return r

    monkeypatch.setattr(ex, "_read_ahead_batches", read_ahead)
    seen = _record_feats(monkeypatch)
    outs, feats = [], []
    for pipelined in (True, False):
        c = dict(cfg, engine=dict(cfg.get("engine", {}), pipelined=pipelined))
        run = tmp_path / ("pipe" if pipelined else "block")
        run.mkdir()
        (run / "cfg.yaml").write_text(yaml.safe_dump(c))
        for n in ("reid-cls.safetensors",):                                    # `model:` is relative to the working directory
            os.link(tmp_path / n, run / n)
        seen.clear()
        cwd = os.getcwd()
        os.chdir(run)
        try:
            ex.main([str(src if pipelined else npy / "clip.npy"), "--cfg", str(run / "cfg.yaml"), "--output-folder", str(run / "out")])
        finally:
            os.chdir(cwd)
        feats.append(list(seen))
        outs.append(run)
    assert routes == [True]                                                    # the pipelined run read through the feeder
    names = sorted(p.name for p in (outs[0] / "out").iterdir())
    assert names == ["clip.txt", "clip_vid_transf.txt"] == sorted(p.name for p in (outs[1] / "out").iterdir())
    assert (tmp_path / "clip.yaml").is_file() and (npy / "clip.yaml").is_file()   # the run's metadata, next to its source
    for n in names:
        assert (outs[0] / "out" / n).read_bytes() == (outs[1] / "out" / n).read_bytes(), n
    t = np.loadtxt(outs[0] / "out" / "clip.txt", delimiter=",", ndmin=2)
    assert len(t) > 50 and t[:, 1].max() >= 1
    _assert_same_feats(feats[0], feats[1])
