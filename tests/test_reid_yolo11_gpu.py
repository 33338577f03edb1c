"""YOLO11-cls as the separate ReID network on the GPU: the attention kernels alone on the crops' small maps (float64 numpy, poisoned
neighbours), the embedder against tests/yolo11_cls_ref.py per layer and per vector, its self-consistency (singles, chunks, the
asynchronous pair, the saturation fallback raised by the attention launch), and the vectors the trackers are handed through
YOLO.track and the pipelined engine. The bars are those of tests/test_yolo11_gpu.py (attention output: 2e-4 of the largest value,
3e-2 under fp16) and tests/test_reid_gpu.py (layers and vectors: 2e-4 of the largest value)."""
import numpy as np
import pytest

import yolo11_cls_ref as cref

pytestmark = pytest.mark.gpu

BAR = 2e-4            # tests/test_reid_gpu.py, tests/test_yolo11_gpu.py::_check_against_oracle (fp32 grade)
BAR_HALF = 3e-2       # tests/test_yolo11_gpu.py::_check_against_oracle (half)
FH, FW = 480, 640


def _frame(seed=0, h=FH, w=FW):
    rng = np.random.default_rng(seed)
    small = rng.integers(0, 256, (h // 8 + 1, w // 8 + 1, 3)).astype(np.float32)
    big = np.repeat(np.repeat(small, 8, 0), 8, 1)[:h, :w]
    return np.clip(big + rng.normal(0, 25, (h, w, 3)), 0, 255).astype(np.uint8)


def _boxes(n, seed=1, h=FH, w=FW):
    rng = np.random.default_rng(seed)
    size = np.exp(rng.uniform(np.log(6), np.log(300), (n, 2)))
    x1, y1 = rng.uniform(-10, w - 20, n), rng.uniform(-10, h - 20, n)
    b = np.stack([x1, y1, x1 + size[:, 0], y1 + size[:, 1]], 1)
    b[:, [0, 2]] = b[:, [0, 2]].clip(0, w)
    b[:, [1, 3]] = b[:, [1, 3]].clip(0, h)
    return b.astype(np.float32)


# ------------------------------------------------------------------ the attention launch alone
FMTS = {"f16": (np.float16, False, BAR_HALF), "f32": (np.float32, False, BAR), "split": (np.float32, True, BAR)}


@pytest.mark.parametrize("fmt", list(FMTS))
@pytest.mark.parametrize("heads", [2, 4])
@pytest.mark.parametrize("hw", [2, 3, 5, 7, 8, 10])
def test_attention_on_small_maps(gtx_ctx, hw, heads, fmt):
    """2 x 2 to 8 x 8 (T = 64 exactly) run psa_attn_small_kernel, 10 x 10 psa_attn_kernel's ragged second stage; 1, 3 and 37 crops
    (odd counts: a (crop, head) pair is found from the workgroup index). The map behind the last crop, the odd crops in a second launch and the channels
    beside the slice hold 1e30: a masking or indexing slip shows as inf / nan or as another bit in a clean crop's output."""
    from geotrax_amd import ops

    dt, split, bar = FMTS[fmt]
    C, cs, coff = heads * 64, heads * 128 + 8, 8
    rng = np.random.default_rng(100 * hw + heads)
    pe_w = (rng.standard_normal((C, 1, 3, 3)) / 3).astype(np.float32)
    pe_b = (rng.standard_normal(C) * 0.05).astype(np.float32)
    for n in (1, 3, 37):
        with np.errstate(over="ignore"):                                       # 1e30 is inf in fp16
            qkv = np.full((n + 1, hw, hw, cs), 1e30, np.float32)                     # poison: beside the slice and behind the last crop
            qkv[:n, ..., coff:] = rng.standard_normal((n, hw, hw, heads * 128)) * 1.5
            qkv = qkv.astype(dt)
            out0 = np.full((n, hw, hw, C + 8), 7.0, dt)
            got, sat, _ = ops.psa_attention(qkv, pe_w, pe_b, heads, n=n, in_coff=coff, out=out0, out_coff=0, split=split, ctx=gtx_ctx)
            assert not sat and np.isfinite(got.astype(np.float32)).all()
            assert (got[..., C:] == dt(7.0)).all()                                   # the channels beside the output slice are untouched
            want = cref.attention_f64(qkv[:n, ..., coff:].astype(np.float64), pe_w, pe_b, heads)
            err = float(np.abs(got[..., :C].astype(np.float64) - want).max() / np.abs(want).max())
            print(f"{hw}x{hw} heads {heads} {fmt} n {n}: rel-to-max error {err:.3e}")
            assert err < bar, (n, err)
            if n > 1:                                                                # every odd crop poisoned: the even ones do not move
                bad = qkv.copy()
                bad[1::2] = dt(1e30)
                again, _, _ = ops.psa_attention(bad, pe_w, pe_b, heads, n=n, in_coff=coff, out=out0, out_coff=0, split=split, ctx=gtx_ctx)
                np.testing.assert_array_equal(again[0::2], got[0::2])


@pytest.mark.parametrize("fmt", list(FMTS))
def test_both_attention_kernels_agree_on_a_small_map(gtx_ctx, fmt):
    """psa_attn_kernel forced onto a 7 x 7 map (one ragged stage, a wave with one valid query) holds the same bar"""
    from geotrax_amd import ops

    dt, split, bar = FMTS[fmt]
    rng = np.random.default_rng(7)
    qkv = (rng.standard_normal((5, 7, 7, 256)) * 1.5).astype(dt)
    pe_w, pe_b = (rng.standard_normal((128, 1, 3, 3)) / 3).astype(np.float32), (rng.standard_normal(128) * 0.05).astype(np.float32)
    want = cref.attention_f64(qkv.astype(np.float64), pe_w, pe_b, 2)
    for form in (1, 2):
        got, _, _ = ops.psa_attention(qkv, pe_w, pe_b, 2, split=split, form=form, ctx=gtx_ctx)
        err = float(np.abs(got.astype(np.float64) - want).max() / np.abs(want).max())
        assert err < bar, (form, err)
    with pytest.raises(Exception):                                               # the small-map kernel holds 64 keys
        ops.psa_attention(np.zeros((1, 10, 10, 256), dt), pe_w, pe_b, 2, split=split, form=2, ctx=gtx_ctx)


def test_attention_launch_raises_the_saturation_flag(gtx_ctx):
    from geotrax_amd import ops

    rng = np.random.default_rng(1)
    qkv = rng.standard_normal((3, 3, 3, 256)).astype(np.float32)
    pe_w, pe_b = np.zeros((128, 1, 3, 3), np.float32), np.zeros(128, np.float32)
    assert not ops.psa_attention(qkv, pe_w, pe_b, 2, split=True, ctx=gtx_ctx)[1]
    pe_b[5] = 1e5
    out, sat, _ = ops.psa_attention(qkv, pe_w, pe_b, 2, split=True, ctx=gtx_ctx)
    assert sat and (out[..., 5] == 65504.0).all()
    assert not ops.psa_attention(qkv, pe_w, pe_b, 2, split=False, ctx=gtx_ctx)[1]     # plain fp32 holds it


# ------------------------------------------------------------------ the embedder against the restatement
# Seeded YOLO11 stacks are bimodal: a stack either stays near activations of 1-5 or amplifies to 1e2-4e3, and
# the amplifying ones carry the restatement's own rounding to the bar. The parity cases are picked by the written rule of
# tests/test_yolo11_gpu.py::parity_weights, on the restatement alone (fp32 against float64 on the CPU, seeds 1-4 at gains 1.7 and
# 1.5, imgsz 64 / 96 / 224 / 320): its own spread on every probed layer and on the vectors is at most a fifth of the bar (4e-5).
# Found: n seed 1 at 1.7 (1.8e-6), s seed 2 at 1.5 (1.8e-6), m seed 2 at 1.5 (1.4e-6). Failing the rule (n seed 4 at 1.7: 2.8e-4;
# m seed 1 at 1.7: 2.4e-3) or near it (s seed 1 at 1.7: 3.7e-5): those stay in the self-consistency tests.
PARITY = {"n": (1, 1.7), "s": (2, 1.5), "m": (2, 1.5)}
AMPLIFYING = ("n", 4, 1.7)
LAYERS = ["model.2", "model.6", "model.8", "model.9.m.0.attn.out", "model.9"]
DIM = {"n": 256, "s": 512, "m": 512}
_REF = {}


def _weights(scale, seed, gain):
    from geotrax_amd.weights import synthetic_yolo11_cls

    return synthetic_yolo11_cls(seed=seed, scale=scale, nc=10, gain=gain)


def _reference(scale, imgsz):
    """Computed once per (scale, imgsz) and shared: weights, frame, boxes, fp32 vectors and crop 0's layers, the fp32-float64 spread"""
    key = (scale, imgsz)
    if key not in _REF:
        t = _weights(scale, *PARITY[scale])
        frame, boxes = _frame(2), _boxes(5, seed=3)
        crops = cref.crops_of(frame, boxes, imgsz)
        a, b = cref.Yolo11ClsRef(t), cref.Yolo11ClsRef(t, double=True)
        ea, eb = a.forward(crops), b.forward(crops)
        spread = {"vectors": float(np.abs(ea - eb).max() / np.abs(eb).max())}
        for l in LAYERS:
            x, y = a.acts[l].numpy(), b.acts[l].numpy()
            spread[l] = float(np.abs(x - y).max() / np.abs(y).max())
        _REF[key] = (t, frame, boxes, ea, {l: a.acts[l][0].permute(1, 2, 0).numpy() for l in LAYERS}, spread)
    return _REF[key]


@pytest.mark.parametrize("split", [True, False], ids=["split", "exact"])
@pytest.mark.parametrize("imgsz", [64, 96, 224, 320])
@pytest.mark.parametrize("scale", ["n", "s", "m"])
def test_embeddings_match_restatement(gtx_ctx, scale, imgsz, split):
    """n: 2 heads, an 8-channel hidden layer; s: 4 heads; m: c3k everywhere. imgsz 64 / 96 / 224: 2 x 2, 3 x 3 and 7 x 7 maps on the
    small-map kernel; 320: 100 tokens on psa_attn_kernel."""
    from geotrax_amd.reid import ReIDEncoder

    t, frame, boxes, want, acts0, spread = _reference(scale, imgsz)
    print("restatement fp32 vs float64:", {k: f"{v:.1e}" for k, v in spread.items()})
    assert max(spread.values()) <= BAR / 5                            # the case is what PARITY claims
    enc = ReIDEncoder(t, ctx=gtx_ctx, fp32_split=split, imgsz=imgsz, max_crops=8)
    assert enc.family == "yolo11-cls" and enc.dim == DIM[scale]
    got = enc(frame, boxes)
    assert got.shape == want.shape == (len(boxes), DIM[scale])
    launches = [n for n, _, _ in enc.profile(len(boxes), iters=1)]
    attn = [n for n in launches if n.startswith("model.9.m.0.attn ")]
    assert attn == ["model.9.m.0.attn " + ("psa_attn_small_kernel" if imgsz <= 256 else "psa_attn_kernel")], attn
    np.testing.assert_array_equal(enc.crop(0), cref.crops_of(frame, boxes[:1], imgsz)[0])
    for layer in LAYERS:
        a, b = enc.layer_output(0, layer), acts0[layer]
        assert a.shape == b.shape, layer
        err = float(np.abs(a - b).max() / np.abs(b).max())
        print(f"{layer}: rel-to-max error {err:.3e}")
        assert err <= BAR, (layer, err)
    err = float(np.abs(got - want).max() / np.abs(want).max())
    print(f"vectors: rel-to-max error {err:.3e}")
    assert err <= BAR, err
    assert not enc.fell_back()
    assert enc(frame, np.zeros((0, 4), np.float32)).shape == (0, enc.dim)
    enc.close()


# ------------------------------------------------------------------ self-consistency (the amplifying seed included)
@pytest.mark.parametrize("case", [("n",) + PARITY["n"], AMPLIFYING], ids=["calm", "amplifying"])
@pytest.mark.parametrize("split", [True, False], ids=["split", "exact"])
def test_pass_equals_singles_chunks_and_async_pair(gtx_ctx, case, split):
    from geotrax_amd.reid import ReIDEncoder

    t = _weights(*case)
    frame, boxes = _frame(4), _boxes(37, seed=5)
    enc = ReIDEncoder(t, ctx=gtx_ctx, fp32_split=split, max_crops=64)
    whole = enc(frame, boxes)
    assert whole.shape == (37, 256) and np.isfinite(whole).all() and not enc.fell_back()
    for i in range(37):                                                          # N crops = the N single-crop passes, bit for bit
        np.testing.assert_array_equal(enc(frame, boxes[i:i + 1])[0], whole[i], err_msg=str(i))
    small = ReIDEncoder(t, ctx=gtx_ctx, fp32_split=split, max_crops=16)          # 16 + 16 + 5
    np.testing.assert_array_equal(small(frame, boxes), whole)
    two = np.stack([frame, frame])                                               # the asynchronous pair over two device frames
    p = gtx_ctx.dev_alloc(two.nbytes)
    try:
        gtx_ctx.dev_upload(p, two)
        small.submit_dev(p, FH, FW, [boxes[:20], boxes[20:]])
        a = small.collect()
    finally:
        gtx_ctx.dev_free(p)
    assert [len(x) for x in a] == [20, 17]
    np.testing.assert_array_equal(np.concatenate(a), whole)
    enc.close()
    small.close()


def test_saturating_attention_falls_back_to_exact(gtx_ctx):
    """Only the attention launch leaves fp16's range here: one channel of pe's bias at 1e5, and proj does not read that channel,
    so no convolution saturates. The split-f16x3 embedder re-runs the pass on its exact twin -- the same graph -- and stays there."""
    from geotrax_amd.reid import ReIDEncoder

    t = dict(_weights("n", *PARITY["n"]))
    t["model.9.m.0.attn.pe.conv.bias"] = t["model.9.m.0.attn.pe.conv.bias"].copy()
    t["model.9.m.0.attn.pe.conv.bias"][3] = 1e5
    t["model.9.m.0.attn.proj.conv.weight"] = t["model.9.m.0.attn.proj.conv.weight"].copy()
    t["model.9.m.0.attn.proj.conv.weight"][:, 3] = 0
    frame, boxes = _frame(3), _boxes(20, seed=7)
    split = ReIDEncoder(t, ctx=gtx_ctx, fp32_split=True)
    exact = ReIDEncoder(t, ctx=gtx_ctx, fp32_split=False)
    a, b = split(frame, boxes), exact(frame, boxes)
    assert split.fell_back() and split.saturated() and not exact.fell_back()
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(split(frame, boxes[:5]), exact(frame, boxes[:5]))
    assert float(exact.layer_output(0, "model.9.m.0.attn.out")[..., 3].min()) > 65504.0
    split.close()
    exact.close()


# ------------------------------------------------------------------ through the trackers
TH, TW, TIMGSZ = 384, 640, 384


def _clip(nf):
    from geotrax_amd.synth import make_scene

    scene = make_scene(seed=2, h=TH, w=TW)
    return [scene.render(t, 150) for t in range(0, nf * 12, 12)]


_DET = {}


def _det_weights(gtx_ctx, family, frame):
    if family not in _DET:
        if family == "yolov8s":
            from geotrax_amd.detector import Detector
            from geotrax_amd.weights import calibrate_cls_bias, synthetic_yolov8

            w = synthetic_yolov8(seed=1, nc=4)
            det = Detector(w, (TH, TW), imgsz=TIMGSZ, rect=True, ctx=gtx_ctx)
            det.detect(frame)
            w = calibrate_cls_bias(w, det.raw_output(logits=True)[:, 4:], 0.25, 30)
            det.close()
        else:
            import test_yolo11_gpu as ty

            w = ty._weights(gtx_ctx, "s", hw=(TH, TW), imgsz=TIMGSZ, per_level=(15, 10, 5), frame=frame, rect=True)
        _DET[family] = w
    return _DET[family]


def _record(monkeypatch):
    """Every tracker.update call's boxes and appearance vectors, in call order"""
    from geotrax_amd.tracker import Tracker

    seen = []
    orig = Tracker.update

    def update(self, xyxy, *a, **kw):
        f = kw.get("feats")
        seen.append((np.array(xyxy, np.float32, copy=True), None if f is None else np.array(f, copy=True)))
        return orig(self, xyxy, *a, **kw)

    monkeypatch.setattr(Tracker, "update", update)
    return seen


@pytest.mark.parametrize("family", ["yolov8s", "yolo11s"])
@pytest.mark.parametrize("ttype", ["botsort", "deepocsort", "tracktrack"])
def test_track_hands_the_tracker_the_restatements_vectors(gtx_ctx, tmp_path, monkeypatch, ttype, family):
    from geotrax_amd.model import YOLO
    from geotrax_amd.weights import save_weights

    frames = _clip(4)
    wdet = _det_weights(gtx_ctx, family, frames[0])
    tcls = _weights("n", *PARITY["n"])
    save_weights(tcls, tmp_path / "yolo11n-cls.safetensors")
    spec = {"tracker_type": ttype, "with_reid": True, "model": str(tmp_path / "yolo11n-cls.safetensors"), "gmc_method": "none",
            "track_high_thresh": 0.25, "new_track_thresh": 0.25}
    seen = _record(monkeypatch)
    model = YOLO(wdet, ctx=gtx_ctx)
    n_ids = n_vec = 0
    for f in frames:
        r = model.track(f, imgsz=TIMGSZ, conf=0.25, rect=True, tracker=spec, persist=True)[0].boxes
        n_ids += 0 if r.id is None else len(r.id)
    assert len(seen) == len(frames)
    for f, (xyxy, feats) in zip(frames, seen):
        if len(xyxy) == 0:
            continue
        assert feats is not None and feats.shape == (len(xyxy), 256)
        want = cref.embed(tcls, f, xyxy[:40])[1]                                 # at most 40 boxes through the CPU restatement
        err = float(np.abs(feats[:40] - want).max() / np.abs(want).max())
        assert err <= BAR, err
        n_vec += len(want)
    assert n_vec > 10 and n_ids > 5
    assert model._reid is not None and model._reid.family == "yolo11-cls" and model._reid.dim == 256


@pytest.mark.parametrize("family", ["yolov8s", "yolo11s"])
def test_engine_equals_the_blocking_loop(gtx_ctx, tmp_path, monkeypatch, family):
    """The pipelined engine (2 detectors, B = 2) hands the tracker the vectors of the frame-at-a-time loop, bit for bit, and
    returns its ids and boxes."""
    from geotrax_amd.engine import ExtractEngine
    from geotrax_amd.model import YOLO
    from geotrax_amd.weights import save_weights

    frames = _clip(8)
    wdet = _det_weights(gtx_ctx, family, frames[0])
    save_weights(_weights("n", *PARITY["n"]), tmp_path / "yolo11n-cls.safetensors")
    spec = {"tracker_type": "botsort", "with_reid": True, "model": str(tmp_path / "yolo11n-cls.safetensors"), "gmc_method": "none",
            "track_high_thresh": 0.25, "new_track_thresh": 0.25}
    det_kw = dict(imgsz=TIMGSZ, conf=0.25, iou=0.7, max_det=300, rect=True, agnostic_nms=False, classes=None, half=False)
    seen = _record(monkeypatch)
    model = YOLO(wdet, ctx=gtx_ctx)
    want = []
    for f in frames:
        b = model.track(f, tracker=spec, persist=True, **det_kw)[0].boxes
        want.append((None if b.id is None else b.id.astype(int).tolist(), np.asarray(b.xyxy)))
    want_feats = list(seen)
    seen.clear()
    tracker = YOLO(wdet, ctx=gtx_ctx)._make_tracker(spec)
    eng = ExtractEngine(wdet, (TH, TW), det_kw, tracker, None, batch=2, det_streams=2)
    assert all(e.family == "yolo11-cls" for e in eng.encoders.values())
    got = list(eng.run([frames[i:i + 2] for i in range(0, len(frames), 2)]))
    eng.close()
    assert len(seen) == len(want_feats) == len(frames) and len(got) == len(want)
    n = 0
    for (xa, fa), (xb, fb) in zip(seen, want_feats):
        np.testing.assert_array_equal(xa, xb)
        if fa is None or fb is None:
            assert (fa is None or len(fa) == 0) and (fb is None or len(fb) == 0)
            continue
        np.testing.assert_array_equal(fa, fb)
        n += len(fa)
    assert n > 20
    for r, (ids, xyxy) in zip(got, want):
        assert (None if r.ids is None else np.asarray(r.ids).astype(int).tolist()) == ids
        np.testing.assert_array_equal(np.asarray(r.xyxy, np.float32), xyxy.astype(np.float32))
