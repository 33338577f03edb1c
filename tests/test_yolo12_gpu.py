"""YOLO12 detectors on the HIP path (A2C2f blocks: area attention at model.6 / 8, C3k members in the neck, Detect = model.21):
the area-attention launch alone against float64, the whole network at scales n and l against tests/yolo12_ref.py, and the
extract chain. Small shapes: 4 x 4 and 2 x 2 attention maps at 64 x 64, 6 x 10 (15 positions per band, bands cut inside map rows)
and 3 x 5 at 96 x 160.

Bars. The launch alone: tests/test_rtdetr_ops_gpu.py's value bar (_value_bar: e_kernel < 8 e_fp32ref + 1e-7, errors relative to the
float64 reference's largest value, the float32 recipe's result stored in the output format, the float64 reference started from what
the input format holds) for all three paths. The whole network: tests/test_yolo11_gpu.py::_check_against_oracle's numbers (layers
2e-4 of the layer's largest value, scores 1e-4, boxes rtol 2e-5 + 2e-3, kept confidences 1e-5, frame boxes 1e-2; `half: true`: 3e-2,
2e-2, rtol 5e-3 + 0.5). The seeded weights of the whole-network cases are chosen on the restatement alone by
tests/test_yolo11_gpu.py::parity_weights' rule, which every case asserts on the CPU before it runs the GPU: fp32 and float64 runs of
the restatement keep the same anchors, their kept confidences lie within 2e-6 of each other and no class score is closer to `conf`
than 5e-6.

`model.*.attn.qkv.conv` is not among the probed layers: the library emits that convolution's rows in another order (q of every head,
k of every head, v of every head) than the checkpoint holds them; what it feeds, `attn.out` and `attn.pe.conv`, is probed."""
import argparse
import functools
import logging
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

logger = logging.getLogger("test_yolo12")
KW = dict(conf=0.25, iou=0.7, max_det=300, classes=[0, 1, 2, 3], agnostic_nms=True)
KEY_TILE = 64          # csrc/yolo_tables.hpp kAreaAttnKeyTile: keys per LDS stage of area_attn_kernel


# ============================================================================ the attention launch alone
# (h, w, area): 4 positions per band; 24 per band (no multiple of 16); an odd number of positions in one band; one past the key tile
ATTN_MAPS = [(4, 4, 4), (8, 12, 4), (5, 7, 1), (5, 13, 1)]
assert ATTN_MAPS[3][0] * ATTN_MAPS[3][1] == KEY_TILE + 1


@functools.lru_cache(maxsize=None)
def _attn_case(h, w, area, heads, n, fmt, variant):
    """Host qkv map [n, h, w, 8 + 96 heads] (8 poisoned channels in front), the output buffer's initial content [n, h, w, 32 heads + 8],
    and the float64 / float32 results of tests/yolo12_ref.py's recipe on what the format holds."""
    import test_rtdetr_ops_gpu as tok
    import torch
    from yolo12_ref import area_attention

    rng = np.random.default_rng(tok._seed("area_attn", h, w, area, heads, n, variant))
    x = rng.standard_normal((n, h, w, 96 * heads))
    if variant == "large":                              # q and k scaled so that the scores inside the bands reach +-60
        qk = x.reshape(n, area, h * w // area, heads, 96)
        s = np.einsum("nbqhd,nbkhd->nbhqk", qk[..., :32], qk[..., 32:64]) / np.sqrt(32.0)
        x.reshape(n, h, w, heads, 96)[..., :64] *= np.sqrt(60.0 / np.abs(s).max())
    host, split = tok._host(x, fmt)
    qkv = np.full((n, h, w, 8 + 96 * heads), 6e4, host.dtype)
    qkv[..., 8:] = host
    held = tok._held(host, fmt)

    def run(dt):
        t = torch.from_numpy(held).to(dt).permute(0, 3, 1, 2)
        return area_attention(t, heads, area).permute(0, 2, 3, 1).numpy()

    ref64, ref32 = run(torch.float64), run(torch.float32)
    out0 = tok._exact_pairs(rng, (n, h, w, 32 * heads + 8)).astype(host.dtype)
    for a in (qkv, out0):
        a.setflags(write=False)
    return qkv, out0, split, ref64, tok._stored(ref32, fmt), held


@pytest.mark.parametrize("fmt", ["f32s", "f32", "f16"])
@pytest.mark.parametrize("heads,n", [(2, 1), (4, 2), (2, 2), (4, 1)])
@pytest.mark.parametrize("h,w,area", ATTN_MAPS)
def test_area_attention_matches_float64(gtx_ctx, h, w, area, heads, n, fmt):
    import test_rtdetr_ops_gpu as tok
    from geotrax_amd import ops

    qkv, out0, split, ref64, ref32, _ = _attn_case(h, w, area, heads, n, fmt, "normal")
    got, sat, _ = ops.area_attention(qkv, heads, area, in_coff=8, out=out0, out_coff=0, split=split, ctx=gtx_ctx)
    c = 32 * heads
    assert not sat and got[..., c:].tobytes() == out0[..., c:].tobytes()          # the channels behind the slice are kept
    tok._value_bar(f"area_attn {h}x{w} area {area} heads {heads} n {n} {fmt}", got[..., :c], ref64, ref32)


@pytest.mark.parametrize("fmt", ["f32s", "f32", "f16"])
def test_area_attention_subtracts_the_row_maximum(gtx_ctx, fmt):
    """Scores of +-60: exp(60) alone is 1e26, a sum of 24 of them still finite in fp32 but exp(-60 - 60) / that is not what the
    shifted form computes; without the shift the fp16-grade inputs of `half` would differ in the first digit."""
    import test_rtdetr_ops_gpu as tok
    from geotrax_amd import ops

    h, w, area, heads, n = 8, 12, 4, 2, 2
    qkv, out0, split, ref64, ref32, held = _attn_case(h, w, area, heads, n, fmt, "large")
    q, k = (held.reshape(n, area, h * w // area, heads, 96)[..., i:i + 32] for i in (0, 32))
    s = np.einsum("nbqhd,nbkhd->nbhqk", q, k) / np.sqrt(32.0)
    assert s.max() > 55 and s.min() < -45                                          # the case is what it claims to be
    got, sat, _ = ops.area_attention(qkv, heads, area, in_coff=8, out=out0, out_coff=0, split=split, ctx=gtx_ctx)
    assert not sat and np.isfinite(got).all()
    tok._value_bar(f"area_attn large logits {fmt}", got[..., :32 * heads], ref64, ref32)


@pytest.mark.parametrize("fmt", ["f32s", "f16"])
def test_area_attention_planar_layout_gives_the_same_map(gtx_ctx, fmt):
    """[q of every head | k of every head | v of every head], the order the trunk emits qkv's rows in: the same output bit for bit"""
    from geotrax_amd import ops

    h, w, area, heads, n = 8, 12, 4, 4, 2
    qkv, out0, split, *_ = _attn_case(h, w, area, heads, n, fmt, "normal")
    a, _, _ = ops.area_attention(qkv, heads, area, in_coff=8, out=out0, split=split, ctx=gtx_ctx)
    per_head = qkv[..., 8:].reshape(n, h, w, heads, 3, 32)
    planar = np.ascontiguousarray(per_head.transpose(0, 1, 2, 4, 3, 5).reshape(n, h, w, 96 * heads))
    b, _, _ = ops.area_attention(planar, heads, area, planar=True, out=out0, split=split, ctx=gtx_ctx)
    assert a.tobytes() == b.tobytes()


def test_a_map_that_does_not_cut_into_its_areas_is_refused(gtx_ctx):
    """5 x 7 positions into 4 areas, 3 x 3 into 2: refused with a message, nothing runs (the buffers come back as they went in).
    YoloTrunk::ablock refuses the same at a detector's creation; no letterbox reaches it, since network sizes are multiples of 32
    and a stride-16 map of even sides always cuts into four."""
    from geotrax_amd import ops
    from geotrax_amd._lib import GtxError

    for h, w, area in ((5, 7, 4), (3, 3, 2)):
        for dt in (np.float32, np.float16):
            with pytest.raises(GtxError, match="equal areas"):
                ops.area_attention(np.zeros((1, h, w, 192), dt), 2, area, ctx=gtx_ctx)
    got, _, _ = ops.area_attention(np.ones((1, 3, 3, 192), np.float32), 2, 3, ctx=gtx_ctx)      # the context still works afterwards
    assert np.allclose(got, 1.0)


# ============================================================================ the whole network
LAYERS = {"n": ["model.2", "model.4", "model.6.m.0.0.attn.out", "model.6.m.0.0.attn.pe.conv", "model.6.m.1", "model.6", "model.8.m.1.1.attn.out",
                "model.8", "model.11", "model.14", "model.17", "model.20", "model.21.feat0", "model.21.feat1", "model.21.feat2"],
          "l": ["model.2", "model.6.m.0.0.attn.out", "model.6.m.3.1.attn.pe.conv", "model.6", "model.8.m.3", "model.8", "model.11", "model.14",
                "model.17", "model.20", "model.21.feat0", "model.21.feat2"]}
SHAPES = {"64": ((64, 64), 64, False), "96x160": ((90, 160), 160, True)}      # frame size, imgsz, rect: 96 x 160 has 3 padding rows above and below
# (seed, gain) per (scale, shape): chosen on the restatement alone by the parity rule in the module docstring
# (seeds 1-8 at gains 1.5 / 1.3 / 1.1 for n and 1.2 to 0.6 for l: a seeded YOLO12 stack, eight or sixteen residual ABlocks without a
# normalisation, amplifies to activations of 1e3 and more at the other families' 1.7 / 1.5; the chosen ones stay below 50 with
# kept-confidence spreads of 2.6e-8 / 9.4e-8 / 2.3e-8 / 1.2e-7 and threshold margins of 2.4e-5 / 2.9e-4 / 1.4e-5 / 1.5e-5)
SEEDS = {("n", "64"): (2, 1.3), ("n", "96x160"): (2, 1.3), ("l", "64"): (2, 0.8), ("l", "96x160"): (1, 0.7)}
# anchors per level calibrated to clear conf (of 64 / 16 / 4 and 240 / 60 / 15)
KEEP = {("n", "64"): (8, 3, 1), ("l", "64"): (8, 3, 1), ("n", "96x160"): (20, 8, 2), ("l", "96x160"): (12, 5, 2)}
# `half: true` adds one figure to the rule, again the restatement's own: its fp16 emulation against its fp32 run, per probed layer and
# relative to the layer's largest value, must stay below 1e-2, a third of the 3e-2 bar. (Scale l at 96 x 160, seed 2 at 0.9 -- fine by
# the fp32 rule -- has 4.2e-2 there by itself: its 3 x 5 attention at model.8 amplifies roundings thirtyfold in every arithmetic, and
# seed 5 at 0.8 has 8e-3 on one CPU and 1.6e-2 on another. The chosen cases have 2.8e-3 / 3.4e-3 / 2.1e-3 / 1.5e-3.)
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
    pixels + confidence differences in units of 1e-5): boxes clipped to the same frame corner tie in any sort by coordinates, two
    whole-frame boxes are told apart by their confidences only, and confidences 1e-7 apart may swap ranks."""
    from scipy.optimize import linear_sum_assignment

    assert len(got) == len(ref_conf) > 0
    d = np.abs(got.xyxy[:, None, :] - ref_xyxy[None, :, :]).max(-1) + 1e5 * np.abs(got.conf[:, None] - ref_conf[None, :])
    i, j = linear_sum_assignment(d)
    assert i.tolist() == list(range(len(got)))
    return j


def _ref64(weights, x):
    from yolo12_ref import Yolo12Ref

    r = Yolo12Ref(weights)
    r.t = {k: v.double() for k, v in r.t.items()}
    return r, r.forward(x.double())[0].numpy()


@functools.lru_cache(maxsize=None)
def _case(scale, shape):
    """Weights (the last class convs calibrated on the restatement's own float64 logits so that KEEP anchors per level clear conf), frame, network input
    and the parity rule's three figures, computed once on the CPU and shared."""
    from geotrax_amd.weights import synthetic_yolo12
    from oracle.yolov8_ref import letterbox, non_max_suppression
    from yolo12_ref import Yolo12Ref

    hw, imgsz, rect = SHAPES[shape]
    seed, gain = SEEDS[scale, shape]
    frame = _frame(hw)
    x, _ = letterbox(frame, imgsz, rect)
    w = synthetic_yolo12(seed=seed, nc=4, scale=scale, box_weight_scale=0.1, gain=gain)
    r64, _ = _ref64(w, x)
    for l, k in enumerate(KEEP[scale, shape]):          # tests/test_yolo11_gpu.py::_calibrated on the restatement's float64 logits: each level's last class
        lv = np.sort(r64.acts[f"model.21.cls{l}"][0].amax(0).flatten().numpy())[::-1]   # conv scaled down to logits of at most 3 and shifted
        f = min(1.0, 3.0 / max(np.abs(lv).max(), 1e-6))
        delta = np.log(KW["conf"] / (1 - KW["conf"])) - f * 0.5 * (lv[k - 1] + lv[k])
        name = f"model.21.cv3.{l}.2"
        w[name + ".weight"] = (w[name + ".weight"] * np.float32(f)).astype(np.float32)
        w[name + ".bias"] = (w[name + ".bias"] * np.float32(f) + np.float32(delta)).astype(np.float32)
    a, b = Yolo12Ref(w).forward(x)[0].numpy(), _ref64(w, x)[1]
    nms = lambda q: non_max_suppression(q.astype(np.float32), KW["conf"], KW["iou"], KW["classes"], True, KW["max_det"], return_idx=True)[1]
    ia, ib = nms(a), nms(b)
    same = np.array_equal(np.sort(ia), np.sort(ib))
    spread = float(np.abs(a[ia, 4:].max(1) - b[ia, 4:].max(1)).max()) if same and len(ia) else np.inf
    return w, frame, x, (same, spread, float(np.abs(a[:, 4:] - KW["conf"]).min()), len(ia))


@functools.lru_cache(maxsize=None)
def _reference(scale, shape, half):
    """The restatement's pass (fp32, or with the fp16 emulation), shared by the paths that compare with it and left unchanged"""
    from oracle.yolov8_ref import detect, letterbox
    from yolo12_ref import Yolo12Ref

    w, frame, _, _ = _case(scale, shape)
    hw, imgsz, rect = SHAPES[shape]
    ref = Yolo12Ref(w, emulate_half=half)
    x, g = letterbox(frame, imgsz, rect, half=half)
    raw = ref.forward(x)[0].numpy()
    acts = {k: ref.acts[k][0].permute(1, 2, 0).numpy() for k in LAYERS[scale]}
    rows = detect(ref, frame, imgsz, rect, KW["conf"], KW["iou"], KW["classes"], True, KW["max_det"])
    return raw, acts, rows, (g["net_h"], g["net_w"])


@pytest.mark.parametrize("path", ["split", "exact", "half"])
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("scale", ["n", "l"])
def test_yolo12_matches_restatement(gtx_ctx, scale, shape, path):
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
    assert det.graph == "yolo12" and det.net_hw == net_hw and det.net_hw == ((64, 64) if shape == "64" else (96, 160))
    got = det.detect(frame)
    assert not det.fell_back()
    rel = 3e-2 if half else 2e-4
    for name in LAYERS[scale]:
        a, r = det.layer_output(name), acts[name]
        assert a.shape == r.shape, name
        err = np.abs(a - r).max() / (np.abs(r).max() + 1e-6)
        print(f"{name}: rel-to-max error {err:.3e}")
        assert err < rel, f"{name}: rel-to-max error {err:.3e}"
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


def test_attention_rows_are_never_skipped(gtx_ctx, monkeypatch):
    """96 x 160 from a 90-row frame, default path: whatever rows the letterbox plan leaves out of the backbone's launches, a detector
    with the plan switched off gives the same rows bit for bit -- the attention outputs count as frame-dependent in every row."""
    from geotrax_amd.detector import Detector

    w, frame, _, _ = _case("n", "96x160")
    hw, imgsz, rect = SHAPES["96x160"]
    det = Detector(w, hw, imgsz=imgsz, rect=rect, ctx=gtx_ctx, **KW)
    with monkeypatch.context() as mp:
        mp.setenv("GTX_PAD_SKIP", "0")
        plain = Detector(w, hw, imgsz=imgsz, rect=rect, ctx=gtx_ctx, **KW)
    assert plain.pad_skip()[0] is False
    for f in (frame, _frame(hw, 5)):
        a, b = det.detect(f), plain.detect(f)
        assert len(a) > 0 and a.xyxy.tobytes() == b.xyxy.tobytes() and a.conf.tobytes() == b.conf.tobytes()
        assert det.raw_output().tobytes() == plain.raw_output().tobytes()
    det.close(); plain.close()


def test_object_features_read_detects_inputs(gtx_ctx):
    """`with_reid: true, model: auto`: Detect's inputs (model.14 / 17 / 20) are ordinary maps, the vectors are obj_feats_table()'s"""
    from geotrax_amd.detector import Detector
    from oracle.yolov8_ref import detect
    from yolo12_ref import Yolo12Ref

    w, frame, _, _ = _case("n", "96x160")
    hw, imgsz, rect = SHAPES["96x160"]
    det = Detector(w, hw, imgsz=imgsz, rect=rect, obj_feats=True, ctx=gtx_ctx, **KW)
    d = det.detect(frame)
    xyxy, conf, cls, feats = detect(Yolo12Ref(w), frame, imgsz, rect, KW["conf"], KW["iou"], KW["classes"], True, KW["max_det"], return_feats=True)
    assert d.feats.shape == feats.shape == (len(conf), 64) and len(conf) > 0
    np.testing.assert_allclose(d.feats, feats[_pair(d, xyxy, conf)], atol=2e-4 * max(1.0, float(np.abs(feats).max())))
    det.close()


def test_saturation_falls_back_to_exact(gtx_ctx):
    """Scale l at gain 2.2 leaves fp16's range somewhere in the stack: the split-f16x3 detector re-runs the pass on its exact-fp32 twin
    (the same YOLO12 graph) and from then on equals the exact detector bit for bit."""
    from geotrax_amd.detector import Detector
    from geotrax_amd.weights import synthetic_yolo12
    from oracle.yolov8_ref import letterbox
    from yolo12_ref import Yolo12Ref

    hw, imgsz, rect = SHAPES["96x160"]
    w = synthetic_yolo12(seed=1, nc=4, scale="l", cls_bias=-3.0, gain=2.2, gamma=1.0)
    frame = _frame(hw)
    ref = Yolo12Ref(w)
    ref.forward(letterbox(frame, imgsz, rect)[0])
    peak = max(float(v.abs().max()) for v in ref.acts.values())
    print("largest activation", peak)
    assert peak > 65504.0                                            # the case is what it claims to be
    kw = dict(imgsz=imgsz, rect=rect, ctx=gtx_ctx, **KW)
    det = Detector(w, hw, fp32_split=True, **kw)
    first = det.detect(frame)
    assert det.saturated() and det.fell_back()
    exact = Detector(w, hw, fp32_split=False, **kw)
    assert first.conf.tobytes() == exact.detect(frame).conf.tobytes()
    assert det.detect(frame).xyxy.tobytes() == exact.detect(frame).xyxy.tobytes()
    assert det.raw_output().tobytes() == exact.raw_output().tobytes()
    det.close(); exact.close()


# ============================================================================ through the product
N_CLIP, CLIP_HW, CLIP_IMGSZ = 6, (96, 160), 160


def _clip_and_cfg(tmp_path, gtx_ctx):
    import test_extract_gpu as te
    import yaml
    from geotrax_amd.detector import Detector
    from geotrax_amd.synth import make_scene
    from geotrax_amd.weights import calibrate_cls_bias, save_weights, synthetic_yolo12

    scene = make_scene(seed=2, h=CLIP_HW[0], w=CLIP_HW[1])
    frames = np.stack([scene.render(t, 150) for t in range(0, N_CLIP * 12, 12)])
    clip = tmp_path / "clip.npy"
    np.save(clip, frames)
    w = synthetic_yolo12(seed=1, nc=4, scale="n", gain=1.7, box_weight_scale=0.002)
    det = Detector(w, CLIP_HW, imgsz=CLIP_IMGSZ, rect=True, ctx=gtx_ctx)
    det.detect(frames[0])
    w = calibrate_cls_bias(w, det.raw_output(logits=True)[:, 4:], 0.25, 12)
    det.close()
    path = tmp_path / "yolo12n.safetensors"
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
    """The extract chain on a YOLO12 file (ExtractEngine: batched, pipelined detector streams, ByteTrack + stabilizer) gives the
    tables of the blocking loop, which is YOLO(file).track frame by frame, byte for byte."""
    from geotrax_amd import extract as ex

    clip, cfg_path = _clip_and_cfg(tmp_path, gtx_ctx)
    model, config = _setup(clip, cfg_path)
    assert model.model.yaml_file == "yolo12n.yaml"
    t1, h1 = ex.track_with_model(model, config, logger)
    model, config = _setup(clip, cfg_path)
    config["main"].setdefault("engine", {})["pipelined"] = False
    t2, h2 = ex.track_with_model_blocking(model, config, logger)
    assert len(t1) > 0
    assert t1.dtype == t2.dtype and t1.tobytes() == t2.tobytes() and h1.tobytes() == h2.tobytes()
