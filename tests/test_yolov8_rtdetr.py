"""YOLOv8-RTDETR detectors (yolov8-rtdetr.yaml, geo-trax's train.sh `-rt`: the YOLOv8 trunk with an RTDETRDecoder at model.22), host
side: the topology every detector file is recognised as, the refusal of other RT-DETR layouts, the seeded weights' trunk, YOLO() /
RTDETR() on such a file, the folding of an unfused input projection on load, and the oracle's trunk. No GPU needed."""
import numpy as np
import pytest
import torch


@pytest.fixture(scope="module")
def hybrid():
    from geotrax_amd.weights import synthetic_yolov8_rtdetr

    return synthetic_yolov8_rtdetr(seed=3, nc=4, scale="s")


def test_every_detector_file_is_recognised_as_what_it_is(hybrid):
    from geotrax_amd.weights import (detector_topology, is_rtdetr, is_yolov8_cls, is_yolov8_p2, synthetic_rtdetr, synthetic_yolov8,
                                     synthetic_yolov8_cls, synthetic_yolov8_p2)

    assert detector_topology(hybrid) == ("yolov8-rtdetr", "model.22")
    assert is_rtdetr(hybrid) and not is_yolov8_p2(hybrid) and not is_yolov8_cls(hybrid)
    rt = synthetic_rtdetr(seed=0, nc=4)
    assert detector_topology(rt) == ("rtdetr-l", "model.28") and is_rtdetr(rt)
    assert detector_topology(synthetic_yolov8_p2(seed=0)) == ("yolov8-p2", "model.28")
    v8 = synthetic_yolov8(seed=0)
    assert detector_topology(v8) == ("yolov8", "model.22") and not is_rtdetr(v8)
    cls = synthetic_yolov8_cls(seed=0)
    assert not is_rtdetr(cls) and is_yolov8_cls(cls)
    # the permissive predicate: any decoder prefix, a partial dict, never raises
    assert is_rtdetr({"model.28.decoder.layers.0.linear1.weight": np.zeros((4, 4), np.float32)})
    assert is_rtdetr({"model.32.decoder.layers.0.linear1.weight": np.zeros((4, 4), np.float32)})
    assert not is_rtdetr({"model.22.cv3.0.2.weight": np.zeros((4, 4, 1, 1), np.float32)})


@pytest.mark.parametrize("layout", ["rtdetr-x", "resnet", "hybrid-without-trunk"])
def test_other_rtdetr_layouts_are_refused_naming_both_topologies(hybrid, layout):
    from geotrax_amd.weights import detector_topology, synthetic_rtdetr

    if layout == "rtdetr-x":          # rtdetr-x.yaml: a longer HGNetv2, decoder at model.32
        t = {k.replace("model.28.", "model.32.", 1): v for k, v in synthetic_rtdetr(seed=0, nc=4).items()}
    elif layout == "resnet":          # rtdetr-resnet50.yaml: ResNetLayer backbone, no HGStem
        t = {k: v for k, v in synthetic_rtdetr(seed=0, nc=4).items() if not k.startswith("model.0.")}
        t["model.0.conv1.conv.weight"] = np.zeros((64, 3, 7, 7), np.float32)
    else:                             # a decoder at model.22 without the YOLOv8 neck in front of it
        t = {k: v for k, v in hybrid.items() if not k.startswith("model.21.")}
    with pytest.raises(NotImplementedError) as e:
        detector_topology(t)
    assert "rtdetr-l" in str(e.value) and "yolov8-rtdetr" in str(e.value)


def test_models_refuse_other_layouts_before_the_yolov8_path():
    from geotrax_amd.detector import Detector
    from geotrax_amd.model import YOLO
    from geotrax_amd.weights import synthetic_rtdetr

    t = {k.replace("model.28.", "model.32.", 1): v for k, v in synthetic_rtdetr(seed=0, nc=4).items()}
    with pytest.raises(NotImplementedError, match="yolov8-rtdetr"):
        YOLO(t)
    with pytest.raises(NotImplementedError, match="yolov8-rtdetr"):
        Detector(t, (432, 768), imgsz=640)


@pytest.mark.parametrize("scale", ["n", "s"])
def test_seeded_trunk_is_the_seeded_yolov8_trunk(scale):
    from geotrax_amd.weights import synthetic_yolov8, synthetic_yolov8_rtdetr

    h = synthetic_yolov8_rtdetr(seed=7, nc=4, scale=scale)
    y = synthetic_yolov8(seed=7, nc=4, scale=scale)
    trunk = [k for k in y if not k.startswith("model.22.")]
    assert trunk and {k for k in h if not k.startswith("model.22.") and k != "rtdetr.meta"} == set(trunk)
    for k in trunk:
        assert h[k].tobytes() == y[k].tobytes(), k
    widths = {"n": (64, 128, 256), "s": (128, 256, 512)}[scale]
    for l, c in enumerate(widths):
        assert h[f"model.22.input_proj.{l}.0.weight"].shape == (256, c, 1, 1)
    assert h["model.22.enc_score_head.weight"].shape == (4, 256)
    assert "model.22.decoder.layers.5.linear1.weight" in h and "model.22.decoder.layers.6.linear1.weight" not in h
    np.testing.assert_array_equal(h["rtdetr.meta"], [8, 4, 300, 8])


def test_model_objects_on_a_hybrid_file(hybrid, tmp_path):
    from geotrax_amd.model import RTDETR, YOLO
    from geotrax_amd.weights import save_weights, synthetic_yolov8_rtdetr

    p = tmp_path / "yolov8s-rtdetr.safetensors"
    save_weights(hybrid, p)
    m = YOLO(str(p))
    assert m.model.yaml_file == "yolov8-rtdetr.yaml" and "rtdetr" in m.model.yaml_file     # the reference's RTDETR test
    assert m.is_rtdetr and not m.is_p2 and len(m.names) == 4
    m = RTDETR(str(p))
    assert m.is_rtdetr
    m80 = YOLO(synthetic_yolov8_rtdetr(seed=0, nc=80, scale="n"))
    assert len(m80.names) == 80 and m80.yaml_file == "yolov8-rtdetr.yaml"


def test_auto_reid_is_refused_for_the_hybrid(hybrid):
    from geotrax_amd.detector import Detector

    with pytest.raises(NotImplementedError):
        Detector(hybrid, (432, 768), imgsz=640, obj_feats=True)


def test_unfused_input_projection_is_folded_on_load(hybrid, tmp_path):
    """A checkpoint as convert_weights.py writes it when fuse() leaves the decoder's Sequential(Conv2d, BatchNorm2d) alone: load_weights
    folds it into .0.weight / .0.bias (it does so once is_rtdetr recognises the file)."""
    from geotrax_amd.weights import BN_EPS, load_weights, save_weights

    rng = np.random.default_rng(0)
    raw = dict(hybrid)
    for l in range(3):
        p = f"model.22.input_proj.{l}"
        w = raw.pop(p + ".0.weight")
        raw.pop(p + ".0.bias")
        raw[p + ".0.weight"] = w
        raw[p + ".1.weight"] = rng.uniform(0.5, 1.5, 256).astype(np.float32)
        raw[p + ".1.bias"] = rng.standard_normal(256).astype(np.float32)
        raw[p + ".1.running_mean"] = rng.standard_normal(256).astype(np.float32)
        raw[p + ".1.running_var"] = rng.uniform(0.5, 2.0, 256).astype(np.float32)
    path = tmp_path / "unfused.safetensors"
    save_weights(raw, path)
    t = load_weights(path)
    assert not any(k.startswith(f"model.22.input_proj.{l}.1.") for k in t for l in range(3))
    for l in range(3):
        p = f"model.22.input_proj.{l}"
        s = raw[p + ".1.weight"].astype(np.float64) / np.sqrt(raw[p + ".1.running_var"].astype(np.float64) + BN_EPS)
        want_w = (raw[p + ".0.weight"].astype(np.float64) * s[:, None, None, None]).astype(np.float32)
        want_b = (raw[p + ".1.bias"] - raw[p + ".1.running_mean"].astype(np.float64) * s).astype(np.float32)
        np.testing.assert_array_equal(t[p + ".0.weight"], want_w)
        np.testing.assert_array_equal(t[p + ".0.bias"], want_b)
    for k in hybrid:                                          # everything else loads as it was saved
        if ".input_proj." not in k:
            np.testing.assert_array_equal(t[k], hybrid[k])


def test_fuse_repconv_without_biases():
    from geotrax_amd.weights import fuse_repconv

    rng = np.random.default_rng(1)
    w3 = rng.standard_normal((8, 8, 3, 3)).astype(np.float32)
    w1 = rng.standard_normal((8, 8, 1, 1)).astype(np.float32)
    f = fuse_repconv({"model.16.m.0.conv1.conv.weight": w3, "model.16.m.0.conv2.conv.weight": w1})
    np.testing.assert_array_equal(f["model.16.m.0.conv.bias"], np.zeros(8, np.float32))
    want = w3.astype(np.float64)
    want[:, :, 1, 1] += w1[:, :, 0, 0]
    np.testing.assert_array_equal(f["model.16.m.0.conv.weight"], want.astype(np.float32))
    b = rng.standard_normal(8).astype(np.float32)
    g = fuse_repconv({"model.16.m.0.conv1.conv.weight": w3, "model.16.m.0.conv2.conv.weight": w1, "model.16.m.0.conv2.conv.bias": b})
    np.testing.assert_array_equal(g["model.16.m.0.conv.bias"], b)


def test_calibration_shifts_the_hybrid_decoder():
    from geotrax_amd.weights import calibrate_rtdetr_scores, synthetic_yolov8_rtdetr

    t = synthetic_yolov8_rtdetr(seed=0, nc=4, scale="n")
    logits = np.random.default_rng(0).standard_normal((300, 4)).astype(np.float32)
    c = calibrate_rtdetr_scores(t, logits, 0.25, 40)
    changed = [k for k in t if not np.array_equal(t[k], c[k])]
    assert changed == ["model.22.dec_score_head.5.bias"]
    shifted = logits.max(1) + float(c[changed[0]][0] - t[changed[0]][0])
    assert abs(int((1 / (1 + np.exp(-shifted)) > 0.25).sum()) - 40) <= 1


def test_oracle_trunk_is_the_yolov8_oracle_trunk():
    """tests/yolov8_rtdetr_ref.py runs YoloV8Ref's arithmetic on model.0-21 and the RT-DETR decoder on model.15 / 18 / 21."""
    from geotrax_amd.weights import synthetic_yolov8, synthetic_yolov8_rtdetr
    from oracle.rtdetr_ref import postprocess
    from oracle.yolov8_ref import YoloV8Ref
    from yolov8_rtdetr_ref import YoloV8RtDetrRef

    h = synthetic_yolov8_rtdetr(seed=2, nc=4, scale="n", nq=50, ndl=2)
    ref = YoloV8RtDetrRef(h)
    assert (ref.nq, ref.ndl, ref.nc) == (50, 2, 4)
    x = torch.rand(1, 3, 128, 128, generator=torch.Generator().manual_seed(0))
    pred = ref.forward(x)
    assert pred.shape == (1, 50, 8) and torch.isfinite(pred).all()
    v8 = YoloV8Ref(synthetic_yolov8(seed=2, nc=4, scale="n"))
    v8.forward(x)
    for name in ("model.0.conv", "model.9", "model.15", "model.18", "model.21"):
        assert torch.equal(ref.acts[name], v8.acts[name]), name
    assert ref.acts["model.22.feats"].shape == (1, 16 * 16 + 8 * 8 + 4 * 4, 256)
    assert "model.22.decoder.layers.1" in ref.acts and not any(k.startswith("model.28") for k in ref.acts)
    xyxy, score, cls, _ = postprocess(pred[0].numpy(), (100, 200), 0.0)
    assert len(score) == 50 and (np.diff(score) <= 0).all()
