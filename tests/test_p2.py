"""YOLOv8-P2 detectors (yolov8-p2.yaml: a fourth Detect level at stride 4), host side: the layer specs against the yaml, the
topology check, YOLO() on a P2 file, the ReID refusal and the oracle's backbone. No GPU needed."""
import numpy as np
import pytest

# yolov8-p2.yaml at each scale: model.18 (P2/4) width, Detect box / class widths (nc = 4), model.27 (P5) width, C2f repeats
P2_SHAPES = {"n": (32, 64, 32, 256, 1), "s": (64, 64, 64, 512, 1), "m": (96, 64, 96, 576, 2)}


@pytest.mark.parametrize("scale", list(P2_SHAPES))
def test_p2_specs_have_the_yaml_widths(scale):
    from geotrax_amd.weights import yolov8_layer_specs, yolov8_p2_layer_specs

    c18, cb, cc, c27, reps = P2_SHAPES[scale]
    spec = {n: s for n, s, _ in yolov8_p2_layer_specs(scale, nc=4)}
    c2, c15 = c18, 2 * c18                                                       # model.2 = P2 width, model.15 = P3 width
    assert spec["model.18.cv2.conv"] == (c18, (2 + reps) * c18 // 2, 1, 1)
    assert spec["model.18.cv1.conv"] == (c18, c15 + c2, 1, 1)                   # Concat(17) = [Upsample(model.15), model.2]
    assert spec["model.19.conv"] == (c18, c18, 3, 3)
    assert spec["model.21.cv1.conv"] == (c15, c18 + c15, 1, 1)                  # Concat(20) = [model.19, model.15]
    assert spec["model.22.conv"] == (c15, c15, 3, 3)
    assert spec["model.27.cv2.conv"][0] == c27
    assert f"model.18.m.{reps - 1}.cv2.conv" in spec and f"model.18.m.{reps}.cv2.conv" not in spec
    for l, cin in enumerate((c18, 2 * c18, 4 * c18, c27)):
        assert spec[f"model.28.cv2.{l}.0.conv"] == (cb, cin, 3, 3)
        assert spec[f"model.28.cv2.{l}.1.conv"] == (cb, cb, 3, 3)
        assert spec[f"model.28.cv2.{l}.2"] == (64, cb, 1, 1)
        assert spec[f"model.28.cv3.{l}.0.conv"] == (cc, cin, 3, 3)
        assert spec[f"model.28.cv3.{l}.2"] == (4, cc, 1, 1)
    assert "model.28.cv2.4.0.conv" not in spec and not any(n.startswith(("model.16.", "model.29.")) for n in spec)
    base = {n: s for n, s, _ in yolov8_layer_specs(scale, nc=4) if int(n.split(".")[1]) <= 9}
    assert {n: s for n, s in spec.items() if int(n.split(".")[1]) <= 9} == base  # the backbone is yolov8.yaml's


def test_synthetic_p2_weights():
    from geotrax_amd.weights import synthetic_yolov8_p2, yolov8_p2_layer_specs

    t = synthetic_yolov8_p2(seed=0, nc=4, scale="s")
    assert {n + ".weight" for n, _, _ in yolov8_p2_layer_specs("s", 4)} <= set(t)
    assert all(v.dtype == np.float32 for v in t.values())
    b = [float(t[f"model.28.cv3.{l}.2.bias"].mean()) for l in range(4)]
    assert b[0] > -5 and b[1] > -5 and b[2] < -1e3 and b[3] < -1e3             # default: only the stride-4 and stride-8 heads can fire
    u = synthetic_yolov8_p2(seed=0, nc=4, scale="s")
    assert all(np.array_equal(t[k], u[k]) for k in t)                           # seeded


def test_yolov8_weights_are_unchanged():
    """synthetic_yolov8 / yolov8_layer_specs are where bench.py's seeded weights come from: same names, shapes and values as before."""
    import hashlib

    from geotrax_amd.weights import synthetic_yolov8, yolov8_layer_specs

    spec = yolov8_layer_specs("s", 4)
    assert len(spec) == 63 and spec[-1] == ("model.22.cv3.2.2", (4, 128, 1, 1), False)
    t = synthetic_yolov8(seed=0, nc=4, scale="s", level_bias=(0.0, -1e4, -1e4), box_weight_scale=0.002, smooth_cls=True,
                         box_decay=(0.2, 0.3, 0.2, 0.3))                       # bench.py's SYNTH_KW
    assert len(t) == 126
    digest = hashlib.sha1(b"".join(t[k].tobytes() for k in sorted(t))).hexdigest()
    assert digest == "e4a3436e1e767942a777e51965015e7976a0f46e"               # the values the parent commit drew


def test_topology_detection():
    from geotrax_amd.weights import (is_rtdetr, is_yolov8_cls, is_yolov8_p2, synthetic_rtdetr, synthetic_yolov8, synthetic_yolov8_cls,
                                     synthetic_yolov8_p2)

    p2 = synthetic_yolov8_p2(seed=0, scale="n", nc=4)
    assert is_yolov8_p2(p2)
    assert not is_rtdetr(p2) and not is_yolov8_cls(p2)
    assert not is_yolov8_p2(synthetic_yolov8(seed=0, scale="n", nc=4))
    assert not is_yolov8_p2(synthetic_rtdetr(seed=0, nc=4, width=0.25, hd=64, ndl=1))
    assert not is_yolov8_p2(synthetic_yolov8_cls(seed=0, scale="n"))


def test_yolo_loads_a_p2_file(tmp_path):
    from geotrax_amd.model import YOLO
    from geotrax_amd.weights import save_weights, synthetic_yolov8, synthetic_yolov8_p2

    save_weights(synthetic_yolov8_p2(seed=0, scale="n", nc=3), tmp_path / "yolov8n-p2.safetensors")
    (tmp_path / "yolov8n-p2.names.yaml").write_text("0: car\n1: bus\n2: truck\n")
    m = YOLO(tmp_path / "yolov8n-p2.safetensors")
    assert m.model.yaml_file == "yolov8-p2.yaml" and not m.is_rtdetr and m.is_p2
    assert m.names == {0: "car", 1: "bus", 2: "truck"}
    save_weights(synthetic_yolov8_p2(seed=0, scale="n", nc=5), tmp_path / "other.safetensors")
    m = YOLO(tmp_path / "other.safetensors")
    assert m.names == {i: str(i) for i in range(5)}
    assert YOLO(synthetic_yolov8(seed=0, scale="n", nc=4)).yaml_file == "yolov8.yaml"


def test_make_tracker_refuses_a_p2_file_as_reid_model(tmp_path):
    from geotrax_amd.model import YOLO
    from geotrax_amd.weights import save_weights, synthetic_yolov8_p2

    save_weights(synthetic_yolov8_p2(seed=0, scale="n", nc=4), tmp_path / "p2.safetensors")
    with pytest.raises(NotImplementedError, match="not a classification checkpoint"):
        YOLO.__new__(YOLO)._make_tracker({"tracker_type": "botsort", "with_reid": True, "model": str(tmp_path / "p2.safetensors")})


def test_oracle_backbone_equals_yolov8_oracle():
    """The P2 oracle's model.0-9 are YoloV8Ref's on the same backbone tensors; its head has the yaml's strides and anchor count."""
    import torch
    from oracle.yolov8_ref import YoloV8Ref
    from geotrax_amd.weights import synthetic_yolov8, synthetic_yolov8_p2
    from yolov8p2_ref import YoloV8P2Ref

    p2 = synthetic_yolov8_p2(seed=2, scale="n", nc=4)
    v8 = synthetic_yolov8(seed=5, scale="n", nc=4)
    v8.update({k: v for k, v in p2.items() if int(k.split(".")[1]) <= 9})
    x = torch.rand(1, 3, 128, 160, generator=torch.Generator().manual_seed(0))
    a, b = YoloV8P2Ref(p2), YoloV8Ref(v8)
    out = a.forward(x)
    b.forward(x)
    for name in ("model.0.conv", "model.1.conv", "model.2", "model.3.conv", "model.4", "model.6", "model.8", "model.9"):
        assert torch.equal(a.acts[name], b.acts[name]), name
    assert out.shape == (1, 32 * 40 + 16 * 20 + 8 * 10 + 4 * 5, 8)
    assert [tuple(t.shape[2:]) for t in a.detect_inputs] == [(32, 40), (16, 20), (8, 10), (4, 5)]
    assert a.acts["model.18"].shape[1] == 32 and a.acts["model.28.feat0"].shape[1] == 64 + 32
    assert a.obj_feats_table().shape == (out.shape[1], 32)
    # anchor 0 of the stride-4 level sits at (2, 2) network pixels: its box centre is within the DFL reach of it
    assert abs(float(out[0, 0, 0]) - 2.0) < 4 * 16 and abs(float(out[0, 32 * 40, 0]) - 4.0) < 8 * 16
