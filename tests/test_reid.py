"""The separate ReID network (`with_reid: true, model: <cls checkpoint>`), host side: YOLOv8-cls weights, the topology check, the
tracker config, the C ABI's symbols and the crop geometry of the reference and of the library. No GPU needed."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent

# yolov8-cls.yaml at each scale: model.0 / model.7 widths, C2f repeats (model.2, 4, 6, 8), embedding dim = model.8's width
CLS_SHAPES = {"n": (16, 256, (1, 2, 2, 1)), "s": (32, 512, (1, 2, 2, 1)), "m": (48, 768, (2, 4, 4, 2)),
              "l": (64, 1024, (3, 6, 6, 3)), "x": (80, 1280, (3, 6, 6, 3))}


@pytest.mark.parametrize("scale", list(CLS_SHAPES))
def test_synthetic_cls_has_the_yaml_shapes(scale):
    from geotrax_amd.weights import is_yolov8_cls, synthetic_yolov8_cls

    c0, c7, reps = CLS_SHAPES[scale]
    t = synthetic_yolov8_cls(seed=1, scale=scale, nc=10)
    assert t["model.0.conv.weight"].shape == (c0, 3, 3, 3)
    assert t["model.7.conv.weight"].shape == (c7, c7 // 2, 3, 3)
    assert t["model.8.cv2.conv.weight"].shape == (c7, (2 + reps[3]) * c7 // 2, 1, 1)
    assert t["model.9.linear.weight"].shape == (10, 1280)
    for i, n in zip((2, 4, 6, 8), reps):
        assert f"model.{i}.m.{n - 1}.cv1.conv.weight" in t and f"model.{i}.m.{n}.cv1.conv.weight" not in t
    assert is_yolov8_cls(t)
    t2 = synthetic_yolov8_cls(seed=1, scale=scale, nc=10)
    assert all(np.array_equal(t[k], t2[k]) for k in t)                           # seeded


def test_cls_weights_round_trip(tmp_path):
    from geotrax_amd.weights import cls_imgsz, load_weights, save_weights, synthetic_yolov8_cls

    t = synthetic_yolov8_cls(seed=2, scale="n")
    t["cls.meta"] = np.array([256], np.float32)
    save_weights(t, tmp_path / "cls.safetensors")
    back = load_weights(tmp_path / "cls.safetensors")
    assert set(back) == set(t) and all(np.array_equal(back[k], t[k]) for k in t)
    assert cls_imgsz(back) == 256 and cls_imgsz({}) == 224


def _yolo11_cls_like(c=16):
    """A YOLO11n-cls-shaped file: C3k2 blocks under C2f's names with a quarter-width hidden layer, C2PSA at model.9, Classify at 10."""
    rng = np.random.default_rng(0)
    w = lambda *s: rng.standard_normal(s).astype(np.float32)
    t = {"model.0.conv.weight": w(c, 3, 3, 3), "model.1.conv.weight": w(2 * c, c, 3, 3)}
    chans = {2: (2 * c, 4 * c), 4: (4 * c, 8 * c), 6: (8 * c, 8 * c), 8: (16 * c, 16 * c)}
    for i, (ci, co) in chans.items():
        h = ci // 4
        t[f"model.{i}.cv1.conv.weight"] = w(2 * h, ci, 1, 1)
        t[f"model.{i}.m.0.cv1.conv.weight"] = w(h // 2, h, 3, 3)
        t[f"model.{i}.m.0.cv2.conv.weight"] = w(h, h // 2, 3, 3)
        t[f"model.{i}.cv2.conv.weight"] = w(co, 3 * h, 1, 1)
    for i, (ci, co) in ((3, (4 * c, 4 * c)), (5, (8 * c, 8 * c)), (7, (8 * c, 16 * c))):
        t[f"model.{i}.conv.weight"] = w(co, ci, 3, 3)
    t["model.9.m.0.attn.qkv.conv.weight"] = w(32, 16 * c, 1, 1)
    t["model.10.linear.weight"] = w(1000, 1280)
    return t


def test_is_yolov8_cls_refuses_other_topologies():
    from geotrax_amd.weights import is_yolov8_cls, synthetic_rtdetr, synthetic_yolov8

    assert not is_yolov8_cls(synthetic_yolov8(seed=0, scale="n", nc=4))
    assert not is_yolov8_cls(synthetic_rtdetr(seed=0, nc=4, width=0.25, hd=64, ndl=1))
    with pytest.raises(NotImplementedError, match="YOLOv8-cls"):
        is_yolov8_cls(_yolo11_cls_like())
    t = _yolo11_cls_like()                                                       # the same without the give-away keys: widths decide
    t = {k: v for k, v in t.items() if ".attn." not in k and not k.startswith("model.10.")}
    with pytest.raises(NotImplementedError, match="YOLOv8-cls"):
        is_yolov8_cls(t)


@pytest.mark.parametrize("ttype", ["botsort", "deepocsort", "tracktrack"])
def test_make_tracker_takes_a_cls_checkpoint(tmp_path, monkeypatch, ttype):
    from geotrax_amd.model import YOLO
    from geotrax_amd.weights import save_weights, synthetic_yolov8_cls

    save_weights(synthetic_yolov8_cls(seed=0, scale="n"), tmp_path / "reid-cls.safetensors")
    monkeypatch.chdir(tmp_path)                                                  # relative: against the working directory
    trk = YOLO.__new__(YOLO)._make_tracker({"tracker_type": ttype, "with_reid": True, "model": "reid-cls.safetensors"})
    assert trk.with_reid and trk.reid_tensors["model.8.cv2.conv.weight"].shape[0] == 256
    auto = YOLO.__new__(YOLO)._make_tracker({"tracker_type": ttype, "with_reid": True, "model": "auto"})
    assert auto.reid_tensors is None


@pytest.mark.parametrize("name", ["osnet_x0_25.pt", "yolov8n-cls.pt", "osnet_x1_0_msmt17", "missing-dir/none.onnx"])
def test_make_tracker_still_refuses_other_models(name):
    from geotrax_amd.model import YOLO

    with pytest.raises(NotImplementedError):
        YOLO.__new__(YOLO)._make_tracker({"tracker_type": "botsort", "with_reid": True, "model": name})


def test_make_tracker_refuses_a_detect_file_as_reid_model(tmp_path):
    from geotrax_amd.model import YOLO
    from geotrax_amd.weights import save_weights, synthetic_yolov8

    save_weights(synthetic_yolov8(seed=0, scale="n", nc=4), tmp_path / "det.safetensors")
    with pytest.raises(NotImplementedError, match="YOLOv8-cls"):
        YOLO.__new__(YOLO)._make_tracker({"tracker_type": "botsort", "with_reid": True, "model": str(tmp_path / "det.safetensors")})


EMBEDDER_SYMBOLS = {"gtx_embedder_create", "gtx_embedder_destroy", "gtx_embedder_set_tensor", "gtx_embedder_finalize", "gtx_embedder_dim",
                    "gtx_embedder_submit_dev", "gtx_embedder_collect", "gtx_embedder_embed_dev", "gtx_embedder_crops",
                    "gtx_embedder_layer_output", "gtx_embedder_saturated", "gtx_embedder_fell_back", "gtx_embedder_profile",
                    "gtx_reid_crop_boxes"}


def test_embedder_abi_symbols():
    from geotrax_amd import _lib

    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "gtx.h").read_text(), flags=re.S)
    declared = set(re.findall(r"\b(gtx_[a-z0-9_]+)\s*\(", text))
    assert EMBEDDER_SYMBOLS <= declared and EMBEDDER_SYMBOLS <= set(_lib._SIGNATURES)
    lib = _lib.load()
    for s in EMBEDDER_SYMBOLS:
        assert hasattr(lib, s), s
    assert lib.gtx_abi_version() == 14


def test_reference_crop_geometry_hand_cases():
    import reid_ref

    h, w = 2160, 3840
    cases = [
        ([0, 0, 40, 30], [0, 0, 45, 35]),                   # top-left corner: xywh (20, 15, 40, 30) -> (50.8, 40.6) wide -> clipped at 0
        ([3800, 2100, 3840, 2160], [3794, 2094, 3840, 2160]),   # bottom-right corner: clipped at w, h
        ([100, 100, 101, 101], [94, 94, 106, 106]),         # a 1-px box: 1 * 1.02 + 10 = 11.02 -> 100.5 -/+ 5.51 -> 94.99 / 106.01 truncated
        ([1000, 500, 1300, 560], [992, 494, 1308, 565]),    # wider than 224: 306 + 10 = 316 -> 1150 -/+ 158; 61.2 + 10 -> 530 -/+ 35.6
        ([-20.0, 50, 30, 90], [0, 44, 35, 95]),             # a box reaching past the left edge
    ]
    for box, want in cases:
        assert reid_ref.crop_box(np.array([box], np.float32), h, w)[0].tolist() == want, (box, want)
    # .long() truncates toward zero: a left edge at -0.9 becomes 0 before the clip, not -1
    assert reid_ref.crop_box(np.array([[4.5, 4.5, 4.5, 4.5]], np.float32), h, w)[0].tolist() == [0, 0, 9, 9]
    # resize + center crop: short side 224, long side int(224 * long / short), offsets with Python's round (ties to even)
    assert reid_ref.resized_size(100, 300, 224) == (224, 672)
    assert reid_ref.resized_size(301, 100, 224) == (674, 224)
    assert reid_ref.center_offset(227, 224) == 2        # 1.5 -> 2
    assert reid_ref.center_offset(229, 224) == 2        # 2.5 -> 2 (even)
    assert reid_ref.center_offset(231, 224) == 4        # 3.5 -> 4
    assert reid_ref.center_offset(226, 224) == 1


def test_library_crop_geometry_equals_reference():
    import reid_ref
    from geotrax_amd.reid import crop_boxes

    rng = np.random.default_rng(5)
    b = rng.uniform(-60, 3900, (3000, 4)).astype(np.float32)
    b[:, 2:] = b[:, :2] + rng.uniform(0, 700, (3000, 2)).astype(np.float32)
    b[:200, 2:] = b[:200, :2] + rng.integers(0, 3, (200, 2)).astype(np.float32)   # tiny boxes
    np.testing.assert_array_equal(crop_boxes(b, (2160, 3840)), reid_ref.crop_box(b, 2160, 3840))
