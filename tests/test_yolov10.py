"""YOLOv10 on the host side: the topology is read off the tensor names, the layer specs follow the yaml table, RepVGGDW and BN
folding, the two-stage cut of v10Detect against one global top-300, the `end2end` config surface and the converter's round trip.
No GPU."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))

from geotrax_amd import weights as W  # noqa: E402
from geotrax_amd.detector import resolve_end2end  # noqa: E402


@pytest.fixture(scope="module", params=["n", "s"])
def scaled(request):
    return request.param, W.synthetic_yolov10(seed=0, nc=4, scale=request.param)


def test_topology_is_read_off_the_names(scaled):
    scale, t = scaled
    assert W.is_yolov10(t)
    assert W.detector_topology(t) == ("yolov10", "model.23")
    assert W.check_yolov10(t) == scale
    fused = {k: v for k, v in t.items() if not k.startswith(("model.23.cv2.", "model.23.cv3."))}   # what ultralytics' fuse() leaves
    assert W.detector_topology(fused) == ("yolov10", "model.23") and not W.yolov10_has_one2many(fused)


def test_other_families_are_unchanged():
    assert W.detector_topology(W.synthetic_yolov8(0, 4, "n")) == ("yolov8", "model.22")
    assert W.detector_topology(W.synthetic_yolov8_p2(0, 4, "n")) == ("yolov8-p2", "model.28")
    assert W.detector_topology(W.synthetic_yolo11(0, 4, "n")) == ("yolo11", "model.23")
    assert W.detector_topology(W.synthetic_yolov8_rtdetr(0, 4, "n")) == ("yolov8-rtdetr", "model.22")
    assert not W.is_yolov10(W.synthetic_yolo11(0, 4, "s"))


def test_refusals(scaled):
    _, t = scaled
    cv4 = dict(t)
    cv4["model.23.cv4.0.0.conv.weight"] = t["model.23.cv2.0.0.conv.weight"]
    moved = dict(t)
    moved["model.8.attn.qkv.conv.weight"] = t["model.10.attn.qkv.conv.weight"]
    at24 = {k.replace("model.23.", "model.24."): v for k, v in t.items()}
    past = dict(t)
    past["model.24.conv.weight"] = t["model.0.conv.weight"]
    half = {k: v for k, v in t.items() if not k.startswith("model.23.cv3.1.")}           # the one-to-many pair only partly there
    for bad in (cv4, moved, at24, past, half):
        with pytest.raises(NotImplementedError, match="yolov10"):
            W.detector_topology(bad)
    wide = dict(t)
    wide["model.0.conv.weight"] = np.zeros((48, 3, 3, 3), np.float32)
    with pytest.raises(NotImplementedError, match="yolov10m"):
        W.detector_topology(wide)


def test_yolo11_with_one2one_still_gives_the_yolo11_message():
    t = W.synthetic_yolo11(0, 4, "n")
    t["model.23.one2one_cv2.0.0.conv.weight"] = t["model.23.cv2.0.0.conv.weight"]
    with pytest.raises(NotImplementedError, match="yolo11.yaml"):
        W.detector_topology(t)
    with pytest.raises(NotImplementedError, match="yolo11.yaml"):
        W.check_yolo11(t)


def test_layer_specs_follow_the_table():
    for scale, c3, c4, c5 in (("n", 64, 128, 256), ("s", 128, 256, 512)):
        sp = {n: (s, a) for n, s, a in W.yolov10_layer_specs(scale, 4)}
        assert sp["model.0.conv"][0] == (c3 // 4, 3, 3, 3)
        assert sp["model.5.cv1.conv"] == ((c4, c3, 1, 1), True)
        assert sp["model.5.cv2.conv"] == ((c4, 1, 3, 3), False)                   # SCDown's depthwise: stride 2, no activation
        assert sp["model.7.cv2.conv"] == ((c5, 1, 3, 3), False) and sp["model.20.cv2.conv"] == ((c4, 1, 3, 3), False)
        c = c5 // 2
        assert sp["model.10.attn.qkv.conv"] == ((2 * c, c, 1, 1), False) and sp["model.10.attn.pe.conv"] == ((c, 1, 3, 3), False)
        assert sp["model.10.attn.proj.conv"][1] is False and sp["model.10.ffn.1.conv"][1] is False and sp["model.10.ffn.0.conv"][1] is True
        assert sp["model.22.m.0.cv1.0.conv"] == ((c, 1, 3, 3), True) and sp["model.22.m.0.cv1.1.conv"] == ((2 * c, c, 1, 1), True)
        assert sp["model.22.m.0.cv1.2.conv"] == ((2 * c, 1, 7, 7), True)          # the fused RepVGGDW of a large-kernel CIB
        assert sp["model.22.m.0.cv1.3.conv"] == ((c, 2 * c, 1, 1), True) and sp["model.22.m.0.cv1.4.conv"] == ((c, 1, 3, 3), True)
        assert ("model.8.m.0.cv1.2.conv" in sp) == (scale == "s") and ("model.8.m.0.cv1.conv" in sp) == (scale == "n")
        assert sp["model.13.m.0.cv1.conv"][0] == (c4 // 2, c4 // 2, 3, 3)         # the neck keeps plain C2f
        for pair in (("cv2", "cv3"), ("one2one_cv2", "one2one_cv3")):
            assert sp[f"model.23.{pair[0]}.2.2"] == ((64, 64, 1, 1), False) and sp[f"model.23.{pair[1]}.2.2"] == ((4, max(c3, 4), 1, 1), False)
            assert sp[f"model.23.{pair[1]}.1.0.0.conv"] == ((c4, 1, 3, 3), True)
        t = W.synthetic_yolov10(0, 4, scale)
        assert set(k[: -len(".weight")] for k in t if k.endswith(".weight")) == set(sp)
        assert not np.array_equal(t["model.23.cv3.0.2.weight"], t["model.23.one2one_cv3.0.2.weight"])     # the two heads are drawn apart


def _bn(rng, c):
    return dict(weight=rng.uniform(0.5, 1.5, c), bias=rng.normal(0, 0.1, c), running_mean=rng.normal(0, 0.1, c), running_var=rng.uniform(0.5, 2.0, c))


def _unfused_repvggdw(rng, p, c):
    t = {}
    for br, k in (("conv", 7), ("conv1", 3)):
        t[f"{p}.{br}.conv.weight"] = rng.normal(0, 0.2, (c, 1, k, k)).astype(np.float32)
        t.update({f"{p}.{br}.bn.{n}": v.astype(np.float32) for n, v in _bn(rng, c).items()})
    return t


def test_repvggdw_folding_equals_the_two_branch_forward():
    from yolov10_ref import repvggdw

    rng = np.random.default_rng(3)
    c = 24
    folded = W.fold_bn(_unfused_repvggdw(rng, "m.cv1.2", c))
    one = W.fold_repvggdw(folded)
    assert set(one) == {"m.cv1.2.conv.weight", "m.cv1.2.conv.bias"} and one["m.cv1.2.conv.weight"].shape == (c, 1, 7, 7)
    x = torch.from_numpy(rng.normal(0, 1, (2, c, 13, 19)).astype(np.float32))
    tt = lambda n: torch.from_numpy(folded[n])
    want = repvggdw(x, tt("m.cv1.2.conv.conv.weight"), tt("m.cv1.2.conv.conv.bias"), tt("m.cv1.2.conv1.conv.weight"), tt("m.cv1.2.conv1.conv.bias"))
    got = F.silu(F.conv2d(x, torch.from_numpy(one["m.cv1.2.conv.weight"]), torch.from_numpy(one["m.cv1.2.conv.bias"]), padding=3, groups=c))
    # fp32 rounding: 49 + 9 products of O(0.2) x O(1) either way, summed in another order -- a few ulp of a sum of magnitude ~2
    assert float((got - want).abs().max()) < 58 * 2.0 ** -23 * 4


def test_bn_folding_of_the_depthwise_noact_conv():
    rng = np.random.default_rng(4)
    c = 16
    w = rng.normal(0, 0.3, (c, 1, 3, 3)).astype(np.float32)
    bn = _bn(rng, c)
    t = {"model.5.cv2.conv.weight": w, **{f"model.5.cv2.bn.{n}": v.astype(np.float32) for n, v in bn.items()}}
    f = W.fold_bn(t)
    x = torch.from_numpy(rng.normal(0, 1, (1, c, 13, 19))).double()
    y = F.conv2d(x, torch.from_numpy(w).double(), None, stride=2, padding=1, groups=c)
    g, b, m, v = (torch.from_numpy(np.asarray(bn[n], np.float32)).double().view(1, c, 1, 1) for n in ("weight", "bias", "running_mean", "running_var"))
    want = (y - m) / torch.sqrt(v + W.BN_EPS) * g + b
    got = F.conv2d(x, torch.from_numpy(f["model.5.cv2.conv.weight"]).double(), torch.from_numpy(f["model.5.cv2.conv.bias"]).double(), stride=2, padding=1, groups=c)
    assert float((got - want).abs().max()) < 1e-5             # the folded weights are rounded to fp32 once


@pytest.mark.parametrize("seed,A,nc", [(0, 336, 4), (1, 5000, 4), (2, 2100, 80), (3, 200, 3)])
def test_two_stage_cut_equals_the_global_top300(seed, A, nc):
    from yolov10_ref import MAX_DET, global_topk, two_stage_topk

    assert MAX_DET == W.V10_MAX_DET == 300
    rng = np.random.default_rng(seed)
    scores = ((rng.permutation(A * nc) + 0.5) / (A * nc)).astype(np.float32).reshape(A, nc)   # a seeded shuffle of distinct fp32 values in (0, 1)
    assert len(np.unique(scores)) == scores.size              # no ties: the two cuts are then the same set in the same order
    a1, c1, s1 = two_stage_topk(scores)
    a2, c2, s2 = global_topk(scores)
    assert len(s1) == min(300, A * nc)
    np.testing.assert_array_equal(a1, a2)
    np.testing.assert_array_equal(c1, c2)
    np.testing.assert_array_equal(s1, s2)


def test_end2end_config_surface():
    v10, v8, v11 = W.synthetic_yolov10(0, 4, "n"), W.synthetic_yolov8(0, 4, "n"), W.synthetic_yolo11(0, 4, "n")
    assert resolve_end2end("yolov10", v10, None) is True and resolve_end2end("yolov10", v10, True) is True
    assert resolve_end2end("yolov10", v10, False) is False
    for g, t in (("yolov8", v8), ("yolo11", v11)):
        assert resolve_end2end(g, t, None) is False and resolve_end2end(g, t, False) is False
        with pytest.raises(ValueError, match="end2end"):
            resolve_end2end(g, t, True)
    fused = {k: v for k, v in v10.items() if not k.startswith(("model.23.cv2.", "model.23.cv3."))}
    assert resolve_end2end("yolov10", fused, None) is True
    with pytest.raises(ValueError, match="cv2 / cv3"):
        resolve_end2end("yolov10", fused, False)
    from geotrax_amd.extract import _engine_kwargs

    cfg = lambda ul: {"ultralytics": ul, "main": {"extraction": {"stabilize": False}}, "stabilo": {}}
    assert "end2end" not in _engine_kwargs(cfg({"end2end": None}))[0] and "end2end" not in _engine_kwargs(cfg({}))[0]
    assert _engine_kwargs(cfg({"end2end": False}))[0]["end2end"] is False and _engine_kwargs(cfg({"end2end": True}))[0]["end2end"] is True
    from geotrax_amd.model import YOLO

    assert YOLO(v10).yaml_file == "yolov10n.yaml" and YOLO(W.synthetic_yolov10(0, 4, "s")).yaml_file == "yolov10s.yaml"


def test_converter_meta_round_trip(tmp_path):
    from convert_weights import convert_state_dict

    rng = np.random.default_rng(5)
    fused = W.synthetic_yolov10(0, 4, "n")
    sd = {}
    for k, v in fused.items():                               # an unfused dict: conv + BN pairs, the RepVGGDW as its two branches
        if k == "model.22.m.0.cv1.2.conv.weight":
            sd.update(_unfused_repvggdw(rng, "model.22.m.0.cv1.2", v.shape[0]))
        elif k == "model.22.m.0.cv1.2.conv.bias":
            continue
        elif k.endswith(".conv.weight"):
            p = k[: -len(".conv.weight")]
            sd[k] = v
            sd.update({f"{p}.bn.{n}": x.astype(np.float32) for n, x in _bn(rng, v.shape[0]).items()})
            sd[f"{p}.bn.num_batches_tracked"] = np.zeros((), np.float32)
        elif k.endswith(".conv.bias"):
            continue
        else:
            sd[k] = v
    out = convert_state_dict(sd)
    assert out["model.22.m.0.cv1.2.conv.weight"].shape == (fused["model.22.m.0.cv1.2.conv.weight"].shape[0], 1, 7, 7)
    assert "model.23.cv2.0.0.conv.weight" in out and "model.23.one2one_cv3.2.2.bias" in out and not any(".bn." in k for k in out)
    np.testing.assert_array_equal(out["detector.meta"], np.asarray([10, 1, 1, 300], np.float32))
    W.save_weights(out, tmp_path / "v10n.safetensors")
    back = W.load_weights(tmp_path / "v10n.safetensors")
    assert W.detector_topology(back) == ("yolov10", "model.23") and W.detector_meta(back) == dict(family="yolov10", one2many=True, end2end=True, max_det=300)
    assert W.detector_meta(fused) is None
