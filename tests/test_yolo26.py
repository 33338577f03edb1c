"""YOLO26 on the host side: the topology is read off the tensor names, the layer specs follow the yaml table per scale, the refusals,
the two-stage cut against one global top-300, the restatement's box decode on a hand-worked map, the `end2end` config surface and
the converter's folding. No GPU."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))

from geotrax_amd import weights as W  # noqa: E402
from geotrax_amd.detector import resolve_end2end  # noqa: E402

SCALES = ["n", "s", "m", "l", "x"]


@pytest.fixture(scope="module")
def small():
    return W.synthetic_yolo26(seed=0, nc=4, scale="n")


@pytest.mark.parametrize("scale", SCALES)
def test_topology_is_read_off_the_names(scale):
    t = W.synthetic_yolo26(seed=0, nc=4, scale=scale)
    assert W.is_yolo26(t) and not W.is_yolov10(t)
    assert W.detector_topology(t) == ("yolo26", "model.23")
    assert W.check_yolo26(t) == scale
    fused = {k: v for k, v in t.items() if not k.startswith(("model.23.cv2.", "model.23.cv3."))}   # what ultralytics' fuse() leaves
    assert W.is_yolo26(fused) and W.detector_topology(fused) == ("yolo26", "model.23") and not W.yolov10_has_one2many(fused)


def test_other_families_are_unchanged():
    assert W.detector_topology(W.synthetic_yolov8(0, 4, "n")) == ("yolov8", "model.22")
    assert W.detector_topology(W.synthetic_yolo11(0, 4, "n")) == ("yolo11", "model.23")
    assert W.detector_topology(W.synthetic_yolov10(0, 4, "n")) == ("yolov10", "model.23")
    assert not W.is_yolo26(W.synthetic_yolo11(0, 4, "s")) and not W.is_yolo26(W.synthetic_yolov10(0, 4, "s"))


@pytest.mark.parametrize("scale,c3,c4,c5,reps,c3k", [("n", 64, 128, 256, 1, False), ("s", 128, 256, 512, 1, False), ("m", 256, 512, 512, 1, True),
                                                      ("l", 256, 512, 512, 2, True), ("x", 384, 768, 768, 2, True)])
def test_layer_specs_follow_the_table(scale, c3, c4, c5, reps, c3k):
    sp = {n: (s, a) for n, s, a in W.yolo26_layer_specs(scale, 4)}
    assert sp["model.0.conv"][0] == (c3 // 4, 3, 3, 3)
    assert sp["model.8.cv2.conv"][0][0] == c5
    # SPPF: the tensors are yolo11.yaml's (the linear cv1 and the residual show in no shape); the spec marks cv1 as activation-free for the seeded draws
    assert sp["model.9.cv1.conv"] == ((c5 // 2, c5, 1, 1), False) and sp["model.9.cv2.conv"] == ((c5, 2 * c5, 1, 1), True)
    c = c5 // 2
    assert sp["model.10.m.0.attn.qkv.conv"] == ((2 * c, c, 1, 1), False)
    assert ("model.2.m.0.cv3.conv" in sp) == c3k and ("model.13.m.0.cv3.conv" in sp) == c3k and "model.6.m.0.cv3.conv" in sp
    assert ("model.2.m.1.cv1.conv" in sp) == (reps == 2)       # the backbone's repeats follow the depth multiple ...
    reps = 1                                                    # ... model.22's do not: the yaml writes one repeat
    for k in range(reps):                                       # model.22: Sequential(Bottleneck(c, c, e 0.5), PSABlock(c)) per repeat
        m = f"model.22.m.{k}"
        assert sp[m + ".0.cv1.conv"] == ((c // 2, c, 3, 3), True) and sp[m + ".0.cv2.conv"] == ((c, c // 2, 3, 3), True)
        assert sp[m + ".1.attn.qkv.conv"] == ((2 * c, c, 1, 1), False) and sp[m + ".1.attn.proj.conv"] == ((c, c, 1, 1), False)
        assert sp[m + ".1.attn.pe.conv"] == ((c, 1, 3, 3), False)
        assert sp[m + ".1.ffn.0.conv"] == ((2 * c, c, 1, 1), True) and sp[m + ".1.ffn.1.conv"] == ((c, 2 * c, 1, 1), False)
    assert f"model.22.m.{reps}.0.cv1.conv" not in sp and "model.22.m.0.cv1.conv" not in sp and "model.22.m.0.cv3.conv" not in sp
    assert sp["model.22.cv1.conv"][0] == (2 * c, c4 + c5, 1, 1) and sp["model.22.cv2.conv"][0] == (c5, (2 + reps) * c, 1, 1)
    assert c // 64 in (2, 4, 6)                                 # the attention's head count at model.10 and model.22
    cb = max(16, c3 // 4, W.YOLO26_BOX_FLOOR)
    for pair in (("cv2", "cv3"), ("one2one_cv2", "one2one_cv3")):
        for l, cin in enumerate((c3, c4, c5)):
            assert sp[f"model.23.{pair[0]}.{l}.0.conv"] == ((cb, cin, 3, 3), True) and sp[f"model.23.{pair[0]}.{l}.1.conv"] == ((cb, cb, 3, 3), True)
            assert sp[f"model.23.{pair[0]}.{l}.2"] == ((4, cb, 1, 1), False)                    # reg_max = 1
            assert sp[f"model.23.{pair[1]}.{l}.0.0.conv"] == ((cin, 1, 3, 3), True)
            assert sp[f"model.23.{pair[1]}.{l}.2"] == ((4, max(c3, 4), 1, 1), False)
    t = W.synthetic_yolo26(0, 4, scale)
    assert set(k[: -len(".weight")] for k in t if k.endswith(".weight")) == set(sp)
    assert not np.array_equal(t["model.23.cv2.0.2.weight"], t["model.23.one2one_cv2.0.2.weight"])       # the two heads are drawn apart
    assert W.YOLO26_YAML[9][3] == (1024, 5, 3, True) and W.YOLO26_YAML[22][3] == (1024, True, 0.5, True)


def test_refusals(small):
    t = small
    reg16 = dict(t)
    for k in t:
        if k.endswith("cv2.0.2.weight") or k.endswith("cv2.1.2.weight") or k.endswith("cv2.2.2.weight"):
            reg16[k] = np.zeros((64,) + t[k].shape[1:], np.float32)
    with pytest.raises(NotImplementedError, match="reg_max = 16"):
        W.detector_topology(reg16)
    no_attn = {k: v for k, v in t.items() if not k.startswith("model.22.m.0.1.")}
    cv4 = dict(t)
    cv4["model.23.cv4.0.0.conv.weight"] = t["model.23.cv2.0.0.conv.weight"]
    at24 = {k.replace("model.23.", "model.24."): v for k, v in t.items()}
    moved = dict(t)
    moved["model.8.m.0.1.attn.qkv.conv.weight"] = t["model.22.m.0.1.attn.qkv.conv.weight"]
    past = dict(t)
    past["model.24.conv.weight"] = t["model.0.conv.weight"]
    half = {k: v for k, v in t.items() if not k.startswith("model.23.cv3.1.")}           # the one-to-many pair only partly there
    for name, bad in (("no_attn", no_attn), ("cv4", cv4), ("moved", moved), ("past", past), ("half", half)):
        with pytest.raises(NotImplementedError, match="yolo26.yaml"):
            W.detector_topology(bad)
    with pytest.raises(NotImplementedError, match="yolo26.yaml"):                         # Detect at model.24: model.22's attention still marks the family
        W.detector_topology(at24)
    with pytest.raises(NotImplementedError, match="yolo26.yaml"):
        W.check_yolo26(at24)


def test_yolo11_with_one2one_still_gives_the_yolo11_message():
    t = W.synthetic_yolo11(0, 4, "n")
    t["model.23.one2one_cv2.0.0.conv.weight"] = t["model.23.cv2.0.0.conv.weight"]
    assert not W.is_yolo26(t)
    with pytest.raises(NotImplementedError, match="yolo11.yaml"):
        W.detector_topology(t)
    for fn in (W.check_yolo11, W.check_yolov10):                 # neither message calls YOLO26 unsupported any more
        with pytest.raises(NotImplementedError) as e:
            fn(t)
        assert "YOLO26" not in str(e.value) and "yolo26" not in str(e.value)
    assert "YOLO26" not in (W.check_yolo11.__doc__ or "") and "yolo26" in W.detector_topology.__doc__


@pytest.mark.parametrize("seed,A,nc", [(0, 336, 4), (1, 5000, 4), (2, 2100, 80), (3, 200, 3)])
def test_two_stage_cut_equals_the_global_top300(seed, A, nc):
    from yolo26_ref import MAX_DET, global_topk, two_stage_topk

    assert MAX_DET == W.V10_MAX_DET == 300
    rng = np.random.default_rng(seed)
    scores = ((rng.permutation(A * nc) + 0.5) / (A * nc)).astype(np.float32).reshape(A, nc)
    assert len(np.unique(scores)) == scores.size              # no ties
    for a, b in zip(two_stage_topk(scores), global_topk(scores)):
        np.testing.assert_array_equal(a, b)


def test_box_decode_on_a_hand_worked_map():
    """A 2 x 2 map at stride 8 with negative distances: xyxy = (ax - l, ay - t, ax + r, ay + b) * 8, anchors at 0.5 / 1.5"""
    from yolo26_ref import decode_ltrb

    dist = torch.tensor([[[1.0, -0.25, 0.5, 2.0],            # l per anchor (row-major: (0,0) (1,0) (0,1) (1,1))
                          [0.5, 0.5, -1.0, 0.0],             # t
                          [1.0, 0.75, -0.25, 3.0],           # r
                          [0.25, -0.5, 2.0, -0.5]]])         # b
    want = np.array([[(0.5 - 1.0) * 8, (0.5 - 0.5) * 8, (0.5 + 1.0) * 8, (0.5 + 0.25) * 8],
                     [(1.5 + 0.25) * 8, (0.5 - 0.5) * 8, (1.5 + 0.75) * 8, (0.5 - 0.5) * 8],
                     [(0.5 - 0.5) * 8, (1.5 + 1.0) * 8, (0.5 - 0.25) * 8, (1.5 + 2.0) * 8],
                     [(1.5 - 2.0) * 8, (1.5 - 0.0) * 8, (1.5 + 3.0) * 8, (1.5 - 0.5) * 8]], np.float32)
    got = decode_ltrb(dist, 2, 2, 8.0)[0].numpy().T
    np.testing.assert_array_equal(got, want)                  # every value is exact in fp32
    assert got[1, 0] > 8 * 1.5 and got[2, 1] > got[2, 3] - 100 and got[3, 3] < got[3, 1]   # sides beyond the centre; an inverted box stays as it is


def test_restatement_blocks(small):
    """The SPPF with a residual and model.22's block, held against plain torch written out longhand on a tiny input."""
    import torch.nn.functional as F
    from yolo26_ref import Yolo26Ref

    ref = Yolo26Ref(small)
    x = torch.from_numpy(np.random.default_rng(0).normal(0, 1, (1, 3, 64, 64)).astype(np.float32))
    ref.forward(x)
    t = ref.t
    x8 = ref.acts["model.8"]
    y = F.conv2d(x8, t["model.9.cv1.conv.weight"], t["model.9.cv1.conv.bias"])                         # no activation
    torch.testing.assert_close(ref.acts["model.9.cv1.conv"], y)
    p1 = F.max_pool2d(y, 5, 1, 2); p2 = F.max_pool2d(p1, 5, 1, 2); p3 = F.max_pool2d(p2, 5, 1, 2)
    want = F.silu(F.conv2d(torch.cat([y, p1, p2, p3], 1), t["model.9.cv2.conv.weight"], t["model.9.cv2.conv.bias"])) + x8
    torch.testing.assert_close(ref.acts["model.9"], want)
    b0 = ref.acts["model.22.m.0.0.cv2.conv"]                                                                    # the Bottleneck's output, its shortcut on
    c = b0.shape[1]
    assert c == 128 and ref.acts["model.22.m.0.1.attn.qkv.conv"].shape[1] == 2 * c
    out = ref.acts["model.22.m.0.1.ffn.1.conv"]
    assert out.shape == b0.shape and float((out - b0).abs().max()) > 0
    raw = ref.forward(x)[0]
    assert raw.shape == (64 + 16 + 4, 8) and bool(((raw[:, 4:] >= 0) & (raw[:, 4:] <= 1)).all())
    many = ref.forward(x, one2one=False)[0]
    assert float((many - raw).abs().max()) > 0


def test_end2end_config_surface(small):
    v11 = W.synthetic_yolo11(0, 4, "n")
    assert resolve_end2end("yolo26", small, None) is True and resolve_end2end("yolo26", small, True) is True
    assert resolve_end2end("yolo26", small, False) is False
    with pytest.raises(ValueError, match="end2end"):
        resolve_end2end("yolo11", v11, True)
    fused = {k: v for k, v in small.items() if not k.startswith(("model.23.cv2.", "model.23.cv3."))}
    assert resolve_end2end("yolo26", fused, None) is True
    with pytest.raises(ValueError, match="YOLO26.*cv2 / cv3"):
        resolve_end2end("yolo26", fused, False)
    from geotrax_amd.model import YOLO

    assert YOLO(small).yaml_file == "yolo26n.yaml" and YOLO(W.synthetic_yolo26(0, 4, "s")).yaml_file == "yolo26s.yaml"
    assert YOLO(small).names == {0: "0", 1: "1", 2: "2", 3: "3"}


def _bn(rng, c):
    return dict(weight=rng.uniform(0.5, 1.5, c), bias=rng.normal(0, 0.1, c), running_mean=rng.normal(0, 0.1, c), running_var=rng.uniform(0.5, 2.0, c))


def test_converter_folds_an_unfused_file(small, tmp_path):
    """Conv + BN pairs under the new names (model.22.m.0.0.cv1, model.22.m.0.1.attn.qkv, ...) fold to the tensors a direct fold_bn
    gives; the Conv2d layers pass through; both head pairs survive; detector.meta names the family."""
    from convert_weights import convert_state_dict

    rng = np.random.default_rng(5)
    sd = {}
    for k, v in small.items():
        if k.endswith(".conv.weight"):
            p = k[: -len(".conv.weight")]
            sd[k] = v
            sd.update({f"{p}.bn.{n}": x.astype(np.float32) for n, x in _bn(rng, v.shape[0]).items()})
            sd[f"{p}.bn.num_batches_tracked"] = np.zeros((), np.float32)
        elif k.endswith(".conv.bias"):
            continue
        else:
            sd[k] = v
    sd["model.23.dfl.conv.weight"] = np.ones((1, 1, 1, 1), np.float32)
    out = convert_state_dict(sd)
    want = W.fold_bn({k: v for k, v in sd.items() if "dfl" not in k and "num_batches_tracked" not in k})
    assert set(out) == set(want) | {"detector.meta"} and not any(".bn." in k or "dfl" in k for k in out)
    assert set(out) - {"detector.meta"} == set(small)
    for k in want:
        np.testing.assert_array_equal(out[k], want[k])
    for k in ("model.22.m.0.0.cv1.conv", "model.22.m.0.1.attn.qkv.conv", "model.22.m.0.1.attn.pe.conv", "model.9.cv1.conv"):
        g, b, m, v = (sd[f"{k[:-5]}.bn.{n}"].astype(np.float64) for n in ("weight", "bias", "running_mean", "running_var"))
        s = g / np.sqrt(v + W.BN_EPS)
        np.testing.assert_allclose(out[k + ".weight"], small[k + ".weight"] * s[:, None, None, None], rtol=1e-6)
        np.testing.assert_allclose(out[k + ".bias"], b - m * s, rtol=1e-5, atol=1e-7)
    np.testing.assert_array_equal(out["model.23.one2one_cv2.1.2.weight"], small["model.23.one2one_cv2.1.2.weight"])
    np.testing.assert_array_equal(out["detector.meta"], np.asarray([26, 1, 1, 300], np.float32))
    W.save_weights(out, tmp_path / "y26n.safetensors")
    back = W.load_weights(tmp_path / "y26n.safetensors")
    assert W.detector_topology(back) == ("yolo26", "model.23")
    assert W.detector_meta(back) == dict(family="yolo26", one2many=True, end2end=True, max_det=300)
