"""YOLO11-cls checkpoints as the trackers' separate ReID network, host side: the weight table and its scales, the strict topology
check next to is_yolov8_cls, the tracker config, and the CPU restatement (tests/yolo11_cls_ref.py) against a longhand C2PSA.
No GPU needed."""
import numpy as np
import pytest

# yolo11-cls.yaml at each scale: model.0 width, model.9 width (= the embedding dim), repeats of every C3k2 / C2PSA, c3k at model.2 / 4
SHAPES = {"n": (16, 256, 1, False), "s": (32, 512, 1, False), "m": (64, 512, 1, True), "l": (64, 512, 2, True), "x": (96, 768, 2, True)}
# parameters ultralytics publishes for yolo11{n,s,m,l,x}-cls, in millions
PUBLISHED_M = {"n": 1.6, "s": 5.5, "m": 10.4, "l": 12.9, "x": 28.4}


@pytest.mark.parametrize("scale", list(SHAPES))
def test_synthetic_yolo11_cls_has_the_yaml_shapes(scale):
    from geotrax_amd.weights import (YOLO11_CLS_YAML, YOLO11_YAML, cls_family, is_yolo11_cls, is_yolov8_cls, synthetic_yolo11_cls,
                                     yolo11_cls_layer_specs)

    assert YOLO11_CLS_YAML[:9] == YOLO11_YAML[:9] and [r[2] for r in YOLO11_CLS_YAML[9:]] == ["C2PSA", "Classify"]
    c0, dim, reps, c3k_early = SHAPES[scale]
    specs = {n: s for n, s, _ in yolo11_cls_layer_specs(scale, nc=10)}
    t = synthetic_yolo11_cls(seed=1, scale=scale, nc=10)
    assert {k[:-7] for k in t if k.endswith(".weight")} == set(specs) and all(t[n + ".weight"].shape == s for n, s in specs.items())
    assert specs["model.0.conv"] == (c0, 3, 3, 3)
    assert specs["model.9.cv2.conv"] == (dim, dim, 1, 1) and specs["model.8.cv2.conv"][0] == dim
    c = dim // 2
    heads = c // 64
    assert specs["model.9.m.0.attn.qkv.conv"] == (heads * 128, c, 1, 1) and specs["model.9.m.0.attn.pe.conv"] == (c, 1, 3, 3)
    assert specs["model.10.linear"] == (10, 1280) and specs["model.10.conv.conv"] == (1280, dim, 1, 1)
    for i in (2, 4, 6, 8):
        assert f"model.{i}.m.{reps - 1}.cv1.conv" in specs and f"model.{i}.m.{reps}.cv1.conv" not in specs
        assert (f"model.{i}.m.0.cv3.conv" in specs) == (c3k_early or i >= 6)
    assert f"model.9.m.{reps - 1}.ffn.1.conv" in specs and f"model.9.m.{reps}.ffn.1.conv" not in specs
    assert not any(k.startswith("model.9.cv1.conv") and specs[k][1] != dim for k in specs)       # no SPPF in front of C2PSA
    assert is_yolo11_cls(t) and cls_family(t) == "yolo11-cls"
    with pytest.raises(NotImplementedError, match="YOLOv8-cls"):
        is_yolov8_cls(t)
    t2 = synthetic_yolo11_cls(seed=1, scale=scale, nc=10)
    assert all(np.array_equal(t[k], t2[k]) for k in t)                           # seeded
    # the fused parameter count at the yaml's default nc = 80 against the published one (fused: a bias per conv where the
    # unfused model has a BatchNorm weight and bias, 0.3 % more at most)
    n_par = sum(int(np.prod(s)) + s[0] for s in (s for _, s, _ in yolo11_cls_layer_specs(scale, nc=80)))
    assert abs(n_par / 1e6 - PUBLISHED_M[scale]) <= 0.06, n_par


def test_is_yolo11_cls_tells_the_families_apart():
    from geotrax_amd.weights import (cls_family, is_yolo11_cls, synthetic_rtdetr, synthetic_yolo11, synthetic_yolo11_cls, synthetic_yolov8,
                                     synthetic_yolov8_cls)

    v8cls = synthetic_yolov8_cls(seed=0, scale="n")
    assert not is_yolo11_cls(synthetic_yolov8(seed=0, scale="n", nc=4)) and cls_family(synthetic_yolov8(seed=0, scale="n", nc=4)) is None
    assert not is_yolo11_cls(v8cls) and cls_family(v8cls) == "yolov8-cls"
    assert not is_yolo11_cls(synthetic_rtdetr(seed=0, nc=4, width=0.25, hd=64, ndl=1))
    assert not is_yolo11_cls(synthetic_yolo11(seed=0, scale="n", nc=4))          # a whole detect file is no classifier
    t = synthetic_yolo11_cls(seed=0, scale="s")
    t["model.6.cv2.conv.weight"] = np.zeros((264, 384, 1, 1), np.float32)        # one width changed
    with pytest.raises(NotImplementedError, match="yolo11-cls"):
        is_yolo11_cls(t)
    t = synthetic_yolo11_cls(seed=0, scale="n")
    del t["model.9.m.0.ffn.0.conv.weight"]                                       # incomplete
    with pytest.raises(NotImplementedError):
        is_yolo11_cls(t)
    t = synthetic_yolo11_cls(seed=0, scale="n")
    t["model.4.extra.conv.weight"] = np.zeros((8, 8, 1, 1), np.float32)          # a layer the yaml does not have
    with pytest.raises(NotImplementedError):
        is_yolo11_cls(t)
    det = synthetic_yolo11(seed=0, scale="n", nc=4)                              # a detect file cut to rows 0-10: SPPF at 9, C2PSA at 10
    cut = {k: v for k, v in det.items() if int(k.split(".")[1]) <= 10}
    with pytest.raises(NotImplementedError):
        is_yolo11_cls(cut)
    with pytest.raises(NotImplementedError):
        cls_family(cut)


@pytest.mark.parametrize("ttype", ["botsort", "deepocsort", "tracktrack"])
def test_make_tracker_takes_a_yolo11_cls_checkpoint(tmp_path, monkeypatch, ttype):
    from geotrax_amd.model import YOLO
    from geotrax_amd.weights import save_weights, synthetic_yolo11_cls

    save_weights(synthetic_yolo11_cls(seed=0, scale="n"), tmp_path / "yolo11n-cls.safetensors")
    monkeypatch.chdir(tmp_path)
    trk = YOLO.__new__(YOLO)._make_tracker({"tracker_type": ttype, "with_reid": True, "model": "yolo11n-cls.safetensors"})
    assert trk.with_reid and trk.reid_tensors["model.9.cv2.conv.weight"].shape[0] == 256


def test_make_tracker_still_refuses_a_detect_file(tmp_path):
    from geotrax_amd.model import YOLO
    from geotrax_amd.weights import save_weights, synthetic_yolo11

    save_weights(synthetic_yolo11(seed=0, scale="n", nc=4), tmp_path / "det.safetensors")
    with pytest.raises(NotImplementedError, match="YOLOv8-cls"):
        YOLO.__new__(YOLO)._make_tracker({"tracker_type": "botsort", "with_reid": True, "model": str(tmp_path / "det.safetensors")})


def test_encoder_refusal_names_both_families():
    from geotrax_amd.reid import ReIDEncoder
    from geotrax_amd.weights import synthetic_yolov8

    with pytest.raises(NotImplementedError, match="YOLO11-cls.*YOLOv8-cls"):     # refused before any GPU call
        ReIDEncoder(synthetic_yolov8(seed=0, scale="n", nc=4), ctx=object())


def test_restatement_agrees_with_longhand_c2psa_on_a_3x3_map():
    """Yolo11ClsRef's model.9 and vector at imgsz 96 (a 3 x 3 map, most of pe's window is padding) against C2PSA written out with
    torch.nn.functional only, and the float64 numpy attention the GPU tests use against both."""
    import torch
    import torch.nn.functional as F
    from geotrax_amd.weights import synthetic_yolo11_cls
    from yolo11_cls_ref import Yolo11ClsRef, attention_f64

    t = synthetic_yolo11_cls(seed=3, scale="n", nc=10, gain=1.5)
    crops = np.random.default_rng(0).integers(0, 256, (2, 96, 96, 3)).astype(np.uint8)
    ref = Yolo11ClsRef(t, double=True)
    emb = ref.forward(crops)
    x8 = ref.acts["model.8"]
    assert x8.shape[2:] == (3, 3)
    w = lambda n: torch.from_numpy(t[n + ".weight"]).double()
    b = lambda n: torch.from_numpy(t[n + ".bias"]).double()
    cv = lambda n, x, act=True, **kw: (F.silu if act else (lambda v: v))(F.conv2d(x, w(n), b(n), **kw))
    y = cv("model.9.cv1.conv", x8)
    c = y.shape[1] // 2
    a_, b_ = y[:, :c], y[:, c:]
    heads = c // 64
    m = "model.9.m.0"
    qkv = cv(m + ".attn.qkv.conv", b_, act=False)
    B, _, H, W = qkv.shape
    outs = []
    for h in range(heads):
        blk = qkv[:, h * 128:(h + 1) * 128].reshape(B, 128, H * W)
        q, k, v = blk[:, :32], blk[:, 32:64], blk[:, 64:]
        att = torch.softmax(q.transpose(1, 2) @ k / 32 ** 0.5, dim=-1)
        outs.append((v @ att.transpose(1, 2)).reshape(B, 64, H, W))
    vmap = torch.cat([qkv[:, h * 128 + 64:(h + 1) * 128] for h in range(heads)], 1)
    att_out = torch.cat(outs, 1) + F.conv2d(vmap, w(m + ".attn.pe.conv"), b(m + ".attn.pe.conv"), padding=1, groups=c)
    b_ = b_ + cv(m + ".attn.proj.conv", att_out, act=False)
    b_ = b_ + cv(m + ".ffn.1.conv", cv(m + ".ffn.0.conv", b_), act=False)
    assert m.replace("m.0", "m.1") + ".attn.qkv.conv.weight" not in t
    out = cv("model.9.cv2.conv", torch.cat([a_, b_], 1))
    np.testing.assert_allclose(ref.acts["model.9"].numpy(), out.numpy(), rtol=0, atol=1e-12 * float(out.abs().max()))
    np.testing.assert_allclose(emb, out.mean((2, 3)).numpy(), rtol=0, atol=1e-12 * float(out.abs().max()))
    mine = attention_f64(qkv.permute(0, 2, 3, 1).numpy(), t[m + ".attn.pe.conv.weight"], t[m + ".attn.pe.conv.bias"], heads)
    np.testing.assert_allclose(mine, att_out.permute(0, 2, 3, 1).numpy(), rtol=0, atol=1e-12 * float(att_out.abs().max()))
    np.testing.assert_allclose(ref.acts[m + ".attn.out"].permute(0, 2, 3, 1).numpy(), mine, rtol=0, atol=1e-12 * float(att_out.abs().max()))
