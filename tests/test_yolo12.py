"""YOLO12 on the host side, no GPU: the graph is recognised from the tensor names with its scale, other arrangements are refused
with YOLO12's own message while every other family keeps its route, the CPU restatement (tests/yolo12_ref.py) has yolo12.yaml's layer
shapes at all five scales, its area attention keeps the bands apart to the bit and equals plain attention at area 1, and the l-scale
residual is x + gamma * y."""
import numpy as np
import pytest
import torch

SCALES = ["n", "s", "m", "l", "x"]
WIDTH = {"n": 0.25, "s": 0.5, "m": 1.0, "l": 1.0, "x": 1.5}


@pytest.mark.parametrize("scale", SCALES)
def test_topology_and_scale_are_read_off_the_tensors(scale):
    from geotrax_amd.weights import check_yolo12, detector_topology, is_yolo12, synthetic_yolo12

    t = synthetic_yolo12(seed=0, nc=4, scale=scale)
    assert is_yolo12(t) and detector_topology(t) == ("yolo12", "model.21") and check_yolo12(t) == scale
    assert ("model.6.gamma" in t) == (scale in "lx") == ("model.8.gamma" in t)


def test_a_changed_shape_is_refused_by_name():
    from geotrax_amd.weights import detector_topology, synthetic_yolo12

    t = synthetic_yolo12(seed=0, nc=4, scale="n")
    cases = {
        "a wider mlp": {**t, "model.6.m.0.1.mlp.0.conv.weight": np.zeros((160, 64, 1, 1), np.float32)},
        "a 3x3 pe": {**t, "model.8.m.1.0.attn.pe.conv.weight": np.zeros((128, 1, 3, 3), np.float32)},
        "a third member": {**t, "model.6.m.2.0.attn.qkv.conv.weight": t["model.6.m.0.0.attn.qkv.conv.weight"]},
        "a gamma at scale n": {**t, "model.6.gamma": np.ones(128, np.float32)},
        "Detect at model.22": {k.replace("model.21.", "model.22."): v for k, v in t.items()},
        "attention in the neck": {**t, "model.11.m.0.0.attn.qkv.conv.weight": t["model.6.m.0.0.attn.qkv.conv.weight"]},
        "a mask / pose branch": {**t, "model.21.cv4.0.0.conv.weight": t["model.21.cv2.0.0.conv.weight"]},
    }
    for what, bad in cases.items():
        with pytest.raises(NotImplementedError, match="yolo12"):
            detector_topology(bad)
            pytest.fail(what)
    l = synthetic_yolo12(seed=0, nc=4, scale="l")
    with pytest.raises(NotImplementedError, match="yolo12"):      # scale l without its gamma
        detector_topology({k: v for k, v in l.items() if k != "model.8.gamma"})


def test_the_other_families_keep_their_route():
    from geotrax_amd.weights import (check_yolo11, detector_topology, is_yolo12, is_yolo26, synthetic_yolo11, synthetic_yolo12, synthetic_yolo26,
                                     synthetic_yolov8, synthetic_yolov10)

    t11, t26 = synthetic_yolo11(seed=0, nc=4, scale="n"), synthetic_yolo26(seed=0, nc=4, scale="n")
    assert not is_yolo12(t11) and detector_topology(t11) == ("yolo11", "model.23")
    assert not is_yolo12(t26) and detector_topology(t26) == ("yolo26", "model.23")
    assert detector_topology(synthetic_yolov10(seed=0, nc=4, scale="n")) == ("yolov10", "model.23")
    assert detector_topology(synthetic_yolov8(seed=0, nc=4, scale="n")) == ("yolov8", "model.22")
    t12 = synthetic_yolo12(seed=0, nc=4, scale="n")
    assert not is_yolo26(t12)                                       # a YOLO12 dict is not mistaken for YOLO26 ...
    with pytest.raises(NotImplementedError, match="yolo11"):       # ... and YOLO11's own check refuses it
        check_yolo11(t12)
    # a YOLO11 file with attention at model.6 in C2PSA's naming stays YOLO11's to refuse (tests/test_yolo11.py pins the message)
    stray = {**t11, "model.6.m.0.attn.qkv.conv.weight": t11["model.10.m.0.attn.qkv.conv.weight"]}
    assert not is_yolo12(stray)
    with pytest.raises(NotImplementedError, match="yolo11"):
        detector_topology(stray)


def test_wrapper_reports_the_yaml():
    from geotrax_amd.model import YOLO
    from geotrax_amd.weights import synthetic_yolo12

    assert YOLO(synthetic_yolo12(seed=0, nc=4, scale="l")).yaml_file == "yolo12l.yaml"


@pytest.mark.parametrize("scale", SCALES)
def test_restatement_layer_shapes_at_64(scale):
    from geotrax_amd.weights import synthetic_yolo12
    from yolo12_ref import Yolo12Ref

    maxc = 1024 if scale in "ns" else 512
    ch = lambda c: int(np.ceil(min(c, maxc) * WIDTH[scale] / 8) * 8)
    ref = Yolo12Ref(synthetic_yolo12(seed=0, nc=4, scale=scale, gain=1.0))
    out = ref.forward(torch.rand(1, 3, 64, 64, generator=torch.Generator().manual_seed(0)))
    assert out.shape == (1, 8 * 8 + 4 * 4 + 2 * 2, 8) and bool(torch.isfinite(out).all())
    want = {"model.0.conv": (ch(64), 32), "model.1.conv": (ch(128), 16), "model.2": (ch(256), 16), "model.3.conv": (ch(256), 8), "model.4": (ch(512), 8),
            "model.5.conv": (ch(512), 4), "model.6": (ch(512), 4), "model.7.conv": (ch(1024), 2), "model.8": (ch(1024), 2), "model.11": (ch(512), 4),
            "model.14": (ch(256), 8), "model.15.conv": (ch(256), 4), "model.17": (ch(512), 4), "model.18.conv": (ch(512), 2), "model.20": (ch(1024), 2)}
    for name, (c, hw) in want.items():
        assert tuple(ref.acts[name].shape) == (1, c, hw, hw), name
    c6, reps = ch(512) // 2, 2 if scale in "nsm" else 4
    for k in range(reps):
        for j in range(2):
            assert tuple(ref.acts[f"model.6.m.{k}.{j}.attn.out"].shape) == (1, c6, 4, 4)
    assert f"model.6.m.{reps}.0.attn.out" not in ref.acts
    assert ref.t["model.6.m.0.0.mlp.0.conv.weight"].shape[0] == int(c6 * (1.2 if scale in "lx" else 2.0))
    assert ref.t["model.6.m.0.0.attn.pe.conv.weight"].shape == (c6, 1, 7, 7) and ref.t["model.6.m.0.0.attn.qkv.conv.weight"].shape[0] == 3 * c6


def _qkv(b, heads, h, w, seed=0):
    return torch.randn(b, 96 * heads, h, w, generator=torch.Generator().manual_seed(seed))


def test_a_band_gives_another_band_exactly_zero_weight():
    """area 4 on an 8 x 6 map: 12 positions per band = two map rows. k and v of every band but the second are perturbed (q as well):
    the second band's output is unchanged to the bit, every other band's moves."""
    from yolo12_ref import area_attention

    heads, H, W = 2, 8, 6
    a = _qkv(2, heads, H, W)
    b = a.clone()
    band = torch.zeros(H * W, dtype=torch.bool)
    band[12:24] = True
    other = ~band.view(1, 1, H, W).expand_as(b)
    b[other] = b[other] * 3 + 1
    ya, yb = area_attention(a, heads, 4).flatten(2), area_attention(b, heads, 4).flatten(2)
    assert torch.equal(ya[..., band], yb[..., band])
    for lo in (0, 24, 36):
        assert not torch.equal(ya[..., lo:lo + 12], yb[..., lo:lo + 12])
    # ... while at area 1 the same perturbation reaches the band
    assert not torch.equal(area_attention(a, heads, 1).flatten(2)[..., band], area_attention(b, heads, 1).flatten(2)[..., band])


def test_area_1_is_plain_attention_over_the_whole_map():
    """Per head and per query, written out longhand on a 5 x 7 map (an odd number of positions)."""
    from yolo12_ref import area_attention

    heads, H, W = 2, 5, 7
    x = _qkv(1, heads, H, W, seed=1).double()
    got = area_attention(x, heads, 1)
    t = x[0].flatten(1)                                              # [96 heads, N]
    for hd in range(heads):
        q, k, v = t[96 * hd:96 * hd + 32], t[96 * hd + 32:96 * hd + 64], t[96 * hd + 64:96 * hd + 96]
        for n in range(H * W):
            s = (q[:, n:n + 1] * k).sum(0) / np.sqrt(32.0)
            p = torch.exp(s - s.max())
            want = (v * (p / p.sum())).sum(1)
            assert torch.allclose(got[0, 32 * hd:32 * hd + 32, n // W, n % W], want, rtol=0, atol=1e-12)


def test_area_4_is_plain_attention_inside_each_band():
    from yolo12_ref import area_attention

    heads, H, W = 4, 4, 4
    x = _qkv(2, heads, H, W, seed=2).double()
    got = area_attention(x, heads, 4)
    for r in range(4):                                               # a band of a 4 x 4 map is one map row
        assert torch.allclose(got[:, :, r:r + 1], area_attention(x[:, :, r:r + 1], heads, 1), rtol=0, atol=1e-12)


def test_the_residual_of_scale_l_is_x_plus_gamma_y():
    from geotrax_amd.weights import synthetic_yolo12
    from yolo12_ref import Yolo12Ref

    t = synthetic_yolo12(seed=2, nc=4, scale="l", gain=1.0)
    x = torch.randn(1, 512, 4, 4, generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        got = Yolo12Ref(t)._a2c2f("model.6", x)
        y = Yolo12Ref({k: v for k, v in t.items() if k != "model.6.gamma"})._a2c2f("model.6", x)
    g = torch.from_numpy(t["model.6.gamma"]).view(1, -1, 1, 1)
    assert float(g.abs().min()) > 0.05 and not torch.equal(got, y)
    assert torch.equal(got, x + g * y)


def test_bn_folding_covers_the_new_blocks():
    """fold_bn on an unfused A2C2f member: qkv / proj / pe / mlp convs each carry a BatchNorm; gamma passes through."""
    from geotrax_amd.weights import BN_EPS, fold_bn

    rng = np.random.default_rng(0)
    raw = {"model.6.gamma": rng.standard_normal(8).astype(np.float32)}
    for name, shape in (("model.6.m.0.0.attn.qkv.conv", (24, 8, 1, 1)), ("model.6.m.0.0.attn.pe.conv", (8, 1, 7, 7)), ("model.6.m.0.0.mlp.1.conv", (8, 9, 1, 1))):
        base = name[: -len(".conv")]
        raw[name + ".weight"] = rng.standard_normal(shape).astype(np.float32)
        for k in ("weight", "bias", "running_mean"):
            raw[f"{base}.bn.{k}"] = rng.standard_normal(shape[0]).astype(np.float32)
        raw[f"{base}.bn.running_var"] = rng.random(shape[0]).astype(np.float32) + 0.5
    out = fold_bn(raw)
    assert np.array_equal(out["model.6.gamma"], raw["model.6.gamma"])
    for name in ("model.6.m.0.0.attn.qkv.conv", "model.6.m.0.0.attn.pe.conv", "model.6.m.0.0.mlp.1.conv"):
        base = name[: -len(".conv")]
        s = raw[f"{base}.bn.weight"] / np.sqrt(raw[f"{base}.bn.running_var"] + BN_EPS)
        np.testing.assert_allclose(out[name + ".weight"], raw[name + ".weight"] * s[:, None, None, None], rtol=1e-6)
        np.testing.assert_allclose(out[name + ".bias"], raw[f"{base}.bn.bias"] - raw[f"{base}.bn.running_mean"] * s, rtol=1e-5, atol=1e-6)
        assert not any(k.startswith(base + ".bn.") for k in out)
