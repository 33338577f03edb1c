"""YOLO11 on the host side, no GPU: the graph is recognised from the tensor names, the layer specs follow yolo11.yaml's table, the
CPU restatement (tests/yolo11_ref.py) agrees with its two new blocks written out longhand, BN folding handles the depthwise and
the activation-free convs, and the ultralytics-shaped wrapper reports the right yaml."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

SCALES = ["n", "s", "m", "l", "x"]


@pytest.mark.parametrize("scale", SCALES)
def test_topology_is_read_off_the_names(scale):
    from geotrax_amd.weights import detector_topology, synthetic_yolo11

    assert detector_topology(synthetic_yolo11(seed=0, nc=4, scale=scale)) == ("yolo11", "model.23")


def test_topology_of_the_other_families_is_unchanged():
    from geotrax_amd.weights import detector_topology, synthetic_rtdetr, synthetic_yolov8, synthetic_yolov8_p2, synthetic_yolov8_rtdetr

    assert detector_topology(synthetic_yolov8(seed=0, nc=4, scale="n")) == ("yolov8", "model.22")
    assert detector_topology(synthetic_yolov8_p2(seed=0, nc=4, scale="n")) == ("yolov8-p2", "model.28")
    assert detector_topology(synthetic_rtdetr(seed=0, nc=4, width=0.25, hd=64, ndl=1)) == ("rtdetr-l", "model.28")
    assert detector_topology(synthetic_yolov8_rtdetr(seed=0, nc=4, scale="n", hd=64, ndl=1)) == ("yolov8-rtdetr", "model.22")


def test_other_arrangements_of_the_blocks_are_refused():
    from geotrax_amd.weights import detector_topology, synthetic_yolo11

    t = synthetic_yolo11(seed=0, nc=4, scale="n")
    cases = {
        "no C2PSA": {k: v for k, v in t.items() if not k.startswith("model.10.")},
        "Detect at model.24": {k.replace("model.23.", "model.24."): v for k, v in t.items()},
        "attention elsewhere (YOLO12)": {**t, "model.6.m.0.attn.qkv.conv.weight": t["model.10.m.0.attn.qkv.conv.weight"]},
        "a mask / pose branch": {**t, "model.23.cv4.0.0.conv.weight": t["model.23.cv2.0.0.conv.weight"]},
        "an end-to-end head (YOLO26)": {**t, "model.23.one2one_cv2.0.0.conv.weight": t["model.23.cv2.0.0.conv.weight"]},
        "yolo11-cls": {k: v for k, v in t.items() if int(k.split(".")[1]) <= 10},
    }
    for what, bad in cases.items():
        with pytest.raises(NotImplementedError, match="yolo11"):
            detector_topology(bad)
            pytest.fail(what)


@pytest.mark.parametrize("scale,width,heads,c3k_all,reps", [("n", 0.25, 2, False, 1), ("s", 0.5, 4, False, 1), ("m", 1.0, 4, True, 1),
                                                            ("l", 1.0, 4, True, 2), ("x", 1.5, 6, True, 2)])
def test_layer_specs_follow_the_yaml(scale, width, heads, c3k_all, reps):
    from geotrax_amd.weights import yolo11_layer_specs

    nc = 4
    specs = {n: (s, a) for n, s, a in yolo11_layer_specs(scale, nc)}
    maxc = 1024 if scale in "ns" else 512
    ch = lambda c: int(np.ceil(min(c, maxc) * width / 8) * 8)
    out = lambda n: specs[n][0][0]
    widths = {0: 64, 1: 128, 3: 256, 5: 512, 7: 1024, 17: 256, 20: 512}
    for i, c in widths.items():
        assert specs[f"model.{i}.conv"][0][0] == ch(c) and specs[f"model.{i}.conv"][0][2] == 3
    blocks = {2: (256, 0.25), 4: (512, 0.25), 6: (512, 0.5), 8: (1024, 0.5), 13: (512, 0.5), 16: (256, 0.5), 19: (512, 0.5), 22: (1024, 0.5)}
    for i, (c2, e) in blocks.items():
        c = int(ch(c2) * e)
        assert specs[f"model.{i}.cv1.conv"][0][0] == 2 * c
        assert specs[f"model.{i}.cv2.conv"][0][:2] == (ch(c2), (2 + reps) * c)
        assert f"model.{i}.m.{reps - 1}.cv1.conv" in specs and f"model.{i}.m.{reps}.cv1.conv" not in specs
        c3k = c3k_all or i in (6, 8, 22)
        assert (f"model.{i}.m.0.cv3.conv" in specs) == c3k
        if c3k:
            assert specs[f"model.{i}.m.0.cv1.conv"][0] == (c // 2, c, 1, 1) and specs[f"model.{i}.m.0.cv3.conv"][0] == (c, c, 1, 1)
            assert specs[f"model.{i}.m.0.m.1.cv2.conv"][0] == (c // 2, c // 2, 3, 3) and f"model.{i}.m.0.m.2.cv1.conv" not in specs
        else:
            assert specs[f"model.{i}.m.0.cv1.conv"][0] == (c // 2, c, 3, 3) and specs[f"model.{i}.m.0.cv2.conv"][0] == (c, c // 2, 3, 3)
    # Concat widths: 13 = [up(10), 6], 16 = [up(13), 4], 19 = [17, 13], 22 = [20, 10]
    assert specs["model.13.cv1.conv"][0][1] == ch(1024) + ch(512) and specs["model.16.cv1.conv"][0][1] == ch(512) + ch(512)
    assert specs["model.19.cv1.conv"][0][1] == ch(256) + ch(512) and specs["model.22.cv1.conv"][0][1] == ch(512) + ch(1024)
    c = ch(1024) // 2
    assert c // 64 == heads
    assert specs["model.10.cv1.conv"][0] == (2 * c, ch(1024), 1, 1) and specs["model.10.cv2.conv"][0] == (ch(1024), 2 * c, 1, 1)
    for k in range(reps):
        m = f"model.10.m.{k}"
        assert specs[m + ".attn.qkv.conv"] == ((c + 2 * heads * 32, c, 1, 1), False)
        assert specs[m + ".attn.proj.conv"] == ((c, c, 1, 1), False) and specs[m + ".attn.pe.conv"] == ((c, 1, 3, 3), False)
        assert specs[m + ".ffn.0.conv"] == ((2 * c, c, 1, 1), True) and specs[m + ".ffn.1.conv"] == ((c, 2 * c, 1, 1), False)
    assert f"model.10.m.{reps}.attn.qkv.conv" not in specs
    ch0 = ch(256)
    c2, c3 = max(16, ch0 // 4, 64), max(ch0, min(nc, 100))
    for l, cin in enumerate((ch(256), ch(512), ch(1024))):
        d = f"model.23.cv2.{l}"
        assert specs[d + ".0.conv"][0] == (c2, cin, 3, 3) and specs[d + ".1.conv"][0] == (c2, c2, 3, 3) and specs[d + ".2"] == ((64, c2, 1, 1), False)
        d = f"model.23.cv3.{l}"
        assert specs[d + ".0.0.conv"] == ((cin, 1, 3, 3), True) and specs[d + ".0.1.conv"] == ((c3, cin, 1, 1), True)
        assert specs[d + ".1.0.conv"] == ((c3, 1, 3, 3), True) and specs[d + ".1.1.conv"] == ((c3, c3, 1, 1), True)
        assert specs[d + ".2"] == ((nc, c3, 1, 1), False)
    assert not any(n.startswith(("model.11.", "model.12.", "model.14.", "model.15.", "model.18.", "model.21.", "model.24.")) for n in specs)


def _conv(t, name, x, act=True, groups=1):
    w = torch.from_numpy(t[name + ".weight"])
    y = F.conv2d(x, w, torch.from_numpy(t[name + ".bias"]), padding=w.shape[-1] // 2, groups=groups)
    return F.silu(y) if act else y


def test_ref_c2psa_against_longhand():
    """One C2PSA block of scale n (2 heads), written out per head and per query with plain tensor arithmetic."""
    from geotrax_amd.weights import synthetic_yolo11
    from yolo11_ref import Yolo11Ref

    t = synthetic_yolo11(seed=3, nc=4, scale="n")
    x = torch.randn(1, 256, 5, 7, generator=torch.Generator().manual_seed(0))
    with torch.no_grad():
        got = Yolo11Ref(t)._c2psa("model.10", x)
        a, b = _conv(t, "model.10.cv1.conv", x).split([128, 128], 1)
        qkv = _conv(t, "model.10.m.0.attn.qkv.conv", b, act=False)[0].reshape(256, 35).double()
        v_all = torch.cat([qkv[h * 128 + 64:(h + 1) * 128] for h in range(2)])               # [128, 35]: the heads' v rows, head-major
        att = torch.zeros(128, 35, dtype=torch.float64)
        for h in range(2):
            q, k, v = qkv[h * 128:h * 128 + 32], qkv[h * 128 + 32:h * 128 + 64], qkv[h * 128 + 64:h * 128 + 128]
            for i in range(35):                                                              # query position i
                s = torch.stack([(q[:, i] * k[:, j]).sum() for j in range(35)]) / np.sqrt(32.0)
                p = torch.exp(s - s.max())
                p = p / p.sum()
                att[h * 64:(h + 1) * 64, i] = (v * p[None, :]).sum(1)
        pe = _conv(t, "model.10.m.0.attn.pe.conv", v_all.float().reshape(1, 128, 5, 7), act=False, groups=128)
        y = att.float().reshape(1, 128, 5, 7) + pe
        b = b + _conv(t, "model.10.m.0.attn.proj.conv", y, act=False)
        b = b + _conv(t, "model.10.m.0.ffn.1.conv", _conv(t, "model.10.m.0.ffn.0.conv", b), act=False)
        want = _conv(t, "model.10.cv2.conv", torch.cat([a, b], 1))
    assert got.shape == want.shape == (1, 256, 5, 7)
    np.testing.assert_allclose(got.numpy(), want.numpy(), atol=2e-5 * float(want.abs().max()))


@pytest.mark.parametrize("shortcut", [True, False])
def test_ref_c3k_against_longhand(shortcut):
    from geotrax_amd.weights import synthetic_yolo11
    from yolo11_ref import Yolo11Ref

    t = synthetic_yolo11(seed=3, nc=4, scale="n")
    m = "model.6.m.0"                                                                         # C3k(64, 64): hidden 32, two 3x3 + 3x3 bottlenecks
    x = torch.randn(1, 64, 6, 9, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        got = Yolo11Ref(t)._c3k(m, x, shortcut)
        y = _conv(t, m + ".cv1.conv", x)
        for j in range(2):
            z = _conv(t, f"{m}.m.{j}.cv2.conv", _conv(t, f"{m}.m.{j}.cv1.conv", y))
            y = y + z if shortcut else z
        want = _conv(t, m + ".cv3.conv", torch.cat([y, _conv(t, m + ".cv2.conv", x)], 1))
    assert t[m + ".m.0.cv1.conv.weight"].shape == (32, 32, 3, 3) and f"{m}.m.2.cv1.conv.weight" not in t
    np.testing.assert_allclose(got.numpy(), want.numpy(), atol=1e-6 * float(want.abs().max()))


def test_fold_bn_on_a_depthwise_and_an_activation_free_conv():
    from geotrax_amd.weights import BN_EPS, fold_bn

    rng = np.random.default_rng(0)
    t = {}
    for name, shape in (("model.23.cv3.0.0.0", (16, 1, 3, 3)), ("model.10.m.0.attn.proj", (16, 16, 1, 1))):
        t[name + ".conv.weight"] = rng.standard_normal(shape).astype(np.float32)
        t[name + ".bn.weight"] = (1 + 0.1 * rng.standard_normal(shape[0])).astype(np.float32)
        t[name + ".bn.bias"] = rng.standard_normal(shape[0]).astype(np.float32)
        t[name + ".bn.running_mean"] = rng.standard_normal(shape[0]).astype(np.float32)
        t[name + ".bn.running_var"] = rng.uniform(0.5, 2, shape[0]).astype(np.float32)
        t[name + ".bn.num_batches_tracked"] = np.asarray(7, np.int64)
    f = fold_bn(t)
    assert sorted(f) == sorted(n + s for n in ("model.23.cv3.0.0.0", "model.10.m.0.attn.proj") for s in (".conv.weight", ".conv.bias"))
    x = torch.randn(2, 16, 5, 6, generator=torch.Generator().manual_seed(2))
    for name, groups in (("model.23.cv3.0.0.0", 16), ("model.10.m.0.attn.proj", 1)):
        w = torch.from_numpy(t[name + ".conv.weight"])
        y = F.conv2d(x, w, None, padding=w.shape[-1] // 2, groups=groups)
        want = F.batch_norm(y, torch.from_numpy(t[name + ".bn.running_mean"]), torch.from_numpy(t[name + ".bn.running_var"]),
                            torch.from_numpy(t[name + ".bn.weight"]), torch.from_numpy(t[name + ".bn.bias"]), False, 0.0, BN_EPS)
        got = F.conv2d(x, torch.from_numpy(f[name + ".conv.weight"]), torch.from_numpy(f[name + ".conv.bias"]), padding=w.shape[-1] // 2, groups=groups)
        np.testing.assert_allclose(got.numpy(), want.numpy(), atol=1e-5)


def test_wrapper_reports_the_yaml_and_the_names(tmp_path):
    from geotrax_amd.model import YOLO
    from geotrax_amd.weights import save_weights, synthetic_yolo11

    w = synthetic_yolo11(seed=0, nc=4, scale="n")
    path = tmp_path / "yolo11n.safetensors"
    save_weights(w, path)
    path.with_suffix(".names.yaml").write_text("{0: car, 1: bus, 2: truck, 3: motorcycle}\n")
    m = YOLO(str(path))
    assert m.yaml_file == m.model.yaml_file == "yolo11.yaml" and not m.is_rtdetr
    assert m.names == {0: "car", 1: "bus", 2: "truck", 3: "motorcycle"}
    m2 = YOLO(w)
    assert m2.yaml_file == "yolo11.yaml" and len(m2.names) == 4
    with pytest.raises(NotImplementedError, match="YOLOv8-cls"):                             # a detect file is no ReID model
        YOLO.__new__(YOLO)._make_tracker({"tracker_type": "botsort", "with_reid": True, "model": str(path)})
