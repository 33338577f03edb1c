"""YOLOv9 on the host side (no GPU): the topology answer, the layer specs of the four scales against a table written out here, the
refusals, the other families' answers, RepConv folding against the unfused two-branch form, tests/yolov9_ref.py's pooling against
torch.nn.functional, the zero-border identity the HIP path's AConv rests on, and the pooling hook's argument checks."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

SCALES = "tsmc"
# per scale: tensor count, then (tensor, OIHW shape) of every row's defining layers -- written out from the yamls, not from weights.py
TABLE = {
    "t": (185, {"model.0.conv": (16, 3, 3, 3), "model.1.conv": (32, 16, 3, 3), "model.2.cv1.conv": (32, 32, 1, 1), "model.2.cv2.conv": (16, 16, 3, 3),
                "model.2.cv3.conv": (16, 16, 3, 3), "model.2.cv4.conv": (32, 64, 1, 1), "model.3.cv1.conv": (64, 32, 3, 3),
                "model.4.cv1.conv": (64, 64, 1, 1), "model.4.cv2.0.cv1.conv": (16, 32, 1, 1), "model.4.cv2.0.m.2.cv1.conv": (16, 16, 3, 3),
                "model.4.cv2.1.conv": (32, 32, 3, 3), "model.4.cv3.0.cv3.conv": (32, 32, 1, 1), "model.4.cv4.conv": (64, 128, 1, 1),
                "model.5.cv1.conv": (96, 64, 3, 3), "model.6.cv2.0.cv1.conv": (24, 48, 1, 1), "model.6.cv4.conv": (96, 192, 1, 1),
                "model.7.cv1.conv": (128, 96, 3, 3), "model.8.cv4.conv": (128, 256, 1, 1), "model.9.cv1.conv": (64, 128, 1, 1),
                "model.9.cv5.conv": (128, 256, 1, 1), "model.12.cv1.conv": (96, 224, 1, 1), "model.15.cv1.conv": (64, 160, 1, 1),
                "model.16.cv1.conv": (48, 64, 3, 3), "model.18.cv1.conv": (96, 144, 1, 1), "model.19.cv1.conv": (64, 96, 3, 3),
                "model.21.cv1.conv": (128, 192, 1, 1), "model.22.cv2.0.0.conv": (64, 64, 3, 3), "model.22.cv3.2.0.conv": (64, 128, 3, 3),
                "model.22.cv3.0.2": (4, 64, 1, 1)}),
    "s": (185, {"model.0.conv": (32, 3, 3, 3), "model.2.cv2.conv": (32, 32, 3, 3), "model.3.cv1.conv": (128, 64, 3, 3), "model.4.cv2.0.m.2.cv2.conv": (32, 32, 3, 3),
                "model.6.cv1.conv": (192, 192, 1, 1), "model.6.cv2.0.cv1.conv": (48, 96, 1, 1), "model.8.cv4.conv": (256, 512, 1, 1),
                "model.9.cv5.conv": (256, 512, 1, 1), "model.12.cv1.conv": (192, 448, 1, 1), "model.15.cv4.conv": (128, 256, 1, 1),
                "model.16.cv1.conv": (96, 128, 3, 3), "model.18.cv1.conv": (192, 288, 1, 1), "model.19.cv1.conv": (128, 192, 3, 3),
                "model.21.cv1.conv": (256, 384, 1, 1), "model.22.cv3.2.0.conv": (128, 256, 3, 3)}),
    "m": (139, {"model.0.conv": (32, 3, 3, 3), "model.2.cv1.conv": (128, 64, 1, 1), "model.2.cv2.0.cv1.conv": (32, 64, 1, 1), "model.2.cv4.conv": (128, 256, 1, 1),
                "model.3.cv1.conv": (240, 128, 3, 3), "model.4.cv2.0.cv1.conv": (60, 120, 1, 1), "model.4.cv2.0.m.0.cv1.conv": (60, 60, 3, 3),
                "model.5.cv1.conv": (360, 240, 3, 3), "model.6.cv2.0.cv3.conv": (180, 180, 1, 1), "model.7.cv1.conv": (480, 360, 3, 3),
                "model.9.cv5.conv": (480, 960, 1, 1), "model.12.cv1.conv": (360, 840, 1, 1), "model.16.cv1.conv": (184, 240, 3, 3),
                "model.18.cv1.conv": (360, 544, 1, 1), "model.19.cv1.conv": (240, 360, 3, 3), "model.21.cv1.conv": (480, 720, 1, 1),
                "model.22.cv3.0.0.conv": (240, 240, 3, 3)}),
    "c": (144, {"model.0.conv": (64, 3, 3, 3), "model.2.cv1.conv": (128, 128, 1, 1), "model.2.cv4.conv": (256, 256, 1, 1), "model.3.cv1.conv": (128, 128, 3, 3),
                "model.3.cv2.conv": (128, 128, 1, 1), "model.4.cv1.conv": (256, 256, 1, 1), "model.4.cv4.conv": (512, 512, 1, 1),
                "model.5.cv1.conv": (256, 256, 3, 3), "model.5.cv2.conv": (256, 256, 1, 1), "model.6.cv2.0.cv1.conv": (128, 256, 1, 1),
                "model.9.cv5.conv": (512, 1024, 1, 1), "model.12.cv1.conv": (512, 1024, 1, 1), "model.15.cv4.conv": (256, 512, 1, 1),
                "model.16.cv1.conv": (128, 128, 3, 3), "model.18.cv1.conv": (512, 768, 1, 1), "model.19.cv2.conv": (256, 256, 1, 1),
                "model.21.cv1.conv": (512, 1024, 1, 1), "model.22.cv3.1.0.conv": (256, 512, 3, 3)}),
}


@pytest.mark.parametrize("scale", SCALES)
def test_topology_and_specs(scale):
    from geotrax_amd.weights import check_yolov9, detector_topology, is_yolov9, synthetic_yolov9, yolov9_layer_specs

    w = synthetic_yolov9(seed=1, nc=4, scale=scale)
    assert detector_topology(w) == ("yolov9", "model.22")          # the parent commit answers ("yolov8", "model.22")
    assert is_yolov9(w) and check_yolov9(w) == scale
    specs = yolov9_layer_specs(scale, 4)
    count, table = TABLE[scale]
    shapes = {n: s for n, s, _ in specs}
    assert len(specs) == len(shapes) == count and len(w) == 2 * count
    for name, shape in table.items():
        assert shapes[name] == shape, name
    assert all(w[n + ".weight"].shape == s and w[n + ".bias"].shape == s[:1] for n, s in shapes.items())
    assert all(not n.startswith(("model.10.", "model.11.", "model.13.", "model.14.", "model.17.", "model.20.")) for n in shapes)   # Upsample / Concat rows
    assert all(act == (not n.endswith(".2")) for n, _, act in specs)


def test_refusals_name_the_topology():
    from geotrax_amd.weights import YOLOV9_TOPOLOGY, detector_topology, synthetic_yolov9

    w = synthetic_yolov9(seed=1, nc=4, scale="c")
    rng = np.random.default_rng(0)
    second = dict(w)                                               # a second backbone behind the head: CBLinear-shaped tensors past model.22
    second["model.23.conv.weight"] = rng.normal(size=(64, 64, 1, 1)).astype(np.float32)
    second["model.23.conv.bias"] = np.zeros(64, np.float32)
    wide = dict(w)                                                 # one ELAN block of another width
    wide["model.6.cv2.1.conv.weight"] = rng.normal(size=(272, 272, 3, 3)).astype(np.float32)
    moved = {k.replace("model.22.", "model.23."): v for k, v in w.items()}   # Detect at another index
    no_spp = {k: v for k, v in w.items() if not k.startswith("model.9.")}     # GELAN blocks without SPPELAN at model.9 (yolov9e's shape)
    for bad in (second, wide, moved, no_spp):
        with pytest.raises(NotImplementedError) as e:
            detector_topology(bad)
        assert YOLOV9_TOPOLOGY in str(e.value)
    assert "yolov9e" in str(e.value)


def test_padded_yolov9m_is_the_same_network():
    """pad_yolov9_channels: yolov9m's maps as multiples of 16 channels (what the convolution kernels take). Every padded tensor keeps
    its values at the layout's positions and zeros elsewhere, every row's width is a multiple of 16, and the restatement run on the
    padded tensors gives the unpadded run's raw output and, through the layout, its layers in float64 -- to 1e-10 of each map's maximum:
    the added zeros change no sum, only the order in which the CPU convolution adds (the padding channels themselves are exact zeros).
    The other scales come back untouched."""
    from geotrax_amd.weights import pad_yolov9_channels, synthetic_yolov9
    from yolov9_ref import Yolov9Ref

    for scale in "tsc":
        w = synthetic_yolov9(seed=1, nc=4, scale=scale)
        p, layout = pad_yolov9_channels(w, scale)
        assert layout == {} and all(p[k] is w[k] for k in w)
    w = synthetic_yolov9(seed=5, nc=4, scale="m", gain=1.6)
    p, layout = pad_yolov9_channels(w, "m")
    assert sorted(layout) == sorted(["model.5", "model.6", "model.7.pool", "model.11", "model.12", "model.13", "model.14", "model.16",
                                     "model.17", "model.18", "model.19.pool"])
    assert p["model.6.cv1.conv.weight"].shape == (384, 368, 1, 1) and p["model.16.cv1.conv.weight"].shape == (192, 240, 3, 3)
    assert p["model.6.cv2.0.cv1.conv.weight"].shape == (90, 192, 1, 1)          # RepCSP's hidden width: padded inside the block by the trunk builder
    for k, v in p.items():
        if k.endswith(".weight") and v.ndim == 4 and ".cv2.0." not in k and ".cv3.0." not in k and not k.endswith(".2.weight"):
            assert v.shape[0] % 16 == 0 and (v.shape[1] % 16 == 0 or k == "model.0.conv.weight"), k
    assert float(np.abs(p["model.16.cv1.conv.weight"][184:]).max()) == 0 and float(np.abs(p["model.16.cv1.conv.bias"][184:]).max()) == 0
    x = torch.randn(1, 3, 64, 64, dtype=torch.float64, generator=torch.Generator().manual_seed(0))
    a, b = Yolov9Ref(w).double(), Yolov9Ref(p).double()
    ya, yb = a.forward(x), b.forward(x)
    close = lambda u, v: float((u - v).abs().max()) <= 1e-10 * float(v.abs().max())
    assert close(ya[..., :4], yb[..., :4]) and close(ya[..., 4:], yb[..., 4:])
    for name in ("model.2", "model.4", "model.5", "model.6", "model.9", "model.12", "model.16", "model.16.pool", "model.18", "model.21"):
        got = b.acts[name][0]
        if name in layout:
            assert float(got[np.setdiff1d(np.arange(got.shape[0]), layout[name])].abs().max()) == 0, name
            got = got[layout[name]]
        assert got.shape == a.acts[name][0].shape and close(got, a.acts[name][0]), name


def test_model_auto_reid_is_refused_by_name_for_scales_t_s_m():
    """Before any native object exists (no GPU is touched): the error names the family, the scale and the widths."""
    from geotrax_amd.detector import Detector
    from geotrax_amd.weights import synthetic_yolov9

    for scale in "tsm":
        with pytest.raises(NotImplementedError, match=f"yolov9{scale}: with_reid"):
            Detector(synthetic_yolov9(seed=1, nc=4, scale=scale), (48, 80), imgsz=64, obj_feats=True)


def test_other_families_answer_what_they_did():
    from geotrax_amd import weights as W

    assert W.detector_topology(W.synthetic_yolov8(0, 4, "n")) == ("yolov8", "model.22")
    assert W.detector_topology(W.synthetic_yolov8_p2(0, 4, "n")) == ("yolov8-p2", "model.28")
    assert W.detector_topology(W.synthetic_yolo11(0, 4, "n")) == ("yolo11", "model.23")
    assert W.detector_topology(W.synthetic_yolov10(0, 4, "n")) == ("yolov10", "model.23")
    for f in (W.synthetic_yolov8, W.synthetic_yolov8_p2, W.synthetic_yolo11, W.synthetic_yolov10):
        assert not W.is_yolov9(f(0, 4, "n"))
    assert not W.is_yolov10(W.synthetic_yolov9(0, 4, "t")) and not W.has_yolo11_blocks(W.synthetic_yolov9(0, 4, "t")) and not W.is_yolov8_p2(W.synthetic_yolov9(0, 4, "t"))


def test_repconv_folding_equals_the_two_branch_form(tmp_path):
    """An unfused RepBottleneck (RepConv's 3x3 and 1x1 branches and the Conv3x3, each with BN statistics) under a YOLOv9 name: fold_bn
    then fuse_repconv -- BN folded per branch BEFORE the branches are summed -- equals the two-branch form evaluated directly in
    float64, to 1e-6 of the output maximum, on a random 8 x 6 x 6 input. load_weights does both for such a file."""
    from geotrax_amd.weights import fold_bn, fuse_repconv, load_weights, save_weights
    from yolov9_ref import rep_bottleneck_unfused

    rng = np.random.default_rng(3)
    p, c = "model.4.cv2.0.m.0", 8
    t = {}
    for name, k in ((p + ".cv1.conv1", 3), (p + ".cv1.conv2", 1), (p + ".cv2", 3)):
        t[name + ".conv.weight"] = rng.normal(0, 0.3, (c, c, k, k)).astype(np.float32)
        q = name + ".bn"
        t[q + ".weight"], t[q + ".bias"] = rng.uniform(0.5, 1.5, c).astype(np.float32), rng.normal(0, 0.2, c).astype(np.float32)
        t[q + ".running_mean"], t[q + ".running_var"] = rng.normal(0, 0.2, c).astype(np.float32), rng.uniform(0.5, 2.0, c).astype(np.float32)
    x = torch.from_numpy(rng.normal(0, 1, (1, c, 6, 6)))
    want = rep_bottleneck_unfused(x, {k: torch.from_numpy(v).double() for k, v in t.items()}, p)
    path = tmp_path / "unfused.safetensors"
    save_weights(t, path)
    for f in (fuse_repconv(fold_bn(t)), load_weights(path)):
        assert sorted(f) == sorted(p + s for s in (".cv1.conv.weight", ".cv1.conv.bias", ".cv2.conv.weight", ".cv2.conv.bias"))
        g = {k: torch.from_numpy(v).double() for k, v in f.items()}
        r = F.silu(F.conv2d(x, g[p + ".cv1.conv.weight"], g[p + ".cv1.conv.bias"], padding=1))
        got = x + F.silu(F.conv2d(r, g[p + ".cv2.conv.weight"], g[p + ".cv2.conv.bias"], padding=1))
        assert float((got - want).abs().max()) <= 1e-6 * float(want.abs().max())


@pytest.mark.parametrize("h,w", [(2, 2), (4, 6), (8, 8)])
def test_reference_pooling_equals_torch(h, w):
    """tests/yolov9_ref.py's written-out pooling against torch.nn.functional in float64; and the identity AConv's HIP path rests on:
    the stride-2 pad-1 convolution of the zero-bordered H x W average equals Conv2d(3, 2, 1) on the (H - 1) x (W - 1) average exactly."""
    from yolov9_ref import avgpool2_s1, maxpool3_s2, zero_border

    g = torch.Generator().manual_seed(h * 10 + w)
    x = torch.randn(2, 5, h, w, dtype=torch.float64, generator=g) - 2.0        # mostly negative: zero padding would show in the maximum
    a = avgpool2_s1(x)
    assert float((a - F.avg_pool2d(x, 2, 1, 0)).abs().max()) <= 2.0 ** -50
    assert torch.equal(maxpool3_s2(a), F.max_pool2d(a, 3, 2, 1))
    wt = torch.randn(7, 5, 3, 3, dtype=torch.float64, generator=g)
    b = zero_border(a)
    assert b.shape[-2:] == (h, w) and not b[..., -1, :].any() and not b[..., :, -1].any()
    assert torch.equal(F.conv2d(b, wt, stride=2, padding=1), F.conv2d(a, wt, stride=2, padding=1))


def test_pool_down_hook_refuses_bad_arguments_before_any_launch():
    """Host only, as in tests/test_abi.py: NULL arrays, odd or too small maps and channel counts, strides or offsets that are no
    multiples of 8 come back as an error code with a message; with every size fine the missing context is what is refused."""
    from geotrax_amd import _lib

    lib = _lib.load()
    f = np.zeros(8192, np.float32)
    p = _lib.ptr

    def call(dtype=1, n=1, na=1, h=4, w=6, ca=8, cb=8, x=f, ics=16, ico=0, avg=f, acs=8, aco=0, mx=f, mcs=8, mco=0):
        return lib.gtx_op_pool_down(None, dtype, n, na, h, w, ca, cb, p(x) if x is not None else None, ics, ico, p(avg) if avg is not None else None, acs, aco,
                                    p(mx) if mx is not None else None, mcs, mco, 0, None)

    assert call() == -1 and b"ctx is NULL" in lib.gtx_last_error()              # the sizes were fine
    assert call(cb=0, mx=None, ics=8) == -1 and b"ctx is NULL" in lib.gtx_last_error()   # AConv: no maximum
    for kw, msg in ((dict(h=5), b"even"), (dict(w=7), b"even"), (dict(h=0), b"2 x 2"), (dict(w=1), b"2 x 2"), (dict(ca=12), b"multiples of 8"),
                    (dict(cb=4), b"multiples of 8"), (dict(ca=0), b"multiples of 8"), (dict(ics=20), b"multiples of 8"), (dict(aco=4), b"multiples of 8"),
                    (dict(ics=8), b"fit its stride"), (dict(mco=8), b"fit its stride"), (dict(dtype=5), b"format"), (dict(n=0, na=0), b"no image"),
                    (dict(n=2, na=1), b"bad sizes"), (dict(x=None), b"x is NULL"), (dict(avg=None), b"avg is NULL"), (dict(mx=None), b"max is NULL")):
        assert call(**kw) == -1, kw
        assert msg in lib.gtx_last_error(), (kw, lib.gtx_last_error())
