"""YOLOv5u on the host side, no GPU: the graph is recognised from the tensors with its scale, every look-alike of the family is
refused by name while every other family keeps its route, the C++ layer table restates the same yaml as the Python one and obeys the
table walker's rules, the CPU restatement (tests/yolov5u_ref.py) has yolov5.yaml's layer shapes at all five scales, its C3 equals the
stacked form the HIP path launches, and the 108-row stem weight layout round-trips."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

SCALES = ["n", "s", "m", "l", "x"]
WIDTH = {"n": 0.25, "s": 0.5, "m": 0.75, "l": 1.0, "x": 1.25}
REPEATS = {"n": (1, 2, 3, 1), "s": (1, 2, 3, 1), "m": (2, 4, 6, 2), "l": (3, 6, 9, 3), "x": (4, 8, 12, 4)}
ROOT = Path(__file__).resolve().parent.parent


@pytest.mark.parametrize("scale", SCALES)
def test_topology_and_scale_are_read_off_the_tensors(scale):
    from geotrax_amd.weights import check_yolov5u, detector_topology, is_yolov5u, synthetic_yolov5u

    t = synthetic_yolov5u(seed=0, nc=4, scale=scale)
    assert is_yolov5u(t) and detector_topology(t) == ("yolov5u", "model.24") and check_yolov5u(t) == scale
    assert t["model.0.conv.weight"].shape == (int(64 * WIDTH[scale]), 3, 6, 6)
    assert t["model.10.conv.weight"].shape[2:] == (1, 1) and t["model.14.conv.weight"].shape[2:] == (1, 1)
    for row, n in zip((2, 4, 6, 8), REPEATS[scale]):
        assert f"model.{row}.m.{n - 1}.cv1.conv.weight" in t and f"model.{row}.m.{n}.cv1.conv.weight" not in t
        assert t[f"model.{row}.m.0.cv1.conv.weight"].shape[2:] == (1, 1) and t[f"model.{row}.m.0.cv2.conv.weight"].shape[2:] == (3, 3)
    assert t["model.8.cv3.conv.weight"].shape[0] == int(1024 * WIDTH[scale])            # max_channels = 1024 at every scale


@pytest.mark.parametrize("scale", SCALES)
def test_wrapper_reports_the_yaml(scale):
    """Fails without the family: the file is taken for YOLOv8 and construction dies on a missing model.22 tensor."""
    from geotrax_amd.model import YOLO
    from geotrax_amd.weights import synthetic_yolov5u

    m = YOLO(synthetic_yolov5u(seed=0, nc=4, scale=scale))
    assert m.yaml_file == f"yolov5{scale}.yaml" and not m.is_end2end and not m.is_rtdetr and len(m.names) == 4


def test_a_changed_shape_is_refused_by_name():
    from geotrax_amd.weights import detector_topology, synthetic_yolov5u

    t = synthetic_yolov5u(seed=0, nc=4, scale="n")
    cases = {
        "a wider C3 hidden layer": {**t, "model.4.cv1.conv.weight": np.zeros((48, 64, 1, 1), np.float32)},
        "a 3x3 bottleneck entry": {**t, "model.2.m.0.cv1.conv.weight": np.zeros((16, 16, 3, 3), np.float32)},
        "a second repeat at scale n": {**t, "model.2.m.1.cv1.conv.weight": t["model.2.m.0.cv1.conv.weight"], "model.2.m.1.cv2.conv.weight": t["model.2.m.0.cv2.conv.weight"]},
        "a 3x3 neck Conv": {**t, "model.10.conv.weight": np.zeros((128, 256, 3, 3), np.float32)},
        "an unknown stem width": {**t, "model.0.conv.weight": np.zeros((24, 3, 6, 6), np.float32)},
        "a layer past the head": {**t, "model.25.conv.weight": t["model.1.conv.weight"]},
        "Detect elsewhere": {k.replace("model.24.", "model.25."): v for k, v in t.items()},
        "a missing tensor": {k: v for k, v in t.items() if k != "model.23.cv3.conv.weight"},
        "another class count on one level": {**t, "model.24.cv3.1.2.weight": np.zeros((5, 64, 1, 1), np.float32)},
    }
    for what, bad in cases.items():
        with pytest.raises(NotImplementedError, match=r"yolov5\.yaml"):
            detector_topology(bad)
            pytest.fail(what)
    m = synthetic_yolov5u(seed=0, nc=4, scale="m")                      # every tensor of scale m behind scale s's stem
    with pytest.raises(NotImplementedError, match=r"yolov5\.yaml"):
        detector_topology({**m, "model.0.conv.weight": np.zeros((32, 3, 6, 6), np.float32)})


def test_the_lookalikes_are_refused_by_name():
    from geotrax_amd.model import YOLO
    from geotrax_amd.weights import detector_topology, synthetic_yolov5u, synthetic_yolov8

    t = synthetic_yolov5u(seed=0, nc=4, scale="n")
    head = {k: v for k, v in t.items() if k.startswith("model.24.")}
    body = {k: v for k, v in t.items() if not k.startswith("model.24.")}
    p6 = {**body, **{k.replace("model.24.", "model.33."): v for k, v in head.items()}, "model.33.cv2.3.0.conv.weight": t["model.24.cv2.2.0.conv.weight"]}
    anchors = {**body, "model.24.anchors": np.zeros((3, 3, 2), np.float32), **{f"model.24.m.{l}.weight": np.zeros((27, 64 << l, 1, 1), np.float32) for l in range(3)}}
    old_focus = {k: v for k, v in anchors.items() if k != "model.0.conv.weight"} | {"model.0.conv.conv.weight": np.zeros((16, 12, 3, 3), np.float32)}
    v8 = synthetic_yolov8(seed=0, nc=4, scale="n")
    v3 = {"model.0.conv.weight": np.zeros((32, 3, 3, 3), np.float32), "model.1.conv.weight": np.zeros((64, 32, 3, 3), np.float32),
          "model.2.cv1.conv.weight": np.zeros((32, 64, 1, 1), np.float32), "model.2.cv2.conv.weight": np.zeros((64, 32, 3, 3), np.float32),
          **{k.replace("model.22.", "model.28."): v for k, v in v8.items() if k.startswith("model.22.")},
          "model.28.dfl.conv.weight": t["model.24.dfl.conv.weight"]}
    seg = {**t, "model.24.cv4.0.0.conv.weight": t["model.24.cv2.0.0.conv.weight"], "model.24.proto.cv1.conv.weight": np.zeros((64, 64, 3, 3), np.float32)}
    cls = {**{k: v for k, v in body.items() if int(k.split(".")[1]) < 9}, "model.9.conv.conv.weight": np.zeros((1280, 256, 1, 1), np.float32),
           "model.9.linear.weight": np.zeros((4, 1280), np.float32)}
    for bad, name in ((p6, "yolov5\\*6u"), (anchors, "anchor-based"), (old_focus, "anchor-based"), (v3, "YOLOv3u"), (seg, "-seg"), (cls, "-cls")):
        with pytest.raises(NotImplementedError, match=name) as e:
            detector_topology(bad)
        assert "yolov5.yaml" in str(e.value) and "only yolov5u detect" in str(e.value)
        with pytest.raises(NotImplementedError, match=name):
            YOLO(bad)


def test_the_other_families_keep_their_route():
    from geotrax_amd import weights as W

    routes = {"synthetic_yolov8": ("yolov8", "model.22"), "synthetic_yolov8_p2": ("yolov8-p2", "model.28"), "synthetic_yolo11": ("yolo11", "model.23"),
              "synthetic_yolov10": ("yolov10", "model.23"), "synthetic_yolo12": ("yolo12", "model.21"), "synthetic_yolo26": ("yolo26", "model.23"),
              "synthetic_yolov9": ("yolov9", "model.22")}
    for fn, want in routes.items():
        for scale in ("n", "s") if fn != "synthetic_yolov9" else ("t", "s"):
            t = getattr(W, fn)(seed=0, nc=4, scale=scale)
            assert not W.is_yolov5u(t) and not W._yolov5_lookalike(t) and W.detector_topology(t) == want, (fn, scale)
            dfl = {**t, want[1] + ".dfl.conv.weight": np.arange(16, dtype=np.float32).reshape(1, 16, 1, 1)}     # as a real file carries it
            assert not W._yolov5_lookalike(dfl) and W.detector_topology(dfl) == want, (fn, scale)
    assert W.detector_topology(W.synthetic_yolov8_rtdetr(seed=0, nc=4, scale="n")) == ("yolov8-rtdetr", "model.22")
    v5 = W.synthetic_yolov5u(seed=0, nc=4, scale="n")
    assert not W.is_yolo12(v5) and not W.is_yolov10(v5) and not W.is_yolo26(v5) and not W.has_yolo11_blocks(v5) and not W.is_yolov9(v5) and not W.is_yolov8_p2(v5)


def _cpp_table(name):
    """The rows of a layer table of csrc/yolo_tables.hpp: (index, module, from tuple, shortcut)"""
    src = (ROOT / "geo-trax_amd" / "csrc" / "yolo_tables.hpp").read_text()
    body = re.search(r"inline constexpr R %s\[\] = \{(.*?)\};" % name, src, re.S).group(1)
    rows = re.findall(r"\{(\d+), R::(\w+), \{([-\d, ]+)\}, (\w+)(?:, \d+)?\}", body)
    return [(int(i), mod, tuple(int(f) for f in frm.split(",")), sc) for i, mod, frm, sc in rows]


def test_the_layer_table_restates_the_yaml_and_obeys_the_walker():
    """kYolov5u row by row against weights.YOLOV5_YAML, and trunk_table_error's rules on it (the C++ function itself runs on the table
    in csrc/hosttest/sanitize_host.cpp, tests/test_sanitizers.py): row i is layer i, reads earlier layers only, a Concat's members feed
    one Concat, an Upsample leads its Concat, every other row reads one layer, Detect comes last."""
    from geotrax_amd.weights import YOLOV5_YAML

    rows = _cpp_table("kYolov5u")
    assert len(rows) == len(YOLOV5_YAML) == 25
    module = {"Conv": "CONV", "C3": "C3", "SPPF": "SPPF", "Upsample": "UPSAMPLE", "Concat": "CONCAT", "Detect": "DETECT"}
    cat_of = {}
    for (i, mod, frm, shortcut), (yfrm, _, ymod, yargs) in zip(rows, YOLOV5_YAML):
        assert rows[i][0] == i and mod == module[ymod] and frm == ((yfrm,) if isinstance(yfrm, int) else tuple(yfrm)), i
        if mod == "C3":
            assert shortcut == ("false" if len(yargs) > 1 and yargs[1] is False else "true") and (shortcut == "true") == (i < 9), i
        src = [i + f if f < 0 else f for f in frm]
        assert all(0 <= f < i for f in src) or i == 0
        assert len(src) == 1 or mod in ("CONCAT", "DETECT")
        if mod == "CONCAT":
            for k, f in enumerate(src):
                assert f not in cat_of and (rows[f][1] != "UPSAMPLE" or k == 0), i
                cat_of[f] = i
    assert rows[-1][1] == "DETECT" and cat_of == {11: 12, 6: 12, 15: 16, 4: 16, 18: 19, 14: 19, 21: 22, 10: 22}
    assert "kYolov5u" in (ROOT / "geo-trax_amd" / "csrc" / "hosttest" / "sanitize_host.cpp").read_text()


@pytest.mark.parametrize("scale", SCALES)
def test_restatement_layer_shapes_at_64(scale):
    from geotrax_amd.weights import synthetic_yolov5u
    from yolov5u_ref import Yolov5uRef

    ch = lambda c: int(np.ceil(min(c, 1024) * WIDTH[scale] / 8) * 8)
    ref = Yolov5uRef(synthetic_yolov5u(seed=0, nc=4, scale=scale, gain=1.0))
    out = ref.forward(torch.rand(1, 3, 64, 64, generator=torch.Generator().manual_seed(0)))
    assert out.shape == (1, 8 * 8 + 4 * 4 + 2 * 2, 8) and bool(torch.isfinite(out).all())
    want = {"model.0.conv": (ch(64), 32), "model.1.conv": (ch(128), 16), "model.2": (ch(128), 16), "model.3.conv": (ch(256), 8), "model.4": (ch(256), 8),
            "model.5.conv": (ch(512), 4), "model.6": (ch(512), 4), "model.7.conv": (ch(1024), 2), "model.8": (ch(1024), 2), "model.9": (ch(1024), 2),
            "model.10.conv": (ch(512), 2), "model.13": (ch(512), 4), "model.14.conv": (ch(256), 4), "model.17": (ch(256), 8), "model.18.conv": (ch(256), 4),
            "model.20": (ch(512), 4), "model.21.conv": (ch(512), 2), "model.23": (ch(1024), 2), "model.2.cv1.conv": (ch(128) // 2, 16)}
    for name, (c, hw) in want.items():
        assert tuple(ref.acts[name].shape) == (1, c, hw, hw), name


def test_the_stem_reads_two_rows_above_and_three_below():
    """Conv(k = 6, s = 2, p = 2) on odd and minimal sides: the output size, and one-hot weights pick image pixel (2 oy - 2 + ky, 2 ox - 2 + kx)."""
    from yolov5u_ref import Yolov5uRef

    for h, w in ((2, 2), (7, 9), (8, 6)):
        x = torch.arange(3 * h * w, dtype=torch.float32).reshape(1, 3, h, w) / (3 * h * w)
        for ky, kx, col in ((0, 0, 0), (5, 5, 2), (2, 3, 1), (0, 5, 1)):
            wt = np.zeros((16, 3, 6, 6), np.float32)
            wt[0, col, ky, kx] = 1.0
            y = Yolov5uRef({"model.0.conv.weight": wt, "model.24.cv3.0.2.weight": np.zeros((1, 1, 1, 1), np.float32)})._stem(x)
            ho, wo = (h - 2) // 2 + 1, (w - 2) // 2 + 1
            assert y.shape == (1, 16, ho, wo)
            for oy in range(ho):
                for ox in range(wo):
                    iy, ix = 2 * oy - 2 + ky, 2 * ox - 2 + kx
                    v = x[0, col, iy, ix] if 0 <= iy < h and 0 <= ix < w else torch.tensor(0.0)
                    # a neighbouring pixel differs by 1 / (3 h w) > 6e-3; torch's vector and scalar SiLU may differ in the last bit
                    assert abs(float(y[0, 0, oy, ox]) - float(torch.nn.functional.silu(v))) < 1e-6, (h, w, ky, kx, oy, ox)


def test_c3_with_stacked_weights_equals_the_two_convolutions():
    """The HIP path runs cv1 and cv2 as one 1x1 launch over [cv2 | cv1]: the stacked convolution's halves are the separate ones bit
    for bit (a 1x1 output channel depends on its own row alone), and cv3 on [m(cv1 x) | cv2 x] read from there is the block."""
    from geotrax_amd.weights import synthetic_yolov5u
    from yolov5u_ref import Yolov5uRef, stack_c3

    ref = Yolov5uRef(synthetic_yolov5u(seed=3, nc=4, scale="n", gain=1.0))
    x = torch.randn(2, 32, 9, 7, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        want = ref._c3("model.2", x, True)
        w, b = stack_c3(ref.t, "model.2")
        both = torch.nn.functional.silu(torch.nn.functional.conv2d(x, w, b))
        c = w.shape[0] // 2
        assert torch.equal(both[:, :c], ref.acts["model.2.cv2.conv"]) and torch.equal(both[:, c:], ref.acts["model.2.cv1.conv"])
        y = ref._bottleneck("model.2.m.0", both[:, c:], True)
        got = ref._conv("model.2.cv3.conv", torch.cat([y, both[:, :c]], 1))
    assert "model.2.m.1.cv1.conv.weight" not in ref.t and torch.equal(got, want)


def test_the_108_row_weight_layout_round_trips():
    from yolov5u_ref import oihw_of, w108_of

    w = np.random.default_rng(0).standard_normal((48, 3, 6, 6)).astype(np.float32)
    w108 = w108_of(w)
    assert w108.shape == (108, 48) and np.array_equal(oihw_of(w108), w)
    for ky, kx, col, o in ((0, 0, 0, 0), (5, 5, 2, 47), (1, 4, 2, 7), (4, 1, 0, 30)):
        assert w108[(ky * 6 + kx) * 3 + col, o] == w[o, col, ky, kx]


def test_bn_folding_covers_the_family():
    """tools/convert_weights.py's route: every Conv of a C3 block and the 6x6 stem carry a BatchNorm, folded like any other family's"""
    from geotrax_amd.weights import BN_EPS, fold_bn

    rng = np.random.default_rng(0)
    raw = {"model.24.dfl.conv.weight": np.arange(16, dtype=np.float32).reshape(1, 16, 1, 1)}
    shapes = {"model.0.conv": (16, 3, 6, 6), "model.2.cv1.conv": (8, 16, 1, 1), "model.2.m.0.cv2.conv": (8, 8, 3, 3), "model.10.conv": (8, 16, 1, 1)}
    for name, shape in shapes.items():
        base = name[: -len(".conv")]
        raw[name + ".weight"] = rng.standard_normal(shape).astype(np.float32)
        for k in ("weight", "bias", "running_mean"):
            raw[f"{base}.bn.{k}"] = rng.standard_normal(shape[0]).astype(np.float32)
        raw[f"{base}.bn.running_var"] = rng.random(shape[0]).astype(np.float32) + 0.5
    out = fold_bn(raw)
    assert np.array_equal(out["model.24.dfl.conv.weight"], raw["model.24.dfl.conv.weight"])
    for name in shapes:
        base = name[: -len(".conv")]
        s = raw[f"{base}.bn.weight"] / np.sqrt(raw[f"{base}.bn.running_var"] + BN_EPS)
        np.testing.assert_allclose(out[name + ".weight"], raw[name + ".weight"] * s[:, None, None, None], rtol=1e-6)
        np.testing.assert_allclose(out[name + ".bias"], raw[f"{base}.bn.bias"] - raw[f"{base}.bn.running_mean"] * s, rtol=1e-5, atol=1e-6)
        assert not any(k.startswith(base + ".bn.") for k in out)
