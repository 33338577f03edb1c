"""The family table of weights.py: which file is claimed by which family, which is refused and with which words, every spec list and
every seeded draw, against pins recorded from the per-family functions the table replaced. No GPU needed (but for the last test).

tests/golden/family_{specs,draws,recognition}.json were written by the code before the table existed; nothing here regenerates them.

Refusal coverage: RAISE_SITES below names every `raise` of the family code and the refusing cases that reach it.
"""
import functools
import hashlib
import inspect
import json
import re
from pathlib import Path

import numpy as np
import pytest

GOLDEN = Path(__file__).parent / "golden"

# every *_layer_specs function and the scales it accepts (digest recipe: test_weights_specs.py)
SPEC_SCALES = {"yolov8_layer_specs": "nsmlx", "yolov8_p2_layer_specs": "nsmlx", "yolo11_layer_specs": "nsmlx", "yolov10_layer_specs": "ns",
               "yolo26_layer_specs": "nsmlx", "yolo12_layer_specs": "nsmlx", "yolo12_gamma_specs": "nsmlx", "yolov5u_layer_specs": "nsmlx",
               "yolov9_layer_specs": "tsmc", "yolov8_cls_layer_specs": "nsmlx", "yolo11_cls_layer_specs": "nsmlx", "rtdetr_layer_specs": ("",)}

_RT = dict(width=0.25, ndl=1)                              # a narrow, one-layer RT-DETR: the names are what recognition reads
BASES = {"yolov8-n": ("synthetic_yolov8", dict(scale="n")), "yolov8-p2-n": ("synthetic_yolov8_p2", dict(scale="n")),
         "yolo11-n": ("synthetic_yolo11", dict(scale="n")), "yolo11-m": ("synthetic_yolo11", dict(scale="m")),
         "yolov10-n": ("synthetic_yolov10", dict(scale="n")), "yolov10-s": ("synthetic_yolov10", dict(scale="s")),
         "yolo26-n": ("synthetic_yolo26", dict(scale="n")),
         "yolo12-n": ("synthetic_yolo12", dict(scale="n")), "yolo12-l": ("synthetic_yolo12", dict(scale="l")),
         "yolov5u-n": ("synthetic_yolov5u", dict(scale="n")),
         "yolov9-t": ("synthetic_yolov9", dict(scale="t")), "yolov9-m": ("synthetic_yolov9", dict(scale="m")), "yolov9-c": ("synthetic_yolov9", dict(scale="c")),
         "rtdetr-l": ("synthetic_rtdetr", _RT), "yolov8-rtdetr-n": ("synthetic_yolov8_rtdetr", dict(scale="n", ndl=1)),
         "v8cls": ("synthetic_yolov8_cls", dict(scale="n", nc=4)), "11cls": ("synthetic_yolo11_cls", dict(scale="n", nc=4))}
DETECTORS = [b for b in BASES if not b.endswith("cls")]

# the draws: every base above at seed 0, and one non-default knob set per family
_KNOBS = dict(cls_bias=-6.0, box_weight_scale=0.002)
_LB = dict(level_bias=(0.0, -1e4, -1e4))
DRAWS = {**BASES,
         "yolov8-n/knobs": ("synthetic_yolov8", dict(scale="n", **_KNOBS, **_LB, smooth_cls=2)),
         "yolov8-p2-n/knobs": ("synthetic_yolov8_p2", dict(scale="n", **_KNOBS, level_bias=(0.0, -1.0, -2.0, -3.0))),
         "yolo11-n/knobs": ("synthetic_yolo11", dict(scale="n", **_KNOBS, **_LB)), "yolov10-n/knobs": ("synthetic_yolov10", dict(scale="n", **_KNOBS, **_LB)),
         "yolo26-n/knobs": ("synthetic_yolo26", dict(scale="n", **_KNOBS)), "yolo12-l/knobs": ("synthetic_yolo12", dict(scale="l", **_KNOBS, **_LB, gamma=0.25)),
         "yolov5u-n/knobs": ("synthetic_yolov5u", dict(scale="n", **_KNOBS, **_LB)), "yolov9-t/knobs": ("synthetic_yolov9", dict(scale="t", **_KNOBS, **_LB)),
         "rtdetr-l/full": ("synthetic_rtdetr", dict(width=0.5))}


def draw(name, table=BASES):
    from geotrax_amd import weights

    fn, kw = table[name]
    return getattr(weights, fn)(seed=0, **({"nc": 4} | kw))


base = functools.lru_cache(maxsize=None)(draw)             # shared and never written to: every mutation below builds a new dict


def spec_digest(fn, scale):
    from geotrax_amd import weights

    specs = getattr(weights, fn)(*([scale] if scale else []), **({} if fn in ("yolo12_gamma_specs", "rtdetr_layer_specs") else
                                                                 {"nc": 1000 if "cls" in fn else 4}))
    rows = [[n, list(s)] + list(rest) for n, s, *rest in specs]
    return [len(specs), hashlib.sha256(json.dumps(rows).encode()).hexdigest()[:16]]


def draw_digest(t):
    h = hashlib.sha256()
    for k in sorted(t):
        a = np.ascontiguousarray(t[k])
        h.update(k.encode() + str(a.dtype).encode() + str(a.shape).encode() + a.tobytes())
    return [len(t), h.hexdigest()[:16]]


# ---- mutations: "drop=<prefix>", "rows=<name>:<n>" (the tensor again with n rows), "add=<name>:<AxBx..>" (zeros), joined by ";"
def mutate(t, ops):
    t = dict(t)
    for op in ops.split(";") if ops else []:
        what, arg = op.split("=", 1)
        if what == "drop":
            t = {k: v for k, v in t.items() if not k.startswith(arg)}
        elif what == "rows":
            name, n = arg.split(":")
            if name in t:
                t[name] = np.zeros((int(n),) + t[name].shape[1:], np.float32)
        elif what == "add":
            name, shp = arg.split(":")
            t[name] = np.zeros(tuple(int(d) for d in shp.split("x")), np.float32)
        else:
            raise ValueError(op)
    return t


def _v5_lookalike(which):
    """test_yolov5u.py's six lookalikes (and its old Focus stem), built the same way"""
    t, v8 = base("yolov5u-n"), base("yolov8-n")
    head = {k: v for k, v in t.items() if k.startswith("model.24.")}
    body = {k: v for k, v in t.items() if not k.startswith("model.24.")}
    anchors = {**body, "model.24.anchors": np.zeros((3, 3, 2), np.float32), **{f"model.24.m.{l}.weight": np.zeros((27, 64 << l, 1, 1), np.float32) for l in range(3)}}
    if which == "p6":
        return {**body, **{k.replace("model.24.", "model.33."): v for k, v in head.items()}, "model.33.cv2.3.0.conv.weight": t["model.24.cv2.2.0.conv.weight"]}
    if which == "anchors":
        return anchors
    if which == "old-focus":
        return {k: v for k, v in anchors.items() if k != "model.0.conv.weight"} | {"model.0.conv.conv.weight": np.zeros((16, 12, 3, 3), np.float32)}
    if which == "yolov3u":
        return {"model.0.conv.weight": np.zeros((32, 3, 3, 3), np.float32), "model.1.conv.weight": np.zeros((64, 32, 3, 3), np.float32),
                "model.2.cv1.conv.weight": np.zeros((32, 64, 1, 1), np.float32), "model.2.cv2.conv.weight": np.zeros((64, 32, 3, 3), np.float32),
                **{k.replace("model.22.", "model.28."): v for k, v in v8.items() if k.startswith("model.22.")},
                "model.28.dfl.conv.weight": t["model.24.dfl.conv.weight"]}
    if which == "seg":
        return {**t, "model.24.cv4.0.0.conv.weight": t["model.24.cv2.0.0.conv.weight"], "model.24.proto.cv1.conv.weight": np.zeros((64, 64, 3, 3), np.float32)}
    if which == "cls":
        return {**{k: v for k, v in body.items() if int(k.split(".")[1]) < 9}, "model.9.conv.conv.weight": np.zeros((1280, 256, 1, 1), np.float32),
                "model.9.linear.weight": np.zeros((4, 1280), np.float32)}
    raise ValueError(which)


def _rtdetr_layout(which):
    """test_yolov8_rtdetr.py's three layouts this build does not run"""
    if which == "rtdetr-x":
        return {k.replace("model.28.", "model.32.", 1): v for k, v in base("rtdetr-l").items()}
    if which == "resnet":
        return {k: v for k, v in base("rtdetr-l").items() if not k.startswith("model.0.")} | {"model.0.conv1.conv.weight": np.zeros((64, 3, 7, 7), np.float32)}
    return {k: v for k, v in base("yolov8-rtdetr-n").items() if not k.startswith("model.21.")}


_HEAD = {"yolov8": 22, "yolov8-p2": 28, "yolo11": 23, "yolov10": 23, "yolo26": 23, "yolo12": 21, "yolov5u": 24, "yolov9": 22}
_GENERIC = {"shape": "rows=model.1.conv.weight:24", "extra-weight": "add=model.3.extra.conv.weight:8x8x1x1", "past-head": "add=model.{past}.conv.weight:8x8x1x1;add=model.{past}.conv.bias:8",
            "cv4": "add=model.{head}.cv4.0.0.conv.weight:8x8x3x3", "proto": "add=model.{head}.proto.cv1.conv.weight:8x8x3x3",
            "stray-attn": "add=model.4.attn.qkv.conv.weight:8x8x1x1", "stray-attn-bias": "add=model.4.attn.qkv.conv.bias:8", "widen-24": "rows=model.0.conv.weight:24",
            "drop-stem": "drop=model.0."}
_MANY = "drop=model.23.cv2.;drop=model.23.cv3."


def _cases():
    """(case id, entry point, builder): every file the recognition fixture holds an answer for"""
    cases = [(b, "detector", functools.partial(base, b)) for b in DETECTORS]
    add = lambda cid, b, ops, entry="detector": cases.append((cid, entry, lambda: mutate(base(b), ops)))
    for b in ("yolov8-n", "yolov8-p2-n", "yolo11-n", "yolov10-n", "yolo26-n", "yolo12-n", "yolov5u-n", "yolov9-t"):
        head = _HEAD[b.rsplit("-", 1)[0]]
        for m, ops in _GENERIC.items():
            add(f"{b}/{m}", b, ops.format(head=head, past=head + 1))
    for b in ("yolov10-n", "yolov10-s", "yolo26-n"):       # the one-to-many pair: absent as a whole, or half of it
        add(f"{b}/one-to-one-only", b, _MANY)
        add(f"{b}/half-pair", b, "drop=model.23.cv3.")
        add(f"{b}/half-level", b, "drop=model.23.cv2.1.")
        add(f"{b}/one-to-one-only/shape", b, _MANY + ";" + _GENERIC["shape"])
    for c in (48, 64, 80):
        add(f"yolov10-n/widen-{c}", "yolov10-n", f"rows=model.0.conv.weight:{c}")
    add("yolov10-s/drop-m8", "yolov10-s", "drop=model.8.m.")
    add("yolov10-n/drop-o2o-cls", "yolov10-n", "drop=model.23.one2one_cv3.")
    add("yolov10-s/small-kernel", "yolov10-s", "add=model.8.m.0.cv1.2.conv.weight:128x1x3x3")
    add("yolo26-n/box-64", "yolo26-n", "rows=model.23.one2one_cv2.0.2.weight:64;rows=model.23.cv2.0.2.weight:64")
    add("yolo26-n/three-m22", "yolo26-n", "add=model.22.m.1.0.cv1.conv.weight:8x8x3x3;add=model.22.m.2.0.cv1.conv.weight:8x8x3x3")
    add("yolo26-n/no-attn-22", "yolo26-n", "drop=model.22.m.0.1.")
    add("yolo12-n/gamma", "yolo12-n", "add=model.6.gamma:128")
    add("yolo12-l/drop-gamma", "yolo12-l", "drop=model.8.gamma")
    add("yolo12-l/gamma-shape", "yolo12-l", "add=model.6.gamma:8")
    add("yolo12-n/plain-attn-6", "yolo12-n", "add=model.6.m.0.attn.qkv.conv.weight:8x8x1x1")
    add("yolo11-n/drop-sppf", "yolo11-n", "drop=model.9.")
    add("yolo11-n/psa-shape", "yolo11-n", "rows=model.10.m.0.attn.qkv.conv.weight:96")
    add("yolo11-n/box-rows", "yolo11-n", "rows=model.23.cv2.0.2.weight:32")
    add("yolo11-n/box-rows-4", "yolo11-n", "rows=model.23.cv2.0.2.weight:4")       # YOLO26's mark: refused in YOLO26's words
    add("yolo11-n/upsample-tensor", "yolo11-n", "add=model.11.conv.weight:8x8x1x1")
    add("yolo11-n/no-c3k-22", "yolo11-n", "drop=model.22.m.0.cv3.")
    add("yolo11-n/one2one", "yolo11-n", "add=model.23.one2one_cv3.0.2.weight:4x8x1x1")
    add("yolov9-t/drop-cv5", "yolov9-t", "drop=model.9.cv5.")
    add("yolov9-m/shape", "yolov9-m", "rows=model.2.cv4.conv.weight:64")
    add("yolov9-t/dfl", "yolov9-t", "add=model.22.dfl.conv.weight:1x16x1x1")
    add("yolov5u-n/drop-dfl", "yolov5u-n", "drop=model.24.dfl.")
    add("yolov8-n/dfl", "yolov8-n", "add=model.22.dfl.conv.weight:1x16x1x1")
    for w in ("p6", "anchors", "old-focus", "yolov3u", "seg", "cls"):
        cases.append((f"yolov5-lookalike/{w}", "detector", functools.partial(_v5_lookalike, w)))
    cases.append(("yolov5-lookalike/no-stem", "check_yolov5u", functools.partial(base, "yolov8-n")))
    for w in ("rtdetr-x", "resnet", "hybrid-without-trunk"):
        cases.append((f"rtdetr/{w}", "detector", functools.partial(_rtdetr_layout, w)))
    # the classifiers, through cls_family
    for b in ("v8cls", "11cls", "yolov8-n", "yolo11-n", "rtdetr-l"):
        add(f"cls/{b}", b, "", "cls_family")
    cases.append(("cls/yolo11-cut", "cls_family", lambda: {k: v for k, v in base("yolo11-n").items() if int(k.split(".")[1]) <= 10}))
    for b in ("v8cls", "11cls"):
        for m in ("shape", "extra-weight", "stray-attn-bias", "widen-24"):
            add(f"cls/{b}/{m}", b, _GENERIC[m], "cls_family")
        add(f"cls/{b}/drop-m2", b, "drop=model.2.m.", "cls_family")
        add(f"cls/{b}/no-head", b, "drop=model.9." if b == "v8cls" else "drop=model.10.", "cls_family")
    add("cls/v8cls/attn", "v8cls", "add=model.10.conv.weight:8x8x1x1", "cls_family")
    add("cls/11cls/widen-48", "11cls", "rows=model.0.conv.weight:48", "cls_family")
    add("cls/11cls/drop-cv2-8", "11cls", "drop=model.8.cv2.", "cls_family")
    add("cls/11cls/attn-7", "11cls", "add=model.7.attn.qkv.conv.bias:8", "cls_family")
    return cases


CASES = _cases()

# "function: which of its `raise` statements" -> refusing cases that reach it. Counted in weights.py by hand; the coverage test counts again.
RAISE_SITES = {
    "_strict_compare: the all-or-nothing group": ["yolov10-n/half-pair", "yolov10-s/half-level", "yolo26-n/half-pair"],
    "_strict_compare: a wanted name or shape": ["yolov10-n/shape", "yolo26-n/shape", "yolo12-l/drop-gamma", "yolov5u-n/shape", "yolov9-m/shape",
                                                "yolov9-t/drop-cv5", "cls/v8cls/shape", "cls/11cls/shape"],
    "_strict_compare: the walk over the file": ["yolov10-n/past-head", "yolo26-n/extra-weight", "yolo12-n/stray-attn-bias", "yolo12-n/gamma",
                                                "yolov5u-n/extra-weight", "yolov9-t/cv4", "cls/v8cls/extra-weight", "cls/11cls/attn-7"],
    "check_yolo11: a listed name is missing": ["yolo11-n/drop-sppf"],
    "check_yolo11: past the head, stray attention, another head branch": ["yolo11-n/past-head", "yolo11-n/stray-attn-bias", "yolo11-n/cv4"],
    "check_yolo11: tensors at an Upsample / Concat row": ["yolo11-n/upsample-tensor"],
    "check_yolo11: C2PSA's shapes": ["yolo11-n/psa-shape"],
    "check_yolo11: Detect's shapes": ["yolo11-n/box-rows"],
    "check_yolov10: a scale that is not implemented, by name": ["yolov10-n/widen-48", "yolov10-n/widen-64", "yolov10-n/widen-80"],
    "check_yolov10: no stem, another width, no one-to-one class branch": ["yolov10-n/drop-stem", "yolov10-n/widen-24", "yolov10-n/drop-o2o-cls"],
    "check_yolov10: a block row without members": ["yolov10-s/drop-m8"],
    "check_yolo26: no stem or no one-to-one class branch": ["yolo26-n/drop-stem"],
    "check_yolo26: reg_max": ["yolo26-n/box-64"],
    "check_yolo26: another width, model.22's repeats": ["yolo26-n/widen-24", "yolo26-n/three-m22"],
    "check_yolo12: no stem, another width": ["yolo12-n/drop-stem", "yolo12-n/widen-24"],
    "check_yolov5u: anchors": ["yolov5-lookalike/anchors", "yolov5-lookalike/old-focus"],
    "check_yolov5u: YOLOv3u": ["yolov5-lookalike/yolov3u"],
    "check_yolov5u: no 6x6 stem": ["yolov5-lookalike/no-stem"],
    "check_yolov5u: -seg": ["yolov5-lookalike/seg", "yolov5u-n/cv4", "yolov5u-n/proto"],
    "check_yolov5u: -cls": ["yolov5-lookalike/cls"],
    "check_yolov5u: P6": ["yolov5-lookalike/p6"],
    "check_yolov5u: no DFL, another width": ["yolov5u-n/drop-dfl", "yolov5u-n/widen-24"],
    "check_yolov9: no scale of these widths": ["yolov9-t/drop-stem", "yolov9-t/widen-24"],
    "detector_family: another RT-DETR layout": ["rtdetr/rtdetr-x", "rtdetr/resnet", "rtdetr/hybrid-without-trunk"],
    "is_yolov8_cls: a model.10": ["cls/v8cls/attn"],
    "is_yolov8_cls: a block row without members": ["cls/v8cls/drop-m2"],
    "is_yolo11_cls: another width": ["cls/11cls/widen-24", "cls/11cls/widen-48", "cls/11cls/drop-cv2-8"],
    "is_yolo11_cls: repeats, c3k or not": ["cls/yolo11-cut", "cls/11cls/drop-m2"],
}


def answer(entry, tensors):
    """What today's code says about a file, in the fixture's form: {"ok": ...} or {"raises": [type name, message]}"""
    from geotrax_amd import weights

    try:
        if entry == "detector":
            f = weights.detector_family(tensors)
            return {"ok": [f.graph, f.head, f.scale]}
        return {"ok": getattr(weights, entry)(tensors)}
    except Exception as e:                                 # noqa: BLE001 -- the type is part of what is compared
        return {"raises": [type(e).__name__, str(e)]}


def _golden(name):
    return json.loads((GOLDEN / f"family_{name}.json").read_text())


# ---------------------------------------------------------------------------------------------------------------------------- the tests
def test_every_spec_list_is_the_pinned_one():
    from test_weights_specs import COUNTS, DIGESTS

    pins = _golden("specs")
    assert set(pins) == {f"{fn}/{s}" for fn, scales in SPEC_SCALES.items() for s in scales}
    for fn, scales in SPEC_SCALES.items():
        for s in scales:
            assert spec_digest(fn, s) == pins[f"{fn}/{s}"], (fn, s)
    for fn, per_scale in DIGESTS.items():                  # the four families pinned before keep the digests they had
        for k, s in enumerate("nsmlx"):
            assert pins[f"{fn}/{s}"] == [COUNTS[fn][k], per_scale[s]], (fn, s)


@pytest.mark.parametrize("name", list(DRAWS))
def test_every_seeded_draw_is_the_pinned_one(name):
    assert draw_digest(base(name) if name in BASES else draw(name, DRAWS)) == _golden("draws")[name]


def test_recognition_and_refusals_are_the_pinned_ones():
    pins = _golden("recognition")
    assert set(pins) == {cid for cid, _, _ in CASES} and len(pins) == len(CASES)
    for cid, entry, build in CASES:
        assert answer(entry, build()) == pins[cid], cid


def test_every_family_and_refusal_site_has_a_refusing_case():
    """One refusing case at least per family's message, and per `raise` site (the module docstring maps sites to cases)."""
    from geotrax_amd import weights

    pins = _golden("recognition")
    refused = {cid: p["raises"] for cid, p in pins.items() if "raises" in p}
    assert all(kind == "NotImplementedError" for kind, _ in refused.values())
    said = " | ".join(msg for _, msg in refused.values())
    for f in weights.FAMILIES:
        if f.check is not None:
            assert f.topology in said, f.graph
    assert all(t in said for t in weights.RTDETR_TOPOLOGIES) and weights.YOLO11_CLS_TOPOLOGY in said and "yolov8{n,s,m,l,x}-cls" in said
    for site, cids in RAISE_SITES.items():
        assert cids and all(c in refused for c in cids), site
    # the number of `raise` statements per function, as the source has them
    src = inspect.getsource(weights)
    for fn in {s.split(":")[0] for s in RAISE_SITES}:
        body = src.split(f"\ndef {fn}(")[1].split("\ndef ")[0]
        assert len(re.findall(r"^\s+raise ", body, re.M)) == sum(s.split(":")[0] == fn for s in RAISE_SITES), fn
    # the by-name refusals, each with words of its own
    for cid, words in {"yolov10-n/widen-48": "yolov10m", "yolov10-n/widen-64": "yolov10b / yolov10l", "yolov10-n/widen-80": "yolov10x",
                       "yolo26-n/box-64": "reg_max = 16", "yolov5-lookalike/p6": "yolov5*6u", "yolov5-lookalike/anchors": "anchor-based",
                       "yolov5-lookalike/yolov3u": "YOLOv3u", "yolov5-lookalike/seg": "-seg", "yolov5-lookalike/cls": "-cls",
                       "yolov5-lookalike/no-stem": "without yolov5.yaml's 6x6 stem", "yolov9-t/drop-cv5": "yolov9e"}.items():
        assert words in refused[cid][1], cid


@pytest.mark.parametrize("name", DETECTORS)
def test_every_family_file_is_claimed_by_its_own_row_first(name):
    from geotrax_amd import weights

    t = base(name)
    first = next(f for f in weights.FAMILIES if f.claims(t))
    assert first.graph == weights.detector_family(t).graph == _golden("recognition")[name]["ok"][0]
    assert [f.graph for f in weights.FAMILIES][-1] == "yolov8" and weights.FAMILIES[-1].claims({})   # the default row claims everything


def _count_checks(monkeypatch):
    """Wraps every row's check with a counter; FAMILIES is replaced by the wrapped rows"""
    import dataclasses

    from geotrax_amd import weights

    calls = []

    def wrap(f):
        def counted(tensors, _check=f.check):
            calls.append(f.graph)
            return _check(tensors)
        return dataclasses.replace(f, check=counted) if f.check is not None else f

    monkeypatch.setattr(weights, "FAMILIES", tuple(wrap(f) for f in weights.FAMILIES))
    return calls


@pytest.mark.parametrize("name,yaml_file", [("yolov10-n", "yolov10n.yaml"), ("yolo26-n", "yolo26n.yaml"), ("yolo12-n", "yolo12n.yaml"),
                                            ("yolov5u-n", "yolov5n.yaml"), ("yolov9-t", "yolov9t.yaml"), ("yolo11-n", "yolo11.yaml")])
def test_a_model_object_checks_its_file_once(monkeypatch, name, yaml_file):
    from geotrax_amd.model import YOLO

    calls = _count_checks(monkeypatch)
    m = YOLO(base(name))
    assert calls == [name.rsplit("-", 1)[0]] and m.yaml_file == yaml_file and len(m.names) == 4


@pytest.mark.gpu
def test_a_detector_checks_its_file_once(monkeypatch, gtx_ctx):
    from geotrax_amd.detector import Detector

    calls = _count_checks(monkeypatch)
    det = Detector(base("yolov9-t"), (48, 64), imgsz=64, ctx=gtx_ctx)
    assert calls == ["yolov9"]
    out = det.detect(np.random.default_rng(0).integers(0, 256, (48, 64, 3), dtype=np.uint8))
    assert out.xyxy.shape == (len(out), 4) and calls == ["yolov9"]
    det.close()
