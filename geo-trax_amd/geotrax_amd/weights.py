"""Detector weights: flat tensor files and seeded synthetic weights.

The reference loads an ultralytics ``.pt`` (geotrax/extract.py:222, cfg extraction.model,
geotrax/cfg/default.yaml:81) -- a pickle of ultralytics classes that cannot be read without that
package. This build reads a flat ``.safetensors`` file with the model's ``state_dict`` names
instead (``tools/convert_weights.py`` writes one where ultralytics is installed). Conv+BN pairs
may be stored fused (``model.0.conv.weight/.bias``) or unfused (``.conv.weight`` +
``.bn.{weight,bias,running_mean,running_var}``); unfused pairs are folded here exactly like
ultralytics' ``fuse_conv_and_bn``.
"""
from __future__ import annotations

import re
from dataclasses import dataclass
from pathlib import Path
from typing import Callable, NamedTuple

import numpy as np

BN_EPS = 1e-3  # ultralytics sets BatchNorm2d.eps = 1e-3 at model build time

# yolov8.yaml scales: depth, width, max_channels
SCALES = {"n": (0.33, 0.25, 1024), "s": (0.33, 0.50, 1024), "m": (0.67, 0.75, 768),
          "l": (1.00, 1.00, 512), "x": (1.00, 1.25, 512)}


def fold_bn(tensors: dict[str, np.ndarray], eps: float = BN_EPS) -> dict[str, np.ndarray]:
    """Folds every ``X.bn.*`` into ``X.conv.{weight,bias}`` (fp64 arithmetic, fp32 result)."""
    out = {}
    for k, v in tensors.items():
        if ".bn." in k or k.endswith("num_batches_tracked"):
            continue
        out[k] = np.asarray(v, dtype=np.float32)
    for k in list(tensors):
        if not k.endswith(".bn.weight"):
            continue
        pfx = k[: -len(".bn.weight")]
        g = tensors[pfx + ".bn.weight"].astype(np.float64)
        b = tensors[pfx + ".bn.bias"].astype(np.float64)
        m = tensors[pfx + ".bn.running_mean"].astype(np.float64)
        var = tensors[pfx + ".bn.running_var"].astype(np.float64)
        w = tensors[pfx + ".conv.weight"].astype(np.float64)
        s = g / np.sqrt(var + eps)
        out[pfx + ".conv.weight"] = (w * s[:, None, None, None]).astype(np.float32)
        cb = tensors.get(pfx + ".conv.bias")
        cb = np.zeros_like(m) if cb is None else cb.astype(np.float64)
        out[pfx + ".conv.bias"] = ((cb - m) * s + b).astype(np.float32)
    return out


def load_weights(path: str | Path) -> dict[str, np.ndarray]:
    from safetensors.numpy import load_file

    t = load_file(str(path))
    t = {k: np.asarray(v, dtype=np.float32) for k, v in t.items()}
    t = fold_bn(t)
    if any(".one2one_cv2." in k for k in t):               # a YOLOv10 file stored unfused: its RepVGGDW pairs become the fused model's one 7x7
        t = fold_repvggdw(t)
    if is_rtdetr(t):
        t = fold_input_proj(fuse_repconv(t))
    elif any(_V9_REPCONV.fullmatch(k) for k in t):         # a YOLOv9 file stored unfused: RepBottleneck's RepConv pairs, BN already folded per branch
        t = fuse_repconv(t)
    return t


_V9_REPCONV = re.compile(r"model\.\d+\.cv[23]\.0\.m\.\d+\.cv1\.conv1\.conv\.weight")   # RepNCSPELAN4 -> RepCSP -> RepBottleneck -> RepConv's 3x3 branch


def save_weights(tensors: dict[str, np.ndarray], path: str | Path) -> None:
    from safetensors.numpy import save_file

    save_file({k: np.ascontiguousarray(v, dtype=np.float32) for k, v in tensors.items()}, str(path))


def _make_divisible(x: float, d: int = 8) -> int:
    return int(np.ceil(x / d) * d)


# --------------------------------------------------------------------------- the model yamls, as tables
# One row per yaml layer, written as the yaml writes it: (from, repeats, module, args). A new family is one more table here (and
# one in csrc/yolo_trunk.cpp); _parse_model() turns a table into the spec list every function below returns.
_UP = (-1, 1, "Upsample", (None, 2, "nearest"))
_V8_BACKBONE = [                                           # model.0-8 of yolov8.yaml, yolov8-p2.yaml and yolov8-cls.yaml
    (-1, 1, "Conv", (64, 3, 2)),
    (-1, 1, "Conv", (128, 3, 2)),
    (-1, 3, "C2f", (128, True)),
    (-1, 1, "Conv", (256, 3, 2)),
    (-1, 6, "C2f", (256, True)),
    (-1, 1, "Conv", (512, 3, 2)),
    (-1, 6, "C2f", (512, True)),
    (-1, 1, "Conv", (1024, 3, 2)),
    (-1, 3, "C2f", (1024, True)),
]
YOLOV8_YAML = _V8_BACKBONE + [
    (-1, 1, "SPPF", (1024, 5)),                            # 9
    _UP,
    ((-1, 6), 1, "Concat", (1,)),
    (-1, 3, "C2f", (512,)),                                # 12
    _UP,
    ((-1, 4), 1, "Concat", (1,)),
    (-1, 3, "C2f", (256,)),                                # 15
    (-1, 1, "Conv", (256, 3, 2)),
    ((-1, 12), 1, "Concat", (1,)),
    (-1, 3, "C2f", (512,)),                                # 18
    (-1, 1, "Conv", (512, 3, 2)),
    ((-1, 9), 1, "Concat", (1,)),
    (-1, 3, "C2f", (1024,)),                               # 21
    ((15, 18, 21), 1, "Detect", ("nc",)),                  # 22
]
YOLOV8_P2_YAML = _V8_BACKBONE + [
    (-1, 1, "SPPF", (1024, 5)),                            # 9
    _UP,
    ((-1, 6), 1, "Concat", (1,)),
    (-1, 3, "C2f", (512,)),                                # 12
    _UP,
    ((-1, 4), 1, "Concat", (1,)),
    (-1, 3, "C2f", (256,)),                                # 15
    _UP,
    ((-1, 2), 1, "Concat", (1,)),
    (-1, 3, "C2f", (128,)),                                # 18
    (-1, 1, "Conv", (128, 3, 2)),
    ((-1, 15), 1, "Concat", (1,)),
    (-1, 3, "C2f", (256,)),                                # 21
    (-1, 1, "Conv", (256, 3, 2)),
    ((-1, 12), 1, "Concat", (1,)),
    (-1, 3, "C2f", (512,)),                                # 24
    (-1, 1, "Conv", (512, 3, 2)),
    ((-1, 9), 1, "Concat", (1,)),
    (-1, 3, "C2f", (1024,)),                               # 27
    ((18, 21, 24, 27), 1, "Detect", ("nc",)),              # 28
]
YOLO11_YAML = [
    (-1, 1, "Conv", (64, 3, 2)),
    (-1, 1, "Conv", (128, 3, 2)),
    (-1, 2, "C3k2", (256, False, 0.25)),
    (-1, 1, "Conv", (256, 3, 2)),
    (-1, 2, "C3k2", (512, False, 0.25)),
    (-1, 1, "Conv", (512, 3, 2)),
    (-1, 2, "C3k2", (512, True)),
    (-1, 1, "Conv", (1024, 3, 2)),
    (-1, 2, "C3k2", (1024, True)),
    (-1, 1, "SPPF", (1024, 5)),                            # 9
    (-1, 2, "C2PSA", (1024,)),                             # 10
    _UP,
    ((-1, 6), 1, "Concat", (1,)),
    (-1, 2, "C3k2", (512, False)),                         # 13
    _UP,
    ((-1, 4), 1, "Concat", (1,)),
    (-1, 2, "C3k2", (256, False)),                         # 16
    (-1, 1, "Conv", (256, 3, 2)),
    ((-1, 13), 1, "Concat", (1,)),
    (-1, 2, "C3k2", (512, False)),                         # 19
    (-1, 1, "Conv", (512, 3, 2)),
    ((-1, 10), 1, "Concat", (1,)),
    (-1, 2, "C3k2", (1024, True)),                         # 22
    ((16, 19, 22), 1, "Detect", ("nc",)),                  # 23: the class branch is DWConv + Conv(1x1) twice
]
YOLOV10_YAML = [                                           # v10/yolov10s.yaml; yolov10n.yaml has a C2f at row 8 (_yolov10_table)
    (-1, 1, "Conv", (64, 3, 2)),
    (-1, 1, "Conv", (128, 3, 2)),
    (-1, 3, "C2f", (128, True)),
    (-1, 1, "Conv", (256, 3, 2)),
    (-1, 6, "C2f", (256, True)),
    (-1, 1, "SCDown", (512, 3, 2)),
    (-1, 6, "C2f", (512, True)),
    (-1, 1, "SCDown", (1024, 3, 2)),
    (-1, 3, "C2fCIB", (1024, True, True)),                 # 8: (c2, shortcut, lk)
    (-1, 1, "SPPF", (1024, 5)),                            # 9
    (-1, 1, "PSA", (1024,)),                               # 10
    _UP,
    ((-1, 6), 1, "Concat", (1,)),
    (-1, 3, "C2f", (512,)),                                # 13
    _UP,
    ((-1, 4), 1, "Concat", (1,)),
    (-1, 3, "C2f", (256,)),                                # 16
    (-1, 1, "Conv", (256, 3, 2)),
    ((-1, 13), 1, "Concat", (1,)),
    (-1, 3, "C2f", (512,)),                                # 19
    (-1, 1, "SCDown", (512, 3, 2)),
    ((-1, 10), 1, "Concat", (1,)),
    (-1, 3, "C2fCIB", (1024, True, True)),                 # 22
    ((16, 19, 22), 1, "v10Detect", ("nc",)),               # 23: YOLO11's Detect layers twice (cv2 / cv3, one2one_cv2 / one2one_cv3)
]
YOLO26_YAML = YOLO11_YAML[:9] + [                          # 26/yolo26.yaml (end2end: True, reg_max: 1): yolo11.yaml's rows but for 9, 22 and 23
    (-1, 1, "SPPF", (1024, 5, 3, True)),                   # 9: (c2, k, n, shortcut): cv1 without activation, the input added to cv2's output
] + YOLO11_YAML[10:22] + [
    (-1, 1, "C3k2", (1024, True, 0.5, True)),              # 22: (c2, c3k, e, attn): every m.{k} is Sequential(Bottleneck, PSABlock)
    ((16, 19, 22), 1, "Detect26", ("nc",)),                # 23: Detect with reg_max = 1 (a 4-output box 1x1) and a one-to-one copy of both branches
]
YOLO12_YAML = YOLO11_YAML[:6] + [                          # 12/yolo12.yaml: 22 layers, no SPPF, no C2PSA
    (-1, 4, "A2C2f", (512, True, 4)),                      # 6: (c2, a2, area): members of two ABlocks, attention cut into 4 horizontal bands
    (-1, 1, "Conv", (1024, 3, 2)),
    (-1, 4, "A2C2f", (1024, True, 1)),                     # 8: attention over the whole map
    _UP,
    ((-1, 6), 1, "Concat", (1,)),
    (-1, 2, "A2C2f", (512, False, -1)),                    # 11: a2 off: every member is a C3k
    _UP,
    ((-1, 4), 1, "Concat", (1,)),
    (-1, 2, "A2C2f", (256, False, -1)),                    # 14
    (-1, 1, "Conv", (256, 3, 2)),
    ((-1, 11), 1, "Concat", (1,)),
    (-1, 2, "A2C2f", (512, False, -1)),                    # 17
    (-1, 1, "Conv", (512, 3, 2)),
    ((-1, 8), 1, "Concat", (1,)),
    (-1, 2, "C3k2", (1024, True)),                         # 20
    ((14, 17, 20), 1, "Detect", ("nc",)),                  # 21: YOLO11's Detect
]
YOLOV5_YAML = [                                            # v5/yolov5.yaml, what the yolov5{n,s,m,l,x}u files are built from: 25 layers
    (-1, 1, "Conv", (64, 6, 2, 2)),                        # 0: (c2, k, s, p): the 6x6 stem
    (-1, 1, "Conv", (128, 3, 2)),
    (-1, 3, "C3", (128,)),
    (-1, 1, "Conv", (256, 3, 2)),
    (-1, 6, "C3", (256,)),
    (-1, 1, "Conv", (512, 3, 2)),
    (-1, 9, "C3", (512,)),
    (-1, 1, "Conv", (1024, 3, 2)),
    (-1, 3, "C3", (1024,)),
    (-1, 1, "SPPF", (1024, 5)),                            # 9
    (-1, 1, "Conv", (512, 1, 1)),                          # 10: 1x1, stride 1
    _UP,
    ((-1, 6), 1, "Concat", (1,)),
    (-1, 3, "C3", (512, False)),                           # 13
    (-1, 1, "Conv", (256, 1, 1)),                          # 14
    _UP,
    ((-1, 4), 1, "Concat", (1,)),
    (-1, 3, "C3", (256, False)),                           # 17
    (-1, 1, "Conv", (256, 3, 2)),
    ((-1, 14), 1, "Concat", (1,)),
    (-1, 3, "C3", (512, False)),                           # 20
    (-1, 1, "Conv", (512, 3, 2)),
    ((-1, 10), 1, "Concat", (1,)),
    (-1, 3, "C3", (1024, False)),                          # 23
    ((17, 20, 23), 1, "Detect", ("nc",)),                  # 24: YOLOv8's Detect
]
YOLOV8_CLS_YAML = _V8_BACKBONE + [(-1, 1, "Classify", ("nc",))]
YOLO11_CLS_YAML = YOLO11_YAML[:9] + [                      # model.0-8 of yolo11.yaml; no SPPF
    (-1, 2, "C2PSA", (1024,)),                             # 9
    (-1, 1, "Classify", ("nc",)),                          # 10
]


def _rows(table, *modules) -> tuple[int, ...]:
    """The layer indices of a table's rows of the given modules."""
    return tuple(i for i, r in enumerate(table) if r[2] in modules)


def _parse_model(table, nc, ch, rep, c3k_all=False, dw_cls=False, a2_residual=False, gammas=None) -> list[tuple[str, tuple[int, ...], bool]]:
    """ultralytics' parse_model over one table: (tensor name, shape, has_act) of every conv of the fused model, in module order.
    ch(c): a yaml width as built; rep(i, n): the repeats of layer i as built; c3k_all: every C3k2 holds C3k blocks (yolo11 m / l / x);
    dw_cls: Detect's class branch is DWConv + Conv(1x1) twice (yolo11.yaml); a2_residual: parse_model's extra A2C2f arguments of
    yolo12 l / x (residual = True, mlp_ratio = 1.2), the `gamma` vectors of which -- no convs -- are appended to `gammas` as (name, (c2,))."""
    specs: list[tuple[str, tuple[int, ...], bool]] = []
    out: list[int] = []                                    # output channels per layer

    def conv(name, cin, cout, k, act=True):
        specs.append((name, (cout, cin, k, k), act))

    def dwconv(name, c, act, k=3):
        specs.append((name, (c, 1, k, k), act))

    def bottleneck(p, c, e):
        conv(p + ".cv1.conv", c, int(c * e), 3)
        conv(p + ".cv2.conv", int(c * e), c, 3)

    def psablock(m, c):
        """PSABlock(c, attn_ratio 0.5, num_heads = c / 64): key_dim 32, head_dim 64"""
        conv(m + ".attn.qkv.conv", c, c + 2 * (c // 64) * 32, 1, act=False)
        conv(m + ".attn.proj.conv", c, c, 1, act=False)
        dwconv(m + ".attn.pe.conv", c, False)
        conv(m + ".ffn.0.conv", c, 2 * c, 1)
        conv(m + ".ffn.1.conv", 2 * c, c, 1, act=False)

    def c2f(pfx, cin, cout, n, c3k=None, e=0.5, cib=None, attn=False):
        """C2f (c3k None: full-width Bottlenecks) or C3k2 (half-width Bottlenecks, or C3k blocks of two Bottlenecks when c3k) or
        C2fCIB (cib = lk: CIB blocks of full hidden width; lk: the middle depthwise layer is the fused RepVGGDW, one 7x7) or
        yolo26.yaml's C3k2 with attn: every m.{k} is Sequential(Bottleneck(c, c, e = 0.5), PSABlock(c))."""
        c = int(cout * e)
        conv(f"{pfx}.cv1.conv", cin, 2 * c, 1)
        for k in range(n):
            m = f"{pfx}.m.{k}"
            if attn:
                bottleneck(m + ".0", c, 0.5)
                psablock(m + ".1", c)
            elif cib is not None:                            # CIB(c, c, shortcut, e=1.0, lk): dw3 -> 1x1 c->2c -> dw3 / dw7 -> 1x1 2c->c -> dw3, SiLU after each
                dwconv(m + ".cv1.0.conv", c, True)
                conv(m + ".cv1.1.conv", c, 2 * c, 1)
                dwconv(m + ".cv1.2.conv", 2 * c, True, 7 if cib else 3)
                conv(m + ".cv1.3.conv", 2 * c, c, 1)
                dwconv(m + ".cv1.4.conv", c, True)
            elif c3k:
                c3k_block(m, c, c)
            else:
                bottleneck(m, c, 1.0 if c3k is None else 0.5)
        conv(f"{pfx}.cv2.conv", (2 + n) * c, cout, 1)

    def c3k_block(m, cin, c, n=2):
        """C3k(cin, c, n): cv1 / cv2 to half the width, n full-width Bottlenecks behind cv1, cv3 on the two. RepCSP(cin, c, n) is the same
        list: its RepBottlenecks of e = 1.0 are the fused RepConv (one 3x3), then a Conv3x3"""
        h = int(c * 0.5)
        conv(m + ".cv1.conv", cin, h, 1)
        conv(m + ".cv2.conv", cin, h, 1)
        conv(m + ".cv3.conv", 2 * h, c, 1)
        for j in range(n):
            bottleneck(f"{m}.m.{j}", h, 1.0)

    def c3_block(pfx, cin, cout, n):
        """C3(c1, c2, n, shortcut, e = 0.5) of yolov5.yaml: cv1 / cv2 1x1 to c_ = c2 / 2, both on the input, cv3 1x1 on the two, then n
        Bottleneck(c_, c_, k = (1x1, 3x3), e = 1.0) behind cv1 -- in the module's own order"""
        c = int(cout * 0.5)
        conv(pfx + ".cv1.conv", cin, c, 1)
        conv(pfx + ".cv2.conv", cin, c, 1)
        conv(pfx + ".cv3.conv", 2 * c, cout, 1)
        for k in range(n):
            conv(f"{pfx}.m.{k}.cv1.conv", c, c, 1)
            conv(f"{pfx}.m.{k}.cv2.conv", c, c, 3)

    def ablock(m, c, mlp_ratio):
        """ABlock(c, heads = c / 32, mlp_ratio, area): AAttn's qkv / proj / pe (depthwise 7x7), none with an activation, then the two-conv mlp"""
        conv(m + ".attn.qkv.conv", c, 3 * c, 1, act=False)
        conv(m + ".attn.proj.conv", c, c, 1, act=False)
        dwconv(m + ".attn.pe.conv", c, False, 7)
        conv(m + ".mlp.0.conv", c, int(c * mlp_ratio), 1)
        conv(m + ".mlp.1.conv", int(c * mlp_ratio), c, 1, act=False)

    def detect(d, chans, box="cv2", cls="cv3", reg_max=16):
        cb = max(16, chans[0] // 4, YOLO26_BOX_FLOOR if reg_max == 1 else 4 * reg_max)
        cc = max(chans[0], min(nc, 100))
        for l, cin in enumerate(chans):
            conv(f"{d}.{box}.{l}.0.conv", cin, cb, 3)
            conv(f"{d}.{box}.{l}.1.conv", cb, cb, 3)
            specs.append((f"{d}.{box}.{l}.2", (4 * reg_max, cb, 1, 1), False))
            if dw_cls:
                dwconv(f"{d}.{cls}.{l}.0.0.conv", cin, True)
                conv(f"{d}.{cls}.{l}.0.1.conv", cin, cc, 1)
                dwconv(f"{d}.{cls}.{l}.1.0.conv", cc, True)
                conv(f"{d}.{cls}.{l}.1.1.conv", cc, cc, 1)
            else:
                conv(f"{d}.{cls}.{l}.0.conv", cin, cc, 3)
                conv(f"{d}.{cls}.{l}.1.conv", cc, cc, 3)
            specs.append((f"{d}.{cls}.{l}.2", (nc, cc, 1, 1), False))

    for i, (frm, n, mod, args) in enumerate(table):
        src = [out[f if f >= 0 else i + f] for f in ((frm,) if isinstance(frm, int) else frm)] if i else [3]
        pfx, cin, n = f"model.{i}", src[0], rep(i, n)
        if mod == "Conv":
            out.append(ch(args[0]))
            conv(pfx + ".conv", cin, out[i], args[1])
        elif mod == "C2f":
            out.append(ch(args[0]))
            c2f(pfx, cin, out[i], n)
        elif mod == "C3":
            out.append(ch(args[0]))
            c3_block(pfx, cin, out[i], n)
        elif mod == "C3k2":
            out.append(ch(args[0]))
            c2f(pfx, cin, out[i], n, c3k_all or args[1], *args[2:3], attn=len(args) > 3 and bool(args[3]))
        elif mod == "SPPF":
            out.append(ch(args[0]))
            conv(pfx + ".cv1.conv", cin, cin // 2, 1, act=not (len(args) > 3 and args[3]))   # yolo26.yaml's SPPF(c2, k, n, shortcut): a linear cv1
            conv(pfx + ".cv2.conv", cin // 2 * 4, out[i], 1)
        elif mod == "C2PSA":                               # heads = c / 64, key_dim 32, head_dim 64
            out.append(ch(args[0]))
            c = cin // 2
            conv(pfx + ".cv1.conv", cin, 2 * c, 1)
            for k in range(n):
                psablock(f"{pfx}.m.{k}", c)
            conv(pfx + ".cv2.conv", 2 * c, out[i], 1)
        elif mod == "A2C2f":                               # (c2, a2, area): c_ = c2 / 2; cv1 -> c_, n members chained, cv2 on all 1 + n
            out.append(ch(args[0]))
            c = int(out[i] * 0.5)
            conv(pfx + ".cv1.conv", cin, c, 1)
            for k in range(n):
                if args[1]:
                    for j in range(2):
                        ablock(f"{pfx}.m.{k}.{j}", c, 1.2 if a2_residual else 2.0)
                else:
                    c3k_block(f"{pfx}.m.{k}", c, c)
            conv(pfx + ".cv2.conv", (1 + n) * c, out[i], 1)
            if args[1] and a2_residual and gammas is not None:
                gammas.append((pfx + ".gamma", (out[i],)))
        elif mod == "C2fCIB":
            out.append(ch(args[0]))
            c2f(pfx, cin, out[i], n, cib=bool(args[2]) if len(args) > 2 else False)
        elif mod == "SCDown":                              # cv1: 1x1 Conv + SiLU; cv2: depthwise 3x3 stride 2, no activation
            out.append(ch(args[0]))
            conv(pfx + ".cv1.conv", cin, out[i], 1)
            dwconv(pfx + ".cv2.conv", out[i], False)
        elif mod == "PSA":                                 # C2PSA's one block directly under the layer: heads = c / 64, key_dim 32
            out.append(ch(args[0]))
            c = cin // 2
            conv(pfx + ".cv1.conv", cin, 2 * c, 1)
            psablock(pfx, c)
            conv(pfx + ".cv2.conv", 2 * c, out[i], 1)
        elif mod in ("ELAN1", "RepNCSPELAN4"):            # (c2, c3, c4[, n]): cv1 -> two chunks; cv2 on the second, cv3 on cv2's; cv4 on all four
            c2, c3, c4 = args[:3]
            out.append(c2)
            conv(pfx + ".cv1.conv", cin, c3, 1)
            if mod == "ELAN1":
                conv(pfx + ".cv2.conv", c3 // 2, c4, 3)
                conv(pfx + ".cv3.conv", c4, c4, 3)
            else:
                c3k_block(pfx + ".cv2.0", c3 // 2, c4, args[3])
                conv(pfx + ".cv2.1.conv", c4, c4, 3)
                c3k_block(pfx + ".cv3.0", c4, c4, args[3])
                conv(pfx + ".cv3.1.conv", c4, c4, 3)
            conv(pfx + ".cv4.conv", c3 + 2 * c4, c2, 1)
        elif mod == "AConv":                               # avg_pool2d(2, 1), then Conv 3x3 stride 2
            out.append(args[0])
            conv(pfx + ".cv1.conv", cin, out[i], 3)
        elif mod == "ADown":                               # avg_pool2d(2, 1), chunk: Conv 3x3 stride 2 | max_pool2d(3, 2, 1) + Conv 1x1
            out.append(args[0])
            conv(pfx + ".cv1.conv", cin // 2, out[i] // 2, 3)
            conv(pfx + ".cv2.conv", cin // 2, out[i] // 2, 1)
        elif mod == "SPPELAN":                             # (c2, c3): cv1 1x1, three chained 5x5 max-pools, cv5 1x1 on the four
            out.append(args[0])
            conv(pfx + ".cv1.conv", cin, args[1], 1)
            conv(pfx + ".cv5.conv", 4 * args[1], out[i], 1)
        elif mod == "Upsample":
            out.append(cin)
        elif mod == "Concat":
            out.append(sum(src))
        elif mod == "Detect":
            out.append(0)
            detect(pfx, src)
        elif mod == "v10Detect":                           # the one-to-many pair, then its copy with weights of its own
            out.append(0)
            detect(pfx, src)
            detect(pfx, src, "one2one_cv2", "one2one_cv3")
        elif mod == "Detect26":                            # reg_max = 1; the one-to-many pair, then its one-to-one copy
            out.append(0)
            detect(pfx, src, reg_max=1)
            detect(pfx, src, "one2one_cv2", "one2one_cv3", reg_max=1)
        elif mod == "Classify":
            out.append(nc)
            conv(pfx + ".conv.conv", cin, 1280, 1)
            specs.append((pfx + ".linear", (nc, 1280), False))
        else:
            raise ValueError(f"model.{i}: module {mod}")
    return specs


def _scaled_specs(table, scales, scale, nc, reps={}, **kw):
    """_parse_model at one of the yaml's scales (depth, width, max_channels); reps: layer -> its repeats as built, where a file tells them."""
    depth, width, maxc = scales[scale]
    return _parse_model(table, nc, lambda c: _make_divisible(min(c, maxc) * width),
                        lambda i, n: reps[i] if i in reps else (max(round(n * depth), 1) if n > 1 else n), **kw)


def family_specs(graph: str, scale: str, nc: int = 4, table=None, **kw) -> list[tuple[str, tuple[int, ...], bool]]:
    """(tensor name, OIHW shape, has_act) for every conv of a fused detect model of FAMILIES' row `graph`, in module order. table: the
    family's yaml table as a check rebuilt it from a file; kw: _parse_model / _scaled_specs keywords that replace the row's own."""
    f = family_row(graph)
    if table is None:
        table = f.table(scale) if callable(f.table) else f.table
    if f.scales is None:                                   # YOLOv9: the tables carry their widths and repeats
        return _parse_model(table, nc, lambda c: c, lambda i, n: n)
    return _scaled_specs(table, f.scales, scale, nc, **(f.kw(scale) | kw))


def family_synthetic(graph: str, seed=0, nc: int = 4, scale: str = "s", **knobs) -> dict[str, np.ndarray]:
    """Seeded random fused weights of FAMILIES' row `graph`: synthetic_yolov8's draws (its docstring explains the knobs) in the order of
    family_specs. seed: an int, or the generator to go on drawing from."""
    return _draw_yolov8(np.random.default_rng(seed), family_specs(graph, scale, nc), **knobs)


def yolov8_layer_specs(scale: str = "s", nc: int = 4) -> list[tuple[str, tuple[int, ...], bool]]:
    """(tensor name, OIHW shape, has_act) for every conv of a fused YOLOv8 detect model."""
    return family_specs("yolov8", scale, nc)


def synthetic_yolov8(seed: int = 0, nc: int = 4, scale: str = "s", cls_bias: float = -4.0,
                     gain: float = 1.7, box_decay: float | tuple = 0.3, level_bias: tuple = (0.0, 0.0, 0.0),
                     box_weight_scale: float = 0.3, smooth_cls: bool | int = False) -> dict[str, np.ndarray]:
    """Seeded random fused weights of the YOLOv8 architecture (no checkpoint is reachable here).

    Conv weights ~ N(0, gain^2 / fan_in) so activations keep O(1) scale through the SiLU stack;
    biases ~ N(0, 0.05^2). ``cls_bias`` shifts the class logits so that only a few percent of the
    anchors clear the confidence threshold, which is the load the decode/NMS stage sees on real
    footage. The box branch's final bias decays over the 16 DFL bins
    (-box_decay * bin) and its weights are damped, so decoded boxes span about six strides per
    side -- localised boxes instead of the frame-filling ones uniform DFL logits give. In practice the random
    stack's activations grow with depth (class logits of O(200) at the coarse heads, DFL logits that swamp the
    decaying bias), so with the defaults the strongest anchors sit on the stride-32 head and the boxes come out
    400-700 px wide in a 4K frame, each overlapping ~30 others. The two knobs below put the post-processing in
    the regime of drone footage: ``level_bias`` is added to the class logits of the stride-8/16/32 heads
    ((0, -1e4, -1e4): only stride-8 anchors can fire) and ``box_weight_scale`` scales the last box conv's weights
    (0.002: the decaying bias decides, every side is ~2.9 bins -> boxes of ~46 network pixels, ~90 px in 4K, few
    of which overlap). ``box_decay`` may be a 4-tuple (left, top, right, bottom) for non-square boxes.
    ``smooth_cls`` makes the two 3x3 convs of every class branch and those of the stride-8 neck stage (model.15)
    tap-uniform (each output channel applies one random channel mix to the 3x3 box mean of its input): class logits
    then vary smoothly over neighbouring anchors, so the
    anchors that clear the confidence threshold come in clusters of several per object and NMS has boxes to
    suppress -- the load SURVEY.md 8d.2 asks for (1-3 k candidates in ~132 clusters) instead of isolated ones."""
    return family_synthetic("yolov8", seed, nc, scale, cls_bias=cls_bias, gain=gain, box_decay=box_decay, level_bias=level_bias,
                            box_weight_scale=box_weight_scale, smooth_cls=smooth_cls)


def _draw_yolov8(rng, specs, cls_bias: float = -4.0, gain: float = 1.7, box_decay: float | tuple = 0.3, level_bias: tuple = (0.0, 0.0, 0.0),
                 box_weight_scale: float = 0.3, smooth_cls: bool | int = False) -> dict[str, np.ndarray]:
    """synthetic_yolov8's draws, layer by layer in spec order from `rng` (synthetic_yolov8_rtdetr draws its trunk with it)."""
    decay = np.broadcast_to(np.asarray(box_decay, dtype=np.float64), (4,))
    t: dict[str, np.ndarray] = {}
    for name, shape, has_act in specs:
        fan_in = int(np.prod(shape[1:]))
        g = gain if has_act else 1.0
        t[name + ".weight"] = (rng.standard_normal(shape) * (g / np.sqrt(fan_in))).astype(np.float32)
        if smooth_cls and shape[2] == 3 and (".cv3." in name or name.startswith("model.15.m.") or
                                             (int(smooth_cls) >= 2 and name.startswith("model.12.m."))):   # 2: the stride-16 neck stage too (twice the radius at stride 8)
            mix = t[name + ".weight"][:, :, 1:2, 1:2] * np.float32(np.sqrt(shape[2] * shape[3]))   # keeps the output variance for smooth inputs
            t[name + ".weight"] = np.broadcast_to(mix / np.float32(shape[2] * shape[3]), shape).astype(np.float32).copy()
        b = rng.standard_normal(shape[0]) * 0.05
        last = re.fullmatch(r"model\.\d+\.(?:one2one_)?cv([23])\.(\d+)\.2", name)   # Detect's closing 1x1 of the box (cv2) / class (cv3) branch of level l (v10Detect: of either pair)
        if last and last.group(1) == "3":
            b = b + cls_bias + float(level_bias[int(last.group(2))])
        if last and last.group(1) == "2":
            t[name + ".weight"] *= np.float32(box_weight_scale)
            if shape[0] == 4:                              # reg_max = 1 (YOLO26): the four outputs are the distances themselves, in strides
                b = b + np.asarray(YOLO26_BOX_BIAS)
            else:
                b = b - np.repeat(decay, 16) * np.tile(np.arange(16), 4)
        t[name + ".bias"] = b.astype(np.float32)
    return t


# --------------------------------------------------------------------------- what every family's check shares
def _layer(k: str) -> int:
    """The N of a `model.N.*` name, -1 for any other"""
    p = k.split(".")
    return int(p[1]) if p[0] == "model" and len(p) > 1 and p[1].isdigit() else -1


def _shape(tensors: dict, name: str) -> tuple | None:
    return tuple(np.shape(tensors[name])) if name in tensors else None


_ONE2MANY = ("model.23.cv2.", "model.23.cv3.")             # v10Detect's / Detect26's one-to-many pair: ultralytics' fuse() drops it as a whole


def _strict_compare(want, tensors: dict, head: int, exc: Exception, ignore=("dfl",), group=(), extra=(), attn=()) -> None:
    """The strict comparison of a file with a family's specs; raises `exc` unless all of this holds. Every name of `want` ((name, shape,
    ...) per conv) is there as `name.weight` with exactly that shape, and so is every (name, shape) of `extra` (YOLO12's gammas); no
    other `.weight` or `.gamma` stands at layers 0 .. head; nothing at all stands past the head row; `.attn.` stands at the layers
    `attn` only. The head row's modules `ignore` (Detect's constant `dfl`; None: the whole row, a classifier's unread Classify) are not
    looked at, and the wanted names that start with one of `group` are there as a whole or missing as a whole."""
    want = [(n, s) for n, s, *_ in want]
    if group:
        have = [n + ".weight" in tensors for n, _ in want if n.startswith(group)]
        if any(have) and not all(have):
            raise exc
        if not any(have):
            want = [(n, s) for n, s in want if not n.startswith(group)]
    specs = {n + ".weight": s for n, s in want} | dict(extra)
    if any(_shape(tensors, n) != s for n, s in specs.items()):
        raise exc
    for k in tensors:
        i = _layer(k)
        if i < 0 or (i == head and (ignore is None or k.split(".")[2] in ignore)):
            continue
        if i > head or (".attn." in k and i not in attn) or (k.endswith((".weight", ".gamma")) and k not in specs):
            raise exc


def _compare_family(graph: str, want, tensors: dict, exc: Exception, **kw) -> None:
    """_strict_compare with the head row and the attention layers of FAMILIES' row `graph`"""
    f = family_row(graph)
    _strict_compare(want, tensors, _layer(f.head + "."), exc, attn=f.attn, **kw)


def _scale_of_yolo11_widths(tensors: dict) -> str | None:
    """The scale letter of a file built on yolo11.yaml's scales (YOLO26 and YOLO12 share them), None for another width: model.0's width
    tells n / s / x apart; m and l share every width and differ in the repeats (model.2: 1 or 2 blocks)"""
    c0 = _shape(tensors, "model.0.conv.weight")
    return {16: "n", 32: "s", 96: "x", 64: "l" if "model.2.m.1.cv1.conv.weight" in tensors else "m"}.get(c0[0]) if c0 else None


def _c3k_off_tensors(table, tensors: dict):
    """The table with every plain C3k2 row's c3k flag read off the tensors (a C3k has `m.0.cv3`), not off a remembered rule"""
    return [(f, n, m, (a[0], f"model.{i}.m.0.cv3.conv.weight" in tensors) + tuple(a[2:])) if m == "C3k2" and len(a) < 4 else (f, n, m, a)
            for i, (f, n, m, a) in enumerate(table)]


# --------------------------------------------------------------------------- YOLOv8-P2 (yolov8-p2.yaml)
# geo-trax's train.sh `-p`: the backbone of yolov8.yaml, a neck that goes one Upsample + Concat(model.2) + C2f further down to
# stride 4 (model.16-18) and back up (model.19-27), and Detect = model.28 on [18, 21, 24, 27] (strides 4 / 8 / 16 / 32). The Detect
# widths follow its finest input: cb = max(16, c18 // 4, 64), cc = max(c18, min(nc, 100)).

def is_yolov8_p2(tensors: dict) -> bool:
    return "model.28.cv2.0.0.conv.weight" in tensors


def yolov8_p2_layer_specs(scale: str = "s", nc: int = 4) -> list[tuple[str, tuple[int, ...], bool]]:
    """(tensor name, OIHW shape, has_act) for every conv of a fused YOLOv8-P2 detect model."""
    return family_specs("yolov8-p2", scale, nc)


def synthetic_yolov8_p2(seed: int = 0, nc: int = 4, scale: str = "s", cls_bias: float = -4.0, gain: float = 1.7,
                        box_decay: float | tuple = 0.3, level_bias: tuple = (0.0, 0.0, -1e4, -1e4),
                        box_weight_scale: float = 0.3) -> dict[str, np.ndarray]:
    """Seeded random fused weights of the YOLOv8-P2 architecture, drawn like synthetic_yolov8's (same knobs, same order of draws
    over yolov8_p2_layer_specs). ``level_bias`` is added to the class logits of the stride-4/8/16/32 heads; the default silences the
    two coarse heads, whose random logits otherwise dominate, so that the stride-4 and stride-8 anchors are the ones that fire."""
    return family_synthetic("yolov8-p2", seed, nc, scale, cls_bias=cls_bias, gain=gain, box_decay=box_decay, level_bias=level_bias, box_weight_scale=box_weight_scale)


# --------------------------------------------------------------------------- YOLO11 (cfg/models/11/yolo11.yaml)
# What `YOLO("yolo11s.pt")` fine-tunes to under the reference's ultralytics: Conv / C3k2 backbone (model.0-8), SPPF (9), C2PSA (10:
# position-sensitive attention), a neck of C3k2 blocks (13 / 16 / 19 / 22) and Detect = model.23 on [16, 19, 22] whose class branch
# is DWConv + Conv(1x1) twice. C3k2 is C2f with half-width Bottlenecks (c3k=False) or C3k blocks (c3k=True: 6 / 8 / 22 for n and s,
# everywhere for m / l / x) as m.{k}. Restated from ultralytics' public source; not checked against the package (it is not installed).

YOLO11_SCALES = {"n": (0.50, 0.25, 1024), "s": (0.50, 0.50, 1024), "m": (0.50, 1.00, 512),
                 "l": (1.00, 1.00, 512), "x": (1.00, 1.50, 512)}   # yolo11.yaml: depth, width, max_channels

YOLO11_TOPOLOGY = "yolo11 detect (yolo11{n,s,m,l,x}: C3k2 backbone + neck, C2PSA = model.10, Detect = model.23 on model.16 / 19 / 22)"


def has_yolo11_blocks(tensors: dict) -> bool:
    """True when the names hold what no YOLOv8 file has: an attention block (`.attn.`) or a Detect class branch that starts with a
    DWConv + Conv pair (`model.<k>.cv3.0.0.0.conv`). Which graph it is, and whether this build runs it: check_yolo11()."""
    for k in tensors:
        if ".attn." in k:
            return True
        p = k.split(".")
        if len(p) >= 8 and p[0] == "model" and p[2] == "cv3" and p[4:7] == ["0", "0", "conv"]:
            return True
    return False


def check_yolo11(tensors: dict) -> None:
    """Raises NotImplementedError unless the names and shapes are those of a fused yolo11.yaml detect model. Other graphs built from
    the same blocks (YOLO12's A2C2f when is_yolo12() does not claim the file, yolo11-cls with C2PSA at model.9 -- the ReID embedder's, is_yolo11_cls --, -seg / -obb / -pose heads with a
    cv4 or proto branch) are never built into the wrong network."""
    # Not _strict_compare: this test is weaker -- a hand-listed subset of the names, a few shapes -- and stays as it is, because the strict
    # one would refuse files that load today (tests/test_families.py pins one: a model.22 without C3k members).
    no = NotImplementedError(f"checkpoint with attention / depthwise-Detect blocks in another arrangement than yolo11.yaml's: of that "
                             f"family only {YOLO11_TOPOLOGY} is implemented")
    shape = lambda n: tuple(np.shape(tensors[n])) if n in tensors else None
    need = [f"model.{i}.conv.weight" for i in _rows(YOLO11_YAML, "Conv")]
    need += [f"model.{i}.{c}.conv.weight" for i in _rows(YOLO11_YAML, "C3k2") for c in ("cv1", "cv2", "m.0.cv1", "m.0.cv2")]
    need += ["model.9.cv1.conv.weight", "model.9.cv2.conv.weight", "model.10.cv1.conv.weight", "model.10.cv2.conv.weight"]
    need += [f"model.10.m.0.{c}.conv.weight" for c in ("attn.qkv", "attn.proj", "attn.pe", "ffn.0", "ffn.1")]
    for l in range(3):
        need += [f"model.23.cv2.{l}.0.conv.weight", f"model.23.cv2.{l}.1.conv.weight", f"model.23.cv2.{l}.2.weight",
                 f"model.23.cv3.{l}.0.0.conv.weight", f"model.23.cv3.{l}.0.1.conv.weight", f"model.23.cv3.{l}.1.0.conv.weight",
                 f"model.23.cv3.{l}.1.1.conv.weight", f"model.23.cv3.{l}.2.weight"]
    if any(n not in tensors for n in need):
        raise no
    for k in tensors:
        p = k.split(".")
        if p[0] != "model" or len(p) < 3 or not p[1].isdigit():
            continue
        i = int(p[1])
        if i > 23 or (".attn." in k and i != 10) or (i == 23 and (p[2] not in ("cv2", "cv3", "dfl") or (p[2] in ("cv2", "cv3") and p[3] not in "012"))):
            raise no
        if i in _rows(YOLO11_YAML, "Upsample", "Concat"):  # no tensors
            raise no
    c = shape("model.10.cv1.conv.weight")[0] // 2
    if c % 64 or shape("model.10.m.0.attn.qkv.conv.weight") != (2 * c, c, 1, 1) or shape("model.10.m.0.attn.pe.conv.weight") != (c, 1, 3, 3):
        raise no                                           # heads = c / 64, key_dim 32 (attn_ratio 0.5), head_dim 64
    if shape("model.23.cv2.0.2.weight")[0] != 64 or shape("model.23.cv3.0.0.0.conv.weight")[1] != 1 or shape("model.23.cv3.0.1.0.conv.weight")[1] != 1:
        raise no


def yolo11_layer_specs(scale: str = "s", nc: int = 4) -> list[tuple[str, tuple[int, ...], bool]]:
    """(tensor name, OIHW shape, has_act) for every conv of a fused YOLO11 detect model (depthwise convs: (C, 1, 3, 3))."""
    return family_specs("yolo11", scale, nc)


def synthetic_yolo11(seed: int = 0, nc: int = 4, scale: str = "s", cls_bias: float = -4.0, gain: float = 1.7,
                     box_decay: float | tuple = 0.3, level_bias: tuple = (0.0, 0.0, 0.0), box_weight_scale: float = 0.3) -> dict[str, np.ndarray]:
    """Seeded random fused weights of the YOLO11 architecture, drawn like synthetic_yolov8's (same knobs, the draws in the order of
    yolo11_layer_specs): weights ~ N(0, g^2 / fan_in) with g = gain in front of a SiLU and 1 for the activation-free layers (qkv,
    proj, pe, ffn.1, Detect's last 1x1s); a depthwise layer's fan-in is its 9 taps."""
    return family_synthetic("yolo11", seed, nc, scale, cls_bias=cls_bias, gain=gain, box_decay=box_decay, level_bias=level_bias, box_weight_scale=box_weight_scale)

# --------------------------------------------------------------------------- YOLOv10 (cfg/models/v10/yolov10{n,s}.yaml)
# What `YOLO("yolov10s.pt")` fine-tunes to: the YOLOv8 backbone and neck with SCDown (1x1 Conv, then a depthwise 3x3 stride 2 without
# activation) in place of the stride-2 Convs at 5 / 7 / 20, PSA (C2PSA's one block directly under the layer) = model.10, C2fCIB (C2f whose
# m.{k} are CIBs: dw3 -> 1x1 -> dw3 or the fused RepVGGDW's dw7 -> 1x1 -> dw3) at model.22 and, from scale s on, model.8, and v10Detect =
# model.23 on [16, 19, 22]: YOLO11's Detect layers twice, cv2 / cv3 (one-to-many, trained with NMS in mind) and one2one_cv2 / one2one_cv3
# (the NMS-free head inference uses: the 300 best (anchor, class) scores, V10_MAX_DET). Restated from ultralytics' public source; not
# checked against the package (it is not installed).

YOLOV10_SCALES = {"n": (0.33, 0.25, 1024), "s": (0.33, 0.50, 1024)}   # yolov10{n,s}.yaml: depth, width, max_channels

YOLOV10_TOPOLOGY = ("yolov10 detect (yolov10{n,s}: SCDown = model.5 / 7 / 20, PSA = model.10, C2fCIB where the tensors say so, "
                    "v10Detect = model.23 on model.16 / 19 / 22 with its one2one_cv2 / one2one_cv3 head)")

V10_MAX_DET = 300   # Detect.max_det: the rows v10Detect.postprocess keeps, whatever the predictor's max_det (csrc: kV10Keep)

_V10_BIGGER = {48: "yolov10m", 64: "yolov10b / yolov10l", 80: "yolov10x"}   # model.0's width of the scales that are not implemented


def _yolov10_table(scale: str):
    """yolov10<scale>.yaml as a table: scale n keeps a plain C2f at model.8."""
    t = list(YOLOV10_YAML)
    if scale == "n":
        t[8] = (-1, 3, "C2f", (1024, True))
    return t


def is_yolov10(tensors: dict) -> bool:
    """True when the names hold what only a YOLOv10 file has: attention directly under model.10 (`model.10.attn.qkv`: PSA; C2PSA has
    `model.10.m.0.attn`), SCDown's depthwise `model.5.cv2.conv` and a one-to-one head (`.one2one_cv2.`). Which graph it is, and
    whether this build runs it: check_yolov10()."""
    w = tensors.get("model.5.cv2.conv.weight")
    return ("model.10.attn.qkv.conv.weight" in tensors and w is not None and np.ndim(w) == 4 and np.shape(w)[1] == 1
            and any(".one2one_cv2." in k for k in tensors))


def check_yolov10(tensors: dict) -> str:
    """The scale ("n" / "s") of a fused yolov10.yaml detect model; raises NotImplementedError for every other arrangement of its blocks
    (a cv4 / proto branch, attention elsewhere, Detect elsewhere, anything past model.23, another width). The table is rebuilt from what
    the tensors tell (C2f or C2fCIB per block row, large-kernel or not) and compared strictly (_strict_compare). The one-to-many pair
    cv2 / cv3 may be missing as a whole (ultralytics' fuse() drops it)."""
    no = NotImplementedError(f"checkpoint with YOLOv10's blocks (PSA, SCDown, a one-to-one head) in another arrangement than yolov10.yaml's: of that "
                             f"family only {YOLOV10_TOPOLOGY} is implemented")
    c0, nc_w = _shape(tensors, "model.0.conv.weight"), _shape(tensors, "model.23.one2one_cv3.0.2.weight")
    if c0 is not None and c0[0] in _V10_BIGGER:
        raise NotImplementedError(f"{_V10_BIGGER[c0[0]]} (model.0 has {c0[0]} channels): of the YOLOv10 scales only n and s are implemented ({YOLOV10_TOPOLOGY})")
    scale = {16: "n", 32: "s"}.get(c0[0]) if c0 else None
    if scale is None or nc_w is None:
        raise no
    table = []
    for i, (frm, n, mod, args) in enumerate(YOLOV10_YAML):
        if mod in ("C2f", "C2fCIB"):
            cib = f"model.{i}.m.0.cv1.0.conv.weight" in tensors
            if f"model.{i}.m.0." + ("cv1.0.conv.weight" if cib else "cv1.conv.weight") not in tensors:
                raise no
            lk = cib and (_shape(tensors, f"model.{i}.m.0.cv1.2.conv.weight") or (0, 0, 0))[2] == 7
            table.append((frm, n, "C2fCIB", (args[0], args[1] if len(args) > 1 else False, lk)) if cib else (frm, n, "C2f", args[:2]))
        else:
            table.append((frm, n, mod, args))
    _compare_family("yolov10", family_specs("yolov10", scale, nc_w[0], table=table), tensors, no, group=_ONE2MANY)
    return scale


def yolov10_has_one2many(tensors: dict) -> bool:
    """True when the file kept v10Detect's one-to-many pair (cv2 / cv3), which `end2end: false` runs through Detect + NMS."""
    return "model.23.cv2.0.0.conv.weight" in tensors and "model.23.cv3.0.2.weight" in tensors


def yolov10_layer_specs(scale: str = "s", nc: int = 4) -> list[tuple[str, tuple[int, ...], bool]]:
    """(tensor name, OIHW shape, has_act) for every conv of a fused YOLOv10 detect model (depthwise convs: (C, 1, k, k); the fused
    RepVGGDW of a large-kernel CIB: (C, 1, 7, 7) at m.{k}.cv1.2.conv), both head pairs included."""
    return family_specs("yolov10", scale, nc)


def synthetic_yolov10(seed: int = 0, nc: int = 4, scale: str = "s", cls_bias: float = -4.0, gain: float = 1.7,
                      box_decay: float | tuple = 0.3, level_bias: tuple = (0.0, 0.0, 0.0), box_weight_scale: float = 0.3) -> dict[str, np.ndarray]:
    """Seeded random fused weights of the YOLOv10 architecture, drawn like synthetic_yolo11's (same knobs, the draws in the order of
    yolov10_layer_specs). Both head pairs are emitted, cv2 / cv3 first, each with draws of its own, so the two heads detect
    different things; the knobs shape both alike."""
    return family_synthetic("yolov10", seed, nc, scale, cls_bias=cls_bias, gain=gain, box_decay=box_decay, level_bias=level_bias, box_weight_scale=box_weight_scale)

# --------------------------------------------------------------------------- YOLO26 (cfg/models/26/yolo26.yaml)
# What `YOLO("yolo26s.pt")` fine-tunes to: yolo11.yaml's rows with three changes. SPPF = model.9 has a cv1 WITHOUT activation and adds
# its input to cv2's output (after cv2's SiLU); the last neck block, model.22, is a C3k2 whose m.{k} are Sequential(Bottleneck, PSABlock)
# (`model.22.m.0.0.cv1.conv`, `model.22.m.0.1.attn.qkv.conv`); Detect = model.23 has reg_max = 1 -- the box branch ends in a 1x1 to FOUR
# channels, the signed distances l, t, r, b in strides, no DFL -- and, like v10Detect, carries one2one_cv2 / one2one_cv3 next to cv2 /
# cv3 and ends in the same two-stage top-300 cut. Restated from memory of ultralytics' public source; not checked against the package
# (it is not installed). The doubts are listed in tests/yolo26_ref.py; the constants below and their twins in csrc/yolo_tables.hpp hold them.

YOLO26_TOPOLOGY = ("yolo26 detect (yolo26{n,s,m,l,x}: yolo11.yaml's rows with SPPF(shortcut) = model.9, C3k2(attn) = model.22 and Detect = "
                   "model.23 on model.16 / 19 / 22 with reg_max = 1 and a one2one_cv2 / one2one_cv3 head)")
YOLO26_BOX_FLOOR = 64        # doubt: Detect's box-branch width is max(16, ch[0] // 4, this). Every other family here has 4 * reg_max = 64 as the third
                             # term; with reg_max = 1 the package may give 16 / 32 channels at scales n / s. Taken as 64; such a file is refused by shape.
YOLO26_BOX_BIAS = (2.0, 2.5, 2.0, -0.5)   # synthetic_yolo26: the means of l, t, r, b (strides): boxes four strides wide and two high whose lower
                             # side lies ABOVE the cell centre -- a negative distance at every anchor of a calm seeded stack


def is_yolo26(tensors: dict) -> bool:
    """True when the names hold what only a YOLO26 file has, all of: YOLO11's blocks, the attention inside model.22's C3k2
    (`model.22.m.0.1.attn.qkv`), a last box convolution of 4 rows (reg_max = 1) and a one-to-one class branch. Which graph it is, and
    whether this build runs it: check_yolo26()."""
    if not has_yolo11_blocks(tensors) or "model.22.m.0.1.attn.qkv.conv.weight" not in tensors:
        return False
    w = tensors.get("model.23.one2one_cv2.0.2.weight")
    if w is None:
        w = tensors.get("model.23.cv2.0.2.weight")
    return w is not None and np.ndim(w) == 4 and np.shape(w)[0] == 4 and any(k.startswith("model.23.one2one_cv3.") for k in tensors)


def _yolo26_marks(tensors: dict) -> bool:
    """A file with YOLO11's blocks and one of YOLO26's own marks, the attention inside model.22 or a 4-row last box convolution, but
    not all that is_yolo26() demands: check_yolo26() refuses it with YOLO26's message. A YOLO11 file with stray one2one_* tensors has
    neither mark and goes to check_yolo11()."""
    if not has_yolo11_blocks(tensors):
        return False
    rows = [np.shape(tensors[k])[0] for k in ("model.23.one2one_cv2.0.2.weight", "model.23.cv2.0.2.weight") if k in tensors and np.ndim(tensors[k]) == 4]
    return "model.22.m.0.1.attn.qkv.conv.weight" in tensors or 4 in rows


def check_yolo26(tensors: dict) -> str:
    """The scale ("n" / "s" / "m" / "l" / "x") of a fused yolo26.yaml detect model; raises NotImplementedError for every other
    arrangement of its blocks (a cv4 / proto branch, attention elsewhere, Detect elsewhere, reg_max other than 1, anything past
    model.23, another width). The table is rebuilt from what the tensors tell (c3k or not per C3k2, model.22's repeats) and compared
    strictly (_strict_compare). The one-to-many pair cv2 / cv3 may be missing as a whole (ultralytics' fuse() drops it)."""
    no = NotImplementedError(f"checkpoint with YOLO26's blocks (attention inside model.22's C3k2, a 4-output box branch, a one-to-one head) in "
                             f"another arrangement than yolo26.yaml's: of that family only {YOLO26_TOPOLOGY} is implemented")
    nc_w = _shape(tensors, "model.23.one2one_cv3.0.2.weight")
    if "model.0.conv.weight" not in tensors or "model.1.conv.weight" not in tensors or nc_w is None:
        raise no
    for k in ("model.23.one2one_cv2.0.2.weight", "model.23.cv2.0.2.weight"):
        rows = (_shape(tensors, k) or (4,))[0]
        if rows != 4:
            raise NotImplementedError(f"{k} has {rows} rows (reg_max = {rows // 4}) in a graph with YOLO26's attention inside model.22: "
                                      f"only reg_max = 1, a 4-row box convolution, is implemented there ({YOLO26_TOPOLOGY})")
    scale = _scale_of_yolo11_widths(tensors)
    n22 = 0                                                # model.22's repeats (the yaml writes 1, which no scale multiplies): off the tensors, 1 or 2
    while f"model.22.m.{n22}.0.cv1.conv.weight" in tensors:
        n22 += 1
    if scale is None or n22 not in (1, 2):
        raise no
    want = family_specs("yolo26", scale, nc_w[0], table=_c3k_off_tensors(YOLO26_YAML, tensors), reps={22: n22}, c3k_all=False)
    _compare_family("yolo26", want, tensors, no, group=_ONE2MANY)
    return scale


def yolo26_layer_specs(scale: str = "s", nc: int = 4) -> list[tuple[str, tuple[int, ...], bool]]:
    """(tensor name, OIHW shape, has_act) for every conv of a fused YOLO26 detect model, both head pairs included (the last box
    convolutions: (4, cb, 1, 1))."""
    return family_specs("yolo26", scale, nc)


def synthetic_yolo26(seed: int = 0, nc: int = 4, scale: str = "s", cls_bias: float = -4.0, gain: float = 1.7,
                     box_weight_scale: float = 0.3) -> dict[str, np.ndarray]:
    """Seeded random fused weights of the YOLO26 architecture, drawn like synthetic_yolov10's (same knobs, the draws in the order of
    yolo26_layer_specs; both head pairs, each with draws of its own). The last box convolutions give the four distances directly:
    damped weights (box_weight_scale) around the biases YOLO26_BOX_BIAS, one of which is negative."""
    return family_synthetic("yolo26", seed, nc, scale, cls_bias=cls_bias, gain=gain, box_weight_scale=box_weight_scale)   # box_decay / level_bias: fixed

# --------------------------------------------------------------------------- YOLO12 (cfg/models/12/yolo12.yaml)
# What `YOLO("yolo12s.pt")` fine-tunes to: yolo11.yaml's first six rows, then A2C2f blocks in place of its C3k2 / SPPF / C2PSA: with
# area attention in the backbone (model.6: 4 horizontal bands, model.8: the whole map; each member two ABlocks of heads = c_ / 32, head
# width 32 for q, k and v, a depthwise 7x7 `pe`, an mlp of ratio 2.0 -- 1.2 at scales l / x, which also scale the block's output by a
# learned per-channel `gamma` and add its input) and with C3k members in the neck (model.11 / 14 / 17); a C3k2 closes the neck (model.20)
# and YOLO11's Detect = model.21 reads [14, 17, 20]. 22 layers. Restated from memory of ultralytics' public source; not checked against
# the package (it is not installed). The doubts are listed in tests/yolo12_ref.py.

YOLO12_TOPOLOGY = ("yolo12 detect (yolo12{n,s,m,l,x}: A2C2f with area attention = model.6 / 8, A2C2f with C3k members = model.11 / 14 / 17, "
                   "C3k2 = model.2 / 4 / 20, Detect = model.21 on model.14 / 17 / 20)")
YOLO12_AREAS = {6: 4, 8: 1}   # the yaml's `area` per attention row; no tensor tells it (csrc/yolo_tables.hpp kYolo12 holds the same)


def is_yolo12(tensors: dict) -> bool:
    """True when the names hold what only a YOLO12 file has: an A2C2f's ABlocks, a Sequential of two inside `m.{k}`, at model.6 or
    model.8 (`model.6.m.0.0.attn.qkv`; YOLO11 and YOLO26 have no attention there, and a stray `model.6.m.0.attn` is YOLO11's to
    refuse). Which graph it is, and whether this build runs it: check_yolo12()."""
    return "model.6.m.0.0.attn.qkv.conv.weight" in tensors or "model.8.m.0.0.attn.qkv.conv.weight" in tensors


def _yolo12_want(tensors_or_none, scale: str, nc: int):
    """(conv specs, gamma specs) of yolo12<scale>.yaml; c3k per C3k2 row off the tensors when some are given, else parse_model's rule"""
    gammas: list = []
    if tensors_or_none is None:
        return family_specs("yolo12", scale, nc, gammas=gammas), gammas
    return family_specs("yolo12", scale, nc, table=_c3k_off_tensors(YOLO12_YAML, tensors_or_none), c3k_all=False, gammas=gammas), gammas


def check_yolo12(tensors: dict) -> str:
    """The scale ("n" / "s" / "m" / "l" / "x") of a fused yolo12.yaml detect model; raises NotImplementedError, with a message that
    names yolo12, for every other arrangement of its blocks (attention elsewhere, Detect elsewhere, a cv4 / proto branch, anything past
    model.21, another width or repeat count, a gamma where the scale has none). The table is rebuilt from model.0's width and the
    repeats and compared strictly (_strict_compare), the gammas with it. yolo12.yaml's scales are yolo11.yaml's."""
    no = NotImplementedError(f"checkpoint with YOLO12's blocks (A2C2f with area attention at model.6 / 8) in another arrangement than yolo12.yaml's: "
                             f"of that family only {YOLO12_TOPOLOGY} is implemented")
    scale, nc_w = _scale_of_yolo11_widths(tensors), _shape(tensors, "model.21.cv3.0.2.weight")
    if scale is None or nc_w is None:
        raise no
    want, gammas = _yolo12_want(tensors, scale, nc_w[0])
    _compare_family("yolo12", want, tensors, no, extra=gammas)
    return scale


def yolo12_layer_specs(scale: str = "s", nc: int = 4) -> list[tuple[str, tuple[int, ...], bool]]:
    """(tensor name, OIHW shape, has_act) for every conv of a fused YOLO12 detect model (depthwise convs: (C, 1, k, k); AAttn's pe is
    7x7). The `gamma` vectors of scales l / x are no convs: yolo12_gamma_specs()."""
    return _yolo12_want(None, scale, nc)[0]


def yolo12_gamma_specs(scale: str = "s") -> list[tuple[str, tuple[int]]]:
    """(tensor name, (c2,)) of A2C2f's learned residual scales: model.6.gamma and model.8.gamma at scales l / x, none below."""
    return _yolo12_want(None, scale, 4)[1]


def synthetic_yolo12(seed: int = 0, nc: int = 4, scale: str = "s", cls_bias: float = -4.0, gain: float = 1.7, box_decay: float | tuple = 0.3,
                     level_bias: tuple = (0.0, 0.0, 0.0), box_weight_scale: float = 0.3, gamma: float = 0.5) -> dict[str, np.ndarray]:
    """Seeded random fused weights of the YOLO12 architecture, drawn like synthetic_yolo11's (same knobs, the draws in the order of
    yolo12_layer_specs), then the gammas of scales l / x ~ N(gamma, (gamma / 4)^2) from the same generator: ultralytics starts them at
    0.01, which would hide the block behind its own input; the default lets both terms of x + gamma * y count."""
    rng = np.random.default_rng(seed)
    t = family_synthetic("yolo12", rng, nc, scale, cls_bias=cls_bias, gain=gain, box_decay=box_decay, level_bias=level_bias, box_weight_scale=box_weight_scale)
    for name, shp in yolo12_gamma_specs(scale):
        t[name] = (gamma + 0.25 * gamma * rng.standard_normal(shp)).astype(np.float32)
    return t

# --------------------------------------------------------------------------- YOLOv5u (cfg/models/v5/yolov5.yaml)
# What `YOLO("yolov5su.pt")` is: yolov5.yaml -- a 6x6 stride-2 stem (Conv(64, 6, 2, 2)), C3 blocks (cv1 and cv2 1x1 on the block's
# input, Bottlenecks of a 1x1 and a 3x3 behind cv1, cv3 on the two; shortcut on in the backbone, off in the neck), SPPF = model.9, a neck
# whose 1x1 Convs (model.10 / 14) feed the Upsamples and the Concats of the way back down -- with YOLOv8's anchor-free Detect = model.24 on
# [17, 20, 23]. 25 layers. Restated from memory of ultralytics' public source; not checked against the package (it is not installed).
# The doubts are listed in tests/yolov5u_ref.py. Not implemented and refused by name: the P6 files (yolov5{n,s,m,l,x}6u: four Detect
# levels, Detect = model.33), an anchor-based export of the original YOLOv5 (model.24.m.* / anchors), YOLOv3u (yolov3.yaml's Darknet
# with the same Detect) and the -seg / -cls heads.

YOLOV5_SCALES = {"n": (0.33, 0.25, 1024), "s": (0.33, 0.50, 1024), "m": (0.67, 0.75, 1024),
                 "l": (1.00, 1.00, 1024), "x": (1.33, 1.25, 1024)}   # yolov5.yaml: depth, width, max_channels

YOLOV5U_TOPOLOGY = ("yolov5u detect (yolov5{n,s,m,l,x}u from yolov5.yaml: 6x6 stem = model.0, C3 blocks, SPPF = model.9, 1x1 Convs = model.10 / 14, "
                    "Detect = model.24 on model.17 / 20 / 23)")


def _stem_kernel(tensors: dict) -> int:
    """model.0's kernel side (6: yolov5.yaml's stem), 0 when there is no 4-d `model.0.conv.weight`"""
    w = tensors.get("model.0.conv.weight")
    return int(np.shape(w)[2]) if w is not None and np.ndim(w) == 4 and np.shape(w)[2] == np.shape(w)[3] else 0


def is_yolov5u(tensors: dict) -> bool:
    """True when model.0 is a 6x6 convolution and an anchor-free Detect (cv2 branch and DFL) stands at model.24: a yolov5{n,s,m,l,x}u
    file. Which scale it is, and whether every shape is yolov5.yaml's: check_yolov5u()."""
    return _stem_kernel(tensors) == 6 and "model.24.cv2.0.0.conv.weight" in tensors and "model.24.dfl.conv.weight" in tensors


def _is_yolov3u(tensors: dict) -> bool:
    """yolov3.yaml / yolov3-spp.yaml / yolov3-tiny.yaml with the anchor-free Detect: a 3x3 stem, a bare Darknet Bottleneck at model.2
    (`model.2.cv2.conv` 3x3 and no `model.2.m.*`; tiny: no `model.2.*` convolution at all, a MaxPool at model.1) and a Detect with a DFL
    that is neither model.22 (yolov8.yaml) nor model.24 (yolov5.yaml)"""
    if _stem_kernel(tensors) != 3:
        return False
    dfl = {k.split(".")[1] for k in tensors if k.startswith("model.") and k.endswith(".dfl.conv.weight") and len(k.split(".")) == 5}
    if not dfl or dfl & {"22", "24"}:
        return False
    w = tensors.get("model.2.cv2.conv.weight")
    darknet = w is not None and np.ndim(w) == 4 and np.shape(w)[2] == 3 and "model.2.m.0.cv1.conv.weight" not in tensors
    tiny = "model.1.conv.weight" not in tensors and "model.2.conv.weight" in tensors
    return darknet or tiny


def _yolov5_lookalike(tensors: dict) -> bool:
    """A file of YOLOv5's wider family that is not a yolov5*u detect file: any other 6x6 stem (the P6 files, -seg, -cls, other Detect
    rows), an anchor-based export (`model.<k>.anchors` / `model.24.m.0.weight`), YOLOv3u. check_yolov5u() refuses each by name."""
    return (_stem_kernel(tensors) == 6 or "model.24.m.0.weight" in tensors or "model.24.anchors" in tensors or "model.33.m.0.weight" in tensors or
            _is_yolov3u(tensors))


def check_yolov5u(tensors: dict) -> str:
    """The scale ("n" / "s" / "m" / "l" / "x") of a fused yolov5.yaml detect model with the anchor-free head; raises NotImplementedError,
    with a message that names yolov5.yaml and what is implemented, for everything else of the family: the P6 files, an anchor-based
    export, YOLOv3u, -seg / -cls heads, and any tensor whose shape is not what model.0's width (16 / 32 / 48 / 64 / 80 = n / s / m / l /
    x) gives through yolov5.yaml's width, depth and max_channels (_strict_compare)."""
    only = f"of that family only {YOLOV5U_TOPOLOGY} is implemented"
    no = lambda what: NotImplementedError(f"{what}: {only}")
    if "model.24.m.0.weight" in tensors or "model.33.m.0.weight" in tensors or any(k.startswith("model.") and k.endswith(".anchors") for k in tensors):
        raise no("an anchor-based export of the original YOLOv5 (Detect with `anchors` and `m.{l}` output convolutions, not yolov5.yaml's "
                 "anchor-free yolov5*u head)")
    if _is_yolov3u(tensors):
        raise no("a YOLOv3u checkpoint (yolov3.yaml's Darknet-53 with the anchor-free Detect; of the files that share yolov5.yaml's head)")
    if _stem_kernel(tensors) != 6:
        raise no("a checkpoint without yolov5.yaml's 6x6 stem")
    if any(re.match(r"model\.\d+\.(cv4|proto)\.", k) for k in tensors):
        raise no("a yolov5*u-seg checkpoint (yolov5.yaml with a Segment head: `cv4` / `proto` branches)")
    if any(re.match(r"model\.\d+\.linear\.", k) for k in tensors):
        raise no("a yolov5*u-cls checkpoint (yolov5.yaml's backbone with a Classify head)")
    if "model.33.cv2.0.0.conv.weight" in tensors or "model.33.dfl.conv.weight" in tensors:
        raise no("a yolov5*6u checkpoint (yolov5-p6.yaml: four Detect levels, Detect = model.33)")
    bad = no("checkpoint with yolov5.yaml's 6x6 stem in another arrangement than yolov5.yaml's")
    nc_w = _shape(tensors, "model.24.cv3.0.2.weight")
    scale = {16: "n", 32: "s", 48: "m", 64: "l", 80: "x"}.get(_shape(tensors, "model.0.conv.weight")[0])
    if not is_yolov5u(tensors) or nc_w is None or scale is None:
        raise bad
    _compare_family("yolov5u", family_specs("yolov5u", scale, nc_w[0]), tensors, bad)
    return scale


def yolov5u_layer_specs(scale: str = "s", nc: int = 4) -> list[tuple[str, tuple[int, ...], bool]]:
    """(tensor name, OIHW shape, has_act) for every conv of a fused YOLOv5u detect model (model.0 is 6x6, model.10 / 14 are 1x1)"""
    return family_specs("yolov5u", scale, nc)


def synthetic_yolov5u(seed: int = 0, nc: int = 4, scale: str = "s", cls_bias: float = -4.0, gain: float = 1.7,
                      box_decay: float | tuple = 0.3, level_bias: tuple = (0.0, 0.0, 0.0), box_weight_scale: float = 0.3) -> dict[str, np.ndarray]:
    """Seeded random fused weights of the YOLOv5u architecture, drawn like synthetic_yolov8's (same knobs, the draws in the order of
    yolov5u_layer_specs), plus Detect's constant DFL convolution `model.24.dfl.conv.weight` (0 .. 15), which every real file carries and
    is_yolov5u() asks for."""
    t = family_synthetic("yolov5u", seed, nc, scale, cls_bias=cls_bias, gain=gain, box_decay=box_decay, level_bias=level_bias, box_weight_scale=box_weight_scale)
    t["model.24.dfl.conv.weight"] = np.arange(16, dtype=np.float32).reshape(1, 16, 1, 1)
    return t


# --------------------------------------------------------------------------- YOLOv9 (cfg/models/v9/yolov9{t,s,m,c}.yaml)
# The GELAN networks: ELAN1 / RepNCSPELAN4 blocks (cv1 1x1 -> two chunks; cv2 and cv3 are Sequential(RepCSP, Conv3x3) -- plain Conv3x3
# in ELAN1 -- each on the output before it; cv4 1x1 on the four pieces), AConv (avg_pool2d(2, 1) then a 3x3 stride-2 Conv; scales t / s /
# m) or ADown (the same pool, then one channel half through a 3x3 stride-2 Conv and the other through max_pool2d(3, 2, 1) + a 1x1 Conv;
# scale c) for downsampling, SPPELAN = model.9 and YOLOv8's legacy Detect = model.22 on [15, 18, 21]. The yamls carry no `scales`: every
# file writes its widths out, so each scale is a table of its own (_yolov9_table). Restated from ultralytics' public source; not checked
# against the package (it is not installed). yolov9e (two backbones joined by CBLinear / CBFuse) is not implemented.

YOLOV9_TOPOLOGY = ("yolov9 detect (yolov9{t,s,m,c}: ELAN1 / RepNCSPELAN4 blocks, AConv or ADown = model.3 / 5 / 7 / 16 / 19, SPPELAN = model.9, "
                   "Detect = model.22 on model.15 / 18 / 21)")

# per scale: model.0, model.1, the block rows 2 / 4 / 6 / 8 / 15 as (c2, c3, c4, n) (n = 0: ELAN1), the widths of the downsampling rows
# 3 / 5 / 7 / 16 / 19, SPPELAN's c3, and the downsampling module
_YOLOV9_WIDTHS = {
    "t": (16, 32, ((32, 32, 16, 0), (64, 64, 32, 3), (96, 96, 48, 3), (128, 128, 64, 3), (64, 64, 32, 3)), (64, 96, 128, 48, 64), 64, "AConv"),
    "s": (32, 64, ((64, 64, 32, 0), (128, 128, 64, 3), (192, 192, 96, 3), (256, 256, 128, 3), (128, 128, 64, 3)), (128, 192, 256, 96, 128), 128, "AConv"),
    "m": (32, 64, ((128, 128, 64, 1), (240, 240, 120, 1), (360, 360, 180, 1), (480, 480, 240, 1), (240, 240, 120, 1)), (240, 360, 480, 184, 240), 240, "AConv"),
    "c": (64, 128, ((256, 128, 64, 1), (512, 256, 128, 1), (512, 512, 256, 1), (512, 512, 256, 1), (256, 256, 128, 1)), (256, 512, 512, 256, 512), 256, "ADown"),
}


def _yolov9_table(scale: str):
    """yolov9<scale>.yaml as a table. The neck's blocks 12 / 18 / 21 repeat the backbone's 6 / 6 / 8; 15 is row 4 again except in scale c."""
    c0, c1, blocks, down, spp, dmod = _YOLOV9_WIDTHS[scale]
    blk = lambda b: (-1, 1, "RepNCSPELAN4", b) if b[3] else (-1, 1, "ELAN1", b[:3])
    dn = lambda k: (-1, 1, dmod, (down[k],))
    return [
        (-1, 1, "Conv", (c0, 3, 2)),
        (-1, 1, "Conv", (c1, 3, 2)),
        blk(blocks[0]),                                    # 2
        dn(0), blk(blocks[1]),                             # 3, 4
        dn(1), blk(blocks[2]),                             # 5, 6
        dn(2), blk(blocks[3]),                             # 7, 8
        (-1, 1, "SPPELAN", (blocks[3][0], spp)),           # 9
        _UP,
        ((-1, 6), 1, "Concat", (1,)),
        blk(blocks[2]),                                    # 12
        _UP,
        ((-1, 4), 1, "Concat", (1,)),
        blk(blocks[4]),                                    # 15
        dn(3),
        ((-1, 12), 1, "Concat", (1,)),
        blk(blocks[2]),                                    # 18
        dn(4),
        ((-1, 9), 1, "Concat", (1,)),
        blk(blocks[3]),                                    # 21
        ((15, 18, 21), 1, "Detect", ("nc",)),              # 22: the legacy head, cv3 = Conv3x3, Conv3x3, Conv2d
    ]


YOLOV9_YAML = _yolov9_table("s")                           # v9/yolov9s.yaml; the other scales: _yolov9_table


def _has_gelan(tensors: dict) -> bool:
    """A Sequential inside an ELAN block (`model.<N>.cv2.0.cv1.conv.weight`: RepNCSPELAN4.cv2[0] is a RepCSP): no other supported family has it"""
    for k in tensors:
        p = k.split(".")
        if len(p) == 7 and p[0] == "model" and p[1].isdigit() and p[2:] == ["cv2", "0", "cv1", "conv", "weight"]:
            return True
    return False


def is_yolov9(tensors: dict) -> bool:
    """True when the names hold what only a YOLOv9 t / s / m / c file has: a RepNCSPELAN4's RepCSP (`model.<N>.cv2.0.cv1.conv`) and
    SPPELAN's closing conv `model.9.cv5.conv`. Which graph it is, and whether this build runs it: check_yolov9()."""
    return "model.9.cv5.conv.weight" in tensors and _has_gelan(tensors)


def check_yolov9(tensors: dict) -> str:
    """The scale ("t" / "s" / "m" / "c") of a fused yolov9.yaml detect model; raises NotImplementedError for every other arrangement of
    its blocks (yolov9e's second backbone, anything past model.22, Detect elsewhere, another width or repeat count). The widths of
    model.0 and of model.2's cv1 name the one candidate scale (s and m share model.0's), whose table is compared strictly (_strict_compare)."""
    no = NotImplementedError(f"checkpoint with YOLOv9's blocks (RepNCSPELAN4, ADown / AConv, SPPELAN) in another arrangement than yolov9{{t,s,m,c}}.yaml's "
                             f"(yolov9e with its CBLinear / CBFuse second backbone included): of that family only {YOLOV9_TOPOLOGY} is implemented")
    c0, c2, nc_w = (_shape(tensors, n) for n in ("model.0.conv.weight", "model.2.cv1.conv.weight", "model.22.cv3.0.2.weight"))
    scale = next((s for s, w in _YOLOV9_WIDTHS.items() if c0 and c2 and (w[0], w[2][0][1]) == (c0[0], c2[0])), None)
    if scale is None or nc_w is None:
        raise no
    _compare_family("yolov9", family_specs("yolov9", scale, nc_w[0]), tensors, no)
    return scale


def yolov9_layer_specs(scale: str = "s", nc: int = 4) -> list[tuple[str, tuple[int, ...], bool]]:
    """(tensor name, OIHW shape, has_act) for every conv of a fused YOLOv9 detect model (RepConv fused: `...m.{k}.cv1.conv` is one 3x3)"""
    return family_specs("yolov9", scale, nc)


def synthetic_yolov9(seed: int = 0, nc: int = 4, scale: str = "s", cls_bias: float = -4.0, gain: float = 1.7,
                     box_decay: float | tuple = 0.3, level_bias: tuple = (0.0, 0.0, 0.0), box_weight_scale: float = 0.3) -> dict[str, np.ndarray]:
    """Seeded random fused weights of the YOLOv9 architecture, drawn like synthetic_yolov8's (same knobs, the draws in the order of
    yolov9_layer_specs)."""
    return family_synthetic("yolov9", seed, nc, scale, cls_bias=cls_bias, gain=gain, box_decay=box_decay, level_bias=level_bias, box_weight_scale=box_weight_scale)


def pad_yolov9_channels(tensors: dict, scale: str) -> tuple[dict, dict]:
    """A fused yolov9<scale> file as an equal network whose maps all have multiples of 16 channels, the convolution kernels' K chunk:
    (tensors, layout). yolov9m's widths are not (360, 184, chunks of 180): every such map gets zero channels appended -- zero
    output weights and biases for them (SiLU(0) = 0; an average, a maximum, an upsampling and a residual of zeros are zero) and zero
    input weights in every layer that reads them -- which changes no sum. An ELAN block's cv1 is padded per chunk, so chunk(2) still
    halves it. RepCSP's hidden maps (60 / 90 channels) stay as they are: the trunk builder pads them inside the block, as for
    yolov9t. layout: layer name -> the positions of its real channels in the padded map (Detector.layer_output reads through it).
    A scale whose widths are multiples of 16 already (t, s, c) comes back unchanged with an empty layout."""
    p16 = lambda c: -(-c // 16) * 16
    ident = lambda c: (np.arange(c), p16(c))                # c real channels, padding behind them
    plain = lambda c: (np.arange(c), c)                     # left as it is
    cat = lambda *ls: (np.concatenate([pos + off for (pos, _), off in zip(ls, np.cumsum([0] + [cp for _, cp in ls[:-1]]))]), sum(cp for _, cp in ls))
    out = {k: np.asarray(v, np.float32) for k, v in tensors.items()}

    def put(name, lin, lout):
        w, b = out[name + ".weight"], out.get(name + ".bias")
        wp = np.zeros((lout[1], lin[1]) + w.shape[2:], np.float32)
        wp[np.ix_(lout[0], lin[0])] = w
        out[name + ".weight"] = wp
        bp = np.zeros(lout[1], np.float32)
        if b is not None:
            bp[lout[0]] = b
        out[name + ".bias"] = bp

    def repcsp(p, lin, lout):
        h = out[p + ".cv1.conv.weight"].shape[0]
        put(p + ".cv1.conv", lin, plain(h))
        put(p + ".cv2.conv", lin, plain(h))
        put(p + ".cv3.conv", plain(2 * h), lout)

    L: list[tuple[np.ndarray, int]] = []
    table = _yolov9_table(scale)
    for i, (frm, _, mod, args) in enumerate(table):
        src = [L[f if f >= 0 else i + f] for f in ((frm,) if isinstance(frm, int) else frm)] if i else [plain(3)]
        pfx, lx = f"model.{i}", src[0]
        if mod == "Conv":
            L.append(ident(args[0]))
            put(pfx + ".conv", lx, L[i])
        elif mod in ("ELAN1", "RepNCSPELAN4"):
            c2, c3, c4 = args[:3]
            h = c3 // 2
            l1 = cat(ident(h), ident(h))
            put(pfx + ".cv1.conv", lx, l1)
            if mod == "ELAN1":
                put(pfx + ".cv2.conv", ident(h), ident(c4))
                put(pfx + ".cv3.conv", ident(c4), ident(c4))
            else:
                repcsp(pfx + ".cv2.0", ident(h), ident(c4))
                put(pfx + ".cv2.1.conv", ident(c4), ident(c4))
                repcsp(pfx + ".cv3.0", ident(c4), ident(c4))
                put(pfx + ".cv3.1.conv", ident(c4), ident(c4))
            L.append(ident(c2))
            put(pfx + ".cv4.conv", cat(l1, ident(c4), ident(c4)), L[i])
        elif mod == "AConv":
            L.append(ident(args[0]))
            put(pfx + ".cv1.conv", lx, L[i])
        elif mod == "ADown":                                # each half of the input and of the output padded on its own
            hi, ho = len(lx[0]) // 2, args[0] // 2
            if lx[1] != len(lx[0]) or hi % 16 or ho % 16:
                raise NotImplementedError(f"model.{i}: an ADown on {len(lx[0])} -> {args[0]} channels cannot be padded ({YOLOV9_TOPOLOGY})")
            L.append(ident(args[0]))
        elif mod == "SPPELAN":
            L.append(ident(args[0]))
            put(pfx + ".cv1.conv", lx, ident(args[1]))
            put(pfx + ".cv5.conv", cat(*[ident(args[1])] * 4), L[i])
        elif mod == "Upsample":
            L.append(lx)
        elif mod == "Concat":
            L.append(cat(*src))
        elif mod == "Detect":
            for l, lin in enumerate(src):
                for br in ("cv2", "cv3"):
                    name = f"{pfx}.{br}.{l}.0.conv"
                    put(name, lin, plain(out[name + ".weight"].shape[0]))
    layout = {}
    for i, (pos, cp) in enumerate(L):
        if cp != len(pos):
            layout[f"model.{i}"] = pos
    for i, row in enumerate(table):                          # a pool's own map is its input row's
        if row[2] in ("AConv", "ADown") and L[i - 1][1] != len(L[i - 1][0]):
            layout[f"model.{i}.pool"] = L[i - 1][0]
    if not layout and all(out[k].shape == np.shape(tensors[k]) for k in tensors):
        return dict(tensors), {}
    return out, layout


def detector_meta(tensors: dict) -> dict | None:
    """The optional `detector.meta` tensor tools/convert_weights.py writes for a YOLOv10 / YOLO26 file: [family 10 / 26, one-to-many pair kept,
    end-to-end head, the head's row count]; None when the file has none."""
    m = tensors.get("detector.meta")
    if m is None or np.size(m) < 4:
        return None
    m = np.asarray(m).ravel()
    return dict(family={f.meta: f.graph for f in FAMILIES if f.meta}.get(int(m[0]), str(int(m[0]))), one2many=bool(m[1]), end2end=bool(m[2]), max_det=int(m[3]))


def fold_repvggdw(t: dict[str, np.ndarray]) -> dict[str, np.ndarray]:
    """RepVGGDW.fuse on BN-folded tensors: `X.conv.conv` (depthwise 7x7) + `X.conv1.conv` (depthwise 3x3, zero-padded to 7x7) ->
    `X.conv` (one depthwise 7x7; biases summed), the fused model's name for it. fp64 sums, fp32 result."""
    out = dict(t)
    for k in list(t):
        if not k.endswith(".conv1.conv.weight"):
            continue
        p = k[: -len(".conv1.conv.weight")]
        w3, w7 = t[k], t.get(p + ".conv.conv.weight")
        if w7 is None or w3.shape[1:] != (1, 3, 3) or w7.shape[1:] != (1, 7, 7) or w3.shape[0] != w7.shape[0]:
            continue
        w = w7.astype(np.float64).copy()
        w[:, :, 2:5, 2:5] += w3.astype(np.float64)
        zero = np.zeros(w3.shape[0], np.float32)
        b = t.get(p + ".conv.conv.bias", zero).astype(np.float64) + t.get(p + ".conv1.conv.bias", zero).astype(np.float64)
        for q in (".conv.conv.weight", ".conv.conv.bias", ".conv1.conv.weight", ".conv1.conv.bias"):
            out.pop(p + q, None)
        out[p + ".conv.weight"], out[p + ".conv.bias"] = w.astype(np.float32), b.astype(np.float32)
    return out


def calibrate_cls_bias(tensors: dict[str, np.ndarray], raw_logits: np.ndarray, conf: float, target: int) -> dict[str, np.ndarray]:
    """Returns a copy of `tensors` whose class-logit biases are shifted by one constant so that
    about `target` anchors of the probed frame clear `conf`. raw_logits: [anchors, nc] class
    logits of one forward pass with the unshifted weights (Detector.raw_output(logits=True)[:, 4:])."""
    logit = np.sort(raw_logits.max(1).astype(np.float64))[::-1]
    k = min(max(int(target), 1), len(logit) - 1)
    delta = np.log(conf / (1 - conf)) - 0.5 * (logit[k - 1] + logit[k])
    out = dict(tensors)
    for name in tensors:
        if ".cv3." in name and name.endswith(".2.bias"):
            out[name] = (tensors[name] + np.float32(delta)).astype(np.float32)
    return out


# --------------------------------------------------------------------------- RT-DETR (rtdetr-l and yolov8-rtdetr topologies)
# The reference swaps YOLO for RTDETR when the model's yaml says so (geotrax/extract.py:222-225). Tensor names are ultralytics'
# state_dict names of cfg/models/rt-detr/rtdetr-l.yaml; load_weights() brings a checkpoint to the fused form the library and the
# oracle read: Conv+BN folded (fold_bn), RepConv's 3x3 + 1x1 pair fused into `.conv` (fuse_repconv), the decoder's
# Sequential(Conv2d, BatchNorm2d) input projections folded into `.0.weight` / `.0.bias` (fold_input_proj).

def is_rtdetr(tensors: dict) -> bool:
    """True when the tensors hold an RTDETRDecoder (`model.<k>.decoder.layers.*`, whatever k): the RTDETR predictor family
    (stretch to the square, no NMS, the 300-query score stage). Which RT-DETR graph it is: detector_topology()."""
    for k in tensors:
        parts = k.split(".", 4)
        if len(parts) == 5 and parts[0] == "model" and parts[1].isdigit() and parts[2:4] == ["decoder", "layers"]:
            return True
    return False


RTDETR_TOPOLOGIES = ("rtdetr-l (HGNetv2 + AIFI + CCFM, RTDETRDecoder = model.28)",
                     "yolov8-rtdetr (the YOLOv8 backbone + neck model.0-21, RTDETRDecoder = model.22)")


def _rtdetr_decoders(tensors: dict) -> list[str]:
    """The layer numbers that hold an RTDETRDecoder, sorted"""
    return sorted({k.split(".")[1] for k in tensors if k.startswith("model.") and ".decoder.layers." in k and k.split(".")[2] == "decoder"})


def _has(tensors: dict, *prefixes: str) -> bool:
    return all(any(k.startswith(p) for k in tensors) for p in prefixes)


# --------------------------------------------------------------------------- the family table
@dataclass(frozen=True)
class Family:
    """One detector graph this build runs: how its files are recognised, checked, spec'd and named."""
    graph: str                      # detector_topology's name for it
    head: str                       # the head's prefix: Detect / v10Detect / RTDETRDecoder
    topology: str                   # the sentence the refusals quote
    claims: Callable[[dict], bool]  # asked in FAMILIES' order; the first row that says yes takes the file, for its check to accept or refuse
    check: Callable[[dict], str | None] | None = None   # raises NotImplementedError for a file that is not the family's; the scale letter where there is one
    table: list | Callable[[str], list] | None = None   # the yaml table, or scale -> table where the scales differ in rows
    scales: dict | None = None      # the yaml's scales; None: the tables carry their widths (YOLOv9)
    kw: Callable[[str], dict] = lambda scale: {}        # _parse_model's keywords at a scale
    end2end: bool = False           # the family's own head is a one-to-one pair (one2one_cv2 / one2one_cv3) with the top-300 cut, no NMS
    attn: tuple = ()                # the layers that may hold `.attn.` tensors
    stem: str | None = None         # ultralytics' yaml file is <stem><scale>.yaml; None: the graph's name
    meta: int = 0                   # the family number tools/convert_weights.py writes into `detector.meta`
    rtdetr: bool = False            # the RTDETR predictor family: stretch to the square, no NMS, the 300-query score stage


_YOLO11_KW = lambda s: dict(c3k_all=s in "mlx", dw_cls=True)   # parse_model: c3k = True in every C3k2 of the larger scales; Detect's class branch is DWConv + Conv
_V8_TOPOLOGY = "yolov8 detect (yolov8{n,s,m,l,x}: Conv / C2f backbone + neck, SPPF = model.9, Detect = model.22 on model.15 / 18 / 21)"
_P2_TOPOLOGY = "yolov8-p2 detect (yolov8{n,s,m,l,x}-p2: yolov8.yaml's backbone, a neck down to stride 4, Detect = model.28 on model.18 / 21 / 24 / 27)"

# The order is the order of asking. Every `claims` is a cheap look at the names; what a row claims, its `check` then accepts or refuses
# in the family's own words, so a near miss of one family never falls through to the next.
FAMILIES: tuple[Family, ...] = (
    # RT-DETR first: a decoder anywhere makes the file the RTDETR predictor's, whatever its trunk (yolov8-rtdetr has YOLOv8's)
    Family("rtdetr-l", "model.28", RTDETR_TOPOLOGIES[0], lambda t: _rtdetr_decoders(t) == ["28"] and _has(t, "model.0.stem1."), rtdetr=True),
    Family("yolov8-rtdetr", "model.22", RTDETR_TOPOLOGIES[1],
           lambda t: _rtdetr_decoders(t) == ["22"] and "model.0.conv.weight" in t and _has(t, "model.9.cv1.", "model.21.cv2."), rtdetr=True),
    # YOLOv10 before the YOLO11 relatives: its PSA has `.attn.` too. check: another arrangement, and the scales that are not implemented
    Family("yolov10", "model.23", YOLOV10_TOPOLOGY, is_yolov10, check_yolov10, _yolov10_table, YOLOV10_SCALES, lambda s: dict(dw_cls=True),
           end2end=True, attn=(10,), meta=10),
    # asked before YOLO11's check, so that a YOLO12 file gets its own messages
    Family("yolo12", "model.21", YOLO12_TOPOLOGY, is_yolo12, check_yolo12, YOLO12_YAML, YOLO11_SCALES,
           lambda s: dict(c3k_all=s in "mlx", dw_cls=True, a2_residual=s in "lx"), attn=tuple(YOLO12_AREAS)),
    # is_yolo26, or one of its marks only: check refuses that in YOLO26's words (reg_max other than 1, -seg / -obb / -pose heads)
    Family("yolo26", "model.23", YOLO26_TOPOLOGY, lambda t: is_yolo26(t) or _yolo26_marks(t), check_yolo26, YOLO26_YAML, YOLO11_SCALES, _YOLO11_KW,
           end2end=True, attn=(10, 22), meta=26),
    # whatever else has attention or a depthwise Detect class branch. check: yolo11-cls, -seg, -obb, -pose, stray attention ...
    Family("yolo11", "model.23", YOLO11_TOPOLOGY, has_yolo11_blocks, check_yolo11, YOLO11_YAML, YOLO11_SCALES, _YOLO11_KW, attn=(10,)),
    # is_yolov9, or GELAN blocks without model.9.cv5: yolov9e, which check refuses by name
    Family("yolov9", "model.22", YOLOV9_TOPOLOGY, _has_gelan, check_yolov9, _yolov9_table),
    # asked last, in front of the YOLOv8 rows only: no other family's route changes. check: the P6 files, an anchor-based export,
    # YOLOv3u, -seg / -cls, a wrong shape
    Family("yolov5u", "model.24", YOLOV5U_TOPOLOGY, lambda t: is_yolov5u(t) or _yolov5_lookalike(t), check_yolov5u, YOLOV5_YAML, YOLOV5_SCALES, stem="yolov5"),
    # the YOLOv8 pair has no check: what nothing above claims is built as YOLOv8, and the library refuses what it cannot build
    Family("yolov8-p2", "model.28", _P2_TOPOLOGY, is_yolov8_p2, None, YOLOV8_P2_YAML, SCALES),
    Family("yolov8", "model.22", _V8_TOPOLOGY, lambda t: True, None, YOLOV8_YAML, SCALES),
)


def family_row(graph: str) -> Family:
    return next(f for f in FAMILIES if f.graph == graph)


class DetectorFamily(NamedTuple):
    """detector_family's answer"""
    graph: str
    head: str
    scale: str | None               # where the family's files differ by scale and its check tells it
    end2end: bool                   # the family has a one-to-one head
    rtdetr: bool
    nc_key: str                     # the tensor whose row count is nc


def detector_family(tensors: dict) -> DetectorFamily:
    """Which of FAMILIES a detector checkpoint belongs to, read off the tensor names the way the reference reads its model yaml; the
    family's check runs here, once. An RT-DETR layout other than the two rows' (rtdetr-x with its decoder at model.32, ResNet
    backbones, ...) raises NotImplementedError, and so does a file with a family's blocks in another arrangement than its yaml's."""
    f = next(f for f in FAMILIES if f.claims(tensors))
    if is_rtdetr(tensors) and not f.rtdetr:
        where = ", ".join(f"model.{d}" for d in _rtdetr_decoders(tensors))
        raise NotImplementedError(f"RT-DETR checkpoint with its decoder at {where}: only {RTDETR_TOPOLOGIES[0]} and "
                                  f"{RTDETR_TOPOLOGIES[1]} are implemented")
    scale = f.check(tensors) if f.check else None
    last = ".enc_score_head.weight" if f.rtdetr else ".one2one_cv3.0.2.weight" if f.end2end else ".cv3.0.2.weight"
    return DetectorFamily(f.graph, f.head, scale, f.end2end, f.rtdetr, f.head + last)


def detector_topology(tensors: dict) -> tuple[str, str]:
    """(graph, head prefix) of a detector checkpoint, detector_family's first two entries: ("yolov8", "model.22"), ("yolov8-p2", "model.28"),
    ("yolo11", "model.23"), ("yolov10", "model.23"), ("yolo26", "model.23"), ("yolo12", "model.21"), ("yolov9", "model.22"), ("yolov5u",
    "model.24"), ("rtdetr-l", "model.28") or ("yolov8-rtdetr", "model.22"); it raises what detector_family raises."""
    return tuple(detector_family(tensors)[:2])


def fuse_repconv(t: dict[str, np.ndarray]) -> dict[str, np.ndarray]:
    """RepConv.fuse_convs on folded tensors: `X.conv1.conv` (3x3) + `X.conv2.conv` (1x1, same Cin) -> `X.conv` (3x3, the 1x1 kernel
    added at the centre tap; biases summed). LightConv's pair (1x1 then depthwise) has other shapes and is left alone."""
    out = dict(t)
    for k in list(t):
        if not k.endswith(".conv1.conv.weight"):
            continue
        p = k[: -len(".conv1.conv.weight")]
        w3, w1 = t[k], t.get(p + ".conv2.conv.weight")
        if w1 is None or w3.shape[2] != 3 or w1.shape[2] != 1 or w1.shape[1] != w3.shape[1] or w3.shape[1] == 1:
            continue
        w = w3.astype(np.float64).copy()
        w[:, :, 1, 1] += w1[:, :, 0, 0].astype(np.float64)
        zero = np.zeros(w3.shape[0], np.float32)
        b = t.get(p + ".conv1.conv.bias", zero).astype(np.float64) + t.get(p + ".conv2.conv.bias", zero).astype(np.float64)
        for s in (".conv1.conv.weight", ".conv1.conv.bias", ".conv2.conv.weight", ".conv2.conv.bias"):
            out.pop(p + s, None)
        out[p + ".conv.weight"], out[p + ".conv.bias"] = w.astype(np.float32), b.astype(np.float32)
    return out


def fold_input_proj(t: dict[str, np.ndarray], eps: float = BN_EPS) -> dict[str, np.ndarray]:
    out = dict(t)
    for k in list(t):
        if ".input_proj." not in k or not k.endswith(".1.running_var"):
            continue
        p = k[: -len(".1.running_var")]
        s = t[p + ".1.weight"].astype(np.float64) / np.sqrt(t[k].astype(np.float64) + eps)
        out[p + ".0.weight"] = (t[p + ".0.weight"].astype(np.float64) * s[:, None, None, None]).astype(np.float32)
        out[p + ".0.bias"] = (t[p + ".1.bias"].astype(np.float64) - t[p + ".1.running_mean"].astype(np.float64) * s).astype(np.float32)
        for q in (".1.weight", ".1.bias", ".1.running_mean", ".1.running_var", ".1.num_batches_tracked"):
            out.pop(p + q, None)
    return out


def rtdetr_layer_specs(nc: int = 80, width: float = 1.0, hd: int = 256, ndl: int = 6, nh: int = 8, npts: int = 4, d_ffn: int = 1024):
    """(name, shape, kind) for every tensor of a fused RT-DETR-l; kind: 'relu' / 'silu' / 'lin' conv or linear weights (with a
    bias of the leading dim), 'ln' LayerNorm pair. width scales the backbone / encoder channel counts (multiples of 16)."""
    ch = lambda c: max(16, int(round(c * width / 16)) * 16)
    specs = []

    def conv(name, cin, cout, k, kind, groups=1):
        specs.append((name, (cout, cin // groups, k, k), kind))

    def lin(name, cin, cout):
        specs.append((name, (cout, cin), "lin"))

    def ln(name, c):
        specs.append((name, (c,), "ln"))

    cm = ch(32)
    conv("model.0.stem1.conv", 3, cm, 3, "relu")
    conv("model.0.stem2a.conv", cm, max(8, cm // 2), 2, "relu")
    conv("model.0.stem2b.conv", max(8, cm // 2), cm, 2, "relu")
    conv("model.0.stem3.conv", 2 * cm, cm, 3, "relu")
    conv("model.0.stem4.conv", cm, ch(48), 1, "relu")

    def hgblock(p, c1, cmid, c2, k, light, n=6):
        for i in range(n):
            cin = c1 if i == 0 else cmid
            if light:
                conv(f"{p}.m.{i}.conv1.conv", cin, cmid, 1, "lin")
                conv(f"{p}.m.{i}.conv2.conv", cmid, cmid, k, "relu", groups=cmid)
            else:
                conv(f"{p}.m.{i}.conv", cin, cmid, k, "relu")
        conv(p + ".sc.conv", c1 + n * cmid, c2 // 2, 1, "relu")
        conv(p + ".ec.conv", c2 // 2, c2, 1, "relu")

    c1, c2, c3, c4 = ch(128), ch(512), ch(1024), ch(2048)
    hgblock("model.1", ch(48), ch(48), c1, 3, False)
    conv("model.2.conv", c1, c1, 3, "lin", groups=c1)
    hgblock("model.3", c1, ch(96), c2, 3, False)
    conv("model.4.conv", c2, c2, 3, "lin", groups=c2)
    hgblock("model.5", c2, ch(192), c3, 5, True)
    hgblock("model.6", c3, ch(192), c3, 5, True)
    hgblock("model.7", c3, ch(192), c3, 5, True)
    conv("model.8.conv", c3, c3, 3, "lin", groups=c3)
    hgblock("model.9", c3, ch(384), c4, 5, True)
    e = hd
    conv("model.10.conv", c4, e, 1, "lin")
    lin("model.11.ma.in_proj", e, 3 * e)
    lin("model.11.ma.out_proj", e, e)
    lin("model.11.fc1", e, d_ffn)
    lin("model.11.fc2", d_ffn, e)
    ln("model.11.norm1", e)
    ln("model.11.norm2", e)

    def repc3(p, cin, c):
        conv(p + ".cv1.conv", cin, c, 1, "silu")
        conv(p + ".cv2.conv", cin, c, 1, "silu")
        for i in range(3):
            conv(f"{p}.m.{i}.conv", c, c, 3, "silu")

    conv("model.12.conv", e, e, 1, "silu")
    conv("model.14.conv", c3, e, 1, "lin")
    repc3("model.16", 2 * e, e)
    conv("model.17.conv", e, e, 1, "silu")
    conv("model.19.conv", c2, e, 1, "lin")
    repc3("model.21", 2 * e, e)
    conv("model.22.conv", e, e, 3, "silu")
    repc3("model.24", 2 * e, e)
    conv("model.25.conv", e, e, 3, "silu")
    repc3("model.27", 2 * e, e)
    specs += rtdetr_decoder_specs("model.28", (e, e, e), nc, hd, ndl, nh, npts, d_ffn)
    return specs


def rtdetr_decoder_specs(d: str, ch: tuple[int, int, int], nc: int = 80, hd: int = 256, ndl: int = 6, nh: int = 8, npts: int = 4,
                         d_ffn: int = 1024):
    """(name, shape, kind) of a fused RTDETRDecoder at prefix d on three maps of ch channels (finest first)."""
    specs = []

    def conv(name, cin, cout, k, kind):
        specs.append((name, (cout, cin, k, k), kind))

    def lin(name, cin, cout):
        specs.append((name, (cout, cin), "lin"))

    def ln(name, c):
        specs.append((name, (c,), "ln"))

    for i in range(3):
        conv(f"{d}.input_proj.{i}.0", ch[i], hd, 1, "lin")
    for i in range(ndl):
        lp = f"{d}.decoder.layers.{i}"
        lin(lp + ".self_attn.in_proj", hd, 3 * hd)
        lin(lp + ".self_attn.out_proj", hd, hd)
        ln(lp + ".norm1", hd)
        lin(lp + ".cross_attn.sampling_offsets", hd, nh * 3 * npts * 2)
        lin(lp + ".cross_attn.attention_weights", hd, nh * 3 * npts)
        lin(lp + ".cross_attn.value_proj", hd, hd)
        lin(lp + ".cross_attn.output_proj", hd, hd)
        ln(lp + ".norm2", hd)
        lin(lp + ".linear1", hd, d_ffn)
        lin(lp + ".linear2", d_ffn, hd)
        ln(lp + ".norm3", hd)
        lin(f"{d}.dec_score_head.{i}", hd, nc)
        for j, (a, b) in enumerate(((hd, hd), (hd, hd), (hd, 4))):
            lin(f"{d}.dec_bbox_head.{i}.layers.{j}", a, b)
    lin(f"{d}.query_pos_head.layers.0", 4, 2 * hd)
    lin(f"{d}.query_pos_head.layers.1", 2 * hd, hd)
    lin(f"{d}.enc_output.0", hd, hd)
    ln(f"{d}.enc_output.1", hd)
    lin(f"{d}.enc_score_head", hd, nc)
    for j, (a, b) in enumerate(((hd, hd), (hd, hd), (hd, 4))):
        lin(f"{d}.enc_bbox_head.layers.{j}", a, b)
    return specs


def synthetic_rtdetr(seed: int = 0, nc: int = 80, width: float = 1.0, hd: int = 256, ndl: int = 6, nh: int = 8, npts: int = 4, nq: int = 300,
                     d_ffn: int = 1024, score_bias: float = -1.5, box_scale: float = 0.3) -> dict[str, np.ndarray]:
    """Seeded random fused weights of the RT-DETR-l architecture (no checkpoint is reachable here). Conv / linear weights
    ~ N(0, g^2 / fan_in) with g = sqrt(2) in front of a ReLU, 1.7 in front of a SiLU, 1 otherwise; biases ~ N(0, 0.05^2);
    LayerNorm weights 1 + N(0, 0.1^2). The box heads' last layers are damped (box_scale) so that refined boxes stay near their
    anchors; the score heads' biases are shifted (score_bias) so that a minority of the queries clears conf = 0.25."""
    rng = np.random.default_rng(seed)
    t = _draw_rtdetr(rng, rtdetr_layer_specs(nc, width, hd, ndl, nh, npts, d_ffn), score_bias, box_scale)
    t["rtdetr.meta"] = np.asarray([nh, npts, nq, 8], np.float32)
    return t


def _draw_rtdetr(rng, specs, score_bias: float, box_scale: float) -> dict[str, np.ndarray]:
    t: dict[str, np.ndarray] = {}
    for name, shape, kind in specs:
        if kind == "ln":
            t[name + ".weight"] = (1 + 0.1 * rng.standard_normal(shape)).astype(np.float32)
            t[name + ".bias"] = (0.05 * rng.standard_normal(shape)).astype(np.float32)
            continue
        fan_in = int(np.prod(shape[1:]))
        g = {"relu": np.sqrt(2.0), "silu": 1.7, "lin": 1.0}[kind]
        w = rng.standard_normal(shape) * (g / np.sqrt(fan_in))
        b = rng.standard_normal(shape[0]) * 0.05
        if name.endswith("bbox_head.layers.2"):
            w *= box_scale
        if "score_head" in name:
            b += score_bias
        if name.endswith("in_proj"):                      # nn.MultiheadAttention keeps in_proj_weight / in_proj_bias as parameters
            t[name + "_weight"], t[name + "_bias"] = w.astype(np.float32), b.astype(np.float32)
        else:
            t[name + ".weight"], t[name + ".bias"] = w.astype(np.float32), b.astype(np.float32)
    return t


# --------------------------------------------------------------------------- YOLOv8-RTDETR (yolov8-rtdetr.yaml)
# geo-trax's train.sh `-rt`: the backbone and neck of yolov8.yaml (model.0-21, Concat orders and shortcut flags unchanged) with an
# RTDETRDecoder(nc) on [15, 18, 21] as model.22 in place of Detect (hd 256, 300 queries, 8 heads, 4 points, 6 layers, d_ffn 1024).
# Its name contains "rtdetr", so the reference runs it through RTDETR (extract.py:222-225): stretched input, no NMS.

def synthetic_yolov8_rtdetr(seed: int = 0, nc: int = 4, scale: str = "s", hd: int = 256, ndl: int = 6, nh: int = 8, npts: int = 4,
                            nq: int = 300, d_ffn: int = 1024, score_bias: float = -1.5, box_scale: float = 0.3) -> dict[str, np.ndarray]:
    """Seeded random fused YOLOv8-RTDETR weights. The trunk comes first from the generator, drawn exactly as synthetic_yolov8 draws
    it (its Detect specs come last there), so model.0-21 equal synthetic_yolov8(seed, scale=scale)'s tensors; then the decoder,
    drawn like synthetic_rtdetr's, at model.22 with input_proj widths taken from the trunk (model.15 / 18 / 21)."""
    rng = np.random.default_rng(seed)
    t = _draw_yolov8(rng, [s for s in yolov8_layer_specs(scale, nc) if not s[0].startswith("model.22.")])
    ch = tuple(int(t[f"model.{i}.cv2.conv.weight"].shape[0]) for i in (15, 18, 21))
    t.update(_draw_rtdetr(rng, rtdetr_decoder_specs("model.22", ch, nc, hd, ndl, nh, npts, d_ffn), score_bias, box_scale))
    t["rtdetr.meta"] = np.asarray([nh, npts, nq, 8], np.float32)   # no AIFI: the encoder-heads entry is unused
    return t


def calibrate_rtdetr_scores(tensors: dict[str, np.ndarray], raw_logits: np.ndarray, conf: float, target: int) -> dict[str, np.ndarray]:
    """A copy of `tensors` whose last decoder score head is shifted by one constant so that about `target` queries of the probed
    frame clear `conf` (the classes keep their order). raw_logits: [queries, nc] class logits of one pass with the unshifted
    weights (Detector.raw_output(logits=True)[:, 4:])."""
    logit = np.sort(raw_logits.max(1).astype(np.float64))[::-1]
    k = min(max(int(target), 1), len(logit) - 1)
    delta = np.log(conf / (1 - conf)) - 0.5 * (logit[k - 1] + logit[k])
    d = detector_topology(tensors)[1]
    last = max(int(n.split(".")[3]) for n in tensors if n.startswith(d + ".dec_score_head.") and n.endswith(".bias"))
    out = dict(tensors)
    name = f"{d}.dec_score_head.{last}.bias"
    out[name] = (tensors[name] + np.float32(delta)).astype(np.float32)
    return out


# --------------------------------------------------------------------------- YOLOv8-cls (the separate ReID network)
# `with_reid: true, model: <cls checkpoint>` (default.yaml:379, :421, :470): ultralytics' ReID runs a classification model over the
# detection crops and keeps the global average pool of its last backbone layer (model.8 of yolov8-cls.yaml). Only the backbone
# is read; the Classify head (model.9) may be present and is ignored.

CLS_SCALES = {"n": (0.33, 0.25, 1024), "s": (0.33, 0.50, 1024), "m": (0.67, 0.75, 1024),
              "l": (1.00, 1.00, 1024), "x": (1.00, 1.25, 1024)}    # yolov8-cls.yaml: depth, width, max_channels


def _cls_backbone_specs(c1: int, c2: int, c3: int, c4: int, c5: int, reps: tuple[int, int, int, int]) -> list[tuple[str, tuple[int, ...]]]:
    """(name, shape) of model.0-8 with the given widths and C2f repeats (is_yolov8_cls reads them off a file)."""
    widths = {64: c1, 128: c2, 256: c3, 512: c4, 1024: c5}
    specs = _parse_model(_V8_BACKBONE, 0, widths.get, lambda i, n: reps[i // 2 - 1] if i in (2, 4, 6, 8) else n)
    return [(n, s) for n, s, _ in specs]


def yolov8_cls_layer_specs(scale: str = "n", nc: int = 1000) -> list[tuple[str, tuple[int, ...], bool]]:
    """(tensor name, shape, has_act) of a fused YOLOv8-cls model: the backbone convs, then Classify's conv and linear layer."""
    return _scaled_specs(YOLOV8_CLS_YAML, CLS_SCALES, scale, nc)


def synthetic_yolov8_cls(seed: int = 0, scale: str = "n", nc: int = 1000, gain: float = 1.7) -> dict[str, np.ndarray]:
    """Seeded random fused YOLOv8-cls weights, drawn like synthetic_yolov8's: conv weights ~ N(0, gain^2 / fan_in), biases ~ N(0, 0.05^2)."""
    return _draw_yolov8(np.random.default_rng(seed), yolov8_cls_layer_specs(scale, nc), gain=gain)


def is_yolov8_cls(tensors: dict) -> bool:
    """True for a YOLOv8-cls checkpoint (fused). A file that is no classification model at all gives False; one that looks like a
    classifier of another family (YOLO11-cls: C3k2 blocks under C2f's tensor names with other widths, C2PSA attention, Classify at
    model.10) raises NotImplementedError: every backbone shape is checked against the layout model.0's width and the C2f repeat
    counts imply, so such a file is never built into the wrong network."""
    if "model.0.conv.weight" not in tensors or is_rtdetr(tensors) or any(k.startswith("model.22.") for k in tensors):
        return False
    unsupported = NotImplementedError("ReID model: only the YOLOv8-cls family (yolov8{n,s,m,l,x}-cls: Conv/C2f backbone model.0-8, "
                                      "Classify at model.9) is implemented; this file has another topology")
    if any(".attn." in k or k.startswith("model.10.") for k in tensors):
        raise unsupported
    c1 = int(np.shape(tensors["model.0.conv.weight"])[0])
    reps = []
    for i in (2, 4, 6, 8):
        n = 0
        while f"model.{i}.m.{n}.cv1.conv.weight" in tensors:
            n += 1
        reps.append(n)
    if min(reps) < 1:
        raise unsupported
    _strict_compare(_cls_backbone_specs(c1, 2 * c1, 4 * c1, 8 * c1, 16 * c1, tuple(reps)), tensors, 9, unsupported, ignore=None)
    return True


# --------------------------------------------------------------------------- YOLO11-cls (cfg/models/11/yolo11-cls.yaml)
# The family the pinned ultralytics names as the trackers' embedder: model.0-8 of yolo11.yaml, C2PSA = model.9 (no SPPF), Classify =
# model.10. ReID embeds layer len(model) - 2 = model.9: the vector is the global average pool of the C2PSA output (YOLOv8-cls pools
# model.8). Restated from ultralytics' public source; not checked against the package (it is not installed).

YOLO11_CLS_SCALES = {"n": (0.50, 0.25, 1024), "s": (0.50, 0.50, 1024), "m": (0.50, 1.00, 512),
                     "l": (1.00, 1.00, 512), "x": (1.00, 1.50, 512)}   # yolo11-cls.yaml: depth, width, max_channels (yolo11.yaml's)

YOLO11_CLS_TOPOLOGY = "yolo11-cls (yolo11{n,s,m,l,x}-cls: Conv/C3k2 backbone model.0-8, C2PSA = model.9, Classify at model.10)"


def yolo11_cls_layer_specs(scale: str = "n", nc: int = 1000) -> list[tuple[str, tuple[int, ...], bool]]:
    """(tensor name, shape, has_act) of a fused YOLO11-cls model: the backbone and C2PSA convs, then Classify's conv and linear layer."""
    return _scaled_specs(YOLO11_CLS_YAML, YOLO11_CLS_SCALES, scale, nc, c3k_all=scale in "mlx")


def synthetic_yolo11_cls(seed: int = 0, scale: str = "n", nc: int = 1000, gain: float = 1.7) -> dict[str, np.ndarray]:
    """Seeded random fused YOLO11-cls weights, drawn like synthetic_yolov8_cls's (the draws in the order of yolo11_cls_layer_specs)."""
    return _draw_yolov8(np.random.default_rng(seed), yolo11_cls_layer_specs(scale, nc), gain=gain)


def is_yolo11_cls(tensors: dict) -> bool:
    """True for a complete fused YOLO11-cls checkpoint. A file that is no classifier of this family (a detect file with its Detect
    head, RT-DETR, a YOLOv8-cls file: no attention block at model.9) gives False; a near miss (C2PSA at model.9 with a width or a
    block that yolo11-cls.yaml does not give, a yolo11 detect file cut to its first rows: SPPF at model.9, C2PSA at model.10)
    raises NotImplementedError. Strict like check_yolo11(): every backbone and C2PSA shape is checked against what model.0's width,
    the repeat counts and c3k-or-not imply, so such a file is never built into the wrong network."""
    if "model.0.conv.weight" not in tensors or is_rtdetr(tensors):
        return False
    if any(_layer(k) > 10 for k in tensors):               # a neck or a Detect head: no classifier
        return False
    if not any(".attn." in k for k in tensors):            # no attention anywhere: YOLOv8-cls or something else, not ours to judge
        return False
    unsupported = NotImplementedError(f"ReID model: of the classifiers with attention blocks only {YOLO11_CLS_TOPOLOGY} is implemented "
                                      f"(next to YOLOv8-cls); this file has another topology")
    c0 = int(np.shape(tensors["model.0.conv.weight"])[0])
    width = 4 * c0 / 64                                    # model.0 is ch(64): the scale's width factor, max_channels aside
    maxc = {0.25: 1024, 0.5: 1024, 1.0: 512, 1.5: 512}.get(width / 4)
    if c0 % 16 or "model.8.cv2.conv.weight" not in tensors or maxc is None:
        raise unsupported
    reps, c3k = {}, {}
    for i in (2, 4, 6, 8):
        n = 0
        while f"model.{i}.m.{n}.cv1.conv.weight" in tensors:
            n += 1
        reps[i], c3k[i] = n, f"model.{i}.m.0.cv3.conv.weight" in tensors
    n9 = 0
    while f"model.9.m.{n9}.attn.qkv.conv.weight" in tensors:
        n9 += 1
    reps[9] = n9
    if min(reps.values()) < 1 or len(set(reps.values())) != 1 or not (c3k[6] and c3k[8]) or c3k[2] != c3k[4] or c3k[2] != (width / 4 >= 1.0):
        raise unsupported
    want = _parse_model(_c3k_off_tensors(YOLO11_CLS_YAML[:10], tensors), 0,lambda c: _make_divisible(min(c, maxc) * width / 4), lambda i, n: reps[i] if n > 1 else n)
    _strict_compare(want, tensors, 10, unsupported, ignore=None, attn=(9,))
    return True


def cls_family(tensors: dict) -> str | None:
    """"yolo11-cls" / "yolov8-cls" for a checkpoint the ReID embedder runs, None for a file that is no classifier; a classifier of
    another topology raises NotImplementedError (is_yolo11_cls is asked first, then is_yolov8_cls)."""
    if is_yolo11_cls(tensors):
        return "yolo11-cls"
    return "yolov8-cls" if is_yolov8_cls(tensors) else None


def cls_imgsz(tensors: dict) -> int:
    """The classifier's input size: the optional ``cls.meta`` tensor ([imgsz], written by tools/convert_weights.py), else 224."""
    m = tensors.get("cls.meta")
    return int(np.asarray(m).ravel()[0]) if m is not None and np.size(m) else 224
