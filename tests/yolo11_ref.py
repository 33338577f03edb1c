"""CPU restatement of the YOLO11 detect model (ultralytics cfg/models/11/yolo11.yaml) for the tests of the YOLO11 graph.

PARITY UNPINNED, like every file in oracle/: ultralytics is not installed where this was written, so nothing here was run against
the real package. It restates the public source from memory; the tensor names and shapes (geotrax_amd.weights.yolo11_layer_specs)
pin the widths and the Concat orders of the n / s scales, the parameter counts of the five scales come out at the published
2.6 / 9.4 / 20.1 / 25.3 / 56.9 M, and the two new blocks are held against plain torch.nn.functional written out longhand in
tests/test_yolo11.py. What neither pins is listed under "Doubt" below.

It subclasses oracle/yolov8_ref.py's YoloV8Ref and reuses its arithmetic (_conv, _conv_res, _sppf, _q; letterbox, detect, NMS and
obj_feats_table work on it as they are). Wiring:
  0 Conv(64,3,2)  1 Conv(128,3,2)  2 C3k2(256, e=0.25)  3 Conv(256,3,2)  4 C3k2(512, e=0.25)  5 Conv(512,3,2)  6 C3k2(512, c3k)
  7 Conv(1024,3,2)  8 C3k2(1024, c3k)  9 SPPF(1024, 5)  10 C2PSA(1024)
  11 Upsample  12 Concat(-1, 6)  13 C3k2(512)  14 Upsample  15 Concat(-1, 4)  16 C3k2(256)
  17 Conv(256,3,2)  18 Concat(-1, 13)  19 C3k2(512)  20 Conv(512,3,2)  21 Concat(-1, 10)  22 C3k2(1024, c3k)  23 Detect(16, 19, 22)
  - C3k2 = C2f whose m.{k} is Bottleneck(c, c, 3x3 + 3x3, e = 0.5) or, when the block has a cv3, C3k: cv3(cat(m(cv1(x)), cv2(x)))
    with m = Bottlenecks of e = 1.0. Which of the two, the widths and the repeat counts are read off the tensors.
  - C2PSA: cv1 -> a | b; per PSABlock b = b + attn(b), b = b + ffn.1(ffn.0(b)); cv2(cat(a, b)). Attention: heads = c / 64, per head
    the qkv channels are [q 32 | k 32 | v 64]; softmax over the keys of (q^T k) * 32^-0.5; x = v attn^T + pe(v); proj(x).
    qkv, proj, pe (depthwise 3x3) and ffn.1 have no activation.
  - Detect: cv2 as in YOLOv8; cv3[l] = DWConv(3x3) + Conv(1x1), DWConv(3x3) + Conv(1x1), Conv2d(1x1); DWConv has a SiLU.
Doubt: the shortcut flag of the neck's C3k2 blocks (13 / 16 / 19 / 22). It is taken as off, as in YOLOv8's neck. The yaml passes
[c2, c3k] only and C3k2's own default for `shortcut` may be True in the package; no tensor name or shape tells the two apart, so a
real checkpoint is the only thing that can settle it (NECK_SHORTCUT here, kNeckShortcut in csrc/yolo_trunk.cpp).
The fp16 emulation rounds where the HIP path stores a map: every conv output, the attention output, the depthwise outputs."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from oracle.yolov8_ref import YoloV8Ref

STRIDES = (8.0, 16.0, 32.0)
NECK_SHORTCUT = False


class Yolo11Ref(YoloV8Ref):
    def __init__(self, tensors, emulate_half: bool = False):   # the parent's, with nc read from Detect = model.23
        self.t = {k: torch.from_numpy(np.asarray(v, dtype=np.float32)) for k, v in tensors.items()}
        self.half = emulate_half
        self.nc = int(self.t["model.23.cv3.0.2.weight"].shape[0])
        self.acts: dict[str, torch.Tensor] = {}

    def _dwconv(self, name: str, x: torch.Tensor, act: bool, quant_out: bool = True) -> torch.Tensor:
        w = self._q(self.t[name + ".weight"])
        y = F.conv2d(x, w, self.t.get(name + ".bias"), padding=1, groups=x.shape[1])
        if act:
            y = F.silu(y)
        return self._q(y) if quant_out else y

    def _bottleneck(self, m: str, x: torch.Tensor, shortcut: bool) -> torch.Tensor:
        return self._conv_res(m + ".cv2.conv", self._conv(m + ".cv1.conv", x), x if shortcut else None)

    def _c3k(self, m: str, x: torch.Tensor, shortcut: bool) -> torch.Tensor:
        y = self._conv(m + ".cv1.conv", x)
        j = 0
        while f"{m}.m.{j}.cv1.conv.weight" in self.t:
            y = self._bottleneck(f"{m}.m.{j}", y, shortcut)
            j += 1
        return self._conv(m + ".cv3.conv", torch.cat([y, self._conv(m + ".cv2.conv", x)], 1))

    def _c3k2(self, pfx: str, x: torch.Tensor, shortcut: bool) -> torch.Tensor:
        y = list(self._conv(pfx + ".cv1.conv", x).chunk(2, 1))
        k = 0
        while f"{pfx}.m.{k}.cv1.conv.weight" in self.t:
            m = f"{pfx}.m.{k}"
            y.append(self._c3k(m, y[-1], shortcut) if m + ".cv3.conv.weight" in self.t else self._bottleneck(m, y[-1], shortcut))
            k += 1
        out = self._conv(pfx + ".cv2.conv", torch.cat(y, 1))
        self.acts[pfx] = out
        return out

    def _attention(self, m: str, x: torch.Tensor) -> torch.Tensor:
        """ultralytics Attention(dim, num_heads = dim / 64, attn_ratio = 0.5).forward"""
        B, C, H, W = x.shape
        heads, N = C // 64, H * W
        qkv = self._conv(m + ".qkv.conv", x, act=False)
        self.acts[m + ".qkv.conv"] = qkv
        q, k, v = qkv.view(B, heads, 128, N).split([32, 32, 64], dim=2)
        attn = ((q.transpose(-2, -1) @ k) * 32 ** -0.5).softmax(dim=-1)
        y = (v @ attn.transpose(-2, -1)).view(B, C, H, W) + self._dwconv(m + ".pe.conv", v.reshape(B, C, H, W), act=False, quant_out=False)
        self.acts[m + ".out"] = y = self._q(y)
        return self._conv(m + ".proj.conv", y, act=False, quant_out=False)

    def _c2psa(self, pfx: str, x: torch.Tensor) -> torch.Tensor:
        a, b = self._conv(pfx + ".cv1.conv", x).chunk(2, 1)
        k = 0
        while f"{pfx}.m.{k}.attn.qkv.conv.weight" in self.t:
            m = f"{pfx}.m.{k}"
            b = self._q(b + self._attention(m + ".attn", b))
            b = self._q(b + self._conv(m + ".ffn.1.conv", self._conv(m + ".ffn.0.conv", b), act=False, quant_out=False))
            k += 1
        out = self._conv(pfx + ".cv2.conv", torch.cat([a, b], 1))
        self.acts[pfx] = out
        return out

    @torch.no_grad()
    def forward(self, x: torch.Tensor) -> torch.Tensor:
        a = self.acts
        x = self._q(x)
        a["model.0.conv"] = x0 = self._conv("model.0.conv", x, 2)
        a["model.1.conv"] = x1 = self._conv("model.1.conv", x0, 2)
        x2 = self._c3k2("model.2", x1, True)
        a["model.3.conv"] = x3 = self._conv("model.3.conv", x2, 2)
        x4 = self._c3k2("model.4", x3, True)
        a["model.5.conv"] = x5 = self._conv("model.5.conv", x4, 2)
        x6 = self._c3k2("model.6", x5, True)
        a["model.7.conv"] = x7 = self._conv("model.7.conv", x6, 2)
        x8 = self._c3k2("model.8", x7, True)
        x9 = self._sppf("model.9", x8)
        x10 = self._c2psa("model.10", x9)
        up = lambda t: F.interpolate(t, scale_factor=2, mode="nearest")
        x13 = self._c3k2("model.13", torch.cat([up(x10), x6], 1), NECK_SHORTCUT)
        x16 = self._c3k2("model.16", torch.cat([up(x13), x4], 1), NECK_SHORTCUT)
        a["model.17.conv"] = x17 = self._conv("model.17.conv", x16, 2)
        x19 = self._c3k2("model.19", torch.cat([x17, x13], 1), NECK_SHORTCUT)
        a["model.20.conv"] = x20 = self._conv("model.20.conv", x19, 2)
        x22 = self._c3k2("model.22", torch.cat([x20, x10], 1), NECK_SHORTCUT)

        self.detect_inputs = (x16, x19, x22)
        outs = []
        for l, (f, stride) in enumerate(zip(self.detect_inputs, STRIDES)):
            d = "model.23"
            b = self._conv(f"{d}.cv2.{l}.1.conv", self._conv(f"{d}.cv2.{l}.0.conv", f))
            c = self._conv(f"{d}.cv3.{l}.0.1.conv", self._dwconv(f"{d}.cv3.{l}.0.0.conv", f, True))
            c = self._conv(f"{d}.cv3.{l}.1.1.conv", self._dwconv(f"{d}.cv3.{l}.1.0.conv", c, True))
            a[f"{d}.feat{l}"] = torch.cat([b, c], 1)
            box = F.conv2d(b, self.t[f"{d}.cv2.{l}.2.weight"], self.t[f"{d}.cv2.{l}.2.bias"])
            cls = F.conv2d(c, self.t[f"{d}.cv3.{l}.2.weight"], self.t[f"{d}.cv3.{l}.2.bias"])
            B, _, H, W = box.shape
            p = box.view(B, 4, 16, H * W).softmax(2)
            dist = (p * torch.arange(16, dtype=torch.float32).view(1, 1, 16, 1)).sum(2)
            ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32) + 0.5,
                                    torch.arange(W, dtype=torch.float32) + 0.5, indexing="ij")
            anc = torch.stack([xs.reshape(-1), ys.reshape(-1)], 0)[None]
            x1y1, x2y2 = anc - dist[:, :2], anc + dist[:, 2:]
            xywh = torch.cat([(x1y1 + x2y2) / 2, x2y2 - x1y1], 1) * stride
            outs.append(torch.cat([xywh, cls.view(B, self.nc, H * W).sigmoid()], 1))
        return torch.cat(outs, 2).transpose(1, 2).contiguous()
