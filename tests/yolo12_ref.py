"""CPU restatement of the YOLO12 detect model (ultralytics cfg/models/12/yolo12.yaml) for the tests of the YOLO12 graph.

PARITY UNPINNED, like every file in oracle/: ultralytics is not installed where this was written, so nothing here was run against
the real package. It restates the public source from memory; the tensor names and shapes (geotrax_amd.weights.yolo12_layer_specs)
pin the widths and the Concat orders, the parameter counts of the five scales come out at 2.56 / 9.23 / 20.1 / 26.3 / 59.0 M (published:
2.6 / 9.3 / 20.2 / 26.4 / 59.1 M, BatchNorm parameters included there), and the attention is held against plain per-band, per-head
arithmetic in tests/test_yolo12.py. What neither pins is listed under "Doubts" below.

It subclasses tests/yolo11_ref.py's Yolo11Ref and reuses its arithmetic (_conv, _conv_res, _q, _bottleneck, _c3k, _c3k2; letterbox,
detect, NMS and obj_feats_table work on it as they are). Wiring (22 layers):
  0 Conv(64,3,2)  1 Conv(128,3,2)  2 C3k2(256, e=0.25)  3 Conv(256,3,2)  4 C3k2(512, e=0.25)  5 Conv(512,3,2)
  6 A2C2f(512, a2, area 4) x4  7 Conv(1024,3,2)  8 A2C2f(1024, a2, area 1) x4
  9 Upsample  10 Concat(-1, 6)  11 A2C2f(512) x2  12 Upsample  13 Concat(-1, 4)  14 A2C2f(256) x2
  15 Conv(256,3,2)  16 Concat(-1, 11)  17 A2C2f(512) x2  18 Conv(512,3,2)  19 Concat(-1, 8)  20 C3k2(1024, c3k) x2  21 Detect(14, 17, 20)
  - A2C2f(c1, c2, n, a2, area, residual, mlp_ratio, e = 0.5): c_ = c2 / 2; y = [cv1(x)]; each member maps the last entry and is
    appended; cv2(cat(y)). A member is two ABlocks in sequence (a2) or a C3k(c_, c_, 2). With a `gamma` tensor (scales l / x) the
    output is x + gamma[c] * that.
  - ABlock: x = x + attn(x); x = x + mlp.1(mlp.0(x)); mlp.0 has a SiLU, mlp.1 none.
  - AAttn(dim, heads = dim / 32, area): qkv = Conv 1x1 to 3 dim without activation; the H W positions, row-major, are cut into `area`
    contiguous runs; per run and head, softmax over the run's keys of (q^T k) * 32^-0.5, times v; runs back in map order; the result
    plus pe(v as a map), pe a depthwise 7x7 without activation, goes through proj (1x1, no activation).
Doubts:
  1. The interleaving of qkv's output channels. Taken as per head [q 32 | k 32 | v 32], heads consecutive (the package's
     `qkv.view(B, N, heads, 3 * head_dim).split(head_dim, dim=3)` as remembered). An older revision may have written
     [q of every head | k of every head | v of every head]; no shape tells the two apart. QKV_PER_HEAD here, the row permutation of
     YoloTrunk::ablock in csrc/yolo_trunk.cpp.
  2. The shortcut of the C3k members of A2C2f without a2 (model.11 / 14 / 17): A2C2f's own default, taken as on (A2C2F_C3K_SHORTCUT;
     kA2C2fC3kShortcut in csrc/yolo_tables.hpp).
  3. The shortcut of the neck's closing C3k2 (model.20): off, as this project takes it for every neck C3k2 (tests/yolo11_ref.py's doubt).
  4. Where the bands are cut when the package pads nothing: H W must be a multiple of `area` (the package's reshape would raise);
     the library refuses such a map at creation. A letterboxed rectangle cuts its bands across padded rows like any others.
  5. mlp.0's width int(c_ * mlp_ratio) at scales l / x (307 of 256, 460 of 384): taken as Python's int() of the product.
  6. gamma multiplies cv2's output after its SiLU, and x is the block's own input (c1 == c2 at both rows that have one).
The fp16 emulation rounds where the HIP path stores a map: every conv output, the attention output, attention + pe, the block sums."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from yolo11_ref import NECK_SHORTCUT, STRIDES, Yolo11Ref

QKV_PER_HEAD = True
A2C2F_C3K_SHORTCUT = True
AREAS = {"model.6": 4, "model.8": 1}


def area_attention(qkv: torch.Tensor, heads: int, area: int) -> torch.Tensor:
    """qkv [B, 96 heads, H, W] (QKV_PER_HEAD layout) -> [B, 32 heads, H, W]: softmax(q^T k / sqrt(32)) v inside each of `area`
    contiguous runs of the row-major positions. Computed in qkv's dtype (float64 for the kernel tests)."""
    B, C3, H, W = qkv.shape
    N = H * W
    assert C3 == heads * 96 and N % area == 0
    t = qkv.flatten(2).transpose(1, 2)                               # [B, N, 96 heads]
    if QKV_PER_HEAD:
        q, k, v = t.reshape(B, N, heads, 96).split(32, dim=3)
    else:
        q, k, v = t.reshape(B, N, 3, heads, 32).unbind(2)
    Nb = N // area
    q, k, v = (z.reshape(B, area, Nb, heads, 32).permute(0, 1, 3, 2, 4) for z in (q, k, v))   # [B, area, heads, Nb, 32]
    attn = ((q @ k.transpose(-2, -1)) * 32 ** -0.5).softmax(dim=-1)
    y = (attn @ v).permute(0, 1, 3, 2, 4).reshape(B, N, heads * 32)   # bands back in map order, head-major channels
    return y.transpose(1, 2).reshape(B, heads * 32, H, W)


def v_map(qkv: torch.Tensor, heads: int) -> torch.Tensor:
    """The v channels of a qkv map as a [B, 32 heads, H, W] map, head-major"""
    B, _, H, W = qkv.shape
    if QKV_PER_HEAD:
        return qkv.reshape(B, heads, 96, H, W)[:, :, 64:].reshape(B, heads * 32, H, W)
    return qkv[:, 64 * heads:]


class Yolo12Ref(Yolo11Ref):
    def __init__(self, tensors, emulate_half: bool = False):
        self.t = {k: torch.from_numpy(np.asarray(v, dtype=np.float32)) for k, v in tensors.items()}
        self.half = emulate_half
        self.nc = int(self.t["model.21.cv3.0.2.weight"].shape[0])
        self.acts: dict[str, torch.Tensor] = {}

    def _aattn(self, m: str, x: torch.Tensor, area: int) -> torch.Tensor:
        heads = x.shape[1] // 32
        qkv = self._conv(m + ".qkv.conv", x, act=False)
        self.acts[m + ".out"] = y = self._q(area_attention(qkv, heads, area))
        w = self._q(self.t[m + ".pe.conv.weight"])
        pe = F.conv2d(v_map(qkv, heads), w, self.t.get(m + ".pe.conv.bias"), padding=3, groups=x.shape[1])
        self.acts[m + ".pe.conv"] = y = self._q(y + pe)
        return self._conv(m + ".proj.conv", y, act=False, quant_out=False)

    def _ablock(self, m: str, x: torch.Tensor, area: int) -> torch.Tensor:
        x = self._q(x + self._aattn(m + ".attn", x, area))
        return self._q(x + self._conv(m + ".mlp.1.conv", self._conv(m + ".mlp.0.conv", x), act=False, quant_out=False))

    def _a2c2f(self, pfx: str, x: torch.Tensor) -> torch.Tensor:
        y = [self._conv(pfx + ".cv1.conv", x)]
        k = 0
        while f"{pfx}.m.{k}.0.attn.qkv.conv.weight" in self.t or f"{pfx}.m.{k}.cv1.conv.weight" in self.t:
            m = f"{pfx}.m.{k}"
            if m + ".0.attn.qkv.conv.weight" in self.t:
                z = self._ablock(m + ".1", self._ablock(m + ".0", y[-1], AREAS[pfx]), AREAS[pfx])
                self.acts[m] = z
            else:
                z = self._c3k(m, y[-1], A2C2F_C3K_SHORTCUT)
            y.append(z)
            k += 1
        out = self._conv(pfx + ".cv2.conv", torch.cat(y, 1))
        if pfx + ".gamma" in self.t:
            out = self._q(x + self.t[pfx + ".gamma"].view(1, -1, 1, 1) * out)
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
        x6 = self._a2c2f("model.6", x5)
        a["model.7.conv"] = x7 = self._conv("model.7.conv", x6, 2)
        x8 = self._a2c2f("model.8", x7)
        up = lambda t: F.interpolate(t, scale_factor=2, mode="nearest")
        x11 = self._a2c2f("model.11", torch.cat([up(x8), x6], 1))
        x14 = self._a2c2f("model.14", torch.cat([up(x11), x4], 1))
        a["model.15.conv"] = x15 = self._conv("model.15.conv", x14, 2)
        x17 = self._a2c2f("model.17", torch.cat([x15, x11], 1))
        a["model.18.conv"] = x18 = self._conv("model.18.conv", x17, 2)
        x20 = self._c3k2("model.20", torch.cat([x18, x8], 1), NECK_SHORTCUT)

        self.detect_inputs = (x14, x17, x20)
        outs = []
        for l, (f, stride) in enumerate(zip(self.detect_inputs, STRIDES)):
            d = "model.21"
            b = self._conv(f"{d}.cv2.{l}.1.conv", self._conv(f"{d}.cv2.{l}.0.conv", f))
            c = self._conv(f"{d}.cv3.{l}.0.1.conv", self._dwconv(f"{d}.cv3.{l}.0.0.conv", f, True))
            c = self._conv(f"{d}.cv3.{l}.1.1.conv", self._dwconv(f"{d}.cv3.{l}.1.0.conv", c, True))
            a[f"{d}.feat{l}"] = torch.cat([b, c], 1)
            box = F.conv2d(b, self.t[f"{d}.cv2.{l}.2.weight"], self.t[f"{d}.cv2.{l}.2.bias"])
            cls = F.conv2d(c, self.t[f"{d}.cv3.{l}.2.weight"], self.t[f"{d}.cv3.{l}.2.bias"])
            a[f"{d}.cls{l}"] = cls                     # class logits, for the tests' calibration
            B, _, H, W = box.shape
            p = box.view(B, 4, 16, H * W).softmax(2)
            dist = (p * torch.arange(16, dtype=p.dtype).view(1, 1, 16, 1)).sum(2)
            ys, xs = torch.meshgrid(torch.arange(H, dtype=p.dtype) + 0.5, torch.arange(W, dtype=p.dtype) + 0.5, indexing="ij")
            anc = torch.stack([xs.reshape(-1), ys.reshape(-1)], 0)[None]
            x1y1, x2y2 = anc - dist[:, :2], anc + dist[:, 2:]
            xywh = torch.cat([(x1y1 + x2y2) / 2, x2y2 - x1y1], 1) * stride
            outs.append(torch.cat([xywh, cls.view(B, self.nc, H * W).sigmoid()], 1))
        return torch.cat(outs, 2).transpose(1, 2).contiguous()
