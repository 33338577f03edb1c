"""CPU restatement of the YOLOv9 detect models (ultralytics cfg/models/v9/yolov9{t,s,m,c}.yaml) for the tests of the YOLOv9 graph.

PARITY UNPINNED, like every file in oracle/ and tests/yolov10_ref.py: ultralytics is not installed where this was written, so nothing
here was run against the real package. It restates the public source from memory; the tensor names and shapes
(geotrax_amd.weights.yolov9_layer_specs) pin the widths, the repeat counts and the Concat orders of the four scales, and the
parameter counts of the four tables come out at 2.1 / 7.2 / 20.1 / 25.4 M (nc = 80; published: 2.0 / 7.2 / 20.1 / 25.5 M). What
they do not pin is listed under "Doubt" below.

It subclasses tests/yolo11_ref.py's Yolo11Ref and reuses its arithmetic (_conv, _conv_res, _bottleneck, _c3k, _q); the ELAN blocks,
the two downsampling modules, SPPELAN and the pooling arithmetic are written out here. Every method follows the dtype of its input,
so a float64 run is `Yolov9Ref(w).double().forward(x.double())`. Wiring (s scale; t the same at smaller widths; m and c with
RepNCSPELAN4(n = 1) at row 2; c with ADown in place of every AConv):
  0 Conv(3,2)  1 Conv(3,2)  2 ELAN1  3 AConv  4 RepNCSPELAN4(n=3)  5 AConv  6 RepNCSPELAN4  7 AConv  8 RepNCSPELAN4  9 SPPELAN
  10 Upsample  11 Concat(-1, 6)  12 RepNCSPELAN4  13 Upsample  14 Concat(-1, 4)  15 RepNCSPELAN4
  16 AConv  17 Concat(-1, 12)  18 RepNCSPELAN4  19 AConv  20 Concat(-1, 9)  21 RepNCSPELAN4  22 Detect(15, 18, 21)
  - RepNCSPELAN4(c1, c2, c3, c4, n): y = chunk(cv1(x), 2); y += [cv2(y[-1])]; y += [cv3(y[-1])]; cv4(cat(y)). cv2 / cv3 =
    Sequential(RepCSP(., c4, n), Conv3x3). ELAN1: the same with a plain Conv3x3 for cv2 and cv3.
  - RepCSP(c1, c2, n) = C3 with e = 0.5: cv3(cat(m(cv1(x)), cv2(x))), m = n RepBottlenecks(c_, c_, e = 1.0) = x + Conv3x3(RepConv(x));
    RepConv = SiLU(conv3x3(x) + conv1x1(x)), no identity branch; fused: one 3x3 (`...m.k.cv1.conv`). That is yolo11_ref's _c3k.
  - AConv: cv1(avg_pool2d(x, 2, 1, 0)), cv1 = Conv 3x3 stride 2 pad 1.
  - ADown: a = avg_pool2d(x, 2, 1, 0); x1, x2 = chunk(a, 2); cat(cv1(x1), cv2(max_pool2d(x2, 3, 2, 1))), cv1 = Conv 3x3 stride 2,
    cv2 = Conv 1x1.
  - SPPELAN: y = [cv1(x)]; three times y += [max_pool2d(y[-1], 5, 1, 2)]; cv5(cat(y)).
  - Detect: YOLOv8's (the legacy head: cv3[l] = Conv3x3, Conv3x3, Conv2d), model.22.
Doubt:
  - the shortcut of the RepBottlenecks (taken as on everywhere: RepNCSPELAN4 builds RepCSP with its default shortcut = True, backbone
    and neck alike; SHORTCUT here, the `true` of every ELAN row of kYolo9 in csrc/yolo_tables.hpp). No tensor tells.
  - avg_pool2d's remaining arguments (ceil_mode False, count_include_pad True: without padding neither changes a value).
  - that parse_model hands Detect its legacy form for the v9 yamls of the pinned ultralytics range (no C3k2 in them, so `legacy`
    stays True); a file with the depthwise class branch is refused by check_yolov9's shape comparison, not misread.
The fp16 emulation rounds where the HIP path stores a map: every conv output, the averaged map, the pooled maximum."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from yolo11_ref import STRIDES, Yolo11Ref

SHORTCUT = True


# ---------------------------------------------------------------------------- the pooling arithmetic, written out
def avgpool2_s1(x: torch.Tensor) -> torch.Tensor:
    """avg_pool2d(x, 2, 1, 0) on [..., H, W] -> [..., H - 1, W - 1]: two horizontal sums, their sum, times 0.25 (the HIP kernel's order)"""
    return 0.25 * ((x[..., :-1, :-1] + x[..., :-1, 1:]) + (x[..., 1:, :-1] + x[..., 1:, 1:]))


def zero_border(a: torch.Tensor) -> torch.Tensor:
    """The (H - 1) x (W - 1) map as the HIP path stores it: H x W with a zero last row and column"""
    return F.pad(a, (0, 1, 0, 1))


def maxpool3_s2(a: torch.Tensor) -> torch.Tensor:
    """max_pool2d(a, 3, 2, 1) on [..., h, w]: the window's taps outside the map are excluded (-inf), not zero"""
    h, w = a.shape[-2:]
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    p = F.pad(a, (1, 2, 1, 2), value=float("-inf"))
    taps = [p[..., dy:dy + 2 * ho:2, dx:dx + 2 * wo:2] for dy in range(3) for dx in range(3)]
    return torch.stack(taps, 0).amax(0)


def store(x: np.ndarray, fmt: str) -> np.ndarray:
    """float64 / fp32 values -> what a map of the format holds, as float64: "f32", "f16", or "split" (the pair format: hi = fp16(x),
    lo = fp16(x - hi), the value hi + lo)"""
    if fmt == "f32":
        return x.astype(np.float32).astype(np.float64)
    if fmt == "f16":
        return x.astype(np.float16).astype(np.float64)
    x32 = x.astype(np.float32)
    hi = x32.astype(np.float16)
    lo = (x32 - hi.astype(np.float32)).astype(np.float16)
    return (hi.astype(np.float32) + lo.astype(np.float32)).astype(np.float64)


def ulp(x: np.ndarray, fmt: str) -> np.ndarray:
    """One unit in the last place of the format at |x| (float64): 11 significand bits for fp16 (subnormal spacing 2^-24), 24 for fp32,
    22 for the pair format (hi carries 11 bits, lo 11 more of the remainder; lo's own floor is fp16's subnormal spacing)"""
    bits, floor = {"f16": (11, -24), "f32": (24, -149), "split": (22, -24)}[fmt]
    e = np.floor(np.log2(np.maximum(np.abs(x), 2.0 ** -140)))
    return 2.0 ** np.maximum(e - (bits - 1), floor)


def pool_down_nhwc(x: np.ndarray, c_avg: int, fmt: str, exact: bool = False):
    """Reference of gtx_op_pool_down on [n, h, w, c] values the format holds exactly: (avg [n, h, w, c_avg] with its zero border, max
    [n, h/2, w/2, c - c_avg] or None) as float64, each rounded once, where the map is stored. "f32" (and exact=True): the sums in
    float64 -- the yardstick for the kernel's own fp32 rounding. "f16" / "split": the format's emulation, sums in fp32 in the kernel's
    order ((a + b) + (c + d), times 0.25: every step one IEEE fp32 operation, as on the GPU), then the one rounding into the format."""
    dt = np.float64 if fmt == "f32" or exact else np.float32
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).permute(0, 3, 1, 2)
    a = avgpool2_s1(t)
    avg = store(zero_border(a[:, :c_avg]).permute(0, 2, 3, 1).numpy().astype(np.float64), fmt)
    mx = store(maxpool3_s2(a[:, c_avg:]).permute(0, 2, 3, 1).numpy().astype(np.float64), fmt) if c_avg < x.shape[3] else None
    return avg, mx


class Yolov9Ref(Yolo11Ref):
    def __init__(self, tensors, emulate_half: bool = False):
        self.t = {k: torch.from_numpy(np.asarray(v, dtype=np.float32)) for k, v in tensors.items()}
        self.half = emulate_half
        self.nc = int(self.t["model.22.cv3.0.2.weight"].shape[0])
        self.acts: dict[str, torch.Tensor] = {}

    def double(self) -> "Yolov9Ref":
        self.t = {k: v.double() for k, v in self.t.items()}
        return self

    def _elan(self, pfx: str, x: torch.Tensor) -> torch.Tensor:
        y = list(self._conv(pfx + ".cv1.conv", x).chunk(2, 1))
        for b in ("cv2", "cv3"):
            if f"{pfx}.{b}.0.cv1.conv.weight" in self.t:         # Sequential(RepCSP, Conv3x3)
                self.acts[f"{pfx}.{b}.0.cv3.conv"] = r = self._c3k(f"{pfx}.{b}.0", y[-1], SHORTCUT)
                y.append(self._conv(f"{pfx}.{b}.1.conv", r))
            else:                                                 # ELAN1
                y.append(self._conv(f"{pfx}.{b}.conv", y[-1]))
        self.acts[pfx] = out = self._conv(pfx + ".cv4.conv", torch.cat(y, 1))
        return out

    def _down(self, pfx: str, x: torch.Tensor) -> torch.Tensor:
        a = avgpool2_s1(x)
        if pfx + ".cv2.conv.weight" not in self.t:                # AConv
            a = self._q(a)
            self.acts[pfx + ".pool"] = zero_border(a)
            self.acts[pfx] = out = self._conv(pfx + ".cv1.conv", a, 2)
            return out
        x1, x2 = a.chunk(2, 1)                                    # ADown
        x1, x2 = self._q(x1), self._q(maxpool3_s2(x2))
        self.acts[pfx + ".pool"], self.acts[pfx + ".maxpool"] = zero_border(x1), x2
        self.acts[pfx] = out = torch.cat([self._conv(pfx + ".cv1.conv", x1, 2), self._conv(pfx + ".cv2.conv", x2)], 1)
        return out

    def _sppelan(self, pfx: str, x: torch.Tensor) -> torch.Tensor:
        y = [self._conv(pfx + ".cv1.conv", x)]
        for _ in range(3):
            y.append(F.max_pool2d(y[-1], 5, 1, 2))
        self.acts[pfx] = out = self._conv(pfx + ".cv5.conv", torch.cat(y, 1))
        return out

    @torch.no_grad()
    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """[B, A, 4 + nc]: xywh in network pixels + sigmoid class scores"""
        a = self.acts
        x = self._q(x)
        a["model.0.conv"] = x0 = self._conv("model.0.conv", x, 2)
        a["model.1.conv"] = x1 = self._conv("model.1.conv", x0, 2)
        x2 = self._elan("model.2", x1)
        x4 = self._elan("model.4", self._down("model.3", x2))
        x6 = self._elan("model.6", self._down("model.5", x4))
        x8 = self._elan("model.8", self._down("model.7", x6))
        x9 = self._sppelan("model.9", x8)
        up = lambda t: F.interpolate(t, scale_factor=2, mode="nearest")
        x12 = self._elan("model.12", torch.cat([up(x9), x6], 1))
        x15 = self._elan("model.15", torch.cat([up(x12), x4], 1))
        x18 = self._elan("model.18", torch.cat([self._down("model.16", x15), x12], 1))
        x21 = self._elan("model.21", torch.cat([self._down("model.19", x18), x9], 1))
        self.detect_inputs = (x15, x18, x21)
        outs, d = [], "model.22"
        for l, (f, stride) in enumerate(zip(self.detect_inputs, STRIDES)):
            b = self._conv(f"{d}.cv2.{l}.1.conv", self._conv(f"{d}.cv2.{l}.0.conv", f))
            c = self._conv(f"{d}.cv3.{l}.1.conv", self._conv(f"{d}.cv3.{l}.0.conv", f))
            a[f"{d}.feat{l}"] = torch.cat([b, c], 1)
            box = F.conv2d(b, self.t[f"{d}.cv2.{l}.2.weight"], self.t[f"{d}.cv2.{l}.2.bias"])
            cls = F.conv2d(c, self.t[f"{d}.cv3.{l}.2.weight"], self.t[f"{d}.cv3.{l}.2.bias"])
            B, _, H, W = box.shape
            p = box.view(B, 4, 16, H * W).softmax(2)
            dist = (p * torch.arange(16, dtype=box.dtype).view(1, 1, 16, 1)).sum(2)
            ys, xs = torch.meshgrid(torch.arange(H, dtype=box.dtype) + 0.5, torch.arange(W, dtype=box.dtype) + 0.5, indexing="ij")
            anc = torch.stack([xs.reshape(-1), ys.reshape(-1)], 0)[None]
            x1y1, x2y2 = anc - dist[:, :2], anc + dist[:, 2:]
            xywh = torch.cat([(x1y1 + x2y2) / 2, x2y2 - x1y1], 1) * stride
            outs.append(torch.cat([xywh, cls.view(B, self.nc, H * W).sigmoid()], 1))
        return torch.cat(outs, 2).transpose(1, 2).contiguous()


def rep_bottleneck_unfused(x: torch.Tensor, t: dict, p: str, eps: float = 1e-3) -> torch.Tensor:
    """RepBottleneck.forward before any fusing, from an unfused state dict under prefix p: x + cv2(cv1(x)), cv1 = RepConv =
    SiLU(BN(conv3x3(x)) + BN(conv1x1(x))), cv2 = SiLU(BN(conv3x3(.))). BatchNorm in eval mode, written out."""
    def bn(y, q):
        s = t[q + ".weight"] / torch.sqrt(t[q + ".running_var"] + eps)
        return (y - t[q + ".running_mean"][None, :, None, None]) * s[None, :, None, None] + t[q + ".bias"][None, :, None, None]

    r = F.silu(bn(F.conv2d(x, t[p + ".cv1.conv1.conv.weight"], padding=1), p + ".cv1.conv1.bn") +
               bn(F.conv2d(x, t[p + ".cv1.conv2.conv.weight"]), p + ".cv1.conv2.bn"))
    return x + F.silu(bn(F.conv2d(r, t[p + ".cv2.conv.weight"], padding=1), p + ".cv2.bn"))
