"""CPU restatement of the YOLOv5u detect model (ultralytics cfg/models/v5/yolov5.yaml with the anchor-free Detect) for the tests of the
YOLOv5u graph.

PARITY UNPINNED, like every file in oracle/: ultralytics is not installed where this was written, so nothing here was run against
the real package. It restates the public source from memory; the tensor names and shapes (geotrax_amd.weights.yolov5u_layer_specs)
pin the widths and the Concat orders, and the parameter counts of the five scales come out at 2.50 / 9.11 / 25.05 / 53.13 / 97.16 M
(published for yolov5{n,s,m,l,x}u: 2.6 / 9.1 / 25.1 / 53.2 / 97.2 M, BatchNorm parameters included there). What neither pins is listed
under "Doubts" below.

It subclasses tests/yolo11_ref.py's Yolo11Ref and reuses its arithmetic (_conv, _conv_res, _q, _bottleneck, _sppf; letterbox, detect,
NMS and obj_feats_table work on it as they are). Wiring (25 layers):
  0 Conv(64,6,2,2)  1 Conv(128,3,2)  2 C3(128) x3  3 Conv(256,3,2)  4 C3(256) x6  5 Conv(512,3,2)  6 C3(512) x9  7 Conv(1024,3,2)
  8 C3(1024) x3  9 SPPF(1024, 5)
  10 Conv(512,1,1)  11 Upsample  12 Concat(-1, 6)  13 C3(512, False) x3  14 Conv(256,1,1)  15 Upsample  16 Concat(-1, 4)  17 C3(256, False) x3
  18 Conv(256,3,2)  19 Concat(-1, 14)  20 C3(512, False) x3  21 Conv(512,3,2)  22 Concat(-1, 10)  23 C3(1024, False) x3  24 Detect(17, 20, 23)
  - Conv(c2, 6, 2, 2): kernel 6, stride 2, padding 2 -- the one layer whose padding is not k // 2: output (oy, ox) reads rows
    2 oy - 2 .. 2 oy + 3 and columns 2 ox - 2 .. 2 ox + 3.
  - C3(c1, c2, n, shortcut, e = 0.5): c_ = c2 / 2; cv3(cat(m(cv1(x)), cv2(x))), cv1 / cv2 / cv3 1x1, m = n x Bottleneck(c_, c_, shortcut,
    k = (1x1, 3x3), e = 1.0).
  - Detect: YOLOv8's (cv2 / cv3 of two 3x3 Convs and a 1x1 Conv2d per level, DFL over 16 bins).
Doubts:
  1. C3's hidden width: e = 0.5 of c2, the module's default, which the yaml never overrides (C3_E).
  2. The depth rounding: parse_model's max(round(n * depth), 1) with Python's round -- 3 / 6 / 9 / 3 repeats become 1 / 2 / 3 / 1 at n and
     s (0.33), 2 / 4 / 6 / 2 at m (0.67), 3 / 6 / 9 / 3 at l, 4 / 8 / 12 / 4 at x (1.33). No product lands on a half, so the rounding mode
     cannot matter; the depth multiples themselves are from memory.
  3. The neck's shortcut flags: the yaml writes `[c2, False]` for model.13 / 17 / 20 / 23 (NECK_SHORTCUT) and nothing -- the module's
     default, True -- in the backbone. No tensor tells either.
  4. max_channels: 1024 at every scale (so that scale x reaches 1280 channels at model.7 - 9 and scale l 1024), unlike yolov8.yaml's
     768 / 512 at m / l / x.
The fp16 emulation rounds where the HIP path stores a map: every conv output, the block sums."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from yolo11_ref import STRIDES, Yolo11Ref

C3_E = 0.5
NECK_SHORTCUT = False
DETECT = "model.24"


def stack_c3(t: dict, pfx: str):
    """cv2's rows on top of cv1's, with their biases: the one 1x1 convolution the HIP path launches for the pair ([cv2 x | cv1 x])"""
    w = torch.cat([t[pfx + ".cv2.conv.weight"], t[pfx + ".cv1.conv.weight"]], 0)
    b = torch.cat([t[pfx + ".cv2.conv.bias"], t[pfx + ".cv1.conv.bias"]], 0)
    return w, b


def w108_of(w_oihw: np.ndarray) -> np.ndarray:
    """[c0][3][6][6] -> the stem kernels' tap-major [108][c0], row (ky * 6 + kx) * 3 + colour"""
    w = np.asarray(w_oihw)
    return np.ascontiguousarray(w.transpose(2, 3, 1, 0).reshape(108, w.shape[0]))


def oihw_of(w108: np.ndarray) -> np.ndarray:
    """w108_of's inverse"""
    w = np.asarray(w108)
    return np.ascontiguousarray(w.reshape(6, 6, 3, -1).transpose(3, 2, 0, 1))


class Yolov5uRef(Yolo11Ref):
    def __init__(self, tensors, emulate_half: bool = False):
        self.t = {k: torch.from_numpy(np.asarray(v, dtype=np.float32)) for k, v in tensors.items()}
        self.half = emulate_half
        self.nc = int(self.t[DETECT + ".cv3.0.2.weight"].shape[0])
        self.acts: dict[str, torch.Tensor] = {}

    def _stem(self, x: torch.Tensor) -> torch.Tensor:
        w = self._q(self.t["model.0.conv.weight"])
        assert tuple(w.shape[1:]) == (3, 6, 6)
        return self._q(F.silu(F.conv2d(x, w, self.t.get("model.0.conv.bias"), stride=2, padding=2)))

    def _c3(self, pfx: str, x: torch.Tensor, shortcut: bool) -> torch.Tensor:
        assert self.t[pfx + ".cv1.conv.weight"].shape[0] == int(self.t[pfx + ".cv3.conv.weight"].shape[0] * C3_E)
        y = self._conv(pfx + ".cv1.conv", x)
        self.acts[pfx + ".cv1.conv"] = y
        j = 0
        while f"{pfx}.m.{j}.cv1.conv.weight" in self.t:
            y = self._bottleneck(f"{pfx}.m.{j}", y, shortcut)
            j += 1
        z = self._conv(pfx + ".cv2.conv", x)
        self.acts[pfx + ".cv2.conv"] = z
        out = self._conv(pfx + ".cv3.conv", torch.cat([y, z], 1))
        self.acts[pfx] = out
        return out

    @torch.no_grad()
    def forward(self, x: torch.Tensor) -> torch.Tensor:
        a = self.acts
        x = self._q(x)
        a["model.0.conv"] = x0 = self._stem(x)
        a["model.1.conv"] = x1 = self._conv("model.1.conv", x0, 2)
        x2 = self._c3("model.2", x1, True)
        a["model.3.conv"] = x3 = self._conv("model.3.conv", x2, 2)
        x4 = self._c3("model.4", x3, True)
        a["model.5.conv"] = x5 = self._conv("model.5.conv", x4, 2)
        x6 = self._c3("model.6", x5, True)
        a["model.7.conv"] = x7 = self._conv("model.7.conv", x6, 2)
        x8 = self._c3("model.8", x7, True)
        x9 = self._sppf("model.9", x8)
        a["model.10.conv"] = x10 = self._conv("model.10.conv", x9)
        up = lambda t: F.interpolate(t, scale_factor=2, mode="nearest")
        x13 = self._c3("model.13", torch.cat([up(x10), x6], 1), NECK_SHORTCUT)
        a["model.14.conv"] = x14 = self._conv("model.14.conv", x13)
        x17 = self._c3("model.17", torch.cat([up(x14), x4], 1), NECK_SHORTCUT)
        a["model.18.conv"] = x18 = self._conv("model.18.conv", x17, 2)
        x20 = self._c3("model.20", torch.cat([x18, x14], 1), NECK_SHORTCUT)
        a["model.21.conv"] = x21 = self._conv("model.21.conv", x20, 2)
        x23 = self._c3("model.23", torch.cat([x21, x10], 1), NECK_SHORTCUT)

        self.detect_inputs = (x17, x20, x23)
        outs = []
        for l, (f, stride) in enumerate(zip(self.detect_inputs, STRIDES)):
            d = DETECT
            b = self._conv(f"{d}.cv2.{l}.1.conv", self._conv(f"{d}.cv2.{l}.0.conv", f))
            c = self._conv(f"{d}.cv3.{l}.1.conv", self._conv(f"{d}.cv3.{l}.0.conv", f))
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
