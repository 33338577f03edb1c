"""CPU restatement of the YOLOv8-P2 detect model (ultralytics cfg/models/v8/yolov8-p2.yaml) for the tests of the P2 graph.

It subclasses oracle/yolov8_ref.py's YoloV8Ref and reuses its arithmetic unchanged (_conv, _c2f, _sppf; letterbox, detect and
obj_feats_table work on it as they are): only the wiring differs. Restated from memory of the public yaml, not checked against
an ultralytics install:
  - backbone model.0-9 as yolov8.yaml; head: 10 Upsample, 11 Concat(-1, 6), 12 C2f(512); 13 Upsample, 14 Concat(-1, 4),
    15 C2f(256); 16 Upsample, 17 Concat(-1, 2), 18 C2f(128) (P2/4); 19 Conv(128, 3, 2), 20 Concat(-1, 15), 21 C2f(256);
    22 Conv(256, 3, 2), 23 Concat(-1, 12), 24 C2f(512); 25 Conv(512, 3, 2), 26 Concat(-1, 9), 27 C2f(1024);
    28 Detect on [18, 21, 24, 27]. Every Concat puts the tensor of the previous layer first. No shortcut in the head's C2f.
  - Detect's widths from its first input: c2 = max(16, ch[0] // 4, 64) (box branch), c3 = max(ch[0], min(nc, 100)) (class branch).
    The tests build their tensors from geotrax_amd.weights.yolov8_p2_layer_specs, so only the wiring here is checked against the
    library, not these widths.
  - anchors: level order P2, P3, P4, P5 (strides 4, 8, 16, 32), row-major within a level, centres at (x + 0.5, y + 0.5) * stride.
Doubt: none about the indices above that the tensor names do not also pin (a wrong Concat order would not match the weight shapes
for the n / s scales)."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from oracle.yolov8_ref import YoloV8Ref

STRIDES = (4.0, 8.0, 16.0, 32.0)


class YoloV8P2Ref(YoloV8Ref):
    def __init__(self, tensors, emulate_half: bool = False):   # the parent's, with nc read from Detect = model.28
        self.t = {k: torch.from_numpy(np.asarray(v, dtype=np.float32)) for k, v in tensors.items()}
        self.half = emulate_half
        self.nc = int(self.t["model.28.cv3.0.2.weight"].shape[0])
        self.acts: dict[str, torch.Tensor] = {}

    @torch.no_grad()
    def forward(self, x: torch.Tensor) -> torch.Tensor:
        a = self.acts
        x = self._q(x)
        a["model.0.conv"] = x0 = self._conv("model.0.conv", x, 2)
        a["model.1.conv"] = x1 = self._conv("model.1.conv", x0, 2)
        x2 = self._c2f("model.2", x1, True)
        a["model.3.conv"] = x3 = self._conv("model.3.conv", x2, 2)
        x4 = self._c2f("model.4", x3, True)
        a["model.5.conv"] = x5 = self._conv("model.5.conv", x4, 2)
        x6 = self._c2f("model.6", x5, True)
        a["model.7.conv"] = x7 = self._conv("model.7.conv", x6, 2)
        x8 = self._c2f("model.8", x7, True)
        x9 = self._sppf("model.9", x8)
        up = lambda t: F.interpolate(t, scale_factor=2, mode="nearest")
        x12 = self._c2f("model.12", torch.cat([up(x9), x6], 1), False)
        x15 = self._c2f("model.15", torch.cat([up(x12), x4], 1), False)
        x18 = self._c2f("model.18", torch.cat([up(x15), x2], 1), False)
        a["model.19.conv"] = x19 = self._conv("model.19.conv", x18, 2)
        x21 = self._c2f("model.21", torch.cat([x19, x15], 1), False)
        a["model.22.conv"] = x22 = self._conv("model.22.conv", x21, 2)
        x24 = self._c2f("model.24", torch.cat([x22, x12], 1), False)
        a["model.25.conv"] = x25 = self._conv("model.25.conv", x24, 2)
        x27 = self._c2f("model.27", torch.cat([x25, x9], 1), False)

        self.detect_inputs = (x18, x21, x24, x27)
        outs = []
        for l, (f, stride) in enumerate(zip(self.detect_inputs, STRIDES)):
            b = self._conv(f"model.28.cv2.{l}.1.conv", self._conv(f"model.28.cv2.{l}.0.conv", f))
            c = self._conv(f"model.28.cv3.{l}.1.conv", self._conv(f"model.28.cv3.{l}.0.conv", f))
            a[f"model.28.feat{l}"] = torch.cat([b, c], 1)
            box = F.conv2d(b, self.t[f"model.28.cv2.{l}.2.weight"], self.t[f"model.28.cv2.{l}.2.bias"])
            cls = F.conv2d(c, self.t[f"model.28.cv3.{l}.2.weight"], self.t[f"model.28.cv3.{l}.2.bias"])
            B, _, H, W = box.shape
            p = box.view(B, 4, 16, H * W).softmax(2)
            d = (p * torch.arange(16, dtype=torch.float32).view(1, 1, 16, 1)).sum(2)
            ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32) + 0.5,
                                    torch.arange(W, dtype=torch.float32) + 0.5, indexing="ij")
            anc = torch.stack([xs.reshape(-1), ys.reshape(-1)], 0)[None]
            x1y1, x2y2 = anc - d[:, :2], anc + d[:, 2:]
            xywh = torch.cat([(x1y1 + x2y2) / 2, x2y2 - x1y1], 1) * stride
            outs.append(torch.cat([xywh, cls.view(B, self.nc, H * W).sigmoid()], 1))
        return torch.cat(outs, 2).transpose(1, 2).contiguous()
