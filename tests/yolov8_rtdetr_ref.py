"""CPU restatement of YOLOv8-RTDETR (ultralytics cfg/models/v8/yolov8-rtdetr.yaml, geo-trax's train.sh `-rt`) for the tests of
that graph: the YOLOv8 backbone + neck of oracle/yolov8_ref.py (YoloV8Ref._conv / _c2f / _sppf, wired as model.0-21) feeding
oracle/rtdetr_ref.py's RTDETRDecoder (RtDetrRef._decoder) on (model.15, model.18, model.21). It stands in for RtDetrRef:
forward(x) returns [B, nq, 4 + nc], and stretch / postprocess / detect of oracle/rtdetr_ref.py work on it unchanged.

PARITY UNPINNED: restated from memory of the public yaml, not checked against an ultralytics install (none is reachable):
  - model.0-21 exactly as yolov8.yaml: 10 Upsample, 11 Concat(-1, 6), 12 C2f; 13 Upsample, 14 Concat(-1, 4), 15 C2f;
    16 Conv(3, 2), 17 Concat(-1, 12), 18 C2f; 19 Conv(3, 2), 20 Concat(-1, 9), 21 C2f. No shortcut in the neck's C2f blocks.
    A wrong Concat order would not fit the weight shapes at the n and s scales (the same argument as tests/yolov8p2_ref.py).
  - model.22 = RTDETRDecoder(nc) on [15, 18, 21] with its defaults (hd 256, 300 queries, 8 heads, 4 points, 6 layers,
    d_ffn 1024); input_proj.l = Conv2d(ch_l, hd, 1, bias=False) + BatchNorm2d, folded by weights.load_weights.
  - the predictor is RTDETRPredictor, as for rtdetr-l: LetterBox(scale_fill=True) and the same postprocess. Unpinned beyond
    the name test the reference applies (`'rtdetr' in yaml_file`, geotrax/extract.py:222-225).
The decoder's arithmetic is RtDetrRef's (see its header for what is unpinned there); the trunk's is YoloV8Ref's at fp32."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from oracle.rtdetr_ref import RtDetrRef
from oracle.yolov8_ref import YoloV8Ref

DEC = "model.22"


class YoloV8RtDetrRef(RtDetrRef):
    def __init__(self, tensors: dict[str, np.ndarray]):
        # RtDetrRef reads its decoder at model.28 (rtdetr-l): hand it the model.22 decoder under that prefix
        moved = {("model.28." + k[len(DEC) + 1:] if k.startswith(DEC + ".") else k): v for k, v in tensors.items()}
        super().__init__(moved)
        trunk = YoloV8Ref.__new__(YoloV8Ref)          # its building blocks only (no Detect: nc is not read)
        trunk.t, trunk.half, trunk.nc, trunk.acts = self.t, False, self.nc, {}
        self.trunk = trunk

    @torch.no_grad()
    def forward(self, x: torch.Tensor) -> torch.Tensor:
        tr = self.trunk
        a = tr.acts = {}
        a["model.0.conv"] = x0 = tr._conv("model.0.conv", x, 2)
        a["model.1.conv"] = x1 = tr._conv("model.1.conv", x0, 2)
        x2 = tr._c2f("model.2", x1, True)
        a["model.3.conv"] = x3 = tr._conv("model.3.conv", x2, 2)
        x4 = tr._c2f("model.4", x3, True)
        a["model.5.conv"] = x5 = tr._conv("model.5.conv", x4, 2)
        x6 = tr._c2f("model.6", x5, True)
        a["model.7.conv"] = x7 = tr._conv("model.7.conv", x6, 2)
        x8 = tr._c2f("model.8", x7, True)
        x9 = tr._sppf("model.9", x8)
        up = lambda t: F.interpolate(t, scale_factor=2, mode="nearest")
        x12 = tr._c2f("model.12", torch.cat([up(x9), x6], 1), False)
        x15 = tr._c2f("model.15", torch.cat([up(x12), x4], 1), False)
        a["model.16.conv"] = x16 = tr._conv("model.16.conv", x15, 2)
        x18 = tr._c2f("model.18", torch.cat([x16, x12], 1), False)
        a["model.19.conv"] = x19 = tr._conv("model.19.conv", x18, 2)
        x21 = tr._c2f("model.21", torch.cat([x19, x9], 1), False)
        self.acts = {}
        out = self._decoder((x15, x18, x21))
        # the decoder's activations under the hybrid's own names (model.22.*), next to the trunk's
        dec = {(DEC + k[len("model.28"):] if k.startswith("model.28") else k): v for k, v in self.acts.items()}
        self.acts = {**a, **dec}
        return out
