"""CPU restatement of a YOLO11-cls checkpoint as ultralytics' separate ReID network runs it (trackers/bot_sort.py ``ReID``), for the
tests of the YOLO11-cls family of geotrax_amd.reid.

PARITY UNPINNED: ultralytics is not installed where this was written, so nothing here was run against the real package. The graph
(cfg/models/11/yolo11-cls.yaml) is restated from memory of the public source:
  0 Conv(64,3,2)  1 Conv(128,3,2)  2 C3k2(256, e=0.25)  3 Conv(256,3,2)  4 C3k2(512, e=0.25)  5 Conv(512,3,2)  6 C3k2(512, c3k)
  7 Conv(1024,3,2)  8 C3k2(1024, c3k)  9 C2PSA(1024)  10 Classify
i.e. rows 0-8 of yolo11.yaml, C2PSA directly behind them (no SPPF), scales as in yolo11.yaml. What holds it: the fused parameter
counts of geotrax_amd.weights.yolo11_cls_layer_specs at the yaml's default nc = 80 come out at the published 1.6 / 5.5 / 10.4 / 12.9 /
28.4 M of yolo11{n,s,m,l,x}-cls (tests/test_reid_yolo11.py), and C2PSA is held against plain torch written out longhand there.
``ReID`` embeds layer len(model) - 2 = model.9: the vector is adaptive_avg_pool2d of the C2PSA output (YOLOv8-cls: model.8).

Built from the blocks of tests/yolo11_ref.py (Yolo11Ref: _c3k2, _c2psa and the arithmetic of oracle/yolov8_ref.py under them) and
the crop / transform chain of tests/reid_ref.py (crop_box, crop_image: PIL's own resample)."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

import reid_ref
from yolo11_ref import Yolo11Ref


class Yolo11ClsRef(Yolo11Ref):
    def __init__(self, tensors, double: bool = False):
        dt = torch.float64 if double else torch.float32
        self.t = {k: torch.from_numpy(np.asarray(v, dtype=np.float32)).to(dt) for k, v in tensors.items() if k.startswith("model.")}
        self.dt = dt
        self.half = False
        self.acts: dict[str, torch.Tensor] = {}

    @torch.no_grad()
    def forward(self, crops_u8: np.ndarray) -> np.ndarray:
        """crops [n, S, S, 3] u8 -> embeddings [n, dim] (float32, or float64 for the double restatement)."""
        a = self.acts
        x = torch.from_numpy(np.ascontiguousarray(crops_u8)).permute(0, 3, 1, 2).float() / 255.0      # ToTensor: fp32 division
        x = x.to(self.dt)
        a["model.0.conv"] = x = self._conv("model.0.conv", x, 2)
        a["model.1.conv"] = x = self._conv("model.1.conv", x, 2)
        x = self._c3k2("model.2", x, True)
        a["model.3.conv"] = x = self._conv("model.3.conv", x, 2)
        x = self._c3k2("model.4", x, True)
        a["model.5.conv"] = x = self._conv("model.5.conv", x, 2)
        x = self._c3k2("model.6", x, True)
        a["model.7.conv"] = x = self._conv("model.7.conv", x, 2)
        x = self._c3k2("model.8", x, True)
        x = self._c2psa("model.9", x)
        return F.adaptive_avg_pool2d(x, (1, 1)).flatten(1).numpy()


def crops_of(frame: np.ndarray, xyxy, S: int) -> np.ndarray:
    boxes = reid_ref.crop_box(xyxy, frame.shape[0], frame.shape[1])
    return np.stack([reid_ref.crop_image(frame, b, S) for b in boxes]) if len(boxes) else np.zeros((0, S, S, 3), np.uint8)


def embed(tensors, frame: np.ndarray, xyxy, S: int = 224, double: bool = False):
    """(crops [n, S, S, 3] u8, embeddings [n, dim], the network) of one frame's boxes."""
    crops = crops_of(frame, xyxy, S)
    ref = Yolo11ClsRef(tensors, double)
    return crops, ref.forward(crops), ref


def attention_f64(qkv: np.ndarray, pe_w: np.ndarray, pe_b: np.ndarray, heads: int) -> np.ndarray:
    """ultralytics' Attention on maps, float64 numpy: qkv [n, h, w, heads * 128] with [q 32 | k 32 | v 64] per head, pe_w
    [heads * 64, 1, 3, 3], pe_b [heads * 64] -> softmax(q^T k * 32^-0.5) v + pe(v), [n, h, w, heads * 64]."""
    q = np.asarray(qkv, np.float64)
    n, h, w, _ = q.shape
    T, C = h * w, heads * 64
    t = q.reshape(n, T, heads, 128)
    qq, kk, vv = t[..., :32], t[..., 32:64], t[..., 64:]
    s = np.einsum("nqhd,nkhd->nhqk", qq, kk) * 32 ** -0.5
    s = s - s.max(-1, keepdims=True)
    p = np.exp(s)
    p /= p.sum(-1, keepdims=True)
    o = np.einsum("nhqk,nkhd->nqhd", p, vv).reshape(n, h, w, C)
    vmap = np.pad(vv.reshape(n, h, w, C), ((0, 0), (1, 1), (1, 1), (0, 0)))
    wt = np.asarray(pe_w, np.float64).reshape(C, 3, 3)
    pe = np.zeros((n, h, w, C)) + np.asarray(pe_b, np.float64)
    for ky in range(3):
        for kx in range(3):
            pe += vmap[:, ky:ky + h, kx:kx + w] * wt[:, ky, kx]
    return o + pe
