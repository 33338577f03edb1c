"""CPU restatement of the YOLOv10 detect model (ultralytics cfg/models/v10/yolov10{n,s}.yaml) for the tests of the YOLOv10 graph.

PARITY UNPINNED, like every file in oracle/ and tests/yolo11_ref.py: ultralytics is not installed where this was written, so nothing
here was run against the real package. It restates the public source from memory; the tensor names and shapes
(geotrax_amd.weights.yolov10_layer_specs) pin the widths and the Concat orders of the n / s scales. What they do not pin is listed
under "Doubt" below.

It subclasses tests/yolo11_ref.py's Yolo11Ref and reuses its arithmetic (_conv, _conv_res, _c2f, _sppf, _attention, _q); SCDown, PSA,
CIB, RepVGGDW and the two-stage postprocess are written out here. Every method follows the dtype of its input, so a float64 run is
`ref.t = {k: v.double() ...}; ref.forward(x.double())`. Wiring:
  0 Conv(64,3,2)  1 Conv(128,3,2)  2 C2f(128, shortcut)  3 Conv(256,3,2)  4 C2f(256, shortcut)  5 SCDown(512,3,2)  6 C2f(512, shortcut)
  7 SCDown(1024,3,2)  8 C2f(1024, shortcut) [n] / C2fCIB(1024, shortcut, lk) [s]  9 SPPF(1024, 5)  10 PSA(1024)
  11 Upsample  12 Concat(-1, 6)  13 C2f(512)  14 Upsample  15 Concat(-1, 4)  16 C2f(256)
  17 Conv(256,3,2)  18 Concat(-1, 13)  19 C2f(512)  20 SCDown(512,3,2)  21 Concat(-1, 10)  22 C2fCIB(1024, shortcut, lk)
  23 v10Detect(16, 19, 22)
  - SCDown: cv2(cv1(x)); cv1 = 1x1 Conv + SiLU, cv2 = depthwise 3x3 stride 2 WITHOUT activation.
  - PSA: a, b = split(cv1(x)); b = b + attn(b); b = b + ffn.1(ffn.0(b)); cv2(cat(a, b)). C2PSA's block with its tensors directly
    under the layer (attn.qkv / attn.proj / attn.pe / ffn.0 / ffn.1).
  - CIB(c, c, shortcut, e = 1.0, lk): dw3x3 + SiLU, 1x1 c -> 2c + SiLU, dw3x3 + SiLU on 2c (lk: RepVGGDW = SiLU(dw7x7(x) + dw3x3(x)),
    both without activation; fused: one dw7x7 + bias, then SiLU), 1x1 2c -> c + SiLU, dw3x3 + SiLU; x + that when shortcut.
    C2fCIB = C2f whose m.{k} are CIBs on the hidden width. Which blocks are C2fCIB and which CIBs are large-kernel is read off the
    tensors (m.0.cv1.0.conv present; a [c, 1, 7, 7] weight at m.k.cv1.2.conv).
  - v10Detect: cv2 / cv3 are YOLO11's Detect layers; one2one_cv2 / one2one_cv3 are copies with weights of their own. Inference
    (postprocess below): one-to-one scores and boxes; the MAX_DET = 300 anchors with the largest row maximum, then the 300 largest
    of their 300 x nc scores; the predictor gates score > conf, keeps `classes`, cuts to max_det and scales to the frame. No NMS.
Doubt:
  - whether the predictor overwrites the head's 300 (Detect.max_det) with `ultralytics.max_det` before the two-stage cut. Taken as
    not: MAX_DET here, V10_MAX_DET in geotrax_amd.weights, kV10Keep in csrc/det_kernels.hpp.
  - the order of `classes` and the max_det cut in the predictor's end-to-end branch (the filter first here, as the issue that asked
    for this family states it; they differ only when max_det < 300 and `classes` drops rows).
  - torch.topk's order among equal scores. The library's rule is the lower flat index (anchor * nc + class) first; the tests use
    weights without ties at the cut and assert that first.
  - the neck's C2f blocks take shortcut = False (yolov8.yaml's neck), model.22's C2fCIB shortcut = True (the yaml's [1024, True, True]).
The fp16 emulation rounds where the HIP path stores a map: every conv output, the attention output, the depthwise outputs."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from yolo11_ref import STRIDES, Yolo11Ref

MAX_DET = 300


class Yolov10Ref(Yolo11Ref):
    def __init__(self, tensors, emulate_half: bool = False):
        self.t = {k: torch.from_numpy(np.asarray(v, dtype=np.float32)) for k, v in tensors.items()}
        self.half = emulate_half
        self.nc = int(self.t["model.23.one2one_cv3.0.2.weight"].shape[0])
        self.acts: dict[str, torch.Tensor] = {}

    def double(self) -> "Yolov10Ref":
        self.t = {k: v.double() for k, v in self.t.items()}
        return self

    def _dw(self, name: str, x: torch.Tensor, act: bool, stride: int = 1, res: torch.Tensor | None = None) -> torch.Tensor:
        """depthwise k x k (k off the weight), pad k / 2; the residual joins after the activation, before the one rounding of the stored map"""
        w = self._q(self.t[name + ".weight"])
        y = F.conv2d(x, w, self.t.get(name + ".bias"), stride=stride, padding=w.shape[-1] // 2, groups=x.shape[1])
        if act:
            y = F.silu(y)
        if res is not None:
            y = y + res
        self.acts[name] = y = self._q(y)
        return y

    def _scdown(self, pfx: str, x: torch.Tensor) -> torch.Tensor:
        self.acts[pfx] = y = self._dw(pfx + ".cv2.conv", self._conv(pfx + ".cv1.conv", x), act=False, stride=2)
        return y

    def _psa(self, pfx: str, x: torch.Tensor) -> torch.Tensor:
        a, b = self._conv(pfx + ".cv1.conv", x).chunk(2, 1)
        b = self._q(b + self._attention(pfx + ".attn", b))
        b = self._q(b + self._conv(pfx + ".ffn.1.conv", self._conv(pfx + ".ffn.0.conv", b), act=False, quant_out=False))
        self.acts[pfx] = out = self._conv(pfx + ".cv2.conv", torch.cat([a, b], 1))
        return out

    def _cib(self, m: str, x: torch.Tensor, shortcut: bool) -> torch.Tensor:
        y = self._dw(m + ".cv1.0.conv", x, True)
        y = self._conv(m + ".cv1.1.conv", y)
        y = self._dw(m + ".cv1.2.conv", y, True)              # 3x3, or the fused RepVGGDW's 7x7
        y = self._conv(m + ".cv1.3.conv", y)
        return self._dw(m + ".cv1.4.conv", y, True, res=x if shortcut else None)

    def _block(self, pfx: str, x: torch.Tensor, shortcut: bool) -> torch.Tensor:
        if f"{pfx}.m.0.cv1.0.conv.weight" not in self.t:
            return self._c2f(pfx, x, shortcut)
        y = list(self._conv(pfx + ".cv1.conv", x).chunk(2, 1))
        k = 0
        while f"{pfx}.m.{k}.cv1.0.conv.weight" in self.t:
            y.append(self._cib(f"{pfx}.m.{k}", y[-1], shortcut))
            k += 1
        self.acts[pfx] = out = self._conv(pfx + ".cv2.conv", torch.cat(y, 1))
        return out

    def _head(self, box_br: str, cls_br: str) -> torch.Tensor:
        outs, a, d = [], self.acts, "model.23"
        for l, (f, stride) in enumerate(zip(self.detect_inputs, STRIDES)):
            b = self._conv(f"{d}.{box_br}.{l}.1.conv", self._conv(f"{d}.{box_br}.{l}.0.conv", f))
            c = self._conv(f"{d}.{cls_br}.{l}.0.1.conv", self._dwconv(f"{d}.{cls_br}.{l}.0.0.conv", f, True))
            c = self._conv(f"{d}.{cls_br}.{l}.1.1.conv", self._dwconv(f"{d}.{cls_br}.{l}.1.0.conv", c, True))
            a[f"{d}.{box_br}.feat{l}"] = torch.cat([b, c], 1)
            box = F.conv2d(b, self.t[f"{d}.{box_br}.{l}.2.weight"], self.t[f"{d}.{box_br}.{l}.2.bias"])
            cls = F.conv2d(c, self.t[f"{d}.{cls_br}.{l}.2.weight"], self.t[f"{d}.{cls_br}.{l}.2.bias"])
            B, _, H, W = box.shape
            p = box.view(B, 4, 16, H * W).softmax(2)
            dist = (p * torch.arange(16, dtype=box.dtype).view(1, 1, 16, 1)).sum(2)
            ys, xs = torch.meshgrid(torch.arange(H, dtype=box.dtype) + 0.5, torch.arange(W, dtype=box.dtype) + 0.5, indexing="ij")
            anc = torch.stack([xs.reshape(-1), ys.reshape(-1)], 0)[None]
            x1y1, x2y2 = anc - dist[:, :2], anc + dist[:, 2:]
            xywh = torch.cat([(x1y1 + x2y2) / 2, x2y2 - x1y1], 1) * stride
            outs.append(torch.cat([xywh, cls.view(B, self.nc, H * W).sigmoid()], 1))
        return torch.cat(outs, 2).transpose(1, 2).contiguous()

    @torch.no_grad()
    def forward(self, x: torch.Tensor, one2one: bool = True) -> torch.Tensor:
        """[B, A, 4 + nc]: xywh in network pixels + class scores of the one-to-one head (or of cv2 / cv3: `end2end: false`)"""
        a = self.acts
        x = self._q(x)
        a["model.0.conv"] = x0 = self._conv("model.0.conv", x, 2)
        a["model.1.conv"] = x1 = self._conv("model.1.conv", x0, 2)
        x2 = self._block("model.2", x1, True)
        a["model.3.conv"] = x3 = self._conv("model.3.conv", x2, 2)
        x4 = self._block("model.4", x3, True)
        x5 = self._scdown("model.5", x4)
        x6 = self._block("model.6", x5, True)
        x7 = self._scdown("model.7", x6)
        x8 = self._block("model.8", x7, True)
        x9 = self._sppf("model.9", x8)
        x10 = self._psa("model.10", x9)
        up = lambda t: F.interpolate(t, scale_factor=2, mode="nearest")
        x13 = self._block("model.13", torch.cat([up(x10), x6], 1), False)
        x16 = self._block("model.16", torch.cat([up(x13), x4], 1), False)
        a["model.17.conv"] = x17 = self._conv("model.17.conv", x16, 2)
        x19 = self._block("model.19", torch.cat([x17, x13], 1), False)
        x20 = self._scdown("model.20", x19)
        x22 = self._block("model.22", torch.cat([x20, x10], 1), True)
        self.detect_inputs = (x16, x19, x22)
        out = self._head("one2one_cv2", "one2one_cv3") if one2one else self._head("cv2", "cv3")
        for l in range(3):                                    # the library names the head that ran "model.23.feat<l>"
            a[f"model.23.feat{l}"] = a[f"model.23.{'one2one_cv2' if one2one else 'cv2'}.feat{l}"]
        return out


def repvggdw(x: torch.Tensor, w7: torch.Tensor, b7: torch.Tensor, w3: torch.Tensor, b3: torch.Tensor) -> torch.Tensor:
    """RepVGGDW.forward before fusing: SiLU(conv(x) + conv1(x)), conv = depthwise 7x7 pad 3, conv1 = depthwise 3x3 pad 1 (BN folded in)"""
    c = x.shape[1]
    return F.silu(F.conv2d(x, w7, b7, padding=3, groups=c) + F.conv2d(x, w3, b3, padding=1, groups=c))


def two_stage_topk(scores: np.ndarray, k: int = MAX_DET) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """v10Detect.postprocess's cut on [A, nc] scores: the k anchors with the largest row maximum, then the k largest of their k x nc
    scores -> (anchor, class, score) in descending score order. Stable sorts: among equals the lower index first."""
    A, nc = scores.shape
    k1 = min(k, A)
    rows = np.argsort(-scores.max(1), kind="stable")[:k1]
    flat = scores[rows].reshape(-1)
    idx = np.argsort(-flat, kind="stable")[:min(k, flat.size)]
    return rows[idx // nc], idx % nc, flat[idx]


def global_topk(scores: np.ndarray, k: int = MAX_DET) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The k largest of all A x nc scores, the lower flat index (anchor * nc + class) first among equals"""
    nc = scores.shape[1]
    flat = scores.reshape(-1)
    idx = np.argsort(-flat, kind="stable")[:min(k, flat.size)]
    return idx // nc, idx % nc, flat[idx]


def postprocess(pred: np.ndarray, conf: float, classes=None, max_det: int = 300, return_idx: bool = False):
    """pred [A, 4 + nc] (xywh + one-to-one scores) of one image -> [n, 6] xyxy, conf, cls in network pixels, descending score: the
    head's two-stage cut to MAX_DET rows, then the predictor's score > conf, `classes`, max_det. return_idx: also the anchors."""
    pred = pred.astype(np.float32)
    anchor, cls, score = two_stage_topk(pred[:, 4:])
    xy, wh = pred[anchor, :2], pred[anchor, 2:4] / np.float32(2)
    rows = np.concatenate([xy - wh, xy + wh, score[:, None], cls[:, None].astype(np.float32)], 1)
    keep = score > np.float32(conf)
    if classes is not None:
        keep &= np.isin(cls, np.asarray(classes))
    rows, anchor = rows[keep][:max_det], anchor[keep][:max_det]
    return (rows, anchor) if return_idx else rows


def detect(model: Yolov10Ref, frame_bgr: np.ndarray, imgsz: int, rect: bool, conf: float, classes=None, max_det: int = 300):
    """Whole end-to-end chain on one frame -> (xyxy [n, 4] frame pixels, conf [n], cls [n])"""
    from oracle.yolov8_ref import letterbox, scale_boxes

    x, g = letterbox(frame_bgr, imgsz, rect, half=model.half)
    det = postprocess(model.forward(x)[0].numpy(), conf, classes, max_det)
    return scale_boxes(det[:, :4], (g["net_h"], g["net_w"]), frame_bgr.shape[:2]), det[:, 4], det[:, 5].astype(np.int32)
