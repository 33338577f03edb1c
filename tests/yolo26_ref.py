"""CPU restatement of the YOLO26 detect model (ultralytics cfg/models/26/yolo26.yaml) for the tests of the YOLO26 graph.

PARITY UNPINNED, like every file in oracle/, tests/yolo11_ref.py and tests/yolov10_ref.py: ultralytics is not installed where this
was written and nobody could fetch it, so nothing here was run against the real package. It restates the public source from memory;
the tensor names and shapes (geotrax_amd.weights.yolo26_layer_specs) pin the widths and the Concat orders. What they do not pin is
listed under "Doubt" below.

It subclasses tests/yolo11_ref.py's Yolo11Ref and reuses its arithmetic (_conv, _conv_res, _c3k2, _c3k, _bottleneck, _attention,
_c2psa, _dwconv, _q) and tests/yolov10_ref.py's two-stage postprocess; the SPPF with a residual, the C3k2 with attention and the
Detect with reg_max = 1 are written out here. Every method follows the dtype of its input, so a float64 run is
`Yolo26Ref(t).double().forward(x.double())`. `end2end: True`, `reg_max: 1`; the scales use yolo11.yaml's depth / width / max-channel
table. Wiring:
  0 Conv(64,3,2)  1 Conv(128,3,2)  2 C3k2(256, e=0.25)  3 Conv(256,3,2)  4 C3k2(512, e=0.25)  5 Conv(512,3,2)  6 C3k2(512, c3k)
  7 Conv(1024,3,2)  8 C3k2(1024, c3k)  9 SPPF(1024, 5, n=3, shortcut)  10 C2PSA(1024)
  11 Upsample  12 Concat(-1, 6)  13 C3k2(512)  14 Upsample  15 Concat(-1, 4)  16 C3k2(256)
  17 Conv(256,3,2)  18 Concat(-1, 13)  19 C3k2(512)  20 Conv(512,3,2)  21 Concat(-1, 10)  22 C3k2(1024, c3k, e=0.5, attn)
  23 Detect(16, 19, 22), reg_max = 1, end2end
  - SPPF(shortcut): cv1 is a 1x1 Conv WITHOUT activation; three cascaded 5x5 max-pools; cv2 = 1x1 Conv + SiLU on the 4-way concat;
    the output is cv2(...) + x.
  - C3k2 with attn: every m.{k} is Sequential(Bottleneck(c, c, shortcut, 3x3 / 3x3, e = 0.5), PSABlock(c, attn_ratio 0.5,
    heads = c / 64)) -- m.{k}.0.cv1 / cv2, then C2PSA's block on m.{k}.1.attn.{qkv, proj, pe} / ffn.{0, 1} with its two residuals.
    Whether the other C3k2 blocks hold Bottlenecks or C3k blocks is read off the tensors (m.{k}.cv3 present), as in Yolo11Ref.
  - Detect: cv2[l] = Conv3x3, Conv3x3, Conv2d 1x1 to FOUR channels; cv3[l] = yolo11.yaml's depthwise pairs, Conv2d 1x1 to nc;
    one2one_cv2 / one2one_cv3 are copies with weights of their own. The DFL is the identity: the four outputs are l, t, r, b in
    strides, signed, unclamped; anchors at cell centres; xyxy = (ax - l, ay - t, ax + r, ay + b) * stride. Inference runs the
    one-to-one branches, sigmoid, and v10Detect's two-stage cut (tests/yolov10_ref.py: postprocess). A fused export may have dropped
    cv2 / cv3.
Doubt (each a constant here and one in the library):
  - the neck's C3k2 shortcut flag (13 / 16 / 19): yolo11_ref.NECK_SHORTCUT, csrc/yolo_tables.hpp kNeckShortcut -- off, as for YOLO11.
  - model.22's Bottleneck shortcut: ATTN_BLOCK_SHORTCUT here, kAttnBlockShortcut there -- taken as on.
  - whether SPPF's residual follows cv2's activation: SPPF_RESIDUAL_AFTER_ACT here, kSppfResidualAfterAct there -- taken as so.
  - the predictor's max_det against the head's 300 rows: yolov10_ref.MAX_DET, weights.V10_MAX_DET, kV10Keep -- the head's 300 first.
  - Detect's box-branch width, max(16, ch[0] // 4, BOX_FLOOR): weights.YOLO26_BOX_FLOOR = 64 as for every other family here; with
    reg_max = 1 the package's third term may be 4, which would give 16 / 32 channels at scales n / s (such a file is refused by shape).
The fp16 emulation rounds where the HIP path stores a map: every conv output, the attention output, the depthwise outputs."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from yolo11_ref import NECK_SHORTCUT, STRIDES, Yolo11Ref
from yolov10_ref import MAX_DET, global_topk, postprocess, two_stage_topk  # noqa: F401  (the tail is YOLOv10's)

ATTN_BLOCK_SHORTCUT = True
SPPF_RESIDUAL_AFTER_ACT = True


def decode_ltrb(dist: torch.Tensor, h: int, w: int, stride: float) -> torch.Tensor:
    """dist [B, 4, h * w] (l, t, r, b in strides) -> xyxy [B, 4, h * w] in network pixels, anchors at cell centres"""
    ys, xs = torch.meshgrid(torch.arange(h, dtype=dist.dtype) + 0.5, torch.arange(w, dtype=dist.dtype) + 0.5, indexing="ij")
    anc = torch.stack([xs.reshape(-1), ys.reshape(-1)], 0)[None]
    return torch.cat([anc - dist[:, :2], anc + dist[:, 2:]], 1) * stride


class Yolo26Ref(Yolo11Ref):
    def __init__(self, tensors, emulate_half: bool = False):
        self.t = {k: torch.from_numpy(np.asarray(v, dtype=np.float32)) for k, v in tensors.items()}
        self.half = emulate_half
        self.nc = int(self.t["model.23.one2one_cv3.0.2.weight"].shape[0])
        self.acts: dict[str, torch.Tensor] = {}

    def double(self) -> "Yolo26Ref":
        self.t = {k: v.double() for k, v in self.t.items()}
        return self

    def _sppf_res(self, pfx: str, x: torch.Tensor) -> torch.Tensor:
        y = [self._conv(pfx + ".cv1.conv", x, act=False)]
        self.acts[pfx + ".cv1.conv"] = y[0]
        for _ in range(3):
            y.append(F.max_pool2d(y[-1], 5, 1, 2))
        self.acts[pfx + ".pools"] = torch.cat(y, 1)
        assert SPPF_RESIDUAL_AFTER_ACT
        self.acts[pfx] = out = self._q(self._conv(pfx + ".cv2.conv", torch.cat(y, 1), quant_out=False) + x)
        return out

    def _psablock(self, m: str, b: torch.Tensor) -> torch.Tensor:
        b = self._q(b + self._attention(m + ".attn", b))
        return self._q(b + self._conv(m + ".ffn.1.conv", self._conv(m + ".ffn.0.conv", b), act=False, quant_out=False))

    def _c3k2_attn(self, pfx: str, x: torch.Tensor, shortcut: bool) -> torch.Tensor:
        y = list(self._conv(pfx + ".cv1.conv", x).chunk(2, 1))
        k = 0
        while f"{pfx}.m.{k}.0.cv1.conv.weight" in self.t:
            m = f"{pfx}.m.{k}"
            self.acts[m + ".0.cv2.conv"] = b = self._bottleneck(m + ".0", y[-1], shortcut)      # the library's names for the two maps
            self.acts[m + ".1.ffn.1.conv"] = b = self._psablock(m + ".1", b)
            y.append(b)
            k += 1
        assert k > 0, f"{pfx}: no Sequential(Bottleneck, PSABlock)"
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
            B, four, H, W = box.shape
            assert four == 4, "reg_max = 1"
            xyxy = decode_ltrb(box.view(B, 4, H * W), H, W, stride)
            xywh = torch.cat([(xyxy[:, :2] + xyxy[:, 2:]) / 2, xyxy[:, 2:] - xyxy[:, :2]], 1)
            outs.append(torch.cat([xywh, cls.view(B, self.nc, H * W).sigmoid()], 1))
        return torch.cat(outs, 2).transpose(1, 2).contiguous()

    @torch.no_grad()
    def forward(self, x: torch.Tensor, one2one: bool = True) -> torch.Tensor:
        """[B, A, 4 + nc]: xywh in network pixels + class scores of the one-to-one head (or of cv2 / cv3: `end2end: false`)"""
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
        x9 = self._sppf_res("model.9", x8)
        x10 = self._c2psa("model.10", x9)
        up = lambda t: F.interpolate(t, scale_factor=2, mode="nearest")
        x13 = self._c3k2("model.13", torch.cat([up(x10), x6], 1), NECK_SHORTCUT)
        x16 = self._c3k2("model.16", torch.cat([up(x13), x4], 1), NECK_SHORTCUT)
        a["model.17.conv"] = x17 = self._conv("model.17.conv", x16, 2)
        x19 = self._c3k2("model.19", torch.cat([x17, x13], 1), NECK_SHORTCUT)
        a["model.20.conv"] = x20 = self._conv("model.20.conv", x19, 2)
        x22 = self._c3k2_attn("model.22", torch.cat([x20, x10], 1), ATTN_BLOCK_SHORTCUT)
        self.detect_inputs = (x16, x19, x22)
        out = self._head("one2one_cv2", "one2one_cv3") if one2one else self._head("cv2", "cv3")
        for l in range(3):                                    # the library names the head that ran "model.23.feat<l>"
            a[f"model.23.feat{l}"] = a[f"model.23.{'one2one_cv2' if one2one else 'cv2'}.feat{l}"]
        return out


def detect(model: Yolo26Ref, frame_bgr: np.ndarray, imgsz: int, rect: bool, conf: float, classes=None, max_det: int = 300):
    """Whole end-to-end chain on one frame -> (xyxy [n, 4] frame pixels, conf [n], cls [n])"""
    from oracle.yolov8_ref import letterbox, scale_boxes

    x, g = letterbox(frame_bgr, imgsz, rect, half=model.half)
    det = postprocess(model.forward(x)[0].numpy(), conf, classes, max_det)
    return scale_boxes(det[:, :4], (g["net_h"], g["net_w"]), frame_bgr.shape[:2]), det[:, 4], det[:, 5].astype(np.int32)
