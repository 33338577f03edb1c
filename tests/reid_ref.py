"""CPU restatement of ultralytics' separate ReID network (trackers/bot_sort.py ``ReID``) for the tests of geotrax_amd.reid.

Pinned: the resample is PIL's own (``PIL.Image.resize(..., BILINEAR)``, what torchvision's Resize does on a PIL image inside
classify_transforms), so the GPU crops are held to PIL's bytes. Restated from memory of the pinned upstream (>= 8.4.80):
  - the box chain: Boxes.xywh in float32; BOTSORT.init_track concatenates the boxes with np.arange (float64 from there);
    ReID.__call__ converts xywh2xyxy; save_one_box(gain=1.02, pad=10, square=False) converts back, scales wh, .long() truncates
    toward zero, clip_boxes clips to the frame;
  - the channel order: save_one_box(BGR=False) reverses the crop's channels and ClassificationPredictor.preprocess applies
    cv2.cvtColor(BGR2RGB) before PIL, so the network sees the frame's B, G, R as channels 0, 1, 2;
  - Resize(S): short side S, long side int(S * long / short); CenterCrop(S): int(round((size - S) / 2.0)); ToTensor: u8 / 255;
    Normalize(0, 1) changes nothing;
  - the embedding: model(embed=[len(model) - 2]) = adaptive_avg_pool2d of model.8's output (yolov8-cls: model.9 is Classify).
The backbone forward is plain F.conv2d + SiLU + C2f in fp32 (the arithmetic of oracle/yolov8_ref.py's _conv / _c2f, which cannot
be constructed on a file without a Detect head)."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

GAIN, PAD = 1.02, 10


def crop_box(xyxy, h: int, w: int) -> np.ndarray:
    """[n, 4] float32 detector boxes -> [n, 4] int64 save_one_box crops (x1, y1, x2, y2), clipped to the h x w frame."""
    b = np.asarray(xyxy, np.float32).reshape(-1, 4)
    xywh = np.stack([(b[:, 0] + b[:, 2]) / np.float32(2), (b[:, 1] + b[:, 3]) / np.float32(2), b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]], 1)
    d = np.concatenate([xywh, np.arange(len(b)).reshape(-1, 1)], axis=-1)[:, :4]        # float64, as BOTSORT.init_track leaves it
    assert d.dtype == np.float64
    x1, x2 = d[:, 0] - d[:, 2] / 2, d[:, 0] + d[:, 2] / 2                                # ReID.__call__: xywh2xyxy
    y1, y2 = d[:, 1] - d[:, 3] / 2, d[:, 1] + d[:, 3] / 2
    cx, cy, bw, bh = (x1 + x2) / 2, (y1 + y2) / 2, x2 - x1, y2 - y1                      # save_one_box: xyxy2xywh
    bw, bh = bw * GAIN + PAD, bh * GAIN + PAD
    q = torch.from_numpy(np.stack([cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2], 1)).long().numpy()   # .long(): toward zero
    q[:, [0, 2]] = q[:, [0, 2]].clip(0, w)
    q[:, [1, 3]] = q[:, [1, 3]].clip(0, h)
    return q


def resized_size(cw: int, ch: int, S: int) -> tuple[int, int]:
    """torchvision Resize(S) of a cw x ch image: (width, height)."""
    if cw <= ch:
        return S, int(S * ch / cw)
    return int(S * cw / ch), S


def center_offset(size: int, S: int) -> int:
    return int(round((size - S) / 2.0))


def crop_image(frame: np.ndarray, box, S: int = 224) -> np.ndarray:
    """The u8 network input [S, S, 3] (channels = the frame's B, G, R) of one crop box."""
    import pytest

    Image = pytest.importorskip("PIL.Image")
    x1, y1, x2, y2 = (int(v) for v in box)
    crop = np.ascontiguousarray(frame[y1:y2, x1:x2])            # BGR bytes: reversed twice on the way to PIL
    rw, rh = resized_size(crop.shape[1], crop.shape[0], S)
    im = Image.fromarray(crop)
    if (rw, rh) != (crop.shape[1], crop.shape[0]):
        im = im.resize((rw, rh), Image.BILINEAR)
    a = np.asarray(im)
    t, l = center_offset(rh, S), center_offset(rw, S)
    return np.ascontiguousarray(a[t:t + S, l:l + S])


class ClsBackboneRef:
    def __init__(self, tensors: dict[str, np.ndarray]):
        self.t = {k: torch.from_numpy(np.asarray(v, np.float32)) for k, v in tensors.items()}
        self.acts: dict[str, torch.Tensor] = {}

    def _conv(self, name, x, stride=1, res=None):
        w = self.t[name + ".weight"]
        y = F.silu(F.conv2d(x, w, self.t.get(name + ".bias"), stride=stride, padding=w.shape[-1] // 2))
        if res is not None:
            y = y + res
        self.acts[name] = y
        return y

    def _c2f(self, pfx, x):
        y = list(self._conv(pfx + ".cv1.conv", x).chunk(2, 1))
        k = 0
        while f"{pfx}.m.{k}.cv1.conv.weight" in self.t:
            inp = y[-1]
            y.append(self._conv(f"{pfx}.m.{k}.cv2.conv", self._conv(f"{pfx}.m.{k}.cv1.conv", inp), res=inp))
            k += 1
        out = self._conv(pfx + ".cv2.conv", torch.cat(y, 1))
        self.acts[pfx] = out
        return out

    @torch.no_grad()
    def forward(self, crops_u8: np.ndarray) -> np.ndarray:
        """crops [n, S, S, 3] u8 -> embeddings [n, dim] float32."""
        x = torch.from_numpy(np.ascontiguousarray(crops_u8)).permute(0, 3, 1, 2).float() / 255.0
        x = self._conv("model.0.conv", x, 2)
        x = self._conv("model.1.conv", x, 2)
        x = self._c2f("model.2", x)
        x = self._conv("model.3.conv", x, 2)
        x = self._c2f("model.4", x)
        x = self._conv("model.5.conv", x, 2)
        x = self._c2f("model.6", x)
        x = self._conv("model.7.conv", x, 2)
        x = self._c2f("model.8", x)
        return F.adaptive_avg_pool2d(x, (1, 1)).flatten(1).numpy()


def embed(tensors, frame: np.ndarray, xyxy, S: int = 224):
    """(crops [n, S, S, 3] u8, embeddings [n, dim], the backbone) of one frame's boxes."""
    boxes = crop_box(xyxy, frame.shape[0], frame.shape[1])
    crops = np.stack([crop_image(frame, b, S) for b in boxes]) if len(boxes) else np.zeros((0, S, S, 3), np.uint8)
    ref = ClsBackboneRef(tensors)
    return crops, ref.forward(crops), ref
