"""``ReIDEncoder``: the separate appearance network of ``with_reid: true, model: <cls checkpoint>`` over the C ABI (gtx_embedder_*).

Reference behaviour replaced (ultralytics >= 8.4.80, trackers/bot_sort.py ``ReID``, used by BoT-SORT, Deep OC-SORT and TrackTrack
when the tracker yaml names a model; geotrax/cfg/default.yaml:379, :421, :470)::

    feats = self.model.predictor([save_one_box(det, img, save=False) for det in xywh2xyxy(torch.from_numpy(dets[:, :4]))])

i.e. one crop per detection (gain 1.02, pad 10), ``classify_transforms(imgsz)`` (PIL bilinear to short side imgsz, center crop,
/255), the classification model's backbone and the global average pool of the layer in front of its Classify head. Two families are
implemented: YOLO11-cls (weights.is_yolo11_cls: the vector is the pool of model.9, the C2PSA output) and YOLOv8-cls
(weights.is_yolov8_cls: model.8). The network runs at fp32 grade whatever the detector's ``half`` says, as upstream's own predictor
does.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib
from ._lib import check, ptr


class ReIDEncoder:
    def __init__(self, tensors: dict[str, np.ndarray], ctx: _lib.Context | None = None, fp32_split: bool | None = None,
                 imgsz: int | None = None, max_crops: int = 300):
        """tensors: a fused YOLO11-cls or YOLOv8-cls checkpoint (weights.load_weights). fp32_split: split-f16x3 convolutions (default, the detector's
        GTX_FP32_SPLIT rule) or exact fp32. imgsz: the classifier's input size (default: the file's ``cls.meta``, else 224).
        max_crops: crops per backbone launch the buffers hold (more run in chunks)."""
        from .weights import cls_family, cls_imgsz

        self.family = cls_family(tensors)                     # raises for a classifier of another topology
        if self.family is None:
            raise NotImplementedError("ReID model: the tensors are not a YOLO11-cls or YOLOv8-cls checkpoint (only those families are implemented)")
        head = {"yolo11-cls": "model.10.", "yolov8-cls": "model.9."}[self.family]   # Classify: never loaded
        if fp32_split is None:
            from .detector import FP32_SPLIT_DEFAULT

            fp32_split = os.environ.get("GTX_FP32_SPLIT", "1" if FP32_SPLIT_DEFAULT else "0") == "1"
        self.fp32_split = bool(fp32_split)
        self.imgsz = int(imgsz or cls_imgsz(tensors))
        self.max_crops = int(max_crops)
        self.ctx = ctx or _lib.default_context()
        lib = self.ctx.lib
        h = C.c_void_p()
        check(lib.gtx_embedder_create(self.ctx.handle, self.imgsz, self.max_crops, int(self.fp32_split), C.byref(h)))
        self.handle = h
        for name, arr in tensors.items():
            if not name.startswith("model.") or name.startswith(head):
                continue
            a = np.ascontiguousarray(arr, dtype=np.float32)
            shape = (C.c_int64 * a.ndim)(*a.shape)
            check(lib.gtx_embedder_set_tensor(h, name.encode(), ptr(a), a.ndim, shape))
        check(lib.gtx_embedder_finalize(h))
        d = C.c_int()
        check(lib.gtx_embedder_dim(h, C.byref(d)))
        self.dim = int(d.value)
        self._frame_dptr, self._frame_bytes = 0, 0
        self._n_flight = None

    def close(self):
        if getattr(self, "handle", None):
            self.ctx.lib.gtx_embedder_destroy(self.handle)
            self.handle = None
        if getattr(self, "_frame_dptr", 0):
            self.ctx.dev_free(self._frame_dptr)
            self._frame_dptr = 0

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _boxes(xyxy) -> np.ndarray:
        return np.ascontiguousarray(np.asarray(xyxy, dtype=np.float32).reshape(-1, 4))

    def __call__(self, frame_bgr: np.ndarray, xyxy) -> np.ndarray:
        """One host BGR u8 frame [h, w, 3] and its boxes [n, 4] (frame pixels) -> vectors [n, dim] float32 (blocking)."""
        frame = np.ascontiguousarray(frame_bgr, dtype=np.uint8)
        boxes = self._boxes(xyxy)
        if len(boxes) == 0:
            return np.zeros((0, self.dim), np.float32)
        if self._frame_bytes < frame.nbytes:
            if self._frame_dptr:
                self.ctx.dev_free(self._frame_dptr)
            self._frame_dptr, self._frame_bytes = self.ctx.dev_alloc(frame.nbytes), frame.nbytes
        self.ctx.dev_upload(self._frame_dptr, frame)
        self.submit_dev(self._frame_dptr, frame.shape[0], frame.shape[1], [boxes])
        return self.collect()[0]

    def submit_dev(self, frames_dptr: int, h: int, w: int, boxes_per_frame: list) -> None:
        """Enqueues the crops of len(boxes_per_frame) device frames [h][w][3] u8 (back to back at frames_dptr) on the context's
        stream: the frames are read in that stream's order, before anything enqueued on it later."""
        boxes = [self._boxes(b) for b in boxes_per_frame]
        counts = np.ascontiguousarray([len(b) for b in boxes], dtype=np.int32)
        allb = np.ascontiguousarray(np.concatenate(boxes, 0) if len(boxes) else np.zeros((0, 4), np.float32))
        check(self.ctx.lib.gtx_embedder_submit_dev(self.handle, C.c_void_p(frames_dptr) if frames_dptr else None, len(boxes), h, w,
                                                   ptr(counts), ptr(allb)))
        self._n_flight = counts

    def collect(self) -> list[np.ndarray]:
        """Waits for the submitted pass; one [n_i, dim] float32 array per frame."""
        counts, self._n_flight = self._n_flight, None
        if counts is None:
            raise _lib.GtxError(-4, "collect without a submitted pass")
        out = np.zeros((max(int(counts.sum()), 1), self.dim), np.float32)
        n = C.c_int()
        check(self.ctx.lib.gtx_embedder_collect(self.handle, ptr(out), out.shape[0], C.byref(n)))
        return np.split(out[: n.value], np.cumsum(counts)[:-1])

    # ---- debug / parity
    def crop(self, i: int) -> np.ndarray:
        """The u8 network input of crop i of the last pass, [imgsz, imgsz, 3] in the network's channel order (the frame's BGR)."""
        out = np.zeros((self.imgsz, self.imgsz, 4), np.uint8)
        check(self.ctx.lib.gtx_embedder_crops(self.handle, i, ptr(out)))
        return out[..., :3]

    def layer_output(self, i: int, layer: str) -> np.ndarray:
        h, w, c = C.c_int(), C.c_int(), C.c_int()
        check(self.ctx.lib.gtx_embedder_layer_output(self.handle, i, layer.encode(), None, C.byref(h), C.byref(w), C.byref(c)))
        out = np.zeros((h.value, w.value, c.value), np.float32)
        check(self.ctx.lib.gtx_embedder_layer_output(self.handle, i, layer.encode(), ptr(out), None, None, None))
        return out

    def saturated(self, clear: bool = False) -> bool:
        f = C.c_int()
        check(self.ctx.lib.gtx_embedder_saturated(self.handle, int(clear), C.byref(f)))
        return bool(f.value)

    def fell_back(self) -> bool:
        f = C.c_int()
        check(self.ctx.lib.gtx_embedder_fell_back(self.handle, C.byref(f)))
        return bool(f.value)

    def profile(self, n: int, iters: int = 10) -> list[tuple[str, float, float]]:
        """(launch, mean ms, FLOPs) of every launch of a forward pass over the first n crops of the last pass."""
        cap = 256
        names = C.create_string_buffer(cap * 128)
        ms = np.zeros(cap, np.float32)
        fl = np.zeros(cap, np.float64)
        k = C.c_int()
        check(self.ctx.lib.gtx_embedder_profile(self.handle, n, iters, cap, names, ptr(ms), ptr(fl), C.byref(k)))
        raw = names.raw
        return [(raw[i * 128:(i + 1) * 128].split(b"\0", 1)[0].decode(), float(ms[i]), float(fl[i])) for i in range(min(k.value, cap))]


def crop_boxes(xyxy, frame_hw) -> np.ndarray:
    """save_one_box's clipped crops [n, 4] (x1, y1, x2, y2) as the library computes them (host only; gtx_reid_crop_boxes)."""
    b = ReIDEncoder._boxes(xyxy)
    out = np.zeros((len(b), 4), np.int32)
    check(_lib.load().gtx_reid_crop_boxes(ptr(b), len(b), int(frame_hw[0]), int(frame_hw[1]), ptr(out)))
    return out
