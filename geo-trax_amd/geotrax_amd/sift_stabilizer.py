"""stabilo's ``detector_name: sift | rsift`` stabilizer on the detector's gray image in HBM (gtx_sift_stab_*).

The surface the engine uses of :class:`geotrax_amd.stabilizer.Stabilizer` -- ``set_ref_gray_dev``, ``submit_gray_dev`` /
``collect``, ``stabilize_gray_dev``, the transform, the counters -- over the stream-ordered chain of csrc/sift_stab.cpp: the
reference frame's features are extracted once, a frame is one chain of launches on the object's stream with no host wait
before ``collect``, and the vehicle mask is applied (after the strongest ``max_features`` were chosen, as cv2's
``detectAndCompute(image, mask)`` does). ``Stabilizer`` itself keeps its blocking host-frame path for these detectors
(reference: stabilo.Stabilizer as driven by geotrax/extract.py:139,177-187; config keys geotrax/cfg/default.yaml:100-145).

Built for ``downsample_ratio`` 0.5 (the detector's half-resolution gray image), ``filter_type`` ratio, ``transformation_type``
projective, ``clahe`` off; anything else raises, and ``extract.pipelined()`` keeps such a run on the blocking loop.

Keywords that do not mean what they say: ``max_features`` below 4 is raised to 4 (a homography needs four pairs; the blocking
path does the same); ``ransac_method`` and ``ransac_confidence`` are accepted for the config block's sake and not used -- the
estimator is always the MSAC kernel with ``clamp(ransac_max_iter, 256, 16384)`` hypotheses and the host refit, as in
``Stabilizer``. The mask holds at most ``MAX_MASK_RECTS`` rectangles: boxes beyond that are left unmasked, with a warning.
"""
from __future__ import annotations

import ctypes as C
import logging

import numpy as np

from . import _lib, geometry
from ._lib import SiftStabConfig, check, ptr

logger = logging.getLogger(__name__)

MAX_MASK_RECTS = 1024          # kMaxMaskRects of csrc/sift.hip: what one frame's mask holds


def resident(stab_kw: dict | None) -> bool:
    """Whether this ``stabilo:`` block runs on SiftStabilizer (else: Stabilizer, whatever it makes of it)."""
    kw = stab_kw or {}
    return (str(kw.get("detector_name", "orb")) in ("sift", "rsift") and float(kw.get("downsample_ratio", 0.5)) == 0.5
            and str(kw.get("filter_type", "ratio")) == "ratio" and str(kw.get("transformation_type", "projective")) == "projective"
            and not kw.get("clahe", False) and str(kw.get("matcher_name", "bf")) in ("bf", "flann"))


class SiftStabilizer:
    def __init__(self, frame_hw: tuple[int, int], *, detector_name: str = "rsift", matcher_name: str = "bf", filter_type: str = "ratio",
                 transformation_type: str = "projective", clahe: bool = False, downsample_ratio: float = 0.5, max_features: int = 2000,
                 ref_multiplier: float = 2.0, filter_ratio: float = 0.9, ransac_method: int = 38, ransac_epipolar_threshold: float = 2.0,
                 ransac_max_iter: int = 5000, ransac_confidence: float = 0.999999, mask_use: bool = True, mask_margin_ratio: float = 0.15,
                 min_good_match_count_warning: int = 20, min_inliers_match_count_warning: int = 10, rsift_eps: float = 1e-8, seed: int = 0,
                 ctx: _lib.Context | None = None, **unused):
        if detector_name not in ("sift", "rsift"):
            raise NotImplementedError(f"detector_name='{detector_name}': SiftStabilizer runs 'sift' and 'rsift' (Stabilizer runs 'orb')")
        if not unused.get("sift_enable_precise_upscale", False):
            logger.warning(f"detector_name='{detector_name}': this build's SIFT doubles the base image with OpenCV's precise (half-pixel aligned) "
                           "upscaling; `sift_enable_precise_upscale: false` (default.yaml:112) is not implemented -- keypoints sit ~0.25 px from where "
                           "stabilo's default would put them, on both frames alike")
        if filter_type != "ratio" or transformation_type != "projective" or clahe:
            raise NotImplementedError(f"detector_name='{detector_name}' is built with filter_type 'ratio', transformation_type 'projective' and clahe off")
        if float(downsample_ratio) != 0.5:
            raise NotImplementedError(f"detector_name='{detector_name}' on the gray image in HBM needs downsample_ratio 0.5 (got {downsample_ratio}): "
                                      "Stabilizer runs other ratios on host frames")
        if matcher_name == "flann":
            logger.warning("matcher_name='flann': matched with the exact brute-force kernel (what FLANN approximates); a stabilo run with FLANN "
                           "may keep slightly different matches")
        elif matcher_name != "bf":
            raise NotImplementedError(f"matcher_name='{matcher_name}': 'bf' (exact brute force) and 'flann' (served by the same exact kernel) are implemented")
        self.ctx = ctx or _lib.default_context()
        self.frame_hw = (int(frame_hw[0]), int(frame_hw[1]))
        self.work_hw = (self.frame_hw[0] // 2, self.frame_hw[1] // 2)
        self._ratio = float(downsample_ratio)
        self.min_good, self.min_inl = min_good_match_count_warning, min_inliers_match_count_warning
        cfg = SiftStabConfig(work_h=self.work_hw[0], work_w=self.work_hw[1], max_features=max(int(max_features), 4), ref_multiplier=ref_multiplier,
                             root=int(detector_name == "rsift"), rsift_eps=rsift_eps, filter_ratio=filter_ratio,
                             ransac_threshold=ransac_epipolar_threshold, ransac_max_iter=ransac_max_iter, ransac_confidence=ransac_confidence,
                             mask_use=int(bool(mask_use)), mask_margin_ratio=mask_margin_ratio, downsample_ratio=self._ratio, seed=int(seed))
        self.handle = None
        h = C.c_void_p()
        check(self.ctx.lib.gtx_sift_stab_create(self.ctx.handle, C.byref(cfg), C.byref(h)))
        self.handle = h
        self._H = None                   # what get_cur_trans_matrix() returns: this frame's transform, else the last known one
        self._H_raw = None               # this frame's own transform, None when the frame could not be registered
        self._H_last_known = None
        self._H_work = None              # this frame's own transform in working-resolution pixels, as the library returned it
        self._stats = np.zeros(4, np.int32)
        self._cur_boxes = None
        self._pending_boxes = None
        self._mask_use = bool(mask_use)
        self._rects_warned = False

    # ---- lifecycle
    def close(self):
        if getattr(self, "handle", None):
            self.ctx.lib.gtx_sift_stab_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _boxes(self, boxes):
        if boxes is None or len(boxes) == 0:
            return None, 0
        b = np.ascontiguousarray(boxes, dtype=np.float32).reshape(-1, 4)
        if len(b) > MAX_MASK_RECTS and self._mask_use and not self._rects_warned:
            self._rects_warned = True
            logger.warning(f"{len(b)} boxes: the vehicle mask holds {MAX_MASK_RECTS} rectangles, keypoints on the boxes beyond them reach the matcher")
        return b, len(b)

    # ---- stabilo interface, on the gray image in HBM
    def set_ref_frame(self, frame, boxes=None) -> None:
        raise NotImplementedError("SiftStabilizer reads the detector's gray image in HBM (set_ref_gray_dev); Stabilizer takes host frames")

    def set_ref_gray_dev(self, gray_dptr: int, gh: int, gw: int, boxes=None) -> None:
        b, n = self._boxes(boxes)
        check(self.ctx.lib.gtx_sift_stab_set_ref_gray_dev(self.handle, C.c_void_p(gray_dptr), gh, gw, ptr(b), n))
        self._H = self._H_raw = self._H_last_known = self._H_work = None
        self._cur_boxes = None

    def _finish(self, Hw, valid, boxes):
        # stabilo keeps `trans_matrix_last_known`: a frame that cannot be registered (too few matches, no model) takes the
        # previous valid transform for its boxes and reports it as its matrix; before the first valid one there is none.
        self._H_work = self._H_raw = None
        if valid.value:
            self._H_work = Hw.reshape(3, 3).copy()
            r = self._ratio
            D = np.diag([r, r, 1.0])
            Hf = np.linalg.inv(D) @ self._H_work @ D                         # working-resolution pixels -> frame pixels on both sides
            self._H_raw = Hf / Hf[2, 2]
            self._H_last_known = self._H_raw
        self._H = self._H_last_known
        self._cur_boxes = boxes
        if self._stats[2] < self.min_good:
            logger.warning(f"Only {int(self._stats[2])} good matches found.")
        elif self._H is not None and self._stats[3] < self.min_inl:
            logger.warning(f"Only {int(self._stats[3])} inliers found.")

    def stabilize_gray_dev(self, gray_dptr: int, gh: int, gw: int, boxes=None) -> None:
        b, n = self._boxes(boxes)
        H, valid = np.zeros(9, np.float64), C.c_int()
        check(self.ctx.lib.gtx_sift_stab_stabilize_gray_dev(self.handle, C.c_void_p(gray_dptr), gh, gw, ptr(b), n, ptr(H), C.byref(valid),
                                                            ptr(self._stats)))
        self._finish(H, valid, b)

    def submit_gray_dev(self, gray_dptr: int, gh: int, gw: int, boxes=None) -> None:
        """Asynchronous stabilize: enqueue on the object's stream; pair with collect()."""
        b, n = self._boxes(boxes)
        check(self.ctx.lib.gtx_sift_stab_submit_gray_dev(self.handle, C.c_void_p(gray_dptr), gh, gw, ptr(b), n))
        self._pending_boxes = b

    def collect(self) -> None:
        H, valid = np.zeros(9, np.float64), C.c_int()
        check(self.ctx.lib.gtx_sift_stab_collect(self.handle, ptr(H), C.byref(valid), ptr(self._stats)))
        self._finish(H, valid, self._pending_boxes)

    def last_ms(self) -> float:
        """GPU time (ms) of the last collected pass."""
        ms = C.c_float()
        check(self.ctx.lib.gtx_sift_stab_last_ms(self.handle, C.byref(ms)))
        return float(ms.value)

    def get_cur_trans_matrix(self, raw: bool = False) -> np.ndarray | None:
        """3x3 float64 mapping current-frame pixels to reference-frame pixels, or None. raw=True: None also when this
        frame itself could not be registered."""
        H = self._H_raw if raw else self._H
        return None if H is None else H.copy()

    def working_matrix(self) -> np.ndarray | None:
        """This frame's own transform in working-resolution pixels, exactly as the library returned it (None: not registered)."""
        return None if self._H_work is None else self._H_work.copy()

    @property
    def registered(self) -> bool:
        """False when the last frame took the last known transform (or none) instead of one of its own."""
        return self._H_raw is not None

    def transform_cur_boxes(self) -> np.ndarray:
        """The boxes given with the last frame, mapped into the reference frame (xywh)."""
        if self._cur_boxes is None:
            return np.zeros((0, 4), np.float32)
        if self._H is None:
            return self._cur_boxes.copy()
        return geometry.warp_boxes(self._H, self._cur_boxes)

    def get_cur_num_keypoints(self) -> tuple[int, int]:
        return int(self._stats[0]), int(self._stats[1])  # (reference, current)

    def get_cur_num_matches(self) -> int:
        return int(self._stats[2])

    def get_cur_inliers_count(self) -> int:
        return int(self._stats[3])

    # ---- introspection for the parity tests
    def keypoints(self, which: str = "cur") -> dict:
        """kp5 rows (x, y, size, angle, response), octave words and descriptors, as gtx_sift_detect reports them."""
        w_ = 0 if which == "ref" else 1
        n = C.c_int()
        check(self.ctx.lib.gtx_sift_stab_keypoints(self.handle, w_, 0, C.byref(n), None, None, None))
        k = n.value
        kp5, octv, desc = np.zeros((k, 5), np.float32), np.zeros(k, np.int32), np.zeros((k, 128), np.float32)
        if k:
            check(self.ctx.lib.gtx_sift_stab_keypoints(self.handle, w_, k, C.byref(n), ptr(kp5), ptr(octv), ptr(desc)))
        return dict(kp5=kp5, octave=octv, desc=desc)

    def pairs(self) -> np.ndarray:
        """The last collected frame's pairs after the ratio test, [n][4] = (x_cur, y_cur, x_ref, y_ref), in query order."""
        n = C.c_int()
        check(self.ctx.lib.gtx_sift_stab_pairs(self.handle, 0, C.byref(n), None))
        pts = np.zeros((n.value, 4), np.float32)
        if n.value:
            check(self.ctx.lib.gtx_sift_stab_pairs(self.handle, n.value, C.byref(n), ptr(pts)))
        return pts

    def counters(self) -> np.ndarray:
        """The extraction's counters of the last collected frame: extrema candidates, refined, oriented, keypoints kept."""
        out = np.zeros(4, np.int32)
        check(self.ctx.lib.gtx_sift_stab_counters(self.handle, ptr(out)))
        return out
