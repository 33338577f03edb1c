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
from .stabilizer_base import _StabilizerBase, check_options

logger = logging.getLogger(__name__)

MAX_MASK_RECTS = 1024          # kMaxMaskRects of csrc/sift.hip: what one frame's mask holds


def resident(stab_kw: dict | None) -> bool:
    """Whether this ``stabilo:`` block runs on SiftStabilizer (else: Stabilizer, whatever it makes of it)."""
    kw = stab_kw or {}
    return (str(kw.get("detector_name", "orb")) in ("sift", "rsift") and float(kw.get("downsample_ratio", 0.5)) == 0.5
            and str(kw.get("filter_type", "ratio")) == "ratio" and str(kw.get("transformation_type", "projective")) == "projective"
            and not kw.get("clahe", False) and str(kw.get("matcher_name", "bf")) in ("bf", "flann"))


class SiftStabilizer(_StabilizerBase):
    _destroy, _log = "gtx_sift_stab_destroy", logger

    def __init__(self, frame_hw: tuple[int, int], *, detector_name: str = "rsift", matcher_name: str = "bf", filter_type: str = "ratio",
                 transformation_type: str = "projective", clahe: bool = False, downsample_ratio: float = 0.5, max_features: int = 2000,
                 ref_multiplier: float = 2.0, filter_ratio: float = 0.9, ransac_method: int = 38, ransac_epipolar_threshold: float = 2.0,
                 ransac_max_iter: int = 5000, ransac_confidence: float = 0.999999, mask_use: bool = True, mask_margin_ratio: float = 0.15,
                 min_good_match_count_warning: int = 20, min_inliers_match_count_warning: int = 10, rsift_eps: float = 1e-8, seed: int = 0,
                 ctx: _lib.Context | None = None, **unused):
        if detector_name not in ("sift", "rsift"):
            raise NotImplementedError(f"detector_name='{detector_name}': SiftStabilizer runs 'sift' and 'rsift' (Stabilizer runs 'orb')")
        check_options(logger, detector_name, matcher_name, filter_type, transformation_type, clahe, unused.get("sift_enable_precise_upscale", False),
                      hbm_ratio=downsample_ratio)
        super().__init__(min_good_match_count_warning, min_inliers_match_count_warning)
        self.ctx = ctx or _lib.default_context()
        self.frame_hw = (int(frame_hw[0]), int(frame_hw[1]))
        self.work_hw = (self.frame_hw[0] // 2, self.frame_hw[1] // 2)
        self._ratio = float(downsample_ratio)
        cfg = SiftStabConfig(work_h=self.work_hw[0], work_w=self.work_hw[1], max_features=max(int(max_features), 4), ref_multiplier=ref_multiplier,
                             root=int(detector_name == "rsift"), rsift_eps=rsift_eps, filter_ratio=filter_ratio,
                             ransac_threshold=ransac_epipolar_threshold, ransac_max_iter=ransac_max_iter, ransac_confidence=ransac_confidence,
                             mask_use=int(bool(mask_use)), mask_margin_ratio=mask_margin_ratio, downsample_ratio=self._ratio, seed=int(seed))
        h = C.c_void_p()
        check(self.ctx.lib.gtx_sift_stab_create(self.ctx.handle, C.byref(cfg), C.byref(h)))
        self.handle = h
        self._H_work = None              # this frame's own transform in working-resolution pixels, as the library returned it
        self._mask_use = bool(mask_use)
        self._rects_warned = False

    def _check_mask(self, b):
        if len(b) > MAX_MASK_RECTS and self._mask_use and not self._rects_warned:
            self._rects_warned = True
            logger.warning(f"{len(b)} boxes: the vehicle mask holds {MAX_MASK_RECTS} rectangles, keypoints on the boxes beyond them reach the matcher")

    # ---- stabilo interface, on the gray image in HBM
    def set_ref_frame(self, frame, boxes=None) -> None:
        raise NotImplementedError("SiftStabilizer reads the detector's gray image in HBM (set_ref_gray_dev); Stabilizer takes host frames")

    def set_ref_gray_dev(self, gray_dptr: int, gh: int, gw: int, boxes=None) -> None:
        b, n = self._boxes(boxes)
        check(self.ctx.lib.gtx_sift_stab_set_ref_gray_dev(self.handle, C.c_void_p(gray_dptr), gh, gw, ptr(b), n))
        self._H_work = None
        self._new_reference()

    def _result(self, Hw, valid, boxes):
        """What the library wrote for a frame: Hw[9] in working-resolution pixels, valid 0 when the frame could not be registered."""
        self._H_work = Hw.reshape(3, 3).copy() if valid.value else None
        self._finish(None if self._H_work is None else geometry.work_to_frame(self._H_work, self._ratio), boxes)

    def stabilize_gray_dev(self, gray_dptr: int, gh: int, gw: int, boxes=None) -> None:
        b, n = self._boxes(boxes)
        H, valid = np.zeros(9, np.float64), C.c_int()
        check(self.ctx.lib.gtx_sift_stab_stabilize_gray_dev(self.handle, C.c_void_p(gray_dptr), gh, gw, ptr(b), n, ptr(H), C.byref(valid),
                                                            ptr(self._stats)))
        self._result(H, valid, b)

    def submit_gray_dev(self, gray_dptr: int, gh: int, gw: int, boxes=None) -> None:
        """Asynchronous stabilize: enqueue on the object's stream; pair with collect()."""
        b, n = self._boxes(boxes)
        check(self.ctx.lib.gtx_sift_stab_submit_gray_dev(self.handle, C.c_void_p(gray_dptr), gh, gw, ptr(b), n))
        self._pending_boxes = b

    def collect(self) -> None:
        H, valid = np.zeros(9, np.float64), C.c_int()
        check(self.ctx.lib.gtx_sift_stab_collect(self.handle, ptr(H), C.byref(valid), ptr(self._stats)))
        self._result(H, valid, self._pending_boxes)

    def last_ms(self) -> float:
        """GPU time (ms) of the last collected pass."""
        ms = C.c_float()
        check(self.ctx.lib.gtx_sift_stab_last_ms(self.handle, C.byref(ms)))
        return float(ms.value)

    def working_matrix(self) -> np.ndarray | None:
        """This frame's own transform in working-resolution pixels, exactly as the library returned it (None: not registered)."""
        return None if self._H_work is None else self._H_work.copy()

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
