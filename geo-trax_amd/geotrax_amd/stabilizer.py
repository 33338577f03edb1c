"""Stabilizer object over the C ABI (gtx_stabilizer_*), with stabilo's method names.

Reference behaviour replaced: ``stabilo.Stabilizer`` as driven by geotrax/extract.py:139,177-187
(per-frame registration against the first processed frame) and geotrax/utils/registration.py:59-85
(image-to-image registration). Constructor keywords are the keys of the reference's ``stabilo:``
config block (geotrax/cfg/default.yaml:100-145); unknown or unsupported choices raise.
"""
from __future__ import annotations

import ctypes as C
import logging

import numpy as np

from . import _lib, geometry
from ._lib import StabConfig, check, ptr
from .stabilizer_base import _StabilizerBase, check_options

logger = logging.getLogger(__name__)


def working_size(frame_hw: tuple[int, int], ratio: float) -> tuple[int, int]:
    """(gh, gw) of the gray image the ORB stabilizer works on for frames of (h, w) at `downsample_ratio` ratio -- the size the
    library's `_gray_dev` entries expect and gtx_op_gray_working_size returns. 0.5 keeps the detector's half-resolution image
    (h // 2, w // 2) and 1.0 the frame's own size; every other ratio in (0, 1]: rint(h * r), rint(w * r), computed in double from the
    float32 ratio the config struct carries, halves to even. Where h * r and w * r are integers this is cv2.resize(fx=r, fy=r)'s
    size and its source step; elsewhere the rule is oracle/yolov8_ref.py::resize_linear_u8's for this size."""
    h, w = int(frame_hw[0]), int(frame_hw[1])
    r = float(np.float32(ratio))
    if not 0.0 < r <= 1.0:
        raise ValueError(f"downsample_ratio must be in (0, 1] (got {ratio})")
    if r == 0.5:
        return h // 2, w // 2
    if r == 1.0:
        return h, w
    return int(np.rint(h * r)), int(np.rint(w * r))


class Stabilizer(_StabilizerBase):
    _destroy, _log = "gtx_stabilizer_destroy", logger

    def __init__(self, frame_hw: tuple[int, int] | None = None, *, detector_name: str = "orb", matcher_name: str = "bf",
                 filter_type: str = "ratio", transformation_type: str = "projective", clahe: bool = False,
                 downsample_ratio: float = 0.5, max_features: int = 2000, ref_multiplier: float = 2.0,
                 filter_ratio: float = 0.9, ransac_method: int = 38, ransac_epipolar_threshold: float = 2.0,
                 ransac_max_iter: int = 5000, ransac_confidence: float = 0.999999, mask_use: bool = True,
                 mask_margin_ratio: float = 0.15, min_good_match_count_warning: int = 20,
                 min_inliers_match_count_warning: int = 10, fast_threshold: int = 20, n_levels: int = 8,
                 scale_factor: float = 1.2, seed: int = 0, match_query_frame: str = "current",
                 ctx: _lib.Context | None = None, **unused):
        if detector_name not in ("orb", "sift", "rsift"):
            raise NotImplementedError(f"detector_name='{detector_name}': 'orb', 'sift' and 'rsift' are implemented (not brisk / kaze / akaze)")
        self._sift = detector_name if detector_name != "orb" else None
        check_options(logger, detector_name, matcher_name, filter_type, transformation_type, clahe, unused.get("sift_enable_precise_upscale", False))
        if filter_type not in ("ratio", "none"):
            raise NotImplementedError(f"filter_type='{filter_type}': only 'ratio' and 'none' are implemented")
        if transformation_type not in ("projective", "affine"):
            raise ValueError(f"transformation_type='{transformation_type}' (choices: projective, affine)")
        self.ctx = ctx or _lib.default_context()
        self._kw = dict(downsample_ratio=downsample_ratio, max_features=max_features, ref_multiplier=ref_multiplier,
                        filter_ratio=filter_ratio, ransac_threshold=ransac_epipolar_threshold, ransac_max_iter=ransac_max_iter,
                        ransac_confidence=ransac_confidence, mask_use=int(mask_use), mask_margin_ratio=mask_margin_ratio,
                        fast_threshold=fast_threshold, n_levels=n_levels, scale_factor=scale_factor, seed=seed, clahe=int(bool(clahe)),
                        affine=int(transformation_type == "affine"), filter_type=int(filter_type == "none"))
        super().__init__(min_good_match_count_warning, min_inliers_match_count_warning)
        self.frame_hw = None
        self._ref_img = None
        self._mask_warned = False
        if frame_hw is not None and not self._sift:
            self._create(frame_hw)
        elif frame_hw is not None:
            self.frame_hw = (int(frame_hw[0]), int(frame_hw[1]))

    # ---- lifecycle
    def _create(self, frame_hw):
        cfg = StabConfig(frame_h=int(frame_hw[0]), frame_w=int(frame_hw[1]), **self._kw)
        h = C.c_void_p()
        check(self.ctx.lib.gtx_stabilizer_create(self.ctx.handle, C.byref(cfg), C.byref(h)))
        self.handle, self.frame_hw = h, (int(frame_hw[0]), int(frame_hw[1]))

    # ---- detector_name sift / rsift (default.yaml:109): the registration stage's kernels (csrc/sift.hip, match_l2.hip, the RANSAC of
    # homography.hip behind gtx_register_images) on the working-resolution frames; one blocking call per frame, host frames only
    def _working(self, frame):
        f = np.ascontiguousarray(frame, dtype=np.uint8)
        r = float(self._kw["downsample_ratio"])
        if r == 1.0:
            return f
        if r != 0.5:
            raise NotImplementedError("detector_name sift / rsift: downsample_ratio 1.0 or 0.5")
        h, w = f.shape[0] // 2 * 2, f.shape[1] // 2 * 2
        q = f[:h, :w].astype(np.uint16)
        return ((q[0::2, 0::2] + q[0::2, 1::2] + q[1::2, 0::2] + q[1::2, 1::2] + 2) >> 2).astype(np.uint8)      # cv2.resize(INTER_LINEAR) at exactly 1/2

    def _sift_register(self, frame, boxes):
        from .registration import register_once

        if boxes is not None and len(boxes) and self._kw["mask_use"] and not self._mask_warned:
            self._mask_warned = True
            logger.warning(f"detector_name='{self._sift}': the vehicle mask (mask_use) is not applied on this path; keypoints on vehicles reach the matcher")
        cur = self._working(frame)
        n_cur = int(self._kw["max_features"])
        Hh, stats, _ = register_once(cur, self._ref_img, max_features=max(n_cur, 4), filter_ratio=self._kw["filter_ratio"],
                                     ransac_epipolar_threshold=self._kw["ransac_threshold"], ransac_max_iter=self._kw["ransac_max_iter"],
                                     ransac_confidence=self._kw["ransac_confidence"], rsift_eps=1e-8 if self._sift == "rsift" else -1.0,
                                     seed=self._kw["seed"], ctx=self.ctx)
        self._stats[:] = (stats[1], stats[0], stats[2], stats[3])          # (reference, current, matches, inliers)
        b, _ = self._boxes(boxes)
        self._finish(None if Hh is None else geometry.work_to_frame(Hh, float(self._kw["downsample_ratio"])), b)

    # ---- stabilo interface
    def set_ref_frame(self, frame: np.ndarray, boxes: np.ndarray | None = None) -> None:
        if self._sift:
            self._ref_img = self._working(frame)
            self.frame_hw = tuple(np.asarray(frame).shape[:2])
            self._new_reference()
            return
        f = np.ascontiguousarray(frame, dtype=np.uint8)
        if self.handle is None:
            self._create(f.shape[:2])
        b, n = self._boxes(boxes)
        check(self.ctx.lib.gtx_stabilizer_set_ref_frame(self.handle, ptr(f), f.shape[0], f.shape[1], ptr(b), n))
        self._new_reference()

    def set_ref_gray_dev(self, gray_dptr: int, gh: int, gw: int, boxes=None) -> None:
        if self._sift:
            raise NotImplementedError(f"detector_name='{self._sift}' takes host frames (set_ref_frame / stabilize): run with engine: {{pipelined: false}}")
        b, n = self._boxes(boxes)
        check(self.ctx.lib.gtx_stabilizer_set_ref_gray_dev(self.handle, C.c_void_p(gray_dptr), gh, gw, ptr(b), n))
        self._new_reference()

    def _result(self, H, valid, boxes):
        """What the library wrote for a frame: H[9] in frame pixels, valid 0 when the frame could not be registered."""
        self._finish(H.reshape(3, 3).copy() if valid.value else None, boxes)

    def stabilize(self, frame: np.ndarray, boxes: np.ndarray | None = None) -> None:
        if self._sift:
            if self._ref_img is None:
                raise RuntimeError("stabilize() before set_ref_frame()")
            return self._sift_register(frame, boxes)
        f = np.ascontiguousarray(frame, dtype=np.uint8)
        b, n = self._boxes(boxes)
        H, valid = np.zeros(9, np.float64), C.c_int()
        check(self.ctx.lib.gtx_stabilizer_stabilize(self.handle, ptr(f), f.shape[0], f.shape[1], ptr(b), n, ptr(H),
                                                    C.byref(valid), ptr(self._stats)))
        self._result(H, valid, b)

    def stabilize_gray_dev(self, gray_dptr: int, gh: int, gw: int, boxes=None) -> None:
        b, n = self._boxes(boxes)
        H, valid = np.zeros(9, np.float64), C.c_int()
        check(self.ctx.lib.gtx_stabilizer_stabilize_gray_dev(self.handle, C.c_void_p(gray_dptr), gh, gw, ptr(b), n, ptr(H),
                                                             C.byref(valid), ptr(self._stats)))
        self._result(H, valid, b)

    def submit_gray_dev(self, gray_dptr: int, gh: int, gw: int, boxes=None) -> None:
        """Asynchronous stabilize: enqueue on the stabilizer's stream; pair with collect()."""
        b, n = self._boxes(boxes)
        check(self.ctx.lib.gtx_stabilizer_submit_gray_dev(self.handle, C.c_void_p(gray_dptr), gh, gw, ptr(b), n))
        self._pending_boxes = b

    def collect(self) -> None:
        H, valid = np.zeros(9, np.float64), C.c_int()
        check(self.ctx.lib.gtx_stabilizer_collect(self.handle, ptr(H), C.byref(valid), ptr(self._stats)))
        self._result(H, valid, self._pending_boxes)

    def last_ms(self) -> float:
        """GPU time (ms) of the last collected asynchronous pass."""
        ms = C.c_float()
        check(self.ctx.lib.gtx_stabilizer_last_ms(self.handle, C.byref(ms)))
        return float(ms.value)

    # ---- introspection for the parity tests
    def promote_cur(self) -> None:
        """The frame stabilized last becomes the reference (its features are kept, nothing is extracted again); ref_multiplier 1 only."""
        check(self.ctx.lib.gtx_stabilizer_promote_cur(self.handle))

    def keypoints(self, which: str = "cur"):
        cap = 1 << 16
        n = C.c_int()
        xy, lvl, ab = np.zeros((cap, 2), np.float32), np.zeros(cap, np.int32), np.zeros(cap, np.int32)
        desc = np.zeros((cap, 32), np.uint8)
        check(self.ctx.lib.gtx_stabilizer_keypoints(self.handle, 0 if which == "ref" else 1, cap, C.byref(n), ptr(xy), ptr(lvl),
                                                    ptr(ab), ptr(desc)))
        k = n.value
        return dict(xy=xy[:k].copy(), level=lvl[:k].copy(), bin=ab[:k].copy(), desc=desc[:k].copy())

    def matches(self):
        cap = 1 << 16
        n = C.c_int()
        q, t, d = np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros(cap, np.int32)
        check(self.ctx.lib.gtx_stabilizer_matches(self.handle, cap, C.byref(n), ptr(q), ptr(t), ptr(d)))
        k = n.value
        return q[:k].copy(), t[:k].copy(), d[:k].copy()

    def keep_pass(self, on: bool = True) -> None:
        """Every later extract pass keeps what level() and candidates() read back (off by default: nothing is kept)."""
        check(self.ctx.lib.gtx_stabilizer_keep_pass(self.handle, int(on)))

    def level(self, which: str, i: int) -> np.ndarray:
        """Pyramid level i of the last extract pass [h, w] u8; `which` ('ref' / 'cur') must name the set that pass filled."""
        w_ = 0 if which == "ref" else 1
        h, w = C.c_int(), C.c_int()
        check(self.ctx.lib.gtx_stabilizer_level(self.handle, w_, i, C.byref(h), C.byref(w), None, 0))
        out = np.zeros((h.value, w.value), np.uint8)
        check(self.ctx.lib.gtx_stabilizer_level(self.handle, w_, i, C.byref(h), C.byref(w), ptr(out), out.size))
        return out

    def candidates(self, which: str, i: int) -> dict:
        """Level i of the last extract pass after FAST, NMS and the mask: pix (y * w + x) and score in no particular order, n_elig
        (what stage 1 handed to the Harris ranking), n_kp (keypoints kept), dropped (candidates that found their sub-list full)."""
        w_ = 0 if which == "ref" else 1
        n, ne, nk, nd = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        check(self.ctx.lib.gtx_stabilizer_candidates(self.handle, w_, i, 0, C.byref(n), None, None, C.byref(ne), C.byref(nk), C.byref(nd)))
        pix, score = np.zeros(n.value, np.int32), np.zeros(n.value, np.int32)
        if n.value:
            check(self.ctx.lib.gtx_stabilizer_candidates(self.handle, w_, i, n.value, C.byref(n), ptr(pix), ptr(score), None, None, None))
        return dict(pix=pix, score=score, n_elig=ne.value, n_kp=nk.value, dropped=nd.value)

    def pattern(self) -> np.ndarray:
        out = np.zeros((256, 256, 4), np.int8)
        check(self.ctx.lib.gtx_stabilizer_pattern(self.handle, ptr(out)))
        return out
