"""What the stabilizer classes share: Stabilizer (stabilizer.py) and SiftStabilizer (sift_stabilizer.py) differ in the library
object they drive and in where a frame's image comes from; the option checks of the ``stabilo:`` block, the transform
bookkeeping after a frame and stabilo's read-out methods are the same and live here.
"""
from __future__ import annotations

import numpy as np

from .geometry import LastKnown, stabilized_boxes


def check_options(logger, detector_name: str, matcher_name: str, filter_type: str, transformation_type: str, clahe: bool,
                  precise_upscale: bool, hbm_ratio: float | None = None) -> None:
    """The checks of a ``stabilo:`` block both classes make, in the order they always made them; the warnings go to `logger`,
    the calling class's own. `hbm_ratio`: the downsample_ratio of an object that reads the detector's half-resolution gray
    image in HBM (SiftStabilizer), which must be 0.5."""
    if detector_name in ("sift", "rsift"):
        if not precise_upscale:
            logger.warning(f"detector_name='{detector_name}': this build's SIFT doubles the base image with OpenCV's precise (half-pixel aligned) "
                           "upscaling; `sift_enable_precise_upscale: false` (default.yaml:112) is not implemented -- keypoints sit ~0.25 px from where "
                           "stabilo's default would put them, on both frames alike")
        if filter_type != "ratio" or transformation_type != "projective" or clahe:
            raise NotImplementedError(f"detector_name='{detector_name}' is built with filter_type 'ratio', transformation_type 'projective' and clahe off")
    if hbm_ratio is not None and float(hbm_ratio) != 0.5:
        raise NotImplementedError(f"detector_name='{detector_name}' on the gray image in HBM needs downsample_ratio 0.5 (got {hbm_ratio}): "
                                  "Stabilizer runs other ratios on host frames")
    if matcher_name == "flann":
        # FLANN returns APPROXIMATE nearest neighbours (LSH for binary descriptors, kd-trees for SIFT); the GPU matcher is exact
        # and faster than either here, so the option runs on it: the matches are the ones FLANN approximates, not FLANN's own
        logger.warning("matcher_name='flann': matched with the exact brute-force kernel (what FLANN approximates); a stabilo run with FLANN "
                       "may keep slightly different matches")
    elif matcher_name != "bf":
        raise NotImplementedError(f"matcher_name='{matcher_name}': 'bf' (exact brute force) and 'flann' (served by the same exact kernel) are implemented")


class _StabilizerBase:
    _destroy = ""                    # the library entry that destroys self.handle
    _log = None                      # the subclass's module logger

    def __init__(self, min_good: int, min_inl: int):
        self.min_good, self.min_inl = min_good, min_inl
        self.handle = None
        self._H = None                   # what get_cur_trans_matrix() returns: this frame's transform, else the last known one
        self._H_raw = None               # this frame's own transform, None when the frame could not be registered
        self._last = LastKnown(copy=False)
        self._stats = np.zeros(4, np.int32)
        self._cur_boxes = None
        self._pending_boxes = None

    # ---- lifecycle
    def close(self):
        if getattr(self, "handle", None):
            getattr(self.ctx.lib, self._destroy)(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _new_reference(self) -> None:
        self._H = self._H_raw = None
        self._last.reset()
        self._cur_boxes = None

    def _boxes(self, boxes):
        if boxes is None or len(boxes) == 0:
            return None, 0
        b = np.ascontiguousarray(boxes, dtype=np.float32).reshape(-1, 4)
        self._check_mask(b)
        return b, len(b)

    def _check_mask(self, b: np.ndarray) -> None:
        """A subclass whose mask cannot hold every box says so here."""

    def _finish(self, H_raw, boxes) -> None:
        """H_raw: the transform of the frame just registered, in frame pixels, None when it could not be registered."""
        self._H_raw = H_raw
        self._H, _ = self._last.update(H_raw)
        self._cur_boxes = boxes
        if self._stats[2] < self.min_good:
            self._log.warning(f"Only {int(self._stats[2])} good matches found.")
        elif self._H is not None and self._stats[3] < self.min_inl:
            self._log.warning(f"Only {int(self._stats[3])} inliers found.")

    # ---- stabilo's read-out
    def get_cur_trans_matrix(self, raw: bool = False) -> np.ndarray | None:
        """3x3 float64 mapping current-frame pixels to reference-frame pixels, or None. raw=True: None also when this
        frame itself could not be registered (the engine, whose stabilizer objects take turns, keeps the last known
        transform in frame order itself)."""
        H = self._H_raw if raw else self._H
        return None if H is None else H.copy()

    @property
    def registered(self) -> bool:
        """False when the last frame took the last known transform (or none) instead of one of its own."""
        return self._H_raw is not None

    def transform_cur_boxes(self) -> np.ndarray:
        """The boxes given with the last frame, mapped into the reference frame (xywh)."""
        if self._cur_boxes is None:
            return np.zeros((0, 4), np.float32)
        return stabilized_boxes(self._H, self._cur_boxes)

    def get_cur_num_keypoints(self) -> tuple[int, int]:
        return int(self._stats[0]), int(self._stats[1])  # (reference, current)

    def get_cur_num_matches(self) -> int:
        return int(self._stats[2])

    def get_cur_inliers_count(self) -> int:
        return int(self._stats[3])
