"""Projective helpers over the C ABI (host, f64): box warp of the stabilizer and the point
transform of the georeference stage; and the transform bookkeeping the stabilizer classes, the
engine and the sharded replay share (last known transform, box warp, working -> frame pixels).

Reference calls replaced: stabilo ``Stabilizer.transform_cur_boxes()`` (geotrax/extract.py:183)
and ``cv2.perspectiveTransform`` inside ``apply_homography`` (geotrax/georeference.py:599-605);
``ortho2geo`` (georeference.py:608-615) is plain affine arithmetic and is restated in numpy.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from ._lib import check, ptr


def warp_boxes(H: np.ndarray, xywh: np.ndarray) -> np.ndarray:
    """Each xywh box -> axis-aligned hull of its four corners mapped through H, as xywh float32."""
    lib = _lib.load()
    Hm = np.ascontiguousarray(H, dtype=np.float64).reshape(9)
    b = np.ascontiguousarray(xywh, dtype=np.float32).reshape(-1, 4)
    out = np.empty_like(b)
    check(lib.gtx_warp_boxes(ptr(Hm), ptr(b), len(b), ptr(out)))
    return out


def xyxy_to_xywh(b: np.ndarray) -> np.ndarray | None:
    """Corner boxes -> centre/size float32; None for a frame without boxes."""
    if len(b) == 0:
        return None
    return np.stack([(b[:, 0] + b[:, 2]) / 2, (b[:, 1] + b[:, 3]) / 2, b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]], 1).astype(np.float32)


def stabilized_boxes(H: np.ndarray | None, xywh: np.ndarray) -> np.ndarray:
    """The boxes of a frame in the reference frame: warped through H, or a copy while no transform is known."""
    return warp_boxes(H, xywh) if H is not None else xywh.copy()


def work_to_frame(Hw: np.ndarray, ratio: float) -> np.ndarray:
    """A transform between working-resolution images (downsample_ratio `ratio`) as one between the frames: working pixels ->
    frame pixels on both sides, D^-1 Hw D with D = diag(ratio, ratio, 1), normalised by its [2, 2]."""
    D = np.diag([ratio, ratio, 1.0])
    Hf = np.linalg.inv(D) @ Hw @ D
    return Hf / Hf[2, 2]


class LastKnown:
    """stabilo's `trans_matrix_last_known`: a frame that cannot be registered (too few matches, no model) takes the previous
    valid transform for its boxes and reports it as its matrix; before the first valid one there is none. `copy`: keep a copy
    of every valid transform and hand out copies of it (False: the caller's own array is kept and handed out)."""

    def __init__(self, copy: bool = True):
        self.H, self._copy = None, copy

    def reset(self) -> None:
        self.H = None

    def update(self, H: np.ndarray | None) -> tuple[np.ndarray | None, bool]:
        """H: this frame's own transform or None -> (the transform the frame takes, whether it is the last known one)."""
        if H is not None:
            self.H = H.copy() if self._copy else H
            return H, False
        if self.H is None:
            return None, False
        return (self.H.copy() if self._copy else self.H), True


def apply_homography(input_x: np.ndarray, input_y: np.ndarray, homography: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """Same name and argument order as the reference function (georeference.py:599-605)."""
    lib = _lib.load()
    Hm = np.ascontiguousarray(homography, dtype=np.float64).reshape(9)
    x = np.ascontiguousarray(input_x, dtype=np.float64).reshape(-1)
    y = np.ascontiguousarray(input_y, dtype=np.float64).reshape(-1)
    ox, oy = np.empty_like(x), np.empty_like(y)
    check(lib.gtx_perspective_points(ptr(Hm), ptr(x), ptr(y), len(x), ptr(ox), ptr(oy)))
    return ox, oy


def ortho2geo(ortho_x: np.ndarray, ortho_y: np.ndarray, ortho_params: tuple) -> tuple[np.ndarray, np.ndarray]:
    """Orthophoto pixel -> (latitude, longitude) by the orthophoto's affine geotransform
    (georeference.py:608-615)."""
    lng0, lat0, dlng, dlat, skew_x, skew_y = ortho_params
    return lat0 + dlat * ortho_y + skew_y * ortho_x, lng0 + dlng * ortho_x + skew_x * ortho_y
