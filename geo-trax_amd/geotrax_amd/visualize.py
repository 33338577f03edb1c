#!/usr/bin/env python3
"""visualize -- the stage that draws the tracking results over the clip, on MI355X.

Host-side restatement of the reference stage geotrax/visualize.py (same function names, argument meaning, file conventions,
flag names and config backfill). The frames never visit the host: the read-ahead feeder puts them into HBM, the frame source of
the mode runs there (gtx_warp_frame_dev for modes 1 / 4, gtx_dev_copy of the kept reference frame for mode 2), the boxes, labels
and tails of the frame are painted in place by one launch of the drawing kernel (gtx_drawer_draw_dev, csrc/draw.hip), and the JPEG
encoder (geotrax_amd.video_writer) takes the frame from there. What the host does per frame is what annotate_frame does around
its cv2 calls: it turns the frame's rows into the list of primitives (build_primitives), one per cv2 call or per line of one --

    cv2.rectangle(outline)  -> 4 SEGMENTs (x1,y1)-(x2,y1), (x2,y1)-(x2,y2), (x2,y2)-(x1,y2), (x1,y2)-(x1,y1)
    cv2.polylines(closed)   -> one SEGMENT per edge, corner i to corner i + 1, the last back to the first
    cv2.line                -> one SEGMENT (the dashes of _draw_dashed_poly are cv2.line calls in the reference, too)
    cv2.rectangle(-1)       -> one FILL
    cv2.putText             -> the label's GLYPH cells, left to right, baseline at the call's origin
    cv2.circle              -> one RING

in the reference's order: per vehicle box, label fill, label text, tail; vehicles in file order.

    python -m geotrax_amd.visualize <clip> [--viz-mode 0 1 3] [--hide-labels] ...      (the flags of `geotrax visualize`)

One output per mode, <output folder>/<stem>_mode_<k>.avi, frames cut_frame_left .. cut_frame_right - 1.

Not built (each is refused with a message):
  --show               there is no window.
  --plot-trajectories  needs a whole-frame alpha blend (cv2.addWeighted), which is another kernel.
  `geotrax batch` does not run this stage yet (geotrax_amd.batch answers --viz-only as before).

Stated differences from the reference's pictures (the geometry handed to the rasteriser is the reference's, tests/test_visualize.py;
the pixels are not OpenCV's):
  - anti-aliased lines follow the coverage rule of geotrax_amd/draw.py (a linear ramp over the distance to the segment, round
    caps), not OpenCV's Gaussian-weighted LINE_AA;
  - circles follow that module's integer ring rule, not OpenCV's midpoint circle;
  - the font is Pillow's default FreeType font at a text height of round(22 * line_width / 3) px, not Hershey simplex; text sizes,
    and with them the label boxes, differ by a few pixels;
  - cv2.perspectiveTransform is restated as float64 arithmetic on the float32 points and matrix, rounded to float32; a projected
    corner within rounding of an integer may truncate to the neighbouring pixel;
  - the container is Motion-JPEG in .avi, not determine_suffix_and_fourcc()'s choice.
"""
from __future__ import annotations

import argparse
import logging
import sys
from collections import defaultdict
from pathlib import Path

import numpy as np

from . import draw
from .draw import FILL, RING, SEGMENT, pack_bgr

VIZ_DEFAULTS = {                        # cfg -> visualization of the reference's default.yaml, for a config that does not carry the section
    "save": True, "show": False, "tail_length": 30, "line_width": 2, "viz_mode": 0, "heading_smoothing": 15, "heading_min_speed": 0.5,
    "edge_clip_margin": 3, "edge_clip_smoothing": 5, "plot_trajectories": False, "plot_delay": 30, "show_conf": False, "show_lanes": False,
    "show_class_names": False, "hide_labels": False, "hide_tracks": False, "hide_speed": False, "speed_unit": "km/h", "speed_deadzone": 1,
    "class_filter": [],
}


class VizColors:
    """utils/data_utils.py VizColors: the palette by class id, most distinct first; txt_color white."""
    HEX = ("1F77B4", "D62728", "FF7F0E", "006400", "9467BD", "8C564B", "17BECF", "E377C2", "BCBD22", "7F7F7F",
           "AEC7E8", "FF9896", "FFBB78", "98DF8A", "C5B0D5", "C49C94", "9EDAE5", "F7B6D2", "DBDB8D", "C7C7C7")

    def __init__(self):
        self.palette = [tuple(int(c[k:k + 2], 16) for k in (0, 2, 4)) for c in self.HEX]
        self.n = len(self.palette)
        self.txt_color = (255, 255, 255)

    def __call__(self, i, bgr: bool = False) -> tuple:
        r, g, b = self.palette[int(i) % self.n]
        return (b, g, r) if bgr else (r, g, b)


# --------------------------------------------------------------------------------------------------------------- reading the results

def normalize_viz_modes(viz_mode, logger: logging.Logger) -> list:
    """One mode or several -> the ordered list without repeats (visualize.py:208-227)."""
    out = []
    for m in (list(viz_mode) if isinstance(viz_mode, (list, tuple)) else [viz_mode]):
        if m not in (0, 1, 2, 3, 4):
            logger.critical(f"Invalid visualization mode '{m}'. Valid modes are 0 (original), 1 (stabilized), 2 (reference), "
                            f"3 (rotated boxes on the original frame), 4 (rotated boxes on the stabilized frame).")
            sys.exit(1)
        if m not in out:
            out.append(m)
    if not out:
        logger.critical("No visualization mode specified.")
        sys.exit(1)
    return out


def _renumber(df):
    df.columns = list(range(df.shape[1]))
    return df


def read_tracks(tracks_txt_filepath: Path, class_names: dict, args, logger: logging.Logger, frame_wh=None) -> tuple:
    """visualize.py:342-385. Layouts of 7 / 10 / 11 / 12 / 14 / 15 columns: a trailing is-interpolated column (11, 15) is set aside
    and comes back as the last column; dimension columns (from column 12) go; modes > 0 keep the stabilized box (columns 6-9) in
    place of the raw one (2-5), mode 0 the raw one. Returns (tracks, tracks_plotting)."""
    import pandas as pd

    from .georef_stage import detect_delimiter

    tracks = pd.read_csv(tracks_txt_filepath, header=None, delimiter=detect_delimiter(tracks_txt_filepath))
    if args.viz_mode in (3, 4):
        return read_tracks_oriented(tracks, tracks_txt_filepath, class_names, args, logger, frame_wh)
    interp = None
    if tracks.shape[1] in (11, 15):
        interp = tracks.iloc[:, -1].values
        tracks = tracks.iloc[:, :-1]
    if tracks.shape[1] == 10 or tracks.shape[1] >= 14:
        tracks = tracks.iloc[:, :12]
    if getattr(args, "plot_trajectories", False) and tracks.shape[1] < 11:
        logger.error(f"No stabilized bounding boxes found in: '{tracks_txt_filepath}'. Disable the trajectory plotting option or re-run the extraction stage.")
        sys.exit(1)
    plotting = _renumber(tracks[[0, 6, 7, 10]].copy()) if tracks.shape[1] >= 11 else None
    if args.viz_mode > 0:
        if tracks.shape[1] < 11:
            logger.error(f"No stabilized bounding boxes found in: '{tracks_txt_filepath}'. Choose a different visualization mode or re-run the extraction stage.")
            sys.exit(1)
        tracks = tracks.drop(tracks.columns[2:6], axis=1)
    elif tracks.shape[1] > 10:
        tracks = tracks.drop(tracks.columns[6:10], axis=1)
    elif tracks.shape[1] < 7:
        logger.error(f"No valid tracking results found in: '{tracks_txt_filepath}'.")
        sys.exit(1)
    tracks = _renumber(tracks.copy())
    if interp is not None:
        tracks[tracks.shape[1]] = interp
    _need_class_names(class_names, tracks[6].max(), logger)
    return tracks, plotting


def _need_class_names(class_names: dict, top, logger) -> None:
    if len(class_names) < top + 1:
        logger.error(f"At least {top + 1} class names must be provided. Current class names defined for the used model are {class_names.values()}.")
        sys.exit(1)


def _estimate_fallback_dims(tracks) -> tuple:
    """Per vehicle, the 25th percentile of the longer and of the shorter raw box side (columns 4, 5) over its track, on every row
    of the vehicle (visualize.py:388-403): the size used where the extract stage's estimate is NaN."""
    import pandas as pd

    sides = pd.DataFrame({"l": tracks[[4, 5]].max(axis=1), "w": tracks[[4, 5]].min(axis=1), "id": tracks[1]})
    q = sides.groupby("id")[["l", "w"]].transform(lambda v: np.percentile(v, 25))
    return q["l"], q["w"]


def compute_headings(tracks, smoothing: float, min_speed: float, logger: logging.Logger):
    """Heading per row in radians, image coordinates (visualize.py:490-523): per track, in frame order, the gradient of the
    stabilized centre (columns 6, 7) smoothed by a Gaussian of sigma `smoothing`; arctan2 where the smoothed speed reaches
    `min_speed`, the nearest reliable heading held elsewhere (forward, then backward); a track that never moves, or of one row, points
    along its longer raw box side (pi / 2 when the median height exceeds the median width, else 0)."""
    import pandas as pd
    from scipy.ndimage import gaussian_filter1d

    out = pd.Series(np.nan, index=tracks.index, dtype=float)
    sigma = max(float(smoothing), 1e-6)
    for _, g in tracks.groupby(1):
        g = g.sort_values(0)
        by_aspect = np.pi / 2 if np.median(g[5]) > np.median(g[4]) else 0.0
        if len(g) < 2:
            out.loc[g.index] = by_aspect
            continue
        dx = gaussian_filter1d(np.gradient(g[6].to_numpy(dtype=float)), sigma, mode="reflect")
        dy = gaussian_filter1d(np.gradient(g[7].to_numpy(dtype=float)), sigma, mode="reflect")
        moving = np.hypot(dx, dy) >= min_speed
        if not moving.any():
            out.loc[g.index] = by_aspect
            continue
        theta = pd.Series(np.where(moving, np.arctan2(dy, dx), np.nan)).ffill().bfill().to_numpy()
        out.loc[g.index] = theta
    return out


def _smooth_clip_dims(oriented, smoothing: float):
    """Columns 10 / 11 (the stabilized detection box's extents) smoothed per track, in frame order, by a Gaussian of sigma
    `smoothing` with reflected ends (visualize.py:526-542)."""
    from scipy.ndimage import gaussian_filter1d

    sigma = max(float(smoothing), 1e-6)
    out = oriented[[10, 11]].astype(float).copy()
    for _, g in oriented.groupby(1):
        g = g.sort_values(0)
        for col in (10, 11):
            out.loc[g.index, col] = gaussian_filter1d(g[col].to_numpy(dtype=float), sigma, mode="reflect")
    return out


def read_tracks_oriented(tracks, tracks_txt_filepath: Path, class_names: dict, args, logger: logging.Logger, frame_wh=None) -> tuple:
    """The rows of modes 3 / 4 (visualize.py:406-487): frame, id, stabilized centre x y, length, width, class, confidence, heading,
    dashed, clip width, clip height, on_border. Length / width are the extract stage's estimates (columns 12, 13) or, where NaN, the
    fallback of _estimate_fallback_dims; dashed = fallback or interpolated row; on_border = the raw box comes within
    edge_clip_margin of a frame edge (frame_wh = (w, h); None: no edge)."""
    import pandas as pd

    if tracks.shape[1] < 14:
        logger.error(f"Visualization mode 3 requires stabilized tracks with dimension estimates (14 columns) in: '{tracks_txt_filepath}'. "
                     f"Re-run the extraction stage with stabilization enabled.")
        sys.exit(1)
    plotting = _renumber(tracks[[0, 6, 7, 10]].copy())
    headings = compute_headings(tracks, args.heading_smoothing, args.heading_min_speed, logger)
    fallback = tracks[12].isna()
    interpolated = tracks[14].astype(bool) if tracks.shape[1] >= 15 else pd.Series(False, index=tracks.index)
    fb_l, fb_w = _estimate_fallback_dims(tracks)
    eps = getattr(args, "edge_clip_margin", 3)
    w_i, h_i = frame_wh if frame_wh is not None else (np.inf, np.inf)
    xc, yc, w, h = tracks[2], tracks[3], tracks[4], tracks[5]
    on_border = (xc - w / 2 <= eps) | (yc - h / 2 <= eps) | (xc + w / 2 >= w_i - 1 - eps) | (yc + h / 2 >= h_i - 1 - eps)
    oriented = pd.DataFrame({
        0: tracks[0], 1: tracks[1], 2: tracks[6], 3: tracks[7],
        4: tracks[12].where(~fallback, fb_l), 5: tracks[13].where(~fallback, fb_w),
        6: tracks[10], 7: tracks[11], 8: headings, 9: (fallback | interpolated).astype(bool),
        10: tracks[8], 11: tracks[9], 12: on_border.astype(bool),
    })
    oriented[[10, 11]] = _smooth_clip_dims(oriented, getattr(args, "edge_clip_smoothing", 5))
    _need_class_names(class_names, oriented[6].max(), logger)
    return oriented, plotting


def read_georeferenced_results(tracks_csv_filepath, tracks, logger: logging.Logger):
    """Frame_ID, Vehicle_ID, Vehicle_Speed, Lane_Number of the georeferenced csv (visualize.py:575-602). Without a Frame_Number
    column the frames are counted from the tracks' first frame over the sorted distinct Timestamp values."""
    import pandas as pd

    if tracks_csv_filepath is None:
        return None
    geo = pd.read_csv(tracks_csv_filepath)
    if "Frame_Number" in geo.columns:
        geo = geo.rename(columns={"Frame_Number": "Frame_ID"})
    elif "Timestamp" in geo.columns:
        first = int(tracks[0].min())
        frame_of = {ts: first + i for i, ts in enumerate(sorted(geo["Timestamp"].unique()))}
        geo["Frame_ID"] = geo["Timestamp"].map(frame_of)
        logger.warning(f"'Frame_Number' column missing from '{Path(tracks_csv_filepath).name}'. Frame IDs reconstructed from tracking results "
                       f"assuming no dropped frames. Re-run the georeference stage to regenerate the CSV with proper frame numbers.")
    else:
        logger.warning(f"Neither 'Frame_Number' nor 'Timestamp' column found in '{Path(tracks_csv_filepath).name}'. Speed/lane data cannot be displayed.")
        return None
    return geo[["Frame_ID", "Vehicle_ID", "Vehicle_Speed", "Lane_Number"]]


def group_by_frame(tracks, speed_lane_data):
    """process_frames' two lookups (visualize.py:241-249): rows by frame, and per frame the speed / lane rows by vehicle id."""
    by_frame = dict(tuple(tracks.groupby(0)))
    speed_lane = None
    if speed_lane_data is not None:
        speed_lane = {f: g.drop(columns=["Frame_ID"]).astype({"Vehicle_ID": int}).set_index("Vehicle_ID") for f, g in speed_lane_data.groupby("Frame_ID")}
    return by_frame, speed_lane, tracks.iloc[0:0]


# --------------------------------------------------------------------------------------------------------------- geometry

def _segment_axis_intersection(p0, p1, axis: int, bound: float):
    denom = p1[axis] - p0[axis]
    t = 0.0 if denom == 0 else (bound - p0[axis]) / denom
    return p0 + t * (p1 - p0)


def _clip_poly_to_rect(corners, xmin: float, ymin: float, xmax: float, ymax: float) -> np.ndarray:
    """Sutherland-Hodgman against x >= xmin, x <= xmax, y >= ymin, y <= ymax in that order (visualize.py:811-845); float64 inside,
    float32 [m][2] out, empty when nothing is left."""
    poly = [np.asarray(c, dtype=float) for c in corners]
    for axis, bound, sign in ((0, xmin, 1), (0, xmax, -1), (1, ymin, 1), (1, ymax, -1)):
        if not poly:
            break
        kept = []
        for i, cur in enumerate(poly):
            prv = poly[i - 1]
            cur_in, prv_in = sign * (cur[axis] - bound) >= 0, sign * (prv[axis] - bound) >= 0
            if cur_in != prv_in:
                kept.append(_segment_axis_intersection(prv, cur, axis, bound))
            if cur_in:
                kept.append(cur)
        poly = kept
    return np.array(poly, dtype=np.float32) if poly else np.empty((0, 2), dtype=np.float32)


def _clip_segment_to_rect(p0, p1, xmin: float, ymin: float, xmax: float, ymax: float):
    """Liang-Barsky (visualize.py:855-879): the clipped end points, or None when the segment misses the rectangle."""
    p0 = np.asarray(p0, dtype=float)
    d = np.asarray(p1, dtype=float) - p0
    t0, t1 = 0.0, 1.0
    for p, q in ((-d[0], p0[0] - xmin), (d[0], xmax - p0[0]), (-d[1], p0[1] - ymin), (d[1], ymax - p0[1])):
        if p == 0:
            if q < 0:
                return None
            continue
        t = q / p
        if p < 0:
            t0 = max(t0, t)
        else:
            t1 = min(t1, t)
        if t0 > t1:
            return None
    return p0 + t0 * d, p0 + t1 * d


def perspective_transform(points: np.ndarray, M: np.ndarray) -> np.ndarray:
    """cv2.perspectiveTransform on float32 points [n][2] with a float32 3x3 matrix, restated: in float64, w = x m6 + y m7 + m8;
    |w| > FLT_EPSILON -> ((x m0 + y m1 + m2) / w, (x m3 + y m4 + m5) / w) with the division as a multiplication by 1 / w, else
    (0, 0); rounded to float32."""
    p = np.asarray(points, np.float32).reshape(-1, 2).astype(np.float64)
    m = np.asarray(M, np.float32).reshape(9).astype(np.float64)
    x, y = p[:, 0], p[:, 1]
    w = x * m[6] + y * m[7] + m[8]
    ok = np.abs(w) > np.finfo(np.float32).eps
    inv = np.where(ok, 1.0 / np.where(ok, w, 1.0), 0.0)
    return np.stack([(x * m[0] + y * m[1] + m[2]) * inv, (x * m[3] + y * m[4] + m[5]) * inv], axis=1).astype(np.float32)


# --------------------------------------------------------------------------------------------------------------- the primitive list

class _List:
    """The frame's primitives in drawing order; `texts` keeps every label as (index of its first glyph in the list, string, origin)."""

    def __init__(self, layout_text=None):
        self.prims: list[tuple] = []
        self.texts: list[tuple] = []
        self.layout_text = layout_text

    def segment(self, a, b, color, t):
        self.prims.append((SEGMENT, int(a[0]), int(a[1]), int(b[0]), int(b[1]), int(t), 0, pack_bgr(color)))

    def outline(self, x1, y1, x2, y2, color, t):
        for a, b in (((x1, y1), (x2, y1)), ((x2, y1), (x2, y2)), ((x2, y2), (x1, y2)), ((x1, y2), (x1, y1))):
            self.segment(a, b, color, t)

    def polyline(self, corners, color, t):
        n = len(corners)
        for i in range(n):
            self.segment(corners[i], corners[(i + 1) % n], color, t)

    def fill(self, a, b, color):
        self.prims.append((FILL, int(a[0]), int(a[1]), int(b[0]), int(b[1]), 0, 0, pack_bgr(color)))

    def ring(self, c, r, color, t):
        self.prims.append((RING, int(c[0]), int(c[1]), int(r), 0, int(t), 0, pack_bgr(color)))

    def text(self, label, origin, color):
        self.texts.append((len(self.prims), label, (int(origin[0]), int(origin[1]))))
        if self.layout_text is not None:
            self.prims.extend(self.layout_text(label, int(origin[0]), int(origin[1]), color))


def _draw_dashed_poly(out: _List, corners: np.ndarray, color, thickness: int, dash: int = 10, gap: int = 5) -> None:
    """The closed polygon as dashes (visualize.py:787-808): along every edge of at least one pixel, a dash from t to
    min(t + dash, length) for t = 0, dash + gap, ..., its end points truncated to integers."""
    n = len(corners)
    for i in range(n):
        p1, p2 = corners[i].astype(float), corners[(i + 1) % n].astype(float)
        dist = float(np.hypot(*(p2 - p1)))
        if dist < 1:
            continue
        direction = (p2 - p1) / dist
        t = 0.0
        while t < dist:
            a = (p1 + direction * t).astype(np.int32)
            b = (p1 + direction * min(t + dash, dist)).astype(np.int32)
            out.segment(a, b, color, thickness)
            t += dash + gap


def draw_oriented_box(out: _List, cx, cy, length, width, heading, Hinv, color, line_width, is_fallback=False, clip_w=None, clip_h=None,
                      on_border=False) -> tuple:
    """The rotated box of modes 3 / 4 and its heading tick (visualize.py:882-940); returns the projected centre. Built in stabilized
    space in float32 -- corners front-left, front-right, rear-right, rear-left --, clipped there to the detection's footprint when
    the vehicle touches a frame edge (the unclipped box stays if fewer than 3 corners remain), then projected through Hinv and
    truncated to integers."""
    if heading is None or np.isnan(heading):
        ux, uy = 1.0, 0.0
    else:
        ux, uy = np.cos(heading), np.sin(heading)
    vx, vy = -uy, ux
    hl, hw = length / 2.0, width / 2.0
    corners = np.array([[cx + hl * ux - hw * vx, cy + hl * uy - hw * vy], [cx + hl * ux + hw * vx, cy + hl * uy + hw * vy],
                        [cx - hl * ux + hw * vx, cy - hl * uy + hw * vy], [cx - hl * ux - hw * vx, cy - hl * uy - hw * vy]], dtype=np.float32)
    front = np.array([cx + hl * ux, cy + hl * uy], dtype=np.float32)
    center = np.array([cx, cy], dtype=np.float32)
    tick = (center, front)
    if on_border and clip_w is not None and clip_h is not None:
        xmin, ymin, xmax, ymax = cx - clip_w / 2.0, cy - clip_h / 2.0, cx + clip_w / 2.0, cy + clip_h / 2.0
        clipped = _clip_poly_to_rect(corners, xmin, ymin, xmax, ymax)
        if len(clipped) >= 3:
            corners = clipped
        tick = _clip_segment_to_rect(center, front, xmin, ymin, xmax, ymax)
    corners_proj = perspective_transform(corners, Hinv).astype(np.int32)
    center_proj = perspective_transform(center, Hinv).reshape(2).astype(np.int32)
    if is_fallback:
        _draw_dashed_poly(out, corners_proj, color, line_width)
    else:
        out.polyline(corners_proj, color, line_width)
    if tick is not None:
        tp = perspective_transform(np.array(tick, dtype=np.float32), Hinv).astype(np.int32)
        out.segment(tp[0], tp[1], color, line_width)
    return int(center_proj[0]), int(center_proj[1])


def build_primitives(frame_num: int, tracks_frame, track_history: dict, class_names: dict, speed_lane_frame, viz_config: dict, args,
                     logger: logging.Logger, text_size, Hinv=None, layout_text=None) -> tuple:
    """annotate_frame (visualize.py:662-784) up to the drawing: the frame's primitive list, and its labels. `track_history` is the
    tails' state and lives across frames. text_size(label) -> (w, h) stands in for cv2.getTextSize; layout_text(label, x, y, color)
    -> GLYPH records for cv2.putText (None: the labels are only listed). Returns (prims, texts)."""
    import pandas as pd

    tail_length, line_width = viz_config["tail_length"], viz_config["line_width"]
    colors = VizColors()
    out = _List(layout_text)
    if tracks_frame.empty:
        logger.warning(f"No detection results for frame {frame_num:05d}")
        return out.prims, out.texts
    oriented = args.viz_mode in (3, 4)
    n = len(tracks_frame)
    col = lambda k: tracks_frame.iloc[:, k].values                   # noqa: E731
    ids, classes = col(1), col(6)
    Xc, Yc, W, H = tracks_frame.iloc[:, 2:6].values.T
    none, false = [None] * n, [False] * n
    if oriented:
        scores, headings, dashed, clip_ws, clip_hs, borders, interp = col(7), col(8), col(9), col(10), col(11), col(12), false
    else:
        scores = col(7) if tracks_frame.shape[1] >= 8 else [""] * n
        headings, dashed, clip_ws, clip_hs, borders = none, false, none, none, false
        k = {9: 8, 11: 10}.get(tracks_frame.shape[1])               # the is-interpolated column of the stabilized / raw layouts
        interp = col(k).astype(bool) if k is not None else false

    for track_id, xc, yc, w, h, c, s, heading, is_fb, clip_w, clip_h, on_border, is_interp in zip(
            ids, Xc, Yc, W, H, classes, scores, headings, dashed, clip_ws, clip_hs, borders, interp):
        if args.class_filter and c in args.class_filter:
            continue
        speed = lane = None
        if speed_lane_frame is not None and int(track_id) in speed_lane_frame.index:
            row = speed_lane_frame.loc[int(track_id)]
            if isinstance(row, pd.DataFrame):
                row = row.iloc[0]
            speed, lane = row["Vehicle_Speed"], row["Lane_Number"]
            if np.isnan(speed):
                speed = None
            else:
                speed = int(speed * 0.621371) if args.speed_unit == "mi/h" else int(speed)
                if speed <= args.speed_deadzone:
                    speed = 0
            lane = int(lane) if lane not in ("", None) and pd.notna(lane) else None

        color = colors(c, True)
        if oriented:
            x1, y1 = draw_oriented_box(out, xc, yc, w, h, heading, Hinv, color, line_width, is_fb, clip_w, clip_h, on_border)
            tail_x, tail_y = x1, y1
        else:
            x1, y1, x2, y2 = int(xc - w / 2), int(yc - h / 2), int(xc + w / 2), int(yc + h / 2)
            if is_interp:
                _draw_dashed_poly(out, np.array([[x1, y1], [x2, y1], [x2, y2], [x1, y2]], dtype=np.int32), color, line_width)
            else:
                out.outline(x1, y1, x2, y2, color, line_width)
            tail_x, tail_y = xc, yc

        if not args.hide_labels:
            parts = []
            if track_id not in {None, -1}:
                parts.append(f"id:{track_id}")
            if args.show_class_names:
                parts.append(class_names[c])
            if not args.hide_speed and speed is not None:
                parts.append(f"{speed} {args.speed_unit}")
            if args.show_lanes and lane is not None:
                parts.append(f"L{lane}")
            if args.show_conf and s != "":
                parts.append(f"{s:.2f}")
            label = " ".join(parts)
            tw, th = text_size(label)
            outside = y1 - th >= 3
            out.fill((x1, y1), (x1 + tw, y1 - th - 3 if outside else y1 + th + 3), color)
            out.text(label, (x1, y1 - 2 if outside else y1 + th + 2), colors.txt_color)

        if not args.hide_tracks:
            track = track_history[track_id]
            track.append((float(tail_x), float(tail_y)))
            if len(track) > tail_length:
                track.pop(0)
            points = np.array(track, dtype=np.int32).reshape(-1, 2)
            for i, p in enumerate(points):
                out.ring(p, int(1 + 8 * (i + 1) / len(points)), color, line_width)
    return out.prims, out.texts


# --------------------------------------------------------------------------------------------------------------- the stage

def _frame_homography(viz_mode: int, transforms, frame_num: int):
    if viz_mode == 3:
        M = transforms.get(frame_num) if transforms is not None else None
        return (np.linalg.inv(M) if M is not None else np.eye(3)).astype(np.float32)
    return np.eye(3, dtype=np.float32) if viz_mode == 4 else None


def visualize_mode(args, viz_mode: int, class_names: dict, viz_config: dict, out_cfg: dict, logger: logging.Logger, ctx=None, quality: int = 90,
                   out_path=None, stats: dict | None = None) -> tuple:
    """One mode's clip. Returns (path, frames written). `stats`, if given, receives per-frame lists of the drawing launch's
    milliseconds and the primitive counts (tools/visualize_time.py); asking for them waits for every frame's launch."""
    import ctypes as C

    from . import _lib
    from .frames import open_source
    from .georef_stage import DEFAULT_FPS, build_result_path
    from .stabilized_video import _open_feeder, load_transforms, visualized_path
    from .video_writer import MjpegWriter

    source = Path(args.source)
    args.viz_mode = viz_mode
    tracks_path = build_result_path(source, "processed", out_cfg)
    if not tracks_path.is_file():
        raise FileNotFoundError(f"Tracking results file '{tracks_path}' not found. Run the extraction stage first.")
    transforms = None
    if viz_mode in (1, 3, 4):
        tpath = build_result_path(source, "video_transformations", out_cfg)
        if not tpath.is_file():
            raise FileNotFoundError(f"Transformation file '{tpath}' not found. Enable stabilization and run the extraction stage first.")
        transforms = load_transforms(tpath)
    csv_path = build_result_path(source, "georeferenced", out_cfg)
    if not csv_path.is_file():
        logger.warning(f"Georeferenced file '{csv_path}' not found. Speed estimates will not be visualized.")
        csv_path = None

    ctx = ctx or _lib.default_context()
    reader = open_source(source)
    fd = drawer = writer = None
    bufs: list[int] = []
    try:
        h, w = reader.frame_hw
        tracks, _ = read_tracks(tracks_path, class_names, args, logger, frame_wh=(w, h))
        by_frame, speed_lane, no_rows = group_by_frame(tracks, read_georeferenced_results(csv_path, tracks, logger))
        atlas = None if args.hide_labels else draw.GlyphAtlas(viz_config["line_width"])
        text_size = atlas.text_size if atlas is not None else None
        layout = atlas.layout if atlas is not None else None
        first = max(int(args.cut_frame_left or 0), 0)
        stop = reader.frame_count if args.cut_frame_right is None else min(reader.frame_count, max(int(args.cut_frame_right), first))
        fps = getattr(reader, "fps", 0.0) or DEFAULT_FPS
        out = Path(out_path) if out_path else visualized_path(source, out_cfg, viz_mode)
        out.parent.mkdir(parents=True, exist_ok=True)
        nbytes = h * w * 3
        batch, n_written, capacity = 2, 0, 16384
        writer = MjpegWriter(out, fps, (w, h), quality=quality, ctx=ctx, entropy=getattr(args, "entropy", None) or "host",
                             restart_interval=getattr(args, "restart_interval", None) or 0)
        keep = writer.ring // batch + 2                    # as geotrax_amd.stabilized_video: a frame stays until the writer's ring has come round
        ring = [ctx.dev_alloc(nbytes) for _ in range(writer.ring)] if viz_mode in (1, 2, 4) else []
        bufs.extend(ring)
        ref = None
        if viz_mode == 2:
            ref = ctx.dev_alloc(nbytes)
            bufs.append(ref)
        drawer = draw.Drawer(ctx, (h, w), capacity, None if atlas is None else atlas.data)
        track_history = defaultdict(list)
        fd = _open_feeder(reader, first, stop, batch, keep + 3, ctx)
        for b in fd.batches(keep):
            b.wait_on(ctx)
            for k in range(b.n):
                frame_num = first + n_written
                frame = b.ptr + k * nbytes
                if viz_mode in (1, 4) and frame_num in transforms:
                    dst = ring[n_written % writer.ring]
                    Hm = np.ascontiguousarray(transforms[frame_num], dtype=np.float64).reshape(9)
                    _lib.check(ctx.lib.gtx_warp_frame_dev(ctx.handle, C.c_void_p(frame), h, w, _lib.ptr(Hm), C.c_void_p(dst)))
                    frame = dst
                elif viz_mode == 2:
                    if frame_num == first:
                        ctx.dev_copy(ref, frame, nbytes)
                    dst = ring[n_written % writer.ring]
                    ctx.dev_copy(dst, ref, nbytes)
                    frame = dst
                prims, _ = build_primitives(frame_num, by_frame.get(frame_num, no_rows), track_history, class_names,
                                            speed_lane.get(frame_num) if speed_lane is not None else None, viz_config, args, logger,
                                            text_size, _frame_homography(viz_mode, transforms, frame_num), layout)
                if len(prims) > capacity:                  # a busier frame than any before: a larger drawer (closing one waits for the stream)
                    drawer.close()
                    capacity = max(2 * capacity, len(prims))
                    drawer = draw.Drawer(ctx, (h, w), capacity, None if atlas is None else atlas.data)
                drawer.draw(frame, prims)
                if stats is not None:
                    stats.setdefault("draw_ms", []).append(drawer.last_ms())
                    stats.setdefault("prims", []).append(len(prims))
                writer.write_dev(frame)
                n_written += 1
        writer.release()
        logger.info(f"'{out}': {n_written} frames at mode {viz_mode}")
        return out, n_written
    finally:
        if writer is not None:
            writer.release()
        if drawer is not None:
            drawer.close()
        for p in bufs:
            ctx.dev_free(p)
        if fd is not None:
            fd.close()
        reader.release()


def add_visualization_args(group, include_frame_range: bool = True) -> None:
    """The flags of `geotrax visualize` (visualize.py:986-1041): every default is None and is backfilled from the config."""
    B = argparse.BooleanOptionalAction
    group.add_argument("--save", "-s", action=B, default=None, help="Save the annotated output video to file.")
    group.add_argument("--show", "-sh", action=B, default=None, help="(not built: there is no window)")
    group.add_argument("--viz-mode", "-vm", type=int, nargs="+", default=None, choices=[0, 1, 2, 3, 4], metavar="MODE",
                       help="0=original, 1=stabilized, 2=reference frame, 3=rotated boxes on the original frame, 4=rotated boxes on the stabilized frame; several values render one video per mode.")
    group.add_argument("--plot-trajectories", "-pt", action=B, default=None, help="(not built: needs a whole-frame alpha blend)")
    group.add_argument("--plot-delay", "-pd", type=int, default=None)
    group.add_argument("--show-conf", "-sc", action=B, default=None, help="Include detection confidence in the labels.")
    group.add_argument("--show-lanes", "-sl", action=B, default=None, help="Include the lane ID in the labels.")
    group.add_argument("--show-class-names", "-scn", action=B, default=None, help="Include the class name in the labels.")
    group.add_argument("--hide-labels", "-hl", action=B, default=None, help="Draw no labels.")
    group.add_argument("--hide-tracks", "-ht", action=B, default=None, help="Draw no track tails.")
    group.add_argument("--hide-speed", "-hs", action=B, default=None, help="Leave the speed out of the labels.")
    group.add_argument("--speed-unit", "-su", type=str, default=None, choices=["km/h", "mi/h"])
    group.add_argument("--speed-deadzone", "-sdz", type=float, default=None, help="Speeds at or below this value are shown as 0.")
    group.add_argument("--class-filter", "-cf", type=int, nargs="+", default=None, help="Class IDs to leave out.")
    group.add_argument("--tail-length", "-tl", type=int, default=None, help="Past positions drawn as the tail [frames].")
    group.add_argument("--line-width", "-lw", type=int, default=None, help="Stroke width of boxes and tails [px].")
    group.add_argument("--heading-smoothing", "-hsm", type=int, default=None, help="(modes 3, 4) Gaussian window of the heading [frames].")
    group.add_argument("--heading-min-speed", "-hms", type=float, default=None, help="(modes 3, 4) Smoothed speed below which the heading is held [px/frame].")
    group.add_argument("--edge-clip-margin", "-ecm", type=float, default=None, help="(modes 3, 4) Distance to a frame edge that counts as touching it [px].")
    group.add_argument("--edge-clip-smoothing", "-ecs", type=float, default=None, help="(modes 3, 4) Gaussian window of the clip rectangle [frames].")
    if include_frame_range:
        group.add_argument("--cut-frame-left", "-cfl", type=int, default=None, help="Skip the first N frames.")
        group.add_argument("--cut-frame-right", "-cfr", type=int, default=None, help="Stop when this frame is reached.")


def visualize_results(args: argparse.Namespace, logger: logging.Logger) -> int:
    """visualize.py:131-194: config backfill, then one clip per mode."""
    from . import _lib
    from .config_utils import backfill_args_from_config, load_config, resolve_class_names

    config = full = load_config(getattr(args, "cfg", None), logger)
    viz = {**VIZ_DEFAULTS, **(config.get("visualization") or {})}
    proc = config.get("processing") or {}
    out_raw = config.get("output") or {}
    backfill_args_from_config(args, {**{k: viz[k] for k in VIZ_DEFAULTS}, "cut_frame_left": proc.get("cut_frame_left", 0),
                                     "cut_frame_right": proc.get("cut_frame_right"), "output_folder": out_raw.get("folder", "results")})
    out_cfg = {**out_raw, "folder": args.output_folder}
    if args.show:
        logger.error("--show is not part of this build: there is no window. Run with --no-show; the clip is written with --save.")
        return 1
    if args.plot_trajectories:
        logger.error("--plot-trajectories is not part of this build: the overlay needs a whole-frame alpha blend, which is another kernel.")
        return 1
    if not args.save:
        logger.warning("--save is off and there is no window: nothing to do.")
        return 0
    class_names, _ = resolve_class_names(None, getattr(args, "class_names", None), (full.get("extraction") or {}).get("class_rename"),
                                         (full.get("ultralytics") or {}).get("classes"), logger)
    viz_config = dict(viz, tail_length=args.tail_length, line_width=args.line_width)
    modes = normalize_viz_modes(args.viz_mode, logger)
    if not Path(args.source).is_file():
        logger.critical(f"Video file '{args.source}' not found.")
        return 1
    try:
        for m in modes:
            visualize_mode(args, m, class_names, viz_config, out_cfg, logger, quality=args.quality)
    except (OSError, ValueError, RuntimeError, _lib.GtxError) as e:
        logger.error(f"An error occurred: {e}")
        return 1
    finally:
        args.viz_mode = modes
    return 0


def main(argv=None) -> int:
    from .extract import add_common_args, setup_logger
    from .video_writer import check_restart_interval

    ap = argparse.ArgumentParser(prog="python -m geotrax_amd.visualize", description="Tracking results visualization")
    ap.add_argument("source", type=Path, help="Path to the input video file.")
    opt = ap.add_argument_group("Optional arguments")
    add_common_args(opt)
    opt.add_argument("--class-names", "-cn", nargs="+", default=None, metavar="ID=NAME|FILE", help="Class-id -> name mapping.")
    opt.add_argument("--quality", type=int, default=90, help="JPEG quality of the output, 1..100")
    opt.add_argument("--entropy", choices=["host", "gpu"], default="host", help="Where the output's pictures are Huffman-coded: host threads, or the GPU.")
    opt.add_argument("--restart-interval", type=int, default=0, metavar="N",
                     help="A restart marker every N MCUs in the output (0: none), so that it is read back one GPU lane per interval; needs --entropy host.")
    add_visualization_args(ap.add_argument_group("Visualization arguments"))
    args = ap.parse_args(argv)
    check_restart_interval(args.entropy, args.restart_interval)   # ValueError: the GPU coder and restart markers do not go together
    logger = setup_logger(__name__, getattr(args, "verbose", False), getattr(args, "log_path", None))
    return visualize_results(args, logger)


if __name__ == "__main__":
    sys.exit(main())
