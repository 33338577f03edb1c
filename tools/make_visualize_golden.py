"""Writes the fixture tests/golden/visualize.json.gz: what the reference's own visualize functions return, and every drawing call its
annotate_frame makes, on a small seeded table -- as data. Run once, by hand, where a checkout of the reference exists:

    python tools/make_visualize_golden.py --reference <path to the geo-trax checkout>

The reference's geotrax/visualize.py is imported with `cv2`, `stabilo` and `ultralytics` replaced by stand-ins (none of them is
needed by the functions called here). The cv2 stand-in draws nothing: it records the arguments of every rectangle / line /
polylines / circle / putText call, answers getTextSize by a fixed rule ((7 * len(text), 14), baseline 5) and answers
perspectiveTransform with the restatement written out below (float64 arithmetic on float32 input, rounded to float32).
tests/test_visualize.py holds geotrax_amd.visualize to this bundle: the input files as text, and the recorded results. No program text.

The table: 12 frames, 6 vehicles, the 15-column layout of the extract stage (frame, id, raw box, stabilized box, class, confidence,
length, width, is_interpolated), with interpolated rows, NaN dimensions, a box touching the frame's edge, a box at the top of the
frame (its label flips inside), a vehicle of a filtered class, a vehicle at rest (speed inside the deadzone) and tails longer than
tail_length; the other layouts (7 / 10 / 11 / 12 / 14 columns) are cut from it.
"""
from __future__ import annotations

import argparse
import json
import logging
import sys
import types
from collections import defaultdict
from pathlib import Path

import numpy as np

BUNDLE = Path(__file__).resolve().parent.parent / "tests" / "golden" / "visualize.json.gz"
LAYOUTS = {15: list(range(15)), 14: list(range(14)), 12: list(range(12)), 11: [0, 1, 2, 3, 4, 5, 10, 11, 12, 13, 14], 10: [0, 1, 2, 3, 4, 5, 10, 11, 12, 13],
           7: [0, 1, 2, 3, 4, 5, 10]}
FRAME_W, FRAME_H = 256, 144
N_FRAMES = 12
TEXT_W, TEXT_H = 7, 14


def perspective_transform(src, M):
    p = np.asarray(src, np.float32).reshape(-1, 2).astype(np.float64)
    m = np.asarray(M, np.float32).reshape(9).astype(np.float64)
    x, y = p[:, 0], p[:, 1]
    w = x * m[6] + y * m[7] + m[8]
    ok = np.abs(w) > np.finfo(np.float32).eps
    inv = np.where(ok, 1.0 / np.where(ok, w, 1.0), 0.0)
    out = np.stack([(x * m[0] + y * m[1] + m[2]) * inv, (x * m[3] + y * m[4] + m[5]) * inv], axis=1).astype(np.float32)
    return out.reshape(np.asarray(src).shape)


def _ints(v):
    return [int(x) for x in np.asarray(v).reshape(-1)]


class RecordingCv2(types.ModuleType):
    LINE_AA = 16
    FONT_HERSHEY_SIMPLEX = 0
    VideoCapture = VideoWriter = error = object                     # named in annotations only

    def __init__(self):
        super().__init__("cv2")
        self.calls = []

    def rectangle(self, img, pt1, pt2, color, thickness=1, lineType=8):
        self.calls.append(["rectangle", _ints(pt1), _ints(pt2), _ints(color), int(thickness)])

    def line(self, img, pt1, pt2, color, thickness=1, lineType=8):
        self.calls.append(["line", _ints(pt1), _ints(pt2), _ints(color), int(thickness)])

    def polylines(self, img, pts, isClosed, color, thickness=1, lineType=8):
        assert isClosed and len(pts) == 1
        self.calls.append(["polylines", np.asarray(pts[0]).reshape(-1, 2).astype(int).tolist(), _ints(color), int(thickness)])

    def circle(self, img, center, radius, color, thickness=1):
        self.calls.append(["circle", _ints(center), int(radius), _ints(color), int(thickness)])

    def putText(self, img, text, org, fontFace, fontScale, color, thickness=1, lineType=8):
        self.calls.append(["putText", str(text), _ints(org), _ints(color)])

    def getTextSize(self, text, fontFace, fontScale, thickness):
        return (TEXT_W * len(text), TEXT_H), 5

    def perspectiveTransform(self, src, M):
        return perspective_transform(src, M)


def import_reference(root: Path):
    cv2 = RecordingCv2()
    sys.modules["cv2"] = cv2
    for name in ("stabilo", "ultralytics"):
        m = types.ModuleType(name)
        m.Stabilizer = m.YOLO = m.RTDETR = object
        sys.modules[name] = m
    sys.path.insert(0, str(root))
    import geotrax.visualize as ref

    ref.get_video_dimensions = lambda source: (FRAME_W, FRAME_H)
    return ref, cv2


def make_table(rng) -> np.ndarray:
    """[rows][15] float64, rows in frame order, vehicles in id order within a frame."""
    # id: (x0, y0, vx, vy, w, h, class, length, width)
    vehicles = {
        1: (40.0, 60.0, 6.5, 1.25, 30.0, 16.0, 0, 28.5, 13.25),       # drives to the right
        2: (200.0, 100.0, -5.0, -2.5, 34.0, 20.0, 1, np.nan, np.nan),  # no dimension estimate: the fallback, dashed in modes 3 / 4
        3: (120.0, 9.0, 0.75, 0.1, 24.0, 14.0, 0, 22.0, 11.0),         # at the top of the frame: its label goes inside the box
        4: (9.0, 120.0, 0.6, -3.5, 18.0, 30.0, 2, 27.0, 12.5),         # touches the left edge, drives up
        5: (150.0, 70.0, 0.0, 0.0, 26.0, 15.0, 0, 25.0, 12.0),         # at rest
        6: (90.0, 110.0, 3.0, 3.0, 20.0, 12.0, 3, 18.0, 9.0),          # class 3: filtered out
    }
    rows = []
    for f in range(N_FRAMES):
        for vid, (x0, y0, vx, vy, w, h, cls, ln, wd) in vehicles.items():
            if vid == 2 and f >= 10:
                continue                                             # leaves early
            if vid == 5 and f < 2:
                continue                                             # appears late
            jitter = rng.normal(0.0, 0.35, 4)
            xc, yc = x0 + vx * f + jitter[0], y0 + vy * f + jitter[1]
            bw, bh = w + jitter[2], h + jitter[3]
            sx, sy = xc + 1.5 * f * 0.1, yc - 0.75 * f * 0.1          # the stabilized box: the raw one moved with the camera
            interp = 1.0 if (vid == 1 and f in (4, 5)) or (vid == 4 and f == 7) else 0.0
            rows.append([f, vid, xc, yc, bw, bh, sx, sy, bw * 1.01, bh * 0.99, cls, 0.5 + 0.04 * vid + 0.01 * f, ln, wd, interp])
    return np.array(rows, dtype=np.float64)


def write_table(path: Path, t: np.ndarray, int_cols) -> None:
    with open(path, "w") as f:
        for r in t:
            f.write(",".join(("nan" if np.isnan(v) else str(int(v))) if k in int_cols and not np.isnan(v) else repr(float(v)) if not np.isnan(v) else "nan"
                             for k, v in enumerate(r)) + "\n")


def write_inputs(inputs: dict, folder: Path) -> None:
    """The bundle's three input files, and the ones cut from them column by column: the other track layouts, the csv without
    Frame_Number (tests/test_visualize.py does the same)."""
    for name, text in inputs.items():
        (folder / name).write_text(text)
    rows = [line.split(",") for line in inputs["tracks_15.txt"].splitlines()]
    for n, cols in LAYOUTS.items():
        (folder / f"tracks_{n}.txt").write_text("".join(",".join(r[c] for c in cols) + "\n" for r in rows))
    geo = [line.split(",") for line in inputs["clip.csv"].splitlines()]
    drop = geo[0].index("Frame_Number")
    (folder / "clip_timestamps_only.csv").write_text("".join(",".join(c for k, c in enumerate(r) if k != drop) + "\n" for r in geo))


def frame_as_lists(df):
    return {"values": [[None if (isinstance(v, float) and np.isnan(v)) else (bool(v) if isinstance(v, (bool, np.bool_)) else float(v)) for v in row]
                       for row in df.to_numpy(dtype=object).tolist()],
            "kinds": [str(df[c].dtype.kind) for c in df.columns]}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reference", type=Path, required=True, help="a checkout of the reference (the folder that holds geotrax/)")
    a = ap.parse_args()
    ref, cv2 = import_reference(a.reference)
    import pandas as pd

    import gzip
    import tempfile

    OUT = Path(tempfile.mkdtemp())
    log = logging.getLogger("golden")
    log.addHandler(logging.NullHandler())
    log.propagate = False
    rng = np.random.default_rng(20240607)
    full = make_table(rng)

    # ---- the inputs: every column layout, the transforms (frame 3 left out), the georeferenced csv in both forms
    layouts = LAYOUTS
    write_table(OUT / "tracks_15.txt", full, {0, 1, 10, 14})
    Hs = {i: np.array([[1 + 0.004 * i, 0.002 * i, 1.5 * i], [-0.003 * i, 1 - 0.002 * i, -0.75 * i], [1e-6 * i, -2e-6 * i, 1.0]]) for i in range(N_FRAMES) if i != 3}
    np.savetxt(OUT / "clip_vid_transf.txt", np.array([[i, *H.ravel()] for i, H in Hs.items()]), fmt="%.16g", delimiter=",")
    geo_rows = []
    for r in full:
        f, vid = int(r[0]), int(r[1])
        if vid == 3 and f % 2:
            continue                                                 # rows without speed data
        speed = {1: 43.7 + 0.3 * f, 2: 61.2 - f, 3: 12.9, 4: 30.0 + f, 5: 0.8, 6: 20.0}[vid]
        if vid == 4 and f == 5:
            speed = np.nan
        lane = {1: 2, 2: 1, 3: np.nan, 4: 3, 5: 2, 6: 1}[vid]
        geo_rows.append({"Vehicle_ID": vid, "Timestamp": f"2022-10-04 10:00:{f * 0.04:06.3f}", "Frame_Number": f, "Vehicle_Speed": speed, "Lane_Number": lane})
    geo = pd.DataFrame(geo_rows)
    geo.to_csv(OUT / "clip.csv", index=False)
    inputs = {name: (OUT / name).read_text() for name in ("tracks_15.txt", "clip_vid_transf.txt", "clip.csv")}
    write_inputs(inputs, OUT)

    class_names = {0: "car", 1: "bus", 2: "truck", 3: "motorcycle"}
    base = dict(source=Path("clip.mp4"), plot_trajectories=False, heading_smoothing=3, heading_min_speed=0.5, edge_clip_margin=3, edge_clip_smoothing=2,
                class_filter=[3], show_class_names=True, show_lanes=True, show_conf=True, hide_labels=False, hide_tracks=False, hide_speed=False,
                speed_unit="km/h", speed_deadzone=1)
    viz_config = {"tail_length": 5, "line_width": 2}
    golden = {"frame_wh": [FRAME_W, FRAME_H], "text_size": [TEXT_W, TEXT_H], "class_names": class_names, "args": {k: (str(v) if isinstance(v, Path) else v) for k, v in base.items()},
              "viz_config": viz_config, "inputs": inputs, "read_tracks": {}, "runs": []}

    # ---- read_tracks over every layout and mode it accepts
    for n in layouts:
        for mode in range(5):
            args = argparse.Namespace(**base, viz_mode=mode)
            try:
                tracks, plotting = ref.read_tracks(OUT / f"tracks_{n}.txt", class_names, args, log)
            except SystemExit:
                golden["read_tracks"][f"{n}/{mode}"] = "exit"
                continue
            golden["read_tracks"][f"{n}/{mode}"] = {"tracks": frame_as_lists(tracks), "plotting": None if plotting is None else frame_as_lists(plotting)}

    # ---- the oriented layout's parts, on the raw 15-column table
    raw = pd.read_csv(OUT / "tracks_15.txt", header=None, delimiter=",")
    fb_l, fb_w = ref._estimate_fallback_dims(raw)
    golden["parts"] = {
        "compute_headings": [[float(s), float(m), [float(v) for v in ref.compute_headings(raw, s, m, log)]] for s, m in ((3, 0.5), (15, 0.5), (0, 2.0), (3, 50.0))],
        "fallback_dims": [[float(v) for v in fb_l], [float(v) for v in fb_w]],
    }
    oriented, _ = ref.read_tracks(OUT / "tracks_15.txt", class_names, argparse.Namespace(**base, viz_mode=3), log)
    golden["parts"]["smooth_clip_dims"] = [[float(s), ref._smooth_clip_dims(oriented, s).to_numpy(dtype=float).tolist()] for s in (0, 2, 5)]

    # ---- the clippers
    rng2 = np.random.default_rng(7)
    polys, segs = [], []
    for _ in range(40):
        c = rng2.uniform(-20, 120, (4, 2)).astype(np.float32)
        c = c[np.argsort(np.arctan2(c[:, 1] - c[:, 1].mean(), c[:, 0] - c[:, 0].mean()))]      # a convex-ish quad in angular order
        rect = sorted(rng2.uniform(0, 100, 2).tolist()) + sorted(rng2.uniform(0, 100, 2).tolist())
        rect = [rect[0], rect[2], rect[1], rect[3]]
        polys.append({"corners": c.astype(float).tolist(), "rect": rect, "out": ref._clip_poly_to_rect(c, *rect).astype(float).tolist()})
        p0, p1 = rng2.uniform(-20, 120, 2).astype(np.float32), rng2.uniform(-20, 120, 2).astype(np.float32)
        if len(segs) % 5 == 0:
            p1[0] = p0[0]                                            # parallel to an edge
        r = ref._clip_segment_to_rect(p0, p1, *rect)
        segs.append({"p0": p0.astype(float).tolist(), "p1": p1.astype(float).tolist(), "rect": rect, "out": None if r is None else [r[0].tolist(), r[1].tolist()]})
    golden["clip_poly"], golden["clip_segment"] = polys, segs
    assert any(not p["out"] for p in polys) and any(s["out"] is None for s in segs)

    # ---- annotate_frame, frame after frame with its persistent tails: all five modes, and mode 0 in miles per hour and on the raw layouts
    runs = [(m, 15, {}) for m in range(5)] + [(0, 15, {"speed_unit": "mi/h", "speed_deadzone": 8}), (0, 11, {"show_conf": False}), (0, 7, {"class_filter": []}),
                                               (1, 12, {"hide_speed": True, "show_lanes": False}), (4, 14, {"hide_labels": True}), (3, 15, {"hide_tracks": True})]
    transforms = ref.read_transforms(OUT / "clip_vid_transf.txt", log)
    for mode, n, over in runs:
        args = argparse.Namespace(**{**base, **over}, viz_mode=mode)
        tracks, _ = ref.read_tracks(OUT / f"tracks_{n}.txt", class_names, args, log)
        speed_lane = ref.read_georeferenced_results(OUT / "clip.csv", tracks, log)
        by_frame = dict(tuple(tracks.groupby(0)))
        sl_by_frame = {f: g.drop(columns=["Frame_ID"]).astype({"Vehicle_ID": int}).set_index("Vehicle_ID") for f, g in speed_lane.groupby("Frame_ID")}
        history = defaultdict(list)
        frames = []
        img = np.zeros((FRAME_H, FRAME_W, 3), np.uint8)
        for f in range(N_FRAMES + 1):                                # one frame past the table: no rows
            Hinv = None
            if mode == 3:
                M = transforms.get(f)
                Hinv = (np.linalg.inv(M) if M is not None else np.eye(3)).astype(np.float32)
            if mode == 4:
                Hinv = np.eye(3, dtype=np.float32)
            cv2.calls = []
            ref.annotate_frame(img, f, by_frame.get(f, tracks.iloc[0:0]), history, class_names, sl_by_frame.get(f), viz_config, args, log, Hinv)
            frames.append(cv2.calls)
        golden["runs"].append({"mode": mode, "layout": n, "args": over, "frames": frames})
        kinds = {c[0] for fr in frames for c in fr}
        print(f"mode {mode} layout {n} {over}: {sum(len(fr) for fr in frames)} calls, {sorted(kinds)}")

    # the timestamp fallback of read_georeferenced_results
    tracks0, _ = ref.read_tracks(OUT / "tracks_15.txt", class_names, argparse.Namespace(**base, viz_mode=0), log)
    golden["georef_timestamps"] = frame_as_lists(ref.read_georeferenced_results(OUT / "clip_timestamps_only.csv", tracks0, log))
    golden["georef_frames"] = frame_as_lists(ref.read_georeferenced_results(OUT / "clip.csv", tracks0, log))
    with open(BUNDLE, "wb") as f, gzip.GzipFile(fileobj=f, mode="wb", mtime=0) as z:
        z.write(json.dumps(golden, separators=(",", ":")).encode())
    print(f"{BUNDLE}: {BUNDLE.stat().st_size / 1024:.0f} KiB")
    return 0


if __name__ == "__main__":
    sys.exit(main())
