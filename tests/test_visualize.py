"""The visualize stage's host logic (geotrax_amd/visualize.py) against the reference's own functions, as data: the fixture
tests/golden/visualize.json.gz (written by tools/make_visualize_golden.py) holds small input files as text, what the reference's read_tracks /
compute_headings / _smooth_clip_dims / clippers / read_georeferenced_results returned on them, and every drawing call its
annotate_frame made over 13 frames in all five modes. Each recorded call is mapped to primitives by the mapping of the module's
docstring, and build_primitives -- given the recording's text-size rule -- must give exactly that list: integer geometry, colours,
thicknesses, order and label strings equal. Float tables match to 1e-12 relative: the same arithmetic on the same numpy, not a
measured tolerance. CPU only."""
import argparse
import gzip
import json
import logging
from collections import defaultdict
from pathlib import Path

import numpy as np
import pytest

from geotrax_amd import visualize as V
from geotrax_amd.draw import FILL, RING, SEGMENT, pack_bgr

BUNDLE = Path(__file__).resolve().parent / "golden" / "visualize.json.gz"
LAYOUTS = {15: list(range(15)), 14: list(range(14)), 12: list(range(12)), 11: [0, 1, 2, 3, 4, 5, 10, 11, 12, 13, 14], 10: [0, 1, 2, 3, 4, 5, 10, 11, 12, 13],
           7: [0, 1, 2, 3, 4, 5, 10]}
LOG = logging.getLogger("test_visualize")
LOG.addHandler(logging.NullHandler())
LOG.propagate = False


def load_bundle():
    g = json.loads(gzip.decompress(BUNDLE.read_bytes()))
    g["class_names"] = {int(k): v for k, v in g["class_names"].items()}
    return g


def write_inputs(inputs: dict, folder: Path) -> Path:
    """The bundle's three input files, and the ones cut from them column by column, as the generator cut them: the other track
    layouts, and the csv without Frame_Number."""
    for name, text in inputs.items():
        (folder / name).write_text(text)
    rows = [line.split(",") for line in inputs["tracks_15.txt"].splitlines()]
    for n, cols in LAYOUTS.items():
        (folder / f"tracks_{n}.txt").write_text("".join(",".join(r[c] for c in cols) + "\n" for r in rows))
    geo = [line.split(",") for line in inputs["clip.csv"].splitlines()]
    drop = geo[0].index("Frame_Number")
    (folder / "clip_timestamps_only.csv").write_text("".join(",".join(c for k, c in enumerate(r) if k != drop) + "\n" for r in geo))
    return folder


@pytest.fixture(scope="module")
def gold(tmp_path_factory):
    g = load_bundle()
    g["dir"] = write_inputs(g["inputs"], tmp_path_factory.mktemp("visualize_inputs"))
    return g


def make_args(gold, mode, **over):
    a = dict(gold["args"])
    a.update(over)
    a["source"] = Path(a["source"])
    return argparse.Namespace(**a, viz_mode=mode)


def same_frame(df, want, where):
    assert df.shape == (len(want["values"]), len(want["kinds"])), where
    assert [str(df[c].dtype.kind) for c in df.columns] == want["kinds"], where
    assert list(df.columns) == list(range(df.shape[1])) or "Frame_ID" in df.columns, where
    got = df.to_numpy(dtype=object).tolist()
    for r, (grow, wrow) in enumerate(zip(got, want["values"])):
        for c, (g, w) in enumerate(zip(grow, wrow)):
            if w is None:
                assert isinstance(g, float) and np.isnan(g), (where, r, c)
            elif isinstance(w, bool):
                assert bool(g) is w, (where, r, c)
            else:
                assert float(g) == pytest.approx(w, rel=1e-12, abs=0), (where, r, c)


def test_read_tracks_every_layout_and_mode(gold):
    seen_exit = seen_ok = 0
    for key, want in gold["read_tracks"].items():
        n, mode = (int(v) for v in key.split("/"))
        args = make_args(gold, mode)
        if want == "exit":
            with pytest.raises(SystemExit):
                V.read_tracks(gold["dir"] / f"tracks_{n}.txt", gold["class_names"], args, LOG, frame_wh=tuple(gold["frame_wh"]))
            seen_exit += 1
            continue
        tracks, plotting = V.read_tracks(gold["dir"] / f"tracks_{n}.txt", gold["class_names"], args, LOG, frame_wh=tuple(gold["frame_wh"]))
        same_frame(tracks, want["tracks"], key)
        assert (plotting is None) == (want["plotting"] is None), key
        if plotting is not None:
            same_frame(plotting, want["plotting"], key + " plotting")
        seen_ok += 1
    assert seen_ok >= 14 and seen_exit >= 8                          # 6 layouts x 5 modes; the layouts without stabilized boxes refuse modes > 0
    # the features the table is there for
    t15 = gold["read_tracks"]["15/3"]["tracks"]["values"]
    assert any(r[9] for r in t15) and any(r[12] for r in t15) and not all(r[12] for r in t15)
    assert gold["read_tracks"]["15/0"]["tracks"]["kinds"][1] == "i"                 # the ids stay integers: the label reads id:3, not id:3.0
    with pytest.raises(SystemExit):                                   # too few class names
        V.read_tracks(gold["dir"] / "tracks_15.txt", {0: "car"}, make_args(gold, 0), LOG)


def test_headings_fallback_dims_and_clip_smoothing(gold):
    import pandas as pd

    raw = pd.read_csv(gold["dir"] / "tracks_15.txt", header=None, delimiter=",")
    for s, m, want in gold["parts"]["compute_headings"]:
        got = V.compute_headings(raw, s, m, LOG).to_numpy()
        np.testing.assert_allclose(got, np.array(want), rtol=1e-12, atol=0, err_msg=f"headings {s} {m}")
    assert len({tuple(w) for _, _, w in gold["parts"]["compute_headings"]}) == 4
    l, w = V._estimate_fallback_dims(raw)
    np.testing.assert_allclose(l.to_numpy(), gold["parts"]["fallback_dims"][0], rtol=1e-12, atol=0)
    np.testing.assert_allclose(w.to_numpy(), gold["parts"]["fallback_dims"][1], rtol=1e-12, atol=0)
    oriented, _ = V.read_tracks(gold["dir"] / "tracks_15.txt", gold["class_names"], make_args(gold, 3), LOG, frame_wh=tuple(gold["frame_wh"]))
    for s, want in gold["parts"]["smooth_clip_dims"]:
        np.testing.assert_allclose(V._smooth_clip_dims(oriented, s).to_numpy(dtype=float), np.array(want), rtol=1e-12, atol=0, err_msg=f"clip dims {s}")


def test_clippers(gold):
    empty = kept = 0
    for k, c in enumerate(gold["clip_poly"]):
        got = V._clip_poly_to_rect(np.array(c["corners"], np.float32), *c["rect"])
        assert got.dtype == np.float32 and got.shape == (len(c["out"]), 2), k
        if len(c["out"]):
            np.testing.assert_allclose(got.astype(float), np.array(c["out"]), rtol=1e-12, atol=0, err_msg=f"poly {k}")
            kept += 1
        else:
            empty += 1
    assert empty and kept
    missed = 0
    for k, c in enumerate(gold["clip_segment"]):
        got = V._clip_segment_to_rect(np.array(c["p0"], np.float32), np.array(c["p1"], np.float32), *c["rect"])
        if c["out"] is None:
            assert got is None, k
            missed += 1
        else:
            np.testing.assert_allclose(np.array(got), np.array(c["out"]), rtol=1e-12, atol=0, err_msg=f"segment {k}")
    assert 0 < missed < len(gold["clip_segment"])


def test_georeferenced_results_and_the_timestamp_fallback(gold):
    tracks, _ = V.read_tracks(gold["dir"] / "tracks_15.txt", gold["class_names"], make_args(gold, 0), LOG)
    same_frame(V.read_georeferenced_results(gold["dir"] / "clip.csv", tracks, LOG), gold["georef_frames"], "Frame_Number")
    same_frame(V.read_georeferenced_results(gold["dir"] / "clip_timestamps_only.csv", tracks, LOG), gold["georef_timestamps"], "Timestamp")
    assert V.read_georeferenced_results(None, tracks, LOG) is None
    assert V.read_georeferenced_results(gold["dir"] / "clip_vid_transf.txt", tracks, LOG) is None      # neither column


def test_normalize_viz_modes():
    assert V.normalize_viz_modes(2, LOG) == [2] and V.normalize_viz_modes([1, 0, 1, 4], LOG) == [1, 0, 4]
    for bad in (5, [0, 7], []):
        with pytest.raises(SystemExit):
            V.normalize_viz_modes(bad, LOG)


def calls_to_primitives(calls):
    """The documented mapping from the reference's drawing calls to primitives (and labels)."""
    prims, texts = [], []
    seg = lambda a, b, color, t: prims.append((SEGMENT, a[0], a[1], b[0], b[1], t, 0, pack_bgr(color)))     # noqa: E731
    for c in calls:
        if c[0] == "rectangle" and c[4] == -1:
            prims.append((FILL, *c[1], *c[2], 0, 0, pack_bgr(c[3])))
        elif c[0] == "rectangle":
            (x1, y1), (x2, y2) = c[1], c[2]
            for a, b in (((x1, y1), (x2, y1)), ((x2, y1), (x2, y2)), ((x2, y2), (x1, y2)), ((x1, y2), (x1, y1))):
                seg(a, b, c[3], c[4])
        elif c[0] == "line":
            seg(c[1], c[2], c[3], c[4])
        elif c[0] == "polylines":
            for i in range(len(c[1])):
                seg(c[1][i], c[1][(i + 1) % len(c[1])], c[2], c[3])
        elif c[0] == "circle":
            prims.append((RING, *c[1], c[2], 0, c[4], 0, pack_bgr(c[3])))
        elif c[0] == "putText":
            assert c[3] == [255, 255, 255]
            texts.append((len(prims), c[1], tuple(c[2])))
        else:
            raise AssertionError(c[0])
    return prims, texts


def test_build_primitives_equals_the_recorded_calls(gold):
    from geotrax_amd.stabilized_video import load_transforms

    tw, th = gold["text_size"]
    text_size = lambda label: (tw * len(label), th)                  # noqa: E731
    transforms = load_transforms(gold["dir"] / "clip_vid_transf.txt")
    assert 3 not in transforms and len(transforms) == 11
    seen = defaultdict(int)
    for run in gold["runs"]:
        mode, where = run["mode"], f"mode {run['mode']} layout {run['layout']} {run['args']}"
        args = make_args(gold, mode, **run["args"])
        tracks, _ = V.read_tracks(gold["dir"] / f"tracks_{run['layout']}.txt", gold["class_names"], args, LOG, frame_wh=tuple(gold["frame_wh"]))
        by_frame, speed_lane, no_rows = V.group_by_frame(tracks, V.read_georeferenced_results(gold["dir"] / "clip.csv", tracks, LOG))
        history = defaultdict(list)
        for f, calls in enumerate(run["frames"]):
            want_prims, want_texts = calls_to_primitives(calls)
            prims, texts = V.build_primitives(f, by_frame.get(f, no_rows), history, gold["class_names"], speed_lane.get(f), gold["viz_config"], args, LOG,
                                              text_size, V._frame_homography(mode, transforms, f))
            assert texts == want_texts, (where, f)
            assert prims == want_prims, (where, f)
            # what the table was built to contain, counted from the recording
            for c in calls:
                seen[c[0]] += 1
                if c[0] == "putText":
                    seen["mi/h"] += " mi/h" in c[1]
                    seen["km/h"] += " km/h" in c[1]
                    seen["zero speed"] += " 0 km/h" in c[1] or " 0 mi/h" in c[1]
                    seen["lane"] += " L" in c[1]
                    seen["class name"] += " car" in c[1] or " truck" in c[1]
                    seen["filtered class"] += "motorcycle" in c[1] and run["args"].get("class_filter") is None
            fills = [c for c in calls if c[0] == "rectangle" and c[4] == -1]
            seen["label inside"] += sum(c[2][1] > c[1][1] for c in fills)
            seen["label outside"] += sum(c[2][1] < c[1][1] for c in fills)
        assert len(run["frames"]) == 13 and not run["frames"][12], where
        if not run["args"].get("hide_tracks"):
            assert all(len(v) <= gold["viz_config"]["tail_length"] for v in history.values()) and any(len(v) == 5 for v in history.values()), where
    for what in ("rectangle", "line", "polylines", "circle", "putText", "mi/h", "km/h", "zero speed", "lane", "class name", "label inside", "label outside"):
        assert seen[what] > 0, what
    assert seen["filtered class"] == 0


def test_not_built_flags_are_refused(tmp_path, capsys):
    clip = tmp_path / "clip.y4m"
    clip.write_bytes(b"")
    for flag, word in (("--show", "no window"), ("--plot-trajectories", "alpha blend")):
        assert V.main([str(clip), flag, "--log-path", str(tmp_path / "log")]) == 1
        assert word in capsys.readouterr().err, flag
    assert "--show" in V.__doc__ and "--plot-trajectories" in V.__doc__ and "Stated differences" in V.__doc__
