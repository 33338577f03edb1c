"""The visualize stage end to end on an 8-frame 256x144 .y4m clip: `python -m geotrax_amd.visualize`'s main() in every mode, and
every picture of every output must be the emitter's bytes for the JPEG twin's record of the twin frame -- the mode's frame source
from the oracle (oracle/warp_ref.py for modes 1 / 4, the first frame for mode 2), painted by the numpy rasteriser
(geotrax_amd.draw.rasterize) with build_primitives' list. No tolerance anywhere. The tracks, the transforms (frame 3 has none)
and the georeferenced csv are the inputs of tests/golden/visualize.json.gz."""
import argparse
import logging
from collections import defaultdict
from pathlib import Path

import numpy as np
import pytest
from test_visualize import load_bundle

pytestmark = pytest.mark.gpu

W, H, N = 256, 144, 8
NAMES = {0: "car", 1: "bus", 2: "truck", 3: "motorcycle"}
CN = ["-cn", "0=car", "1=bus", "2=truck", "3=motorcycle"]
LOG = logging.getLogger("test_visualize_gpu")
LOG.addHandler(logging.NullHandler())
LOG.propagate = False


def make_clip(folder: Path):
    from geotrax_amd.frames import Y4mReader, write_y4m
    from geotrax_amd.synth import make_scene

    scene = make_scene(seed=1, h=H, w=W)
    clip = folder / "clip.y4m"
    write_y4m(clip, [scene.render(4 * i) for i in range(N)])
    rd = Y4mReader(clip)
    frames = [rd.read()[1] for _ in range(N)]
    frames = [np.ascontiguousarray(f.bgr() if hasattr(f, "bgr") else f) for f in frames]
    rd.release()
    (folder / "results").mkdir()
    inputs = load_bundle()["inputs"]
    for name, to in (("tracks_15.txt", "clip.txt"), ("clip_vid_transf.txt", "clip_vid_transf.txt"), ("clip.csv", "clip.csv")):
        (folder / "results" / to).write_text(inputs[name])
    return clip, frames


@pytest.fixture(scope="module")
def clip(tmp_path_factory):
    return make_clip(tmp_path_factory.mktemp("viz"))


@pytest.fixture(scope="module")
def warped(clip):
    """The oracle's stabilized frames, computed once."""
    from geotrax_amd.stabilized_video import load_transforms
    from geotrax_amd.warp import inverse_homography
    from oracle.warp_ref import warp_perspective as warp_ref

    path, frames = clip
    T = load_transforms(path.parent / "results" / "clip_vid_transf.txt")
    assert 3 not in T and all(i in T for i in range(N) if i != 3)
    return {i: warp_ref(frames[i], T[i], M_inv=inverse_homography(T[i])) for i in range(N) if i in T}


def twin_frames(clip, warped, mode, first=0, stop=N, **flags):
    """The frames the stage must have encoded, from the twin alone."""
    from geotrax_amd import draw
    from geotrax_amd import visualize as V
    from geotrax_amd.stabilized_video import load_transforms

    path, frames = clip
    res = path.parent / "results"
    opts = {k: V.VIZ_DEFAULTS[k] for k in ("heading_smoothing", "heading_min_speed", "edge_clip_margin", "edge_clip_smoothing", "class_filter", "show_class_names",
                                           "show_lanes", "show_conf", "hide_labels", "hide_tracks", "hide_speed", "speed_unit", "speed_deadzone", "plot_trajectories")}
    opts.update(flags)
    args = argparse.Namespace(**opts, viz_mode=mode, source=path)
    viz_config = {"tail_length": V.VIZ_DEFAULTS["tail_length"], "line_width": V.VIZ_DEFAULTS["line_width"]}
    tracks, _ = V.read_tracks(res / "clip.txt", NAMES, args, LOG, frame_wh=(W, H))
    by_frame, speed_lane, no_rows = V.group_by_frame(tracks, V.read_georeferenced_results(res / "clip.csv", tracks, LOG))
    T = load_transforms(res / "clip_vid_transf.txt")
    atlas = None if args.hide_labels else draw.GlyphAtlas(viz_config["line_width"])
    history = defaultdict(list)
    out, counts = [], []
    for i in range(first, stop):
        src = warped.get(i, frames[i]) if mode in (1, 4) else frames[first] if mode == 2 else frames[i]
        prims, texts = V.build_primitives(i, by_frame.get(i, no_rows), history, NAMES, speed_lane.get(i), viz_config, args, LOG,
                                          atlas.text_size if atlas else None, V._frame_homography(mode, T, i), atlas.layout if atlas else None)
        draw.validate(prims, atlas.data.size if atlas else 0)
        out.append(draw.rasterize(src, prims, atlas.data if atlas else None))
        counts.append((len(prims), len(texts)))
    return out, counts


def pictures(path):
    from geotrax_amd.frames import AviMjpegReader

    rd = AviMjpegReader(path)
    assert rd.frame_hw == (H, W)
    got = [rd._bytes(i) for i in range(rd.frame_count)]
    rd.release()
    return got


@pytest.mark.parametrize("mode", [0, 1, 2, 3, 4])
def test_every_picture_of_a_mode_is_the_twins(gtx_ctx, clip, warped, mode):
    from geotrax_amd import jpeg, visualize

    path, frames = clip
    assert visualize.main([str(path), "--viz-mode", str(mode), "--quality", "85", "--show-class-names", "--show-lanes", *CN]) == 0
    got = pictures(path.parent / "results" / f"clip_mode_{mode}.avi")
    want, counts = twin_frames(clip, warped, mode, show_class_names=True, show_lanes=True)
    assert len(got) == N == len(want)
    assert all(n > 20 and t >= 4 for n, t in counts), counts          # boxes, label fills, glyphs and tails on every frame
    for i, (g, f) in enumerate(zip(got, want)):
        src = warped.get(i, frames[i]) if mode in (1, 4) else frames[0] if mode == 2 else frames[i]
        assert (f != src).any(), i                                    # the twin did draw
        assert g == jpeg.record_to_bytes(jpeg.bgr_to_record(f, 85)), f"mode {mode} frame {i}"
    if mode in (1, 4):
        assert (warped[1] != frames[1]).any() and 3 not in warped


def test_cut_range_hidden_labels_and_tracks_several_modes_in_one_run(gtx_ctx, tmp_path, warped):
    """--viz-mode 0 2 3 -cfl 2 -cfr 6 --hide-labels --hide-tracks: three files of frames 2..5, numbered as in the clip; mode 2 draws on
    frame 2, the first of the range; no label and no tail is in the lists."""
    from geotrax_amd import jpeg, visualize

    cut = make_clip(tmp_path)
    path, frames = cut
    assert visualize.main([str(path), "--viz-mode", "0", "2", "3", "2", "-cfl", "2", "-cfr", "6", "--hide-labels", "--hide-tracks", *CN]) == 0
    for mode in (0, 2, 3):
        got = pictures(path.parent / "results" / f"clip_mode_{mode}.avi")
        want, counts = twin_frames(cut, warped, mode, first=2, stop=6, hide_labels=True, hide_tracks=True)
        assert len(got) == 4 and all(t == 0 and 0 < n for n, t in counts)
        for k, (g, f) in enumerate(zip(got, want)):
            assert g == jpeg.record_to_bytes(jpeg.bgr_to_record(f, 90)), f"mode {mode} frame {2 + k}"
    assert not (path.parent / "results" / "clip_mode_1.avi").exists()
    # a stage that cannot run says so and writes nothing
    (path.parent / "results" / "clip_vid_transf.txt").unlink()
    assert visualize.main([str(path), "--viz-mode", "1", *CN]) == 1
    assert not (path.parent / "results" / "clip_mode_1.avi").exists()
