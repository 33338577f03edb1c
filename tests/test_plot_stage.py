"""The plot stage (geotrax_amd/plot.py) end to end on a cut of the reference's recorded csv (tests/golden/plot/U_video_cut.csv, 12
vehicles x 40 rows) and a synthetic 400 x 300 orthophoto: file names, and that --id, --plot-points, the class filter and the
aggregation of two sources change the picture where they should. The twin is the back-end on the CPU; one GPU case shows that
the canvases the kernels leave equal the twin's."""
from pathlib import Path

import numpy as np
import pytest

GOLDEN = Path(__file__).resolve().parent / "golden" / "plot" / "U_video_cut.csv"
SCALE = 20.0                                              # the recorded orthophoto is 15 000 px wide; the synthetic one 400


def make_inputs(tmp_path, stems=("U_video_cut",), offsets=(0.0,), segmentation=True):
    import pandas as pd
    from PIL import Image

    res, ortho = tmp_path / "results", tmp_path / "ORTHOPHOTOS"
    res.mkdir(), (ortho / "segmentations").mkdir(parents=True)
    df = pd.read_csv(GOLDEN)
    for stem, off in zip(stems, offsets):
        d = df.copy()
        d["Ortho_X"], d["Ortho_Y"] = d["Ortho_X"] / SCALE, d["Ortho_Y"] / SCALE + off
        d.to_csv(res / f"{stem}.csv", index=False)
    rng = np.random.default_rng(0)
    base = np.clip(rng.normal(120, 6, (300, 400, 3)), 0, 255).astype(np.uint8)      # a dull, faintly noisy ground
    Image.fromarray(base).save(ortho / "U.png")
    if segmentation:
        seg = np.dstack([np.roll(base, 50, axis=1), np.full((300, 400), 255, np.uint8)])
        Image.fromarray(seg, "RGBA").save(ortho / "segmentations" / "U.png")
    return res, ortho


def run(tmp_path, target, ortho, *flags, backend="twin"):
    from geotrax_amd import plot

    rc = plot.main([str(target), "--ortho-folder", str(ortho), "--backend", backend, "--dump", "--log-path", str(tmp_path / "logs"), *flags])
    assert rc == 0
    return {p.stem: np.load(p) for p in sorted((Path(target).parent if Path(target).is_file() else Path(target)).joinpath("plots").glob("*.npy"))}


def tracks(scale=SCALE):
    import pandas as pd

    df = pd.read_csv(GOLDEN)
    return df.assign(x=df["Ortho_X"] / scale, y=df["Ortho_Y"] / scale)


def near(df, canvas_shape, radius=1):
    """bool [h][w]: pixels within `radius` of an observation."""
    m = np.zeros(canvas_shape[:2], bool)
    for x, y in zip(df["x"], df["y"]):
        xi, yi = int(round(x)), int(round(y))
        m[max(yi - radius, 0):yi + radius + 1, max(xi - radius, 0):xi + radius + 1] = True
    return m


def test_three_pictures_with_the_expected_names(tmp_path):
    res, ortho = make_inputs(tmp_path)
    pics = run(tmp_path, res / "U_video_cut.csv", ortho, "--plot-segmentations")
    names = ["U_video_cut_Orthophoto_image_coordinates", "U_video_cut_Orthophoto_image_coordinates_on_orthophoto",
             "U_video_cut_Orthophoto_image_coordinates_on_segmentation_overlay"]
    assert sorted(pics) == names
    for n in names:
        jpg = (res / "plots" / f"{n}.jpg").read_bytes()
        assert jpg[:2] == b"\xff\xd8" and jpg[-2:] == b"\xff\xd9"
        assert pics[n].shape == (300, 400, 3)
    from PIL import Image

    plain, on_ortho, on_seg = (pics[n] for n in names)
    base = np.asarray(Image.open(ortho / "U.png"))[:, :, ::-1]
    t = tracks()
    hit = near(t, plain.shape)
    assert (plain[~hit] == 255).all() and (plain[hit] < 255).any()             # a white page, black tracks (single source: black, width 0.5 pt)
    assert np.array_equal(on_ortho[~hit], base[~hit]) and (on_ortho[hit] != base[hit]).any()
    assert not np.array_equal(on_seg, on_ortho) and np.array_equal(on_seg[~hit], np.roll(base, 50, axis=1)[~hit])
    without = run(tmp_path, res / "U_video_cut.csv", ortho)                      # the overlay picture only on request
    assert len(list((res / "plots").glob("*.jpg"))) == 3 and sorted(without) == names


def test_id_points_and_class_filter_change_the_expected_pixels(tmp_path):
    res, ortho = make_inputs(tmp_path, segmentation=False)
    name = "U_video_cut_Orthophoto_image_coordinates"
    t = tracks()
    plain = run(tmp_path, res / "U_video_cut.csv", ortho)[name]
    vid = int(t["Vehicle_ID"].iloc[0])
    one, rest = t[t["Vehicle_ID"] == vid], t[t["Vehicle_ID"] != vid]
    with_id = run(tmp_path, res / "U_video_cut.csv", ortho, "--id", str(vid))[name]
    changed = (with_id != plain).any(axis=2)
    assert changed.any() and not (changed & ~near(one, plain.shape, 2)).any()
    red = with_id[changed]
    assert (red[:, 2] >= red[:, 0]).all() and (red[:, 2] > red[:, 0]).any()     # BGR: that vehicle is red, nothing else moved
    truck = t[t["Vehicle_Class"] == 2]
    assert 0 < len(truck) < len(t)
    filtered = run(tmp_path, res / "U_video_cut.csv", ortho, "--plot-class-filter", "2")[name]
    gone = (filtered != plain).any(axis=2)
    assert gone.any() and not (gone & ~near(truck, plain.shape, 1)).any() and (filtered[gone] >= plain[gone]).all()
    points = run(tmp_path, res / "U_video_cut.csv", ortho, "--plot-points")[name]
    assert not np.array_equal(points, plain) and (points[~near(t, plain.shape, 1)] == 255).all()
    assert (points < 255).any(axis=2).sum() < (plain < 255).any(axis=2).sum() + len(t) * 9


def test_two_sources_aggregate_into_one_coloured_picture(tmp_path):
    res, ortho = make_inputs(tmp_path, stems=("U1_a", "U2_b"), offsets=(0.0, 40.0), segmentation=False)
    pics = run(tmp_path, res, ortho, "--plot-aggregate")
    assert sorted(pics) == ["agg_U1_a_U2_b_Orthophoto_image_coordinates", "agg_U1_a_U2_b_Orthophoto_image_coordinates_on_orthophoto"]
    page = pics["agg_U1_a_U2_b_Orthophoto_image_coordinates"]
    t = tracks()
    first, second = near(t, page.shape), near(t.assign(y=t["y"] + 40.0), page.shape)
    inked = (page < 250).any(axis=2)
    assert not (inked & ~(first | second)).any()
    a, b = page[inked & first & ~second], page[inked & second & ~first]
    assert len(a) > 50 and len(b) > 50
    # plotting.colors: source 0 is #76b041 (green above blue), source 1 is #3274d9 (blue above green), both semi-transparent over white
    assert (a[:, 1].astype(int) - a[:, 0]).mean() > 5 and (b[:, 0].astype(int) - b[:, 1]).mean() > 5
    assert a.min() > 60                                   # alpha 0.45 at the most: never the pure colour


@pytest.mark.gpu
def test_gpu_dump_equals_the_twins(tmp_path, gtx_ctx):
    res, ortho = make_inputs(tmp_path)
    twin = run(tmp_path, res / "U_video_cut.csv", ortho, "--plot-segmentations", "--id", "2")
    gpu = run(tmp_path, res / "U_video_cut.csv", ortho, "--plot-segmentations", "--id", "2", backend="gpu")
    assert sorted(gpu) == sorted(twin) and len(gpu) == 3
    for name in twin:
        assert np.array_equal(gpu[name], twin[name]), name
        jpg = (res / "plots" / f"{name}.jpg").read_bytes()
        assert jpg[:2] == b"\xff\xd8" and jpg[-2:] == b"\xff\xd9"
