"""gtx_op_georef_tracks: the georeference stage's per-track columns computed in HBM -- visibility,
dimensions in metres, gap-filled and smoothed speed / acceleration, road-section quad -- against the host functions of
geotrax_amd/georeference.py that stay the default, on the smallest tables at which each kernel can go wrong.

Exactly equal: visibility, every column's NaN pattern, the rows that receive values, section / lane. Speed and acceleration: the
same formulas are evaluated in numpy.longdouble (64-bit mantissa: products and the 85-term sums carry < 0.05 ulp of a double)
from the same local coordinates and weights; the host's worst error against that is measured and the GPU's may be at most twice
it: speed in ulps of the value, acceleration in ulps of max(|v[i]|, |v[i-1]|) * fps (the operands of the difference; in ulps of
its own value the error is unbounded, the exact value passes zero, and a bound on that scale could not fail), both also as plain
absolute errors. Dimensions: the 1e-6 m tests/test_georef_gpu.py allows the chain they come from.

Measured on MI355X (profiles/georef_tracks.txt): the kernels sum in scipy's own order without contraction, and speed and
acceleration came out bit-identical to the host's on every table here (worst host = worst GPU error: see that file)."""
import argparse
import logging
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ORTHO = (126.6412, 37.3951, 2.4e-7, -1.9e-7, 1.1e-9, -0.7e-9)
HOM = np.array([[1.91, 0.08, 5120.5], [-0.07, 1.88, 3310.25], [1.3e-6, -0.9e-6, 1.0]])
FRAME = (2160, 3840)
FPS = 29.97
CRS = ("EPSG:4326", "EPSG:5186")


# ------------------------------------------------------------------------------------------------ tables

def _track(tid, frames, rng, hidden=(), interp=(), dims=(40.0, 18.0), dims_nan_rows=()):
    """Rows of one track: a vehicle moving across the frame; rows in `hidden` get a box that touches the frame's edge."""
    frames = np.asarray(frames)
    k = len(frames)
    x0, y0 = rng.uniform(300, 3500), rng.uniform(300, 1800)
    vx, vy = rng.uniform(-1.5, 1.5), rng.uniform(-1.0, 1.0)
    t = frames - frames[0]
    xs = x0 + vx * t + 0.002 * t ** 2 + rng.normal(0, 0.3, k)
    ys = y0 + vy * t + rng.normal(0, 0.3, k)
    bbox = np.column_stack((np.clip(xs, 60, 3700), np.clip(ys, 60, 2000), np.full(k, 40.0), np.full(k, 20.0)))
    for r in hidden:
        bbox[r, 0] = 22.0                                               # x - w/2 = 2 <= margin 4
    it = np.zeros(k, int)
    it[list(interp)] = 1
    d = np.tile(np.asarray(dims, float), (k, 1))
    for r in dims_nan_rows:
        d[r, 0] = np.nan
    return dict(tid=np.full(k, tid), frame=frames, x=xs, y=ys, bbox=bbox, interp=it, dims=d)


def _table(tracks):
    """The tracks' rows in file order: by frame, then by track id, so the tracks interleave."""
    cat = {k: np.concatenate([t[k] for t in tracks]) for k in tracks[0]}
    seq = np.concatenate([np.arange(len(t["tid"])) for t in tracks])   # keeps a track's own order where a frame number repeats
    o = np.lexsort((seq, cat["tid"], cat["frame"]))
    return {k: v[o] for k, v in cat.items()}


def _main_table():
    rng = np.random.default_rng(5)
    tr, tid = [], 1000
    def add(frames, **kw):
        nonlocal tid
        tid -= 7                                                        # ids fall while the file goes on: the sort has work to do
        tr.append(_track(tid, frames, rng, **kw))
    for m in (42, 43, 84, 85, 86, 1000):                                # speed-series lengths around the radius and its double
        add(np.arange(m + 1) + 3)
    add(np.arange(12), hidden=range(12))                                # 0 used rows
    add(np.arange(12), hidden=range(2, 12))                             # 2 used rows
    add(np.arange(3))                                                   # 3 used rows: a speed series of 2 under radius 42
    add(np.arange(9), hidden=(0, 1, 2, 3, 7, 8), dims_nan_rows=(0,))    # 3 used rows inside a longer track; NaN length on the first row
    add(np.r_[0:10, 11:30], dims_nan_rows=(5,))                         # a gap of 2; NaN length on a later row only
    add(np.r_[0:10, 69:90])                                             # a gap of 60, longer than the radius
    add(np.r_[0:10, 9, 10:30])                                          # a repeated frame number (gap 0)
    add(np.arange(60), hidden=range(20, 31))                            # invisible rows in the middle
    add(np.arange(60), interp=(0, 5, 6, 7, 40, 59))                     # filled-in rows
    add(np.arange(50), hidden=(10, 11), interp=(11, 12, 30))            # both
    while len(tr) < 130:
        k = int(rng.integers(4, 60))
        frames = np.sort(rng.choice(np.arange(int(rng.integers(0, 50)), 200), k, replace=False))
        add(frames, hidden=tuple(rng.choice(k, int(rng.integers(0, 3)), replace=False)), interp=tuple(rng.choice(k, int(rng.integers(0, 3)), replace=False)))
    return _table(tr)


def _long_table():
    """One track whose gap-filled series has 25 001 points (5 001 samples five frames apart) beside two short ones."""
    rng = np.random.default_rng(6)
    return _table([_track(3, np.arange(40), rng), _track(2, np.arange(5001) * 5, rng), _track(1, np.arange(30) + 7, rng)])


def _segmentation():
    import pandas as pd

    rows = [("A", 1, 100, 100, 100, 400, 400, 400, 400, 100),            # tl bl br tr: one winding
            ("A", 2, 300, 300, 600, 300, 600, 600, 300, 600),            # the other winding; overlaps A1 in [300, 400]^2
            ("B", 1, 700, 100, 1000, 200, 900, 500, 650, 350),           # slanted edges
            ("B", 2, 0, 0, 30, 10, 30, 40, 0, 30),
            ("C", 1, 6000, 4000, 6000, 6000, 9000, 6000, 9000, 4000),    # where HOM puts the main table's vehicles
            ("C", 2, 8000, 5000, 11000, 5000, 11000, 7000, 8000, 7000)]
    return pd.DataFrame(rows, columns=["Section", "Lane", "tlx", "tly", "blx", "bly", "brx", "bry", "trx", "try"])


def _both(ctx, tb, filter_type="gaussian", kernel_size=14, seg=None, interp=True, hom=HOM):
    from geotrax_amd import georeference as G

    it = tb["interp"] if interp else None
    args = (tb["tid"], tb["frame"], tb["bbox"], tb["x"], tb["y"], tb["dims"], it, FRAME, FPS, hom, ORTHO, *CRS, seg, filter_type, kernel_size)
    gpu = G.track_columns(*args, backend="gpu", ctx=ctx)
    # the host functions on the coordinates the device chain produced: what the stage feeds them too
    host = dict(gpu)
    host["visibility"] = G.calculate_visibility(tb["tid"], tb["bbox"], FRAME, 4)
    host["length_m"], host["width_m"] = G.convert_dimensions(tb["tid"], tb["dims"], FRAME, hom, ORTHO, *CRS)
    host["speed"], host["accel"] = G.compute_kinematics(tb["tid"], tb["frame"], gpu["x_local"], gpu["y_local"], host["visibility"], FPS, filter_type,
                                                        kernel_size, is_interpolated=it)
    host["section"], host["lane"] = G.assign_road_section_lane(gpu["ortho_x"], gpu["ortho_y"], seg)
    return gpu, host


# ------------------------------------------------------------------------------------------------ the exact reference

def _exact_kinematics(tb, x_local, y_local, vis, it, weights, boundary, conv=3.6):
    """compute_kinematics' formulas in numpy.longdouble -> (speed, accel, accel_scale) as longdouble arrays, NaN where the host
    leaves NaN. accel_scale is max(|v[i]|, |v[i-1]|) * fps, the size of the operands of the difference an acceleration is: the
    acceleration itself passes zero (it is exactly 0 between equal gap fills), the operands do not."""
    L = np.longdouble
    n = len(tb["tid"])
    speed, accel, scale = np.full(n, np.nan, L), np.full(n, np.nan, L), np.full(n, np.nan, L)
    w = weights.astype(L)
    r = len(w) // 2
    for tid in np.unique(tb["tid"]):
        idx = np.flatnonzero(tb["tid"] == tid)
        use = vis[idx] & ((it[idx] == 0) if it is not None else True)
        if use.sum() < 3:
            continue
        rows = idx[use]
        f, x, y = tb["frame"][rows].astype(np.int64), x_local[rows].astype(L), y_local[rows].astype(L)
        xs, ys, present = [x[0]], [y[0]], [0]
        for i in range(1, len(f)):
            gap = int(f[i] - f[i - 1])
            for step in range(1, gap):
                xs.append(x[i - 1] + L(step) * ((x[i] - x[i - 1]) / L(gap)))
                ys.append(y[i - 1] + L(step) * ((y[i] - y[i - 1]) / L(gap)))
            xs.append(x[i]); ys.append(y[i]); present.append(len(xs) - 1)
        xs, ys, present = np.array(xs, L), np.array(ys, L), np.array(present)
        sp = np.sqrt(np.diff(xs) ** 2 + np.diff(ys) ** 2) * L(FPS)
        m = len(sp)
        pos = np.arange(-r, m + r)
        if boundary == 1:
            pos = np.clip(pos, 0, m - 1)
        else:
            pos = np.mod(pos, 2 * m)
            pos = np.where(pos >= m, 2 * m - 1 - pos, pos)
        ext = sp[pos]
        v = np.zeros(m, L)
        for k in range(2 * r + 1):
            v += w[k] * ext[k:k + m]
        a = np.concatenate(([np.nan, np.nan], np.diff(v) * L(FPS))).astype(L)
        sc = np.concatenate(([np.nan, np.nan], np.maximum(np.abs(v[1:]), np.abs(v[:-1])) * L(FPS))).astype(L)
        v = np.concatenate(([np.nan], v * L(conv))).astype(L)
        speed[rows], accel[rows], scale[rows] = v[present], a[present], sc[present]
    return speed, accel, scale


def _ulps(got, exact, scale=None):
    """Worst |got - exact| over the cells that hold a value, in ulps of the (double) value, or of `scale` where one is given."""
    ok = ~np.isnan(exact)
    e = exact[ok]
    of = e if scale is None else scale[ok]
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.max(np.abs(got[ok].astype(np.longdouble) - e) / np.spacing(np.abs(of.astype(np.float64)))))


def _check(gpu, host, tb, it, filter_type, kernel_size, report):
    from geotrax_amd import georeference as G

    np.testing.assert_array_equal(gpu["visibility"], host["visibility"])
    for k in ("speed", "accel", "length_m", "width_m"):
        np.testing.assert_array_equal(np.isnan(gpu[k]), np.isnan(host[k]), err_msg=k)
    np.testing.assert_allclose(gpu["length_m"], host["length_m"], atol=1e-6, rtol=0)
    np.testing.assert_allclose(gpu["width_m"], host["width_m"], atol=1e-6, rtol=0)
    w, b = G.kinematics_weights(filter_type, kernel_size)
    es, ea, scale = _exact_kinematics(tb, gpu["x_local"], gpu["y_local"], host["visibility"], it, w, b)
    np.testing.assert_array_equal(np.isnan(es), np.isnan(host["speed"]))
    np.testing.assert_array_equal(np.isnan(ea), np.isnan(host["accel"]))
    assert np.nanmin(scale.astype(np.float64)) > 1e-3                  # no operand scale near zero: the bound below can fail
    # speed in ulps of the value; acceleration in ulps of its operands (of the value it is unbounded: the exact value passes zero)
    # and, beside it, as the plain absolute error
    for k, e, sc, unit in (("speed", es, None, "ulp of the value"), ("accel", ea, scale, "ulp of max(|v[i]|, |v[i-1]|) * fps")):
        uh, ug = _ulps(host[k], e, sc), _ulps(gpu[k], e, sc)
        ok = ~np.isnan(e)
        ah, ag = (float(np.max(np.abs(c[k][ok].astype(np.longdouble) - e[ok]))) for c in (host, gpu))
        same = bool(np.array_equal(gpu[k], host[k], equal_nan=True))
        print(f"{report} {filter_type}/{kernel_size} {k}: worst error host {uh:.3g}, gpu {ug:.3g} {unit}; absolute host {ah:.3g}, gpu {ag:.3g}; "
              f"bit-identical {same}")
        assert np.isfinite(uh) and ug <= 2 * uh, (k, ug, uh)
        assert ag <= 2 * ah, (k, ag, ah)


# ------------------------------------------------------------------------------------------------ tests

@pytest.fixture(scope="module")
def main(gtx_ctx):
    tb = _main_table()
    return tb, _both(gtx_ctx, tb, seg=_segmentation())


def test_main_table_shape(main):
    """The table is what the cases need: 130 interleaved tracks, used-row counts 0, 2, 3, every gap kind."""
    from geotrax_amd import georeference as G

    tb, (gpu, host) = main
    ids = np.unique(tb["tid"])
    assert len(ids) == 130 and np.count_nonzero(np.diff(tb["tid"]) != 0) > 1000          # interleaved, not grouped
    plan = G.track_plan(tb["tid"], tb["frame"], host["visibility"], tb["interp"])
    assert {0, 2, 3, 43, 44, 85, 86, 87, 1001} <= set(plan["n_used"].tolist())
    assert len(plan["order"]) > 256 * 8                                                  # row kernels run more than one workgroup


def test_columns_match_host_gaussian(main):
    tb, (gpu, host) = main
    _check(gpu, host, tb, tb["interp"], "gaussian", 14, "main")
    assert np.isnan(gpu["speed"]).sum() > 130 and (~np.isnan(gpu["accel"])).sum() > 2000


def test_lanes_on_the_main_table(main):
    tb, (gpu, host) = main
    for k in ("section", "lane"):
        a, b = gpu[k], host[k]
        assert a.dtype == object and len(a) == len(b)
        assert all((x == y) or (x != x and y != y) for x, y in zip(a, b)), k
    assert {("C", 1), ("C", 2)} <= set(zip(gpu["section"], gpu["lane"])) and any(v != v for v in gpu["lane"])


@pytest.mark.parametrize("filter_type,kernel_size", [("savgol", 14), ("savgol", 5), ("gaussian", 5)])
def test_columns_match_host_other_filters(gtx_ctx, main, filter_type, kernel_size):
    """Savitzky-Golay (an even size: the window is size + 1; boundary rule 'nearest') and a narrow Gaussian."""
    tb = main[0]
    gpu, host = _both(gtx_ctx, tb, filter_type, kernel_size)
    _check(gpu, host, tb, tb["interp"], filter_type, kernel_size, "main")
    assert gpu["section"] is None and gpu["lane"] is None and host["section"] is None     # no segmentation: (None, None)


def test_without_is_interpolated(gtx_ctx, main):
    tb = main[0]
    gpu, host = _both(gtx_ctx, tb, interp=False)
    _check(gpu, host, tb, None, "gaussian", 14, "no-interp")
    assert (~np.isnan(gpu["speed"])).sum() > (~np.isnan(main[1][0]["speed"])).sum()


def test_long_series_lives_in_scratch(gtx_ctx):
    """25 001 gap-filled points in one track: 200 KB per scratch array, more than a CU's LDS."""
    from geotrax_amd import georeference as G

    tb = _long_table()
    gpu, host = _both(gtx_ctx, tb)
    plan = G.track_plan(tb["tid"], tb["frame"], host["visibility"], tb["interp"])
    assert int(np.diff(plan["exp_off"]).max()) == 25001
    _check(gpu, host, tb, tb["interp"], "gaussian", 14, "long")


def test_two_calls_give_the_same_bits(gtx_ctx, main):
    tb, (gpu, _) = main
    again, _ = _both(gtx_ctx, tb, seg=_segmentation())
    for k in ("ortho_x", "ortho_y", "latitude", "longitude", "x_local", "y_local", "length_m", "width_m", "speed", "accel"):
        assert gpu[k].tobytes() == again[k].tobytes(), k
    np.testing.assert_array_equal(gpu["visibility"], again["visibility"])
    lab = lambda c: [None if v != v else v for v in c]
    for k in ("section", "lane"):
        assert lab(gpu[k]) == lab(again[k]) and len(set(lab(gpu[k]))) > 1, k


def test_chain_columns_are_gtx_op_georef_points(gtx_ctx, main):
    from geotrax_amd.georeference import transform_points

    tb, (gpu, _) = main
    want = transform_points(tb["x"], tb["y"], HOM, ORTHO, *CRS, ctx=gtx_ctx)
    for k, v in want.items():
        assert gpu[k].tobytes() == v.tobytes(), k


def test_empty_and_single_track(gtx_ctx):
    from geotrax_amd import georeference as G

    e = np.zeros(0)
    got = G.track_columns(e.astype(int), e.astype(int), np.zeros((0, 4)), e, e, np.zeros((0, 2)), None, FRAME, FPS, HOM, ORTHO, *CRS, None, "gaussian",
                          14, backend="gpu", ctx=gtx_ctx)
    assert all(len(got[k]) == 0 for k in ("visibility", "speed", "accel", "length_m", "ortho_x"))
    rng = np.random.default_rng(9)
    tb = _table([_track(4, np.r_[0:30, 33:60], rng, hidden=(3,), dims_nan_rows=(7,))])
    gpu, host = _both(gtx_ctx, tb)
    _check(gpu, host, tb, tb["interp"], "gaussian", 14, "single")
    assert not np.isnan(gpu["length_m"]).any()


def test_dimensions_nan_rules(main):
    """NaN on the track's first row in file order -> NaN for the whole track; NaN on a later row only -> no NaN."""
    tb, (gpu, host) = main
    first = {t: np.flatnonzero(tb["tid"] == t)[0] for t in np.unique(tb["tid"])}
    nan_first = [t for t, r in first.items() if np.isnan(tb["dims"][r, 0])]
    nan_later = [t for t in first if t not in nan_first and np.isnan(tb["dims"][tb["tid"] == t, 0]).any()]
    assert len(nan_first) == 1 and len(nan_later) == 1
    assert np.isnan(gpu["length_m"][tb["tid"] == nan_first[0]]).all() and np.isnan(gpu["width_m"][tb["tid"] == nan_first[0]]).all()
    assert not np.isnan(gpu["length_m"][tb["tid"] == nan_later[0]]).any()
    assert np.isnan(gpu["length_m"]).sum() == (tb["tid"] == nan_first[0]).sum()


def test_lane_rule_on_edges_vertices_and_overlaps(gtx_ctx):
    """An identity homography makes the orthophoto point the table's own (x, y), so every point sits where it is put."""
    from geotrax_amd import georeference as G

    seg = _segmentation()
    pts = [(250, 250), (350, 350), (500, 500), (650, 650), (50, 50),      # inside A1; in A1 and A2 (A1 wins); inside A2; none; none
           (100, 250), (250, 100), (400, 350), (300, 450),                # on edges of A1 / A2 (the edge of A1 at x = 400 lies inside A2)
           (100, 100), (400, 400), (600, 600), (300, 300),                # on vertices (400, 400 is a vertex of A1 inside A2; 300, 300 the reverse)
           (850, 150), (800, 300), (700, 100), (850, 300), (675, 225),    # B1: on its slanted edge, inside, vertex, inside, on the edge tr -> tl
           (250, 400), (600, 400), (200, 100), (50, 400),                 # a horizontal edge at the point's y: on it, beside it, on it, off the quad
           (15, 5), (15, 20), (3, 1), (0.3, 0.1), (29.999999999999996, 25), (30, 25), (6.0000000000000009, 2)]
    rng = np.random.default_rng(3)
    pts = np.array(pts + [tuple(p) for p in rng.uniform(0, 1100, (600, 2))] + [(3 * t, t) for t in rng.uniform(0, 10, 100)])
    n = len(pts)
    tb = dict(tid=np.arange(n) // 4, frame=np.arange(n), x=pts[:, 0], y=pts[:, 1], bbox=np.tile([500.0, 500, 40, 20], (n, 1)),
              interp=np.zeros(n, int), dims=np.tile([40.0, 18.0], (n, 1)))
    gpu, host = _both(gtx_ctx, tb, seg=seg, hom=np.eye(3))
    np.testing.assert_array_equal(gpu["ortho_x"], pts[:, 0])
    np.testing.assert_array_equal(gpu["ortho_y"], pts[:, 1])
    lab = lambda c: [None if v != v else v for v in c]
    assert lab(gpu["section"]) == lab(host["section"]) and lab(gpu["lane"]) == lab(host["lane"])
    got = list(zip(lab(gpu["section"]), lab(gpu["lane"])))
    assert got[:5] == [("A", 1), ("A", 1), ("A", 2), (None, None), (None, None)]
    assert got[5:9] == [(None, None), (None, None), ("A", 2), (None, None)]
    assert got[9:13] == [(None, None), ("A", 2), (None, None), ("A", 1)]
    assert got[13:18] == [(None, None), ("B", 1), (None, None), ("B", 1), (None, None)]
    assert len({g for g in got[29:]}) >= 4                                 # the random points reach several quads and none


def test_plan_that_does_not_fit_the_table_is_an_error_not_a_write(gtx_ctx):
    """A plan that passes the size checks but miscounts a track's used rows or its gaps: the kernels find out, write nothing for
    that track and the call fails."""
    from geotrax_amd import _lib, ops
    from geotrax_amd import georeference as G

    rng = np.random.default_rng(1)
    tb = _table([_track(1, np.r_[0:10, 14:20], rng), _track(2, np.arange(12), rng)])
    vis = G.calculate_visibility(tb["tid"], tb["bbox"], FRAME, 4)
    w, b = G.kinematics_weights("gaussian", 14)
    kw = dict(frame_size=FRAME, visibility_margin=4, fps=FPS, boundary=b, ctx=gtx_ctx)
    args = (G.georef_chain(HOM, ORTHO, *CRS), tb["x"], tb["y"], tb["bbox"], tb["dims"], tb["frame"], tb["interp"])
    good = G.track_plan(tb["tid"], tb["frame"], vis, tb["interp"])
    assert good["n_used"].tolist() == [16, 12] and good["exp_off"].tolist() == [0, 20, 32]
    ops.georef_tracks(*args, good, None, w, **kw)
    for n_used, exp_off in (([15, 12], [0, 20, 32]), ([16, 12], [0, 19, 31]), ([16, 12], [0, 20, 33])):
        bad = dict(good, n_used=np.array(n_used, np.int32), exp_off=np.array(exp_off, np.int64))
        with pytest.raises(_lib.GtxError, match="plan does not fit"):
            ops.georef_tracks(*args, bad, None, w, **kw)


# ------------------------------------------------------------------------------------------------ end to end

def _stage_rows(sc, n_frames=24):
    """The track rows of tests/test_georef_stage_gpu.py's scene, with what that clip lacks: every third vehicle accelerates
    (0.05 px / frame^2 = 1-2 m/s^2 on the ground), and three tracks miss frames (gaps of 2, 3 and 6)."""
    missing = {2: (5,), 5: (10, 11), 8: (12, 13, 14, 15, 16)}
    rows = []
    for t in range(n_frames):
        cam = sc.boxes(t, 150)
        for k, ((x, y, w, h), v) in enumerate(zip(sc.veh_xywh, sc.veh_vel)):
            if t in missing.get(k, ()):
                continue
            acc = 0.025 * t * t if k % 3 == 0 else 0.0
            rows.append([t, k + 1, *cam[k], x + v[0] * t + acc, y + v[1] * t - 0.5 * acc, w, h, k % 4, 0.9, max(w, h), min(w, h)])
    return rows


def test_stage_end_to_end_gpu_columns_equal_host_csv(gtx_ctx, tmp_path):
    """The stage with --track-columns gpu on the scene tests/test_georef_stage_gpu.py uses (plus a lane file), against the host
    columns under the homography that run wrote: every CSV cell equal, except where the two unrounded values straddle a rounding
    boundary -- at most 1 cell in 10 000."""
    import pandas as pd
    from PIL import Image

    from geotrax_amd import georef_stage as gs
    from geotrax_amd.synth import make_scene

    H, W = 1080, 1920
    sc = make_scene(seed=2, h=H, w=W)
    src = tmp_path / "DATASET" / "U_clip.npy"
    src.parent.mkdir(parents=True)
    np.save(src, np.stack([sc.render(t, 150) for t in range(2)]))
    rows = _stage_rows(sc)
    (src.parent / "results").mkdir()
    np.savetxt(src.parent / "results" / "U_clip.txt", np.asarray(rows), fmt="%.16g", delimiter=",")
    of = tmp_path / "ORTHOPHOTOS"
    (of / "master_frames").mkdir(parents=True)
    ortho, _ = sc.orthophoto(size=2600, scale=1.15, angle=0.2)
    Image.fromarray(ortho[:, :, ::-1]).save(of / "U.png")
    Image.fromarray(sc.render(6, 150)[:, :, ::-1]).save(of / "master_frames" / "U.png")
    (of / "U.txt").write_text("126.6412 37.3951 2.4e-07 -1.9e-07\n")
    (of / "segmentations").mkdir()
    (of / "segmentations" / "U.csv").write_text("Section,Lane,tlx,tly,blx,bly,brx,bry,trx,try\nN,1,200,200,200,1400,1300,1400,1300,200\n"
                                                "N,2,1000,900,2400,900,2400,2400,1000,2400\n")
    log = logging.getLogger("georef-tracks-gpu")
    a = argparse.Namespace(source=Path(src), cfg=None, output_folder=None, log_path=None, verbose=False, ortho_folder=None, geo_source=None,
                           ref_frame=None, no_master=None, master_folder=None, recompute=None, segmentation_folder=None, track_columns="gpu")
    gs.georeference(a, log, ctx=gtx_ctx)
    res = src.parent / "results"
    g = pd.read_csv(res / "U_clip.csv", dtype=str, keep_default_na=False)
    # the host columns under the homography that run registered (the file holds it to 20 digits), through the stage's own steps
    from geotrax_amd import georeference as G
    from geotrax_amd.config_utils import load_config_all

    Hw = np.loadtxt(res / "U_clip_geo_transf.txt", delimiter=",").reshape(3, 3)
    config = load_config_all(a, log, needs_model=False)["georef"]
    tid, fn, bbox, xs, ys, cls, dims, interp = gs.get_tracking_data(src, log, {"folder": a.output_folder})
    _, frame_size, fps = gs.get_video_data(src, a.ref_frame, log)
    params = gs.get_ortho_parameters(of, "U", "text-file", config["transformation"]["cutout_width_px"], log)
    df = gs.georeference_tracks(tid, fn, bbox, xs, ys, cls, dims, interp, gs.get_timestamps(src, fn, log), frame_size, fps, Hw, params,
                                gs.get_road_section_lane_geometry(of, None, "U", log), config, log, ctx=gtx_ctx)
    G.save_georeferenced_data(tmp_path / "host.csv", df, log)
    h = pd.read_csv(tmp_path / "host.csv", dtype=str, keep_default_na=False)
    assert list(h.columns) == list(g.columns) and len(h) == len(g) == len(rows)
    assert (h["Lane_Number"] != "").sum() > 0 and (h["Vehicle_Speed"] != "").sum() > 0.5 * len(h)
    acc = pd.to_numeric(h["Vehicle_Acceleration"]).abs()
    assert (acc >= 0.01).sum() > 150 and len(h) < 24 * len(sc.veh_xywh)   # accelerations that do not round to 0.00; rows missing
    differ = int((h.to_numpy() != g.to_numpy()).sum())
    print(f"end to end: {differ} of {h.size} CSV cells differ between the host and the gpu track columns")
    assert differ <= h.size / 10000
