"""The plot stage's kernels (csrc/plot_draw.hip, behind gtx_op_plot_draw / gtx_op_plot_reduce / gtx_plot_canvas_*) against the numpy
twin (geotrax_amd/plot_draw.py) byte for byte, on canvases of at most 200 x 150. Both sides are integer arithmetic: there is no
tolerance. Each edge case first shows from the twin's boxes that it is the edge it claims to be."""
import re
from pathlib import Path

import numpy as np
import pytest
from test_plot_draw import noise, random_polylines

from geotrax_amd import plot_draw as P

pytestmark = pytest.mark.gpu

_hpp = (Path(__file__).resolve().parent.parent / "geo-trax_amd" / "csrc" / "plot_draw.hpp").read_text()
CHUNK = int(re.search(r"kPlotChunk\s*=\s*(\d+)", _hpp).group(1))
TW, TH = (int(v) for v in re.search(r"kPlotTileW\s*=\s*(\d+),\s*kPlotTileH\s*=\s*(\d+)", _hpp).groups())
SIZES = [(1, 1), (15, 63), (17, 65), (97, 130), (150, 200)]          # (h, w): tile edges inside and outside the canvas
WIDTHS, ALPHAS = (0.25, 0.5, 0.6, 1.2, 7.5), (1, 115, 256)


def tiles_of(prims, h, w):
    """[n][tiles_y][tiles_x] bool: the tiles each record is binned to, restated from the twin's boxes."""
    b = P.bounding_boxes(P.quantise(prims))
    tx0, ty0 = np.arange(0, w, TW), np.arange(0, h, TH)
    tx1, ty1 = np.minimum(tx0 + TW, w) - 1, np.minimum(ty0 + TH, h) - 1
    hx = (b[:, 0, None] <= tx1) & (b[:, 2, None] >= tx0)
    hy = (b[:, 1, None] <= ty1) & (b[:, 3, None] >= ty0)
    return hy[:, :, None] & hx[:, None, :]


def equal(ctx, f, prims, label):
    P.validate(prims)
    want = P.rasterize(f, prims)
    got = P.draw_dev(ctx, f, prims)
    bad = np.argwhere((got != want).any(axis=2))
    assert len(bad) == 0, f"{label}: {len(bad)} pixels differ, first at (y, x) = {bad[0].tolist()}: kernel {got[tuple(bad[0])]}, twin {want[tuple(bad[0])]}"
    return want


@pytest.mark.parametrize("h,w", SIZES)
def test_seeded_polylines_on_every_canvas_size(gtx_ctx, h, w):
    prims = np.concatenate([random_polylines(60, h, w, seed=h * 1000 + w, pts=(2, 12)), P.as_prims([P.stroke(-3, -2, 4.5, 3, 1.2, (1, 2, 3), 115, 9999)])])
    assert set(np.round(prims["width"].astype(np.float64), 3).tolist()) == {0.25, 0.5, 0.6, 1.2, 7.5} and set(prims["alpha"].tolist()) == {1, 115, 256}
    f = noise(h, w, 4)
    want = equal(gtx_ctx, f, prims, f"{h} x {w}")
    assert (want != f).any()


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("alpha", ALPHAS)
def test_every_width_and_alpha(gtx_ctx, width, alpha):
    h, w = 40, 150
    prims = np.concatenate([P.polyline([3.2, 70.7, 146.1], [5.5, 33.3, 2.9], width, (250, 20, 130), alpha, 0),
                            P.as_prims([P.disc(100.4, 20.2, width / 2, (5, 200, 90), alpha, 1)])])
    f = noise(h, w, 5)
    want = equal(gtx_ctx, f, prims, f"width {width} alpha {alpha}")
    assert (want != f).any()


def test_segments_on_tile_borders_and_across_many_tiles(gtx_ctx):
    h, w = 97, 130
    rows = [P.stroke(0, TH, w - 1, TH, 0.5, (255, 0, 0), 256, 0), P.stroke(0, TH - 0.5, w - 1, TH - 0.5, 1.2, (0, 255, 0), 115, 1),
            P.stroke(TW, 0, TW, h - 1, 0.6, (0, 0, 255), 256, 2), P.stroke(TW - 0.5, 0, TW - 0.5, h - 1, 7.5, (9, 9, 9), 115, 3),
            P.stroke(0, 0, w - 1, h - 1, 1.2, (200, 100, 0), 115, 4), P.stroke(w - 1, 0, 0, h - 1, 7.5, (0, 100, 200), 115, 5)]
    hit = tiles_of(P.as_prims(rows), h, w)
    assert hit[0, 0:2].all() and not hit[0, 2:].any()           # the stroke on the border row reaches the tiles on both sides of it
    assert hit[2, :, 0:2].all() and not hit[2, :, 2:].any()
    assert hit[4].sum() >= 7 and hit[5].sum() >= 7              # the diagonals cross many tiles
    equal(gtx_ctx, noise(h, w, 6), rows, "tile borders")


def test_segments_off_the_canvas_and_negative_coordinates(gtx_ctx):
    h, w = 17, 65
    rows = [P.stroke(-500, -300, -20, -10, 7.5, (255, 255, 0), 256, 0),        # wholly off: binned nowhere
            P.stroke(300, 5, 900, 8, 1.2, (255, 0, 255), 256, 1),
            P.stroke(-40.5, 8.25, 30.75, 8.25, 1.2, (0, 255, 255), 115, 2),     # partly off, negative start
            P.stroke(60, -30, 70, 40, 7.5, (90, 90, 255), 256, 3),              # leaves through the corner tile
            P.stroke(-2000, -100, 40, 12, 0.6, (1, 2, 3), 256, 4),              # the longest a record may be
            P.stroke(-32768, -32768, -32000, -32768, 0.5, (4, 5, 6), 256, 5)]
    hit = tiles_of(P.as_prims(rows), h, w)
    assert not hit[0].any() and not hit[1].any() and not hit[5].any() and hit[2].any() and hit[3].any() and hit[4].any()
    f = noise(h, w, 7)
    want = equal(gtx_ctx, f, rows, "off-canvas")
    assert (want != f).any()
    only_off = [rows[0], rows[1], rows[5]]
    assert np.array_equal(P.draw_dev(gtx_ctx, f, only_off), f)


def test_one_tile_takes_more_than_a_chunk_and_keeps_the_order(gtx_ctx):
    """Three chunks' worth of semi-transparent polylines of alternating colours through one tile: one dropped or swapped entry changes the blend."""
    h, w = 17, 65
    n = 3 * CHUNK + 37
    rng = np.random.default_rng(8)
    rows = []
    for k in range(n):
        x0, y0, x1, y1 = rng.uniform(2, 60), rng.uniform(1, 8), rng.uniform(2, 60), rng.uniform(1, 8)
        rows.append(P.stroke(x0, y0, x1, y1, 1.2, tuple(int(v) for v in rng.integers(0, 256, 3)), 115, k))
    rows[CHUNK - 1] = P.stroke(5, 13, 60, 13, 1.2, (255, 0, 0), 115, CHUNK - 1)      # the two entries on either side of the first chunk boundary
    rows[CHUNK] = P.stroke(30, 11, 36, 15, 1.2, (0, 0, 255), 115, CHUNK)              # cross where nothing else reaches
    rows[-1] = P.stroke(2, 2, 60, 7, 1.2, (0, 255, 0), 256, n - 1)                    # the last entry is opaque
    prims = P.as_prims(rows)
    assert tiles_of(prims, h, w)[:, 0, 0].sum() == n > CHUNK
    f = noise(h, w, 9)
    want = equal(gtx_ctx, f, prims, "long list")
    swapped = prims.copy()
    swapped[[CHUNK - 1, CHUNK]] = swapped[[CHUNK, CHUNK - 1]]
    assert not np.array_equal(P.rasterize(f, swapped), want)    # the case can tell an order error at a chunk boundary
    assert not np.array_equal(P.rasterize(f, prims[:-1]), want)  # ... and a dropped last entry


def test_three_thousand_polylines(gtx_ctx):
    h, w = 150, 200
    prims = random_polylines(3000, h, w, seed=10, pts=(2, 40), step=4.0)
    assert len(prims) > 30000
    equal(gtx_ctx, noise(h, w, 11), prims, "3000 polylines")


def test_discs_at_the_corners(gtx_ctx):
    for h, w in SIZES:
        rows = [P.disc(x, y, r, (30 * k, 255 - 40 * k, 17 * k), a, k)
                for k, (x, y, r, a) in enumerate([(0, 0, 3.75, 256), (w - 1, 0, 0.3, 115), (0, h - 1, 2.0, 115), (w - 1, h - 1, 3.75, 1), (w - 0.5, h - 0.5, 0.125, 256),
                                                  (-3.0, -3.0, 3.75, 256)])]
        f = noise(h, w, 12)
        want = equal(gtx_ctx, f, rows, f"corner discs {h} x {w}")
        assert not np.array_equal(want[0, 0], f[0, 0])


def test_bytes_outside_the_canvas_come_back_untouched(gtx_ctx):
    """A pitched canvas inside a larger allocation: sentinel bytes between the rows and live bytes behind the last row."""
    h, w = 17, 65
    pitch, tail = 3 * w + 13, 4096
    rng = np.random.default_rng(13)
    buf = rng.integers(0, 256, h * pitch + tail, dtype=np.uint8)
    rows = buf[:h * pitch].reshape(h, pitch)
    f = np.ascontiguousarray(rows[:, :3 * w]).reshape(h, w, 3)
    prims = np.concatenate([random_polylines(80, h, w, seed=14, pts=(2, 8)), P.as_prims([P.stroke(0, h - 1, w - 1, h - 1, 7.5, (255, 255, 255), 256, 999),
                                                                                          P.disc(w - 1, h - 1, 3.75, (0, 0, 0), 256, 1000)])])
    got = P.draw_dev_pitched(gtx_ctx, buf, h, w, pitch, prims)
    want = buf.copy()
    want[:h * pitch].reshape(h, pitch)[:, :3 * w] = P.rasterize(f, prims).reshape(h, 3 * w)
    assert not np.array_equal(want, buf)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("h,w", [(7, 5), (64, 48), (131, 67)])
@pytest.mark.parametrize("k", [1, 2, 3])
def test_reduce_equals_the_twin(gtx_ctx, h, w, k):
    rng = np.random.default_rng(h + k)
    for shape in ((h, w), (h, w, 3), (h, w, 4)):
        img = rng.integers(0, 256, shape, dtype=np.uint8)
        assert np.array_equal(P.reduce_dev(gtx_ctx, img, k), P.reduce(img, k)), (shape, k)


def test_canvas_object_reduces_draws_reads_and_encodes(gtx_ctx):
    from geotrax_amd import jpeg

    rng = np.random.default_rng(15)
    img = rng.integers(0, 256, (131, 201, 4), dtype=np.uint8)
    prims = random_polylines(50, 66, 101, seed=16)
    c = P.PlotCanvas(gtx_ctx, img, 2)
    try:
        assert (c.h, c.w) == (66, 101)
        base = P.reduce(img, 2)
        assert np.array_equal(c.read(), base)
        c.draw(prims)
        want = P.rasterize(base, prims)
        assert np.array_equal(c.read(), want)
        st = c.stats()
        assert st["prims"] == len(prims) and st["tiles"] == 2 * 5 and st["entries"] >= st["max_per_tile"] > 0
        data = c.encode_jpeg(90)
        assert data[:2] == b"\xff\xd8" and data[-2:] == b"\xff\xd9"
        back = jpeg.decode_host(data)
        assert back.shape == want.shape and np.abs(back.astype(int) - want.astype(int)).mean() < 40     # noise survives 4:2:0 only roughly: a picture of this canvas, not another
    finally:
        c.close()
