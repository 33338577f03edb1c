"""The pixel rule of the plot stage's trajectory maps (geotrax_amd/plot_draw.py): the properties the rule is written for, the box
average against a float64 block mean, and the twin against Matplotlib's Agg renderer, which is what the reference draws with.
No GPU: tests/test_plot_draw_gpu.py holds the kernels to this twin byte for byte."""
import numpy as np
import pytest

from geotrax_amd import plot_draw as P

WHITE = (255, 255, 255)


def noise(h, w, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def page(h, w, value=255):
    return np.full((h, w, 3), value, np.uint8)


def random_polylines(n, h, w, seed, widths=(0.25, 0.5, 0.6, 1.2, 7.5), alphas=(1, 115, 256), pts=(2, 40), margin=30.0, step=9.0):
    """n seeded polylines of pts[0]..pts[1] points: random walks that start up to `margin` pixels outside the canvas."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        m = int(rng.integers(pts[0], pts[1] + 1))
        x = rng.uniform(-margin, w + margin) + np.cumsum(rng.normal(0, step, m))
        y = rng.uniform(-margin, h + margin) + np.cumsum(rng.normal(0, step, m))
        col = tuple(int(v) for v in rng.integers(0, 256, 3))
        out.append(P.polyline(x, y, float(rng.choice(widths)), col, int(rng.choice(alphas)), poly=k))
    return np.concatenate(out)


def min_distance(prims, h, w):
    """[h][w] float64 distance from every pixel centre to the nearest quantised segment (the rule's own endpoints)."""
    q = P.quantise(prims).astype(np.float64)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    best = np.full((h, w), np.inf)
    for ax, ay, bx, by in q[:, :4] / 16.0:
        vx, vy = bx - ax, by - ay
        L = vx * vx + vy * vy
        t = np.clip(((xs - ax) * vx + (ys - ay) * vy) / L, 0, 1) if L > 0 else np.zeros_like(xs)
        best = np.minimum(best, np.hypot(xs - (ax + t * vx), ys - (ay + t * vy)))
    return best


def test_empty_list_leaves_the_canvas():
    f = noise(20, 30)
    assert np.array_equal(P.rasterize(f, []), f)


@pytest.mark.parametrize("width", [0.25, 0.5, 0.6, 1.2, 7.5])
def test_nothing_is_touched_beyond_half_width_plus_half(width):
    f = noise(60, 90, 1)
    prims = np.concatenate([P.polyline([10.3, 70.9, 80.2], [50.1, 8.4, 30.0], width, (0, 0, 255), 256, 0), np.array([], P.PRIM_DTYPE)])
    out = P.rasterize(f, prims)
    d = min_distance(prims, 60, 90)
    wq = np.floor(np.float32(width).astype(np.float64) * 256 + 0.5) / 256
    far = d >= wq / 2 + 0.5
    assert far.any() and (~far).any()
    assert np.array_equal(out[far], f[far])
    inside = d <= wq / 2 - 0.5
    if inside.any():                                   # alpha 256, coverage 256: the colour exactly
        assert (out[inside] == np.array([0, 0, 255], np.uint8)).all()
    assert (out != f).any()


def test_full_alpha_full_coverage_writes_the_colour():
    out = P.rasterize(noise(40, 40, 2), [P.stroke(5, 20, 35, 20, 7.5, (12, 200, 77), 256)])
    assert (out[18:23, 8:33] == np.array([12, 200, 77], np.uint8)).all()


def test_order_matters_between_polylines():
    a = P.polyline([5, 35], [20, 20], 7.5, (255, 0, 0), 115, poly=0)
    b = P.polyline([20, 20], [5, 35], 7.5, (0, 0, 255), 115, poly=1)
    f = page(40, 40)
    ab, ba = P.rasterize(f, np.concatenate([a, b])), P.rasterize(f, np.concatenate([b, a]))
    assert not np.array_equal(ab[20, 20], ba[20, 20])
    assert np.array_equal(ab[20, 8], ba[20, 8]) and np.array_equal(ab[8, 20], ba[8, 20])


def test_a_polyline_crossing_itself_is_no_darker_at_the_crossing():
    f = page(60, 60)
    one = P.polyline([5, 55, 55, 30, 30], [30, 30, 50, 50, 5], 7.5, (0, 0, 0), 115, poly=0)      # crosses itself at (30, 30)
    out = P.rasterize(f, one)
    assert np.array_equal(out[30, 30], out[30, 15]) and np.array_equal(out[30, 30], out[15, 30])
    two = one.copy()
    two["poly"][3:] = 1                                 # the same records as two polylines do darken
    assert P.rasterize(f, two)[30, 30, 0] < out[30, 30, 0]


def test_a_zero_length_segment_is_the_disc():
    f = noise(30, 30, 3)
    for r in (0.125, 0.3, 2.0, 3.75):
        a = P.rasterize(f, [P.stroke(14.3, 15.6, 14.3, 15.6, 2 * r, (9, 8, 7), 200)])
        b = P.rasterize(f, [P.disc(14.3, 15.6, r, (9, 8, 7), 200)])
        assert np.array_equal(a, b) and (a != f).any()


def test_coverage_is_the_rounded_ramp_of_the_true_distance():
    """The integer rule against the float64 formula it restates, away from the rounding ties of the latter."""
    prims = P.as_prims([P.stroke(3.3, 4.9, 41.2, 29.7, 1.2, WHITE)])
    q = P.quantise(prims)[0]
    xs, ys = np.arange(0, 48), np.arange(0, 36)
    cov = P.coverage(q, xs, ys)
    d = min_distance(prims, 36, 48)
    want = (q[4] / 512.0 - d) * 256 + 0.5
    clear = np.abs(want - np.round(want)) > 1e-6
    assert np.array_equal(cov[clear], np.clip(np.floor(want), 0, 256).astype(np.int64)[clear])
    assert cov.max() == 256 and (cov == 0).any() and ((cov > 0) & (cov < 256)).any()


def test_boxes_hold_every_covered_pixel():
    prims = random_polylines(40, 80, 120, 5)
    q = P.quantise(prims)
    boxes = P.bounding_boxes(q)
    for rec, (x0, y0, x1, y1) in zip(q, boxes.tolist()):
        xs, ys = np.arange(x0 - 3, x1 + 4), np.arange(y0 - 3, y1 + 4)
        cov = P.coverage(rec, xs, ys)
        outside = ~((xs[None, :] >= x0) & (xs[None, :] <= x1) & (ys[:, None] >= y0) & (ys[:, None] <= y1))
        assert not cov[outside].any()


def test_validate_names_the_bad_record():
    ok = P.stroke(1, 1, 5, 5, 0.5, WHITE)
    for bad, word in ((P.stroke(1, 1, 5, 5, 0.2, WHITE), "width"), (P.stroke(1, 1, 5, 5, 65, WHITE), "width"), (P.stroke(1, 1, 5, 5, 0.5, WHITE, 0), "alpha"),
                      (P.stroke(1, 1, 5, 5, 0.5, WHITE, 257), "alpha"), (P.stroke(np.nan, 1, 5, 5, 0.5, WHITE), "coordinate"),
                      (P.stroke(1, 1, 40000, 5, 0.5, WHITE), "coordinate"), (P.stroke(0, 0, 2049, 0, 0.5, WHITE), "spans"),
                      (P.stroke(1, 1, 5, 5, 0.6, WHITE), "polyline")):
        with pytest.raises(ValueError, match=f"primitive 1: .*{word}"):
            P.validate([ok, bad])
    assert len(P.split_long([P.stroke(0, 0, 5000, 100, 0.5, WHITE)])) == 3
    P.validate(P.split_long([P.stroke(0, 0, 5000, 100, 0.5, WHITE)]))


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("channels", [1, 3, 4])
def test_reduce_is_the_block_mean_rounded_half_up(k, channels):
    rng = np.random.default_rng(7 + k)
    img = rng.integers(0, 256, (7, 5) if channels == 1 else (7, 5, channels), dtype=np.uint8)
    got = P.reduce(img, k)
    rgb = np.repeat(img[:, :, None], 3, 2) if channels == 1 else img[:, :, :3]
    ho, wo = -(-7 // k), -(-5 // k)
    assert got.shape == (ho, wo, 3)
    for oy in range(ho):
        for ox in range(wo):
            block = rgb[oy * k:(oy + 1) * k, ox * k:(ox + 1) * k].astype(np.float64)      # ragged at the right and bottom edges
            want = np.floor(block.reshape(-1, 3).mean(axis=0) + 0.5)[::-1]               # RGB -> BGR
            assert np.array_equal(got[oy, ox], want.astype(np.uint8)), (oy, ox)


def test_reduce_rounds_a_half_up():
    assert P.reduce(np.array([[0, 1]], np.uint8), 2)[0, 0, 0] == 1
    assert P.reduce(np.array([[0, 1], [0, 0]], np.uint8), 2)[0, 0, 0] == 0


def agg_render(canvas_hw, lines, width_px, color, alpha):
    """The reference's renderer: Matplotlib's Agg, one figure pixel per canvas pixel, imshow's pixel-centre convention."""
    from matplotlib.backends.backend_agg import FigureCanvasAgg
    from matplotlib.figure import Figure

    h, w = canvas_hw
    fig = Figure(figsize=(w / 100.0, h / 100.0), dpi=100)
    FigureCanvasAgg(fig)
    ax = fig.add_axes([0, 0, 1, 1])
    ax.set_xlim(-0.5, w - 0.5)
    ax.set_ylim(h - 0.5, -0.5)
    ax.axis("off")
    for x, y in lines:
        ax.plot(x, y, color=color, linewidth=width_px * 72.0 / 100.0, alpha=alpha, antialiased=True, solid_capstyle="round", solid_joinstyle="round")
    fig.canvas.draw()
    rgba = np.asarray(fig.canvas.buffer_rgba())
    assert rgba.shape[:2] == (h, w)
    return np.ascontiguousarray(rgba[:, :, 2::-1])


def test_twin_against_agg():
    """20 seeded polylines, width 1.2 px, black at alpha 115 / 256 on a white 200 x 150 page, through Agg (antialiased, round caps
    and joins, dpi = one figure pixel per canvas pixel) and through the twin.

    Measured here (Matplotlib 3.10.8, CPU): mean absolute difference 0.926 grey levels over all pixels and channels, 0.49 % of
    the pixels differ by more than 32 levels. The two differ by construction: Agg integrates the stroke's area over a pixel's
    square (with its own sub-pixel grid and gamma-free 8-bit spans), the twin ramps linearly over one pixel of distance from
    the centre line to the pixel's centre; both are anti-aliasing filters of one pixel's support, so they part only on the
    pixels along the strokes' edges. The asserted bounds are twice the measured figures (mean <= 1.86, share <= 0.98 %): a
    margin for other Matplotlib versions' path snapping and stroking, still 4.6 times below what shifting the strokes by one
    pixel gives (measured: mean 8.55). The structural condition is fixed: the touched pixels are the same set up to a
    one-pixel dilation either way."""
    h, w = 150, 200
    rng = np.random.default_rng(11)
    lines = []
    for _ in range(20):
        m = int(rng.integers(2, 41))
        lines.append((rng.uniform(0, w) + np.cumsum(rng.normal(0, 7, m)), rng.uniform(0, h) + np.cumsum(rng.normal(0, 7, m))))
    agg = agg_render((h, w), lines, 1.2, "black", 115 / 256.0)
    prims = np.concatenate([P.polyline(x, y, 1.2, (0, 0, 0), 115, poly=k) for k, (x, y) in enumerate(lines)])
    twin = P.rasterize(page(h, w), prims)
    diff = np.abs(agg.astype(np.int64) - twin.astype(np.int64))
    mean, share = diff.mean(), (diff.max(axis=2) > 32).mean()
    shifted = np.abs(np.roll(twin, 1, axis=1).astype(np.int64) - twin.astype(np.int64)).mean()
    print(f"agg vs twin: mean abs diff {mean:.4f}, share of pixels differing by more than 32: {share:.5f}, one-pixel shift of the twin: {shifted:.3f}")
    assert mean <= 1.86 and share <= 0.0098

    def dilate(m):
        out = m.copy()
        out[1:] |= m[:-1]; out[:-1] |= m[1:]; out[:, 1:] |= m[:, :-1]; out[:, :-1] |= m[:, 1:]
        out[1:, 1:] |= m[:-1, :-1]; out[:-1, :-1] |= m[1:, 1:]; out[1:, :-1] |= m[:-1, 1:]; out[:-1, 1:] |= m[1:, :-1]
        return out

    touched_agg, touched_twin = (agg != 255).any(axis=2), (twin != 255).any(axis=2)
    assert touched_agg.sum() > 1000 and touched_twin.sum() > 1000
    assert not (touched_agg & ~dilate(touched_twin)).any()
    assert not (touched_twin & ~dilate(touched_agg)).any()
