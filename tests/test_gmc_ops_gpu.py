"""The sparse-optical-flow GMC (csrc/gmc.hip, `gmc_method: sparseOptFlow`) kernel by kernel against oracle/gmc_ref.py, at the sizes
and inputs its one synthetic scene (tests/test_gmc_gpu.py) never reaches: partial tiles, the radix branch of the corner selection and
its tie rule, candidate lists fuller than a quarter of the image, every exit of the Lucas-Kanade loop, compaction with holes and the
RANSAC kernels away from the happy path. Hooks: gtx_op_gmc_{corners, lk, ransac}, gtx_gmc_counts. Every case first asserts, from
the oracle alone, that its input reaches the branch it is there for."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K_SEL_CAP, K_NMS_LIST, K_NMS_ROWS = 4096, 1024, 8        # csrc/gmc.hip: kSelCap, kNmsList, kNmsRows (a workgroup: 256 columns x 8 rows)
LK_HW = (200, 240)                                        # pyramid level 3 is 25 x 30: the smallest size at which some points keep all four levels


def as_frame(g):
    """A BGR frame whose half-resolution gray image is exactly g: equal channels pass the fixed-point gray conversion unchanged
    (1868 + 9617 + 4899 = 2^14) and the 2x2 mean of four equal pixels is the pixel."""
    return np.ascontiguousarray(np.repeat(np.repeat(g, 2, 0), 2, 1)[..., None].repeat(3, -1))


def noise(h, w, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (h, w)).astype(np.uint8)


def dot_grid(n, jitter_seed=None, per_pixel=False):
    """2x2 dots of 220 on 40 every 5 px. jitter_seed: +-1 gray per dot (one draw for the dot), or per pixel of the dot's 4x4
    neighbourhood (per_pixel)."""
    g = np.full((n, n), 40, np.int32)
    rng = np.random.default_rng(jitter_seed)
    for y in range(4, n - 4, 5):
        for x in range(4, n - 4, 5):
            g[y:y + 2, x:x + 2] = 220
            if jitter_seed is not None and per_pixel:
                g[y - 1:y + 3, x - 1:x + 3] += rng.integers(-1, 2, (4, 4))
            elif jitter_seed is not None:
                g[y:y + 2, x:x + 2] += int(rng.integers(-1, 2))
    return g.astype(np.uint8)


def period3(h, w):
    """Period 3 in x and y: the 3x3-summed structure tensor is the same at every pixel away from the border, so each is a maximum."""
    t = np.array([[10, 200, 90], [250, 40, 160], [70, 130, 220]], np.uint8)
    return np.ascontiguousarray(np.tile(t, (h // 3 + 1, w // 3 + 1))[:h, :w])


def texture(h, w, seed, k=2, passes=2):
    """Low-passed noise rescaled to 0..255 (box filter of 2k + 1, `passes` times, periodic)."""
    a = np.random.default_rng(seed).random((h, w))
    for _ in range(passes):
        c = np.cumsum(np.pad(a, ((k + 1, k), (0, 0)), mode="wrap"), 0)
        a = c[2 * k + 1:] - c[:-2 * k - 1]
        c = np.cumsum(np.pad(a, ((0, 0), (k + 1, k)), mode="wrap"), 1)
        a = c[:, 2 * k + 1:] - c[:, :-2 * k - 1]
    a = (a - a.min()) / (a.max() - a.min())
    return np.round(a * 255).astype(np.uint8)


def moved_pair(seed, dx, dy, k=2, hw=LK_HW, margin=32):
    """(previous, current): two windows of one texture, the content moving by (+dx, +dy) pixels."""
    h, w = hw
    t = texture(h + 2 * margin, w + 2 * margin, seed, k)
    return t[margin:margin + h, margin:margin + w].copy(), t[margin - dy:margin - dy + h, margin - dx:margin - dx + w].copy()


# --------------------------------------------------------------------------- corners
def check_corners(ctx, g):
    """Bit-exact, in order and in count; the record against the oracle's number of maxima. -> (record, maxima pixel indices, values)"""
    from geotrax_amd import ops
    from oracle.gmc_ref import good_features, local_maxima

    pix, val = local_maxima(g)
    got, rec = ops.gmc_corners(g, ctx=ctx)
    print(f"gray {g.shape}: oracle maxima {len(pix)}, record {rec}")
    assert rec["found"] == len(pix) and rec["stored"] == len(pix)          # nothing is dropped on the way to the selection
    assert rec["gathered"] <= K_SEL_CAP                                     # ... or on the way into LDS
    np.testing.assert_array_equal(got, good_features(g))
    return rec, pix, val


@pytest.mark.parametrize("hw", [(64, 64), (65, 67), (79, 258), (81, 259), (80, 321)])
def test_corners_of_noise_at_partial_tiles(gtx_ctx, hw):
    """64 x 64: the smallest image the object accepts, one nms workgroup wide; 258 / 259: one workgroup (256 columns inside the border)
    and one more column; 259 / 321 = 4 x 64 + 3 / 5 x 64 + 1: a last response tile 3 and 1 columns wide; 79 / 81 / 65 rows: partial
    16-row response tiles and 8-row nms bands."""
    g = noise(*hw, seed=hw[1])
    rec, pix, _ = check_corners(gtx_ctx, g)
    assert len(pix) > 50 and rec["gathered"] == len(pix) and rec["passes"] == 0


def test_gray_half_of_an_odd_frame(gtx_ctx):
    """131 x 135 BGR noise (unequal channels) -> 65 x 67: the last row and column of the frame are not read; corners of the object
    against corners of the oracle's gray image."""
    from geotrax_amd.gmc import GMC
    from oracle.gmc_ref import good_features, local_maxima
    from oracle.yolov8_ref import bgr2gray_half

    f = np.random.default_rng(7).integers(0, 256, (131, 135, 3)).astype(np.uint8)
    g = bgr2gray_half(f[:130, :134])
    assert g.shape == (65, 67) and len(local_maxima(g)[0]) > 50
    m = GMC((131, 135), ctx=gtx_ctx)
    m.apply(f)
    np.testing.assert_array_equal(m.points(0)[0], good_features(g))
    assert m.counts()["found"] == len(local_maxima(g)[0])
    m.close()


def test_more_maxima_than_the_sort_holds_without_ties(gtx_ctx):
    """256 x 256 noise: more than kSelCap maxima, all different, so the 16-bit histogram alone finds a cut that fits LDS."""
    from oracle.gmc_ref import local_maxima

    g = noise(256, 256, seed=0)
    pix, val = local_maxima(g)
    assert len(pix) > K_SEL_CAP and len(np.unique(val)) == len(val)
    rec, *_ = check_corners(gtx_ctx, g)
    assert rec["gathered"] < rec["found"] and rec["passes"] == 0


def cut_bucket(val, want=1000):
    """select_kernel's first cut, from the oracle's values: (candidates above the 16-bit bucket holding the want-th strongest, in it)."""
    key = val.view(np.uint64) >> np.uint64(48)
    rel = np.clip(int(key.max()) - key.astype(np.int64), 0, 255)
    hist, acc = np.bincount(rel, minlength=256), 0
    for b in range(256):
        if acc + hist[b] >= min(want, len(val)):
            return acc, int(hist[b])
        acc += hist[b]


@pytest.mark.parametrize("case", ["per pixel 340", "per dot 200"])
def test_near_ties_need_the_narrowing_passes(gtx_ctx, case):
    """The jittered dot grid: thousands of maxima within one 6 %-wide bucket, so the bucket of the 1000th strongest plus everything
    above it passes kSelCap - 64 = 4032 and is narrowed 8 key bits at a time. 'per pixel 340': +-1 on every pixel around a dot leaves
    one maximum per dot and no tie group above 64 -- 4489 dots at 340 x 340 (at 200 x 200 the jittered grid has 1522 maxima, fewer than
    kSelCap: the branch is not reached, so the case is run at the smallest grid that reaches it). 'per dot 200': one +-1 draw per dot
    keeps the dot's four equal maxima: 6084 in the bucket at 200 x 200, in tie groups of about 2000 which fit LDS once the values are
    narrowed."""
    from oracle.gmc_ref import local_maxima

    g = dot_grid(340, 1, per_pixel=True) if case == "per pixel 340" else dot_grid(200, 5)
    pix, val = local_maxima(g)
    above, inside = cut_bucket(val)
    groups = np.unique(val, return_counts=True)[1]
    print(case, "maxima", len(pix), "above", above, "in the bucket", inside, "largest tie group", groups.max())
    assert len(pix) > K_SEL_CAP and above + inside > K_SEL_CAP - 64
    assert groups.max() <= (64 if case == "per pixel 340" else K_SEL_CAP - 64)
    rec, *_ = check_corners(gtx_ctx, g)
    assert rec["passes"] >= 1 and rec["gathered"] <= K_SEL_CAP - 64


def test_a_tie_group_larger_than_the_sort(gtx_ctx):
    """The dot grid without jitter, 200 x 200: 6084 exactly equal maxima, fewer candidates than a quarter of the image. The value
    bits cannot separate them; the order among equals (larger pixel index first) has to come from narrowing on the pixel index."""
    from oracle.gmc_ref import local_maxima

    g = dot_grid(200)
    pix, val = local_maxima(g)
    groups = np.unique(val, return_counts=True)[1]
    assert groups.max() == 6084 > K_SEL_CAP and len(pix) < g.size // 4
    rec, *_ = check_corners(gtx_ctx, g)
    assert rec["passes"] >= 7                                # six passes use up the 48 low value bits, then the pixel index


@pytest.mark.parametrize("hw", [(64, 96), (66, 261)])
def test_every_interior_pixel_a_maximum(gtx_ctx, hw):
    """The period-3 tile: equal maxima at every pixel two or more away from the border, more than a quarter of the image. 64 x 96 is the smallest; a workgroup's band
    there is 8 x 94 = 752 candidates, inside its LDS list, so 66 x 261 (bands of 8 x 256 = 2048 and a second, 3-column workgroup) is
    the smallest at which the list of kNmsList = 1024 overflows into the global one within one workgroup."""
    from oracle.gmc_ref import local_maxima

    h, w = hw
    g = period3(h, w)
    pix, val = local_maxima(g)
    assert len(pix) > h * w // 4 and len(np.unique(val)) == 1
    ys, xs = pix // w, pix % w
    per_group = np.bincount(((ys - 1) // K_NMS_ROWS) * ((w - 2 + 255) // 256) + (xs - 1) // 256)
    assert (per_group.max() > K_NMS_LIST) == (w > 131)
    check_corners(gtx_ctx, g)


def test_corner_state_from_frame_to_frame(gtx_ctx):
    """One object: a frame that fills the candidate list, two ordinary frames (both parities), a flat frame (no corner), an
    ordinary one (nothing to track from the flat frame: identity, not valid; the flat frame's own warp is whatever the previous
    frame's corners give on it, as in the oracle). The counters a frame leaves behind must not leak into the next frame of its
    parity."""
    from geotrax_amd.gmc import GMC
    from oracle.gmc_ref import good_features, local_maxima

    h, w = 64, 96
    frames = [period3(h, w), noise(h, w, 1), noise(h, w, 2), np.full((h, w), 100, np.uint8), noise(h, w, 3)]
    assert len(local_maxima(frames[0])[0]) > h * w // 4 and len(good_features(frames[3])) == 0
    m = GMC((2 * h, 2 * w), ctx=gtx_ctx)
    for k, g in enumerate(frames):
        A = m.apply(as_frame(g))
        np.testing.assert_array_equal(m.points(0)[0], good_features(g), err_msg=f"frame {k}")
        assert m.counts()["found"] == len(local_maxima(g)[0]), k
        if k == 3:
            assert len(m.points(0)[0]) == 0 and m.counts()["found"] == 0
        if k == 4:                                           # the flat frame left nothing to track: identity, not valid
            np.testing.assert_array_equal(A, np.eye(2, 3))
            assert not m.valid
    m.close()


# --------------------------------------------------------------------------- Lucas-Kanade
def check_lk(ctx, prev, cur, pts, label=""):
    """Status equal and positions within 2e-3 px (the bar tests/test_gmc_gpu.py holds this kernel to against this oracle: float64 on
    both sides, another summation order) for every point but the unsettled ones -- those the oracle's trace shows at the 30-iteration
    cap on some level, at most 5 % of a case. -> (next, status, trace) of the oracle and the kernel's (next, status)."""
    from geotrax_amd import ops
    from oracle.gmc_ref import build_pyramid, lk_track

    pts = np.asarray(pts, np.float32).reshape(-1, 2)
    trace = []
    nxt_o, st_o = lk_track(build_pyramid(prev), build_pyramid(cur), pts, trace)
    unsettled = np.array(["cap of 30" in t for t in trace], bool)
    assert unsettled.sum() <= 0.05 * len(pts), (label, int(unsettled.sum()), len(pts))
    nxt, st = ops.gmc_lk(prev, cur, pts, ctx=ctx)
    s = ~unsettled
    err = np.abs(nxt[s] - nxt_o[s]).max() if s.any() else 0.0
    print(f"lk {label}: {len(pts)} points, {int(st_o.sum())} tracked, {int(unsettled.sum())} unsettled, largest difference {err:.2e} px")
    np.testing.assert_array_equal(st[s], st_o[s])
    assert err <= 2e-3, err
    return nxt_o, st_o, trace, nxt, st


@functools.lru_cache(maxsize=None)
def small_motion():
    from oracle.gmc_ref import good_features

    prev, cur = moved_pair(1, 3, 2)
    return prev, cur, good_features(prev)


def exits(trace, level=None):
    return {t[level] for t in trace} if level is not None else {r for t in trace for r in t}


def test_lk_identical_frames_do_not_move_a_point(gtx_ctx):
    prev, _, pts = small_motion()
    assert len(pts) == 1000
    _, st_o, _, nxt, st = check_lk(gtx_ctx, prev, prev, pts, "identical frames")
    assert st.sum() > 700
    np.testing.assert_array_equal(nxt[st], pts[st])          # b = 0 exactly: the first step is zero


def test_lk_small_translation_with_oscillating_points(gtx_ctx):
    """Content moving by (3, 2) under the previous image's own corners (integer points); seed 1 is one whose trace holds exits by
    oscillation (two steps that cancel: the half step back) beside the ordinary ones."""
    prev, cur, pts = small_motion()
    nxt_o, st_o, trace, nxt, st = check_lk(gtx_ctx, prev, cur, pts, "translation (3, 2)")
    assert {"eps", "oscillation", "left the image", "skipped"} <= exits(trace)
    assert 0.6 * len(pts) < st_o.sum() < len(pts)
    assert np.abs(np.median(nxt[st] - pts[st], 0) - (3, 2)).max() < 0.01


def test_lk_large_translation_needs_the_coarse_levels(gtx_ctx):
    """(14, 9): beyond what level 0 alone converges from. A smoother texture (box filter 17) keeps the points at the iteration
    cap under 5 %."""
    from oracle.gmc_ref import good_features

    prev, cur = moved_pair(2, 14, 9, k=8)
    pts = good_features(prev)
    nxt_o, st_o, trace, nxt, st = check_lk(gtx_ctx, prev, cur, pts, "translation (14, 9)")
    assert len(pts) > 500 and st_o.sum() > 0.5 * len(pts)
    assert np.abs(np.median(nxt[st] - pts[st], 0) - (14, 9)).max() < 0.05


def test_lk_levels_skipped_near_the_borders(gtx_ctx):
    """Points 10, 11, 12, 21, 22, 43, 44, 87 and 88 px from each border: a level is used when the 22-sample window fits around the
    point's position on it (10 px before, 11 px after, in that level's pixels). A skipped level 0 is status 0."""
    prev, cur, _ = small_motion()
    h, w = LK_HW
    d = np.array([10, 11, 12, 21, 22, 43, 44, 87, 88], np.float32)
    pts = np.concatenate([np.stack([d, np.full_like(d, h // 2)], 1), np.stack([w - 1 - d, np.full_like(d, h // 2)], 1),
                          np.stack([np.full_like(d, w // 2), d], 1), np.stack([np.full_like(d, w // 2), h - 1 - d], 1)])
    nxt_o, st_o, trace, nxt, st = check_lk(gtx_ctx, prev, cur, pts, "border distances")
    for level in range(4):
        assert "skipped" in exits(trace, level) and exits(trace, level) - {"skipped"}, level
    skipped0 = np.array([t[0] == "skipped" for t in trace])
    assert skipped0.sum() >= 2 and not st[skipped0].any()


def test_lk_fractional_points(gtx_ctx):
    """(x.25, y.75): all four bilinear weights of the previous image's window differ from 0 and 1 (corners are integers)."""
    prev, cur, pts = small_motion()
    nxt_o, st_o, *_ = check_lk(gtx_ctx, prev, cur, pts[:300] + np.float32([0.25, 0.75]), "fractional points")
    assert st_o.sum() > 150


def test_lk_flat_patch_is_rejected(gtx_ctx):
    """Points whose whole 22 x 22 neighbourhood is one gray value: the smaller eigenvalue is 0 < 1e-4 on level 0, status 0."""
    prev, cur, _ = small_motion()
    prev, cur = prev.copy(), cur.copy()
    prev[80:120, 100:140] = 128
    cur[80:120, 100:140] = 128
    pts = np.float32([[x, y] for y in (92, 100, 107) for x in (112, 120, 127)])
    nxt_o, st_o, trace, nxt, st = check_lk(gtx_ctx, prev, cur, pts, "flat patch")
    assert all(t[0] == "min-eig" for t in trace) and not st.any()


def test_lk_track_leaving_the_image(gtx_ctx):
    """Points 12 px from the right border, the content moving 4 px to the right: the window fits around the point and no longer
    around the estimate after a step or two, status 0."""
    h, w = LK_HW
    prev, cur = moved_pair(1, 4, 0)
    pts = np.float32([[w - 1 - 12, y] for y in range(15, h - 15, 6)])
    nxt_o, st_o, trace, nxt, st = check_lk(gtx_ctx, prev, cur, pts, "leaving the image")
    left = np.array([t[0] == "left the image" for t in trace])
    assert left.sum() >= len(pts) // 2 and not st[left].any()


def test_lk_checkerboard_at_the_derivative_extremes(gtx_ctx):
    """8-px squares of 0 and 255: the Scharr numerators reach +-(3 + 10 + 3) * 255 = +-4080 in the short they are staged as."""
    from oracle.gmc_ref import _scharr

    h, w = LK_HW
    yy, xx = np.mgrid[0:h + 8, 0:w + 8]
    board = (((yy // 8) + (xx // 8)) % 2 * 255).astype(np.uint8)
    prev, cur = board[4:4 + h, 4:4 + w].copy(), board[4:4 + h, 3:3 + w].copy()      # the content moves by (1, 0)
    ix, iy = _scharr(prev)
    assert ix.max() * 32 == 4080 and ix.min() * 32 == -4080 and iy.max() * 32 == 4080 and iy.min() * 32 == -4080
    pts = np.float32([[x, y] for y in range(20, h - 20, 16) for x in range(20, w - 20, 16)])
    nxt_o, st_o, trace, nxt, st = check_lk(gtx_ctx, prev, cur, pts, "checkerboard")
    assert st_o.all() and np.abs(nxt[st] - pts[st] - (1, 0)).max() < 0.05


@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 1000])
def test_lk_point_counts_around_a_workgroup_of_four_waves(gtx_ctx, n):
    from geotrax_amd import ops

    prev, cur, pts = small_motion()
    if n == 0:
        nxt, st = ops.gmc_lk(prev, cur, np.zeros((0, 2), np.float32), ctx=gtx_ctx)
        assert nxt.shape == (0, 2) and st.shape == (0,)
        return
    check_lk(gtx_ctx, prev, cur, pts[-n:], f"n = {n}")


# --------------------------------------------------------------------------- compaction and the chain
def test_compaction_with_holes_and_the_whole_chain(gtx_ctx):
    """The object on 200 x 240 gray images. Dots of 255 on 0 six pixels from the top border are the strongest corners and cannot
    be tracked (level 0 is skipped): holes at the front of the status list. The texture's own lost points make the runs between,
    and seed 3 is one whose weakest corner is lost too: a hole at the back."""
    from geotrax_amd.gmc import GMC
    from oracle.gmc_ref import GmcRef

    h, w = LK_HW
    prev, cur = (a.copy() for a in moved_pair(3, 3, 2))
    for im in (prev, cur):
        for x in range(20, w - 20, 24):
            im[1:9, x - 3:x + 5] = 0
            im[5:7, x:x + 2] = 255
    o = GmcRef(seed=0)
    o.apply(prev)
    n_prev = len(o.prev_pts)
    Ao = o.apply(cur)
    st_o = o.last["status"]
    print("corners", n_prev, "tracked", int(st_o.sum()), "first", st_o[:4], "last", st_o[-4:])
    assert n_prev < 1000 and not st_o[0] and not st_o[-1] and st_o.sum() > 100
    mid = st_o[8:-8]
    assert (~mid).any() and any((~mid[i:i + 2]).all() for i in range(len(mid) - 1)) and mid.any()
    m = GMC((2 * h, 2 * w), ctx=gtx_ctx)
    m.apply(as_frame(prev))
    A = m.apply(as_frame(cur))
    nxt, st = m.points(2)
    np.testing.assert_array_equal(m.points(1)[0], o.last["prev"])
    np.testing.assert_array_equal(st, st_o)
    np.testing.assert_allclose(nxt[st], o.last["next"][st], atol=2e-3)
    np.testing.assert_allclose(A, Ao, rtol=0, atol=2e-4)
    p, q = o.last["prev"][st_o].astype(np.float64), o.last["next"][st_o].astype(np.float64)
    M = Ao.copy()
    M[:, 2] /= 2.0
    e = p @ M[:, :2].T + M[:, 2] - q
    err = np.sqrt((e * e).sum(1))
    assert np.abs(err - 3.0).min() > 1e-3                     # no pair near the inlier threshold: the count is the same on both sides
    assert o.last["inliers"] == int((err < 3.0).sum()) > 100
    assert m.valid and list(m.stats) == [n_prev, int(st_o.sum()), o.last["inliers"]]
    m.close()


# --------------------------------------------------------------------------- RANSAC
def check_ransac(ctx, p, q, seed=0):
    from geotrax_amd import ops
    from oracle.gmc_ref import ransac_hypotheses

    p, q = np.asarray(p, np.float32).reshape(-1, 2), np.asarray(q, np.float32).reshape(-1, 2)
    want = ransac_hypotheses(p, q, seed)
    assert want["margin"] > 1e-6                             # no error within 1e-6 px of the 3 px threshold: counts are exact
    got = ops.gmc_ransac(np.concatenate([p, q], 1), seed, ctx=ctx)
    np.testing.assert_array_equal(got["count"], want["count"])
    assert got["winner"] == want["winner"] and got["best_count"] == want["best_count"]
    np.testing.assert_allclose(got["model"], want["best_model"], rtol=1e-9, atol=0)
    return want, got


def similarity_pairs(n, seed, outliers=0.0):
    rng = np.random.default_rng(seed)
    p = (rng.random((n, 2)) * (240, 200)).astype(np.float32)
    a, b = 1.01 * np.cos(0.02), 1.01 * np.sin(0.02)
    q = p.astype(np.float64) @ np.array([[a, -b], [b, a]]).T + (3.5, -2.25) + rng.normal(0, 0.3, (n, 2))
    bad = rng.random(n) < outliers
    q[bad] += rng.uniform(-60, 60, (int(bad.sum()), 2))
    return p, q.astype(np.float32)


@pytest.mark.parametrize("n", [0, 1, 2, 4, 5, 6, 63, 64, 65, 1000])
def test_ransac_pair_counts_around_a_wave(gtx_ctx, n):
    """0 and 1: no hypothesis at all; 2: every hypothesis draws from two pairs (i == j half the time); 63, 64, 65: the scoring loop's
    stride of one wave."""
    want, got = check_ransac(gtx_ctx, *similarity_pairs(n, seed=n, outliers=0.2), seed=n)
    if n < 2:
        assert got["best_count"] == -1 and got["winner"] == -1 and (got["count"] == -1).all()
        np.testing.assert_array_equal(got["model"], [1, 0, 0, 0])
    else:
        assert got["best_count"] >= 2 and got["winner"] >= 0
        if n == 2:
            assert (want["count"] == -1).any() and got["best_count"] == 2      # the same pair drawn twice: no hypothesis


def test_ransac_all_pairs_identical(gtx_ctx):
    p = np.tile(np.float32([[50.5, 60.25]]), (40, 1))
    want, got = check_ransac(gtx_ctx, p, p + np.float32([1, 2]))
    assert (want["count"] == -1).all() and got["best_count"] == -1 and got["winner"] == -1
    np.testing.assert_array_equal(got["model"], [1, 0, 0, 0])


def test_ransac_duplicated_pairs(gtx_ctx):
    """Every pair twice: hypotheses with i != j whose two first points coincide (den < 1e-12) are not made."""
    from oracle.gmc_ref import N_HYP, _hash

    p, q = similarity_pairs(20, seed=11)
    p, q = np.concatenate([p, p]), np.concatenate([q, q])
    idx = [(_hash(_hash(2 * k)) % 40, _hash(_hash(2 * k + 1)) % 40) for k in range(N_HYP)]
    twins = [k for k, (i, j) in enumerate(idx) if i != j and i % 20 == j % 20]
    assert len(twins) >= 3
    want, got = check_ransac(gtx_ctx, p, q)
    assert (got["count"][twins] == -1).all() and got["best_count"] == 40


def test_ransac_with_outliers(gtx_ctx):
    p, q = similarity_pairs(400, seed=21, outliers=0.4)
    want, got = check_ransac(gtx_ctx, p, q)
    assert 0.5 * 400 < got["best_count"] < 0.7 * 400


def test_ransac_equal_counts_the_first_wins(gtx_ctx):
    """Two groups of 30 pairs, each an exact translation of its own, far apart: a hypothesis from either group counts exactly its 30.
    Several hypotheses tie for the maximum; the lowest index wins."""
    rng = np.random.default_rng(31)
    p = np.round(rng.random((60, 2)) * 200).astype(np.float32)
    q = p.copy()
    q[:30] += np.float32([8, 0])
    q[30:] += np.float32([-40, 25])
    order = rng.permutation(60)
    want, got = check_ransac(gtx_ctx, p[order], q[order])
    ties = np.flatnonzero(want["count"] == want["count"].max())
    assert want["count"].max() == 30 and len(ties) >= 2 and got["winner"] == ties[0]
    groups = {tuple(np.round(want["model"][k][2:]).astype(int)) for k in ties}
    assert groups == {(8, 0), (-40, 25)}                      # both groups are among the tied
