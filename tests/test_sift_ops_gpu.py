"""SIFT (csrc/sift.hip) stage by stage against oracle/sift_ref.py, at the sizes and inputs the one registration scene
(tests/test_registration_gpu.py) passes over: every blur form and radius at the tile edges, pyramids of odd sizes on a reused
object, the extrema test's border / plateau / threshold rules, every exit of the refinement, orientation windows clipped by the image
or larger than it, several peaks, the 0 / 360 wrap, and plain as well as RootSIFT descriptors next to the border.
Hooks: gtx_op_sift_{blur, extrema, refine, orient, describe}. Every expected value comes from the oracle or its float64 variants.

The two measured margins (CPU only, oracle float32 against oracle float64, over every keypoint of the scenes below and the hand-made
cases; each is used with a factor of 4 because the device's expf / atan2f may be an ulp worse than libm's):
  REL_HIST  orientation histogram: largest |float32 - float64| in excess of the bin-hop bound, relative to the histogram's
            maximum: measured 1.61e-7 -> 6.44e-7;
  DELTA_DESC  unrounded descriptor value (0..512 scale): largest |float32 - float64|: measured 1.21e-4 -> 4.84e-4.
Counts behind the conditions (oracle alone): scenes (seed, h, w) = (5, 97, 131), (17, 64, 200), (8, 33, 47) give 45 + 49 + 9 refined
keypoints, of which 0 + 1 + 0 are undecided (limit 5 % of a scene), 9 + 16 + 5 have clipped windows, 0 + 1 + 1 sit in an octave
smaller than their window and 11 + 10 + 3 have two or more peaks; 57 + 60 + 12 descriptors with 18 of their 16 512 bins (0.11 %)
within DELTA_DESC of a half-integer or just below the knee (limit 2 %). Seeds 3, 5, 3 left 15 % of a scene undecided: their
shapes put many gradients at exactly 45 degrees, which is bin 4.5.

The buffers of detect_and_compute hold at least 65 536 candidates; a noise image of 400 x 400 yields 373, so no image a test can
afford reaches them. The overflow rule (count = the true total, never a silent subset) is tested through the hooks' cap argument."""
import functools
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F = np.float32
SCENES = ((5, 97, 131), (17, 64, 200), (8, 33, 47))
REL_HIST = 4 * 1.61e-7
DELTA_DESC = 4 * 1.21e-4
HALF_TOL = 2.0 ** -10


def R():
    from oracle import sift_ref

    return sift_ref


# --------------------------------------------------------------------------- shared oracle data (computed once, never written to)
@functools.lru_cache(maxsize=None)
def scene(k):
    """Oracle pyramids, candidates, refined keypoints (with their histograms) and final keypoints of scene k."""
    from geotrax_amd.synth import make_scene

    seed, h, w = SCENES[k]
    img = make_scene(seed=seed, h=h, w=w).render(0)
    gauss, dog = R().build_pyramids(R().bgr_to_gray(img))
    cand = R().find_candidates(dog)
    refined = {}
    for o, layer, r, c in cand.tolist():
        res = R().refine(dog[o], o, layer, r, c)
        if res is not None:
            refined[(o, layer, r, c)] = res
    return dict(img=img, gauss=gauss, dog=dog, cand=cand, refined=refined)


def refined_records(items, octave):
    """ops.SIFT_REFINED records of oracle refine results: items = [(key, result)]."""
    from geotrax_amd import ops

    rec = np.zeros(len(items), ops.SIFT_REFINED)
    for i, (key, (x, y, word, size, resp, layer, r, c)) in enumerate(items):
        rec[i] = (x, y, size, resp, word, octave, layer, r, c) + tuple(key)
    return rec


def window(size, octave):
    scl = float(F(size)) * 0.5 / (1 << octave)
    return R().cv_round(R().ORI_RADIUS * scl), R().ORI_SIG_FCTR * scl


@functools.lru_cache(maxsize=None)
def orient_cases(k):
    """Per (octave, layer) of scene k: the Gaussian layer, the refined records and, per record, the float32 and float64 histograms
    with the bin-hop bound."""
    s = scene(k)
    groups = {}
    for key, res in s["refined"].items():
        groups.setdefault((key[0], res[5]), []).append((key, res))
    out = []
    for (o, layer), items in sorted(groups.items()):
        img = s["gauss"][o][layer]
        hists = []
        for key, res in items:
            radius, sigma = window(res[3], o)
            h64, amb = R().orientation_hist64(img, res[6], res[7], radius, sigma, ambiguous=HALF_TOL)
            hists.append(dict(h32=R().orientation_hist(img, res[6], res[7], radius, sigma), h64=h64, amb=amb, radius=radius, r=res[6], c=res[7]))
        out.append(dict(o=o, layer=layer, img=img, rec=refined_records(items, o), hists=hists))
    return out


def hist_bound(h):
    return h["amb"] + REL_HIST * h["h64"].max()


def peak_status(h64, B):
    """Per bin: 1 = a peak whatever the histogram is within +- B, 0 = never a peak, -1 = undecided."""
    n = len(h64)
    st = np.zeros(n, int)
    mx, bmax = h64.max(), B.max()
    for j in range(n):
        l, r = (j - 1) % n, (j + 1) % n
        conds = ((h64[j] - h64[l], B[j] + B[l]), (h64[j] - h64[r], B[j] + B[r]), (h64[j] - 0.8 * mx, B[j] + 0.8 * bmax))
        if any(d < -m for d, m in conds):
            st[j] = 0
        elif all(d > m for d, m in conds):
            st[j] = 1
        else:
            st[j] = -1
    return st


def angle_interval(h64, B, j):
    """(middle, half width) in degrees of the angles the parabola through bin j gives while its three bins move within +- B."""
    n = len(h64)
    l, r = (j - 1) % n, (j + 1) % n
    bs = []
    for sl in (-1, 1):
        for sj in (-1, 1):
            for sr in (-1, 1):
                a, b, c = h64[l] + sl * B[l], h64[j] + sj * B[j], h64[r] + sr * B[r]
                bs.append(j + 0.5 * (a - c) / (a - 2 * b + c))
    lo, hi = 360.0 - 10.0 * max(bs), 360.0 - 10.0 * min(bs)
    return 0.5 * (lo + hi), 0.5 * (hi - lo)


@functools.lru_cache(maxsize=None)
def describe_cases(k):
    """Per (octave, layer) of scene k: the Gaussian layer and (px, py, ori, scl) of every final keypoint, as detect_and_compute makes them."""
    out = []
    for g in orient_cases(k):
        rows = []
        for rec, h in zip(g["rec"], g["hists"]):
            scale = 1.0 / (1 << g["o"])
            for a in R().keypoint_angles(h["h32"]):
                ori = 360.0 - a
                ori = 0.0 if abs(ori - 360.0) < 1.19e-7 else ori
                rows.append((F(float(rec["x"]) * scale), F(float(rec["y"]) * scale), ori, F(float(rec["size"]) * scale * 0.5)))
        if rows:
            out.append(dict(img=g["img"], rows=rows))
    return out


# --------------------------------------------------------------------------- blur
BLUR_SIZES = ((1, 1), (1, 70), (70, 1), (2, 3), (5, 7), (31, 63), (32, 64), (33, 65), (45, 130))
# sigma -> radius: the five layer sigmas of the default scale space (compile-time instances), then radii without one
BLUR_SIGMAS = tuple(zip([1.2262734984654078, 1.5450077936447955, 1.9465878414647133, 2.4525469969308156, 3.090015587289591, 0.25, 0.75, 4.0],
                        [5, 6, 8, 10, 13, 1, 3, 16]))


def spiky(h, w, seed):
    rng = np.random.default_rng(seed)
    a = (rng.random((h, w)) * 255).astype(F)
    for y, x, v in ((0, 0, 1e4), (h - 1, w - 1, -1e4), (0, w - 1, -1e4), (h - 1, 0, 1e4), (min(1, h - 1), min(2, w - 1), 1e4), (h // 2, w - 1, -1e4)):
        a[y, x] = v
    return a


@pytest.mark.parametrize("hw", BLUR_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_blur_forms_equal_the_oracle(gtx_ctx, hw):
    """The pyramid's dispatch, the generic tile kernel and the row / column / subtraction passes: the same bits as the oracle's
    blur, and dog = dst - src, at the tile edges (64 x 32), the n == 1 reflection and images narrower than the radius."""
    from geotrax_amd import ops

    assert R().layer_sigmas()[1:] == [s for s, _ in BLUR_SIGMAS[:5]]
    src = spiky(*hw, seed=hw[0] * 1000 + hw[1])
    for sigma, radius in BLUR_SIGMAS:
        assert len(R().gaussian_taps(sigma)) == 2 * radius + 1
        want = R().blur(src, sigma)
        want_dog = (want - src).astype(F)
        for form in (0, 1, 2):
            dst, dog = ops.sift_blur(src, sigma, form, ctx=gtx_ctx)
            np.testing.assert_array_equal(dst, want, err_msg=f"radius {radius} form {form}")
            np.testing.assert_array_equal(dog, want_dog, err_msg=f"dog, radius {radius} form {form}")
        dst, dog = ops.sift_blur(src, sigma, 0, dog=False, ctx=gtx_ctx)
        assert dog is None
        np.testing.assert_array_equal(dst, want)


def test_blur_radius_17_is_an_error_not_a_launch(gtx_ctx):
    from geotrax_amd import _lib, ops

    assert len(R().gaussian_taps(4.25)) == 35
    for form in (0, 1, 2):
        with pytest.raises(_lib.GtxError, match="radius 17 exceeds 16") as e:
            ops.sift_blur(np.zeros((40, 40), F), 4.25, form, ctx=gtx_ctx)
        assert e.value.code == -3


# --------------------------------------------------------------------------- pyramid and object reuse
PYR_SIZES = ((8, 8), (9, 200), (200, 9), (33, 47), (97, 131))


def test_pyramids_of_a_reused_object_equal_the_oracle_and_a_fresh_object(gtx_ctx):
    """One object, built larger than all five images (256 x 256: the 200-row image does not fit 128 rows), takes them in turn: every
    pyramid image equals build_pyramids bit for bit, the octave count is n_octaves, and keypoints and descriptors are those of an
    object built at exactly the image's size."""
    from geotrax_amd.registration import Sift
    from geotrax_amd.synth import make_scene

    big = Sift((256, 256), ctx=gtx_ctx)
    total = 0
    for k, (h, w) in enumerate(PYR_SIZES):
        if min(h, w) >= 33:
            img = make_scene(seed=3, h=h, w=w).render(0)
        else:
            t = np.random.default_rng(k).integers(0, 256, (h // 4 + 2, w // 4 + 2, 1)).astype(np.uint8)
            img = np.ascontiguousarray(np.repeat(np.repeat(t, 4, 0), 4, 1)[:h, :w].repeat(3, -1))
        got = big.detect_and_compute(img)
        gauss, dog = R().build_pyramids(R().bgr_to_gray(img))
        assert big.n_octaves() == len(gauss) == R().n_octaves(2 * h, 2 * w)
        for o in range(len(gauss)):
            for i in range(6):
                np.testing.assert_array_equal(big.pyramid(0, o, i), gauss[o][i], err_msg=f"{h}x{w} gauss {o},{i}")
            for i in range(5):
                np.testing.assert_array_equal(big.pyramid(1, o, i), dog[o][i], err_msg=f"{h}x{w} dog {o},{i}")
        exact = Sift((h, w), ctx=gtx_ctx).detect_and_compute(img)
        assert got["count"] == exact["count"]
        for name in ("xy", "size", "angle", "response", "octave", "desc"):
            np.testing.assert_array_equal(got[name], exact[name], err_msg=f"{h}x{w} {name}")
        total += got["count"]
    assert total > 50


# --------------------------------------------------------------------------- extrema
def as_set(c):
    return sorted(map(tuple, np.asarray(c).reshape(-1, 4).tolist()))


def oracle_candidates(stack, octave):
    c = R().find_candidates([list(stack)])
    c[:, 0] = octave
    return as_set(c)


@pytest.mark.parametrize("k", range(len(SCENES)))
def test_extrema_of_the_scenes_equal_the_oracle(gtx_ctx, k):
    from geotrax_amd import ops

    s = scene(k)
    want_all = as_set(s["cand"])
    assert len(want_all) >= (40, 40, 5)[k]
    for o, d in enumerate(s["dog"]):
        stack = np.stack(d)
        n, got = ops.sift_extrema(stack, o, ctx=gtx_ctx)
        want = [c for c in want_all if c[0] == o]
        assert n == len(want) == len(got), (o, n, len(want))
        assert as_set(got) == want, f"octave {o}"


def hand_stack():
    """16 x 20: the border of 5 leaves rows 5..10 and columns 5..14."""
    d = np.zeros((5, 16, 20), F)
    d[2, 5, 5] = d[2, 5, 6] = 5.0                       # a plateau of two: both are candidates (>=)
    d[1, 7, 8] = 1.0                                    # |v| == threshold: rejected
    d[1, 9, 7] = np.nextafter(F(1.0), F(2.0))           # the next float: accepted
    d[3, 9, 6], d[3, 9, 9] = 7.0, -7.0                  # a maximum and a minimum of equal magnitude
    d[1, 4, 10] = 9.0                                   # row 4: outside
    d[1, 5, 13] = 9.0                                   # row 5: inside
    d[1, 10, 5] = -9.0                                  # row h - 6, column 5: inside
    d[1, 11, 9] = 9.0                                   # row h - 5: outside
    d[3, 7, 4] = 9.0                                    # column 4: outside
    d[3, 10, 14] = 9.0                                  # column w - 6: inside
    d[3, 5, 15] = 9.0                                   # column w - 5: outside
    d[2, 8, 12], d[3, 8, 13] = 4.0, 6.0                 # layer 2's pixel tops its own layer but not its neighbour in layer 3 (which is one)
    return d


def test_extrema_rules_on_hand_made_stacks(gtx_ctx):
    from geotrax_amd import ops

    d = hand_stack()
    want = oracle_candidates(d, 2)
    assert want == sorted([(2, 2, 5, 5), (2, 2, 5, 6), (2, 1, 9, 7), (2, 3, 9, 6), (2, 3, 9, 9), (2, 1, 5, 13), (2, 1, 10, 5), (2, 3, 10, 14), (2, 3, 8, 13)])
    n, got = ops.sift_extrema(d, 2, ctx=gtx_ctx)
    assert n == len(want) and as_set(got) == want
    one = np.zeros((5, 11, 11), F)                      # one interior pixel
    one[1, 5, 5], one[2, 5, 5], one[3, 5, 5] = -2.0, -3.0, -1.5
    one[2, 4, 4] = -2.5                                 # a neighbour outside the interior still counts in the comparison
    assert oracle_candidates(one, 0) == [(0, 2, 5, 5)]
    n, got = ops.sift_extrema(one, 0, ctx=gtx_ctx)
    assert n == 1 and as_set(got) == [(0, 2, 5, 5)]
    one[2, 4, 4] = -3.5
    assert oracle_candidates(one, 0) == []
    assert ops.sift_extrema(one, 0, ctx=gtx_ctx)[0] == 0
    for hw in ((10, 30), (30, 10)):                     # no interior: no candidate (and no launch: a grid of 0 rows would be an error)
        flat = (np.random.default_rng(1).random((5,) + hw) * 40 - 20).astype(F)
        assert oracle_candidates(flat, 1) == []
        n, got = ops.sift_extrema(flat, 1, ctx=gtx_ctx)
        assert n == 0 and len(got) == 0


def test_extrema_count_is_the_true_total_when_the_list_is_full(gtx_ctx):
    from geotrax_amd import ops

    s = scene(0)
    want = [c for c in as_set(s["cand"]) if c[0] == 0]
    assert len(want) >= 20
    for cap in (1, len(want) // 2, len(want) - 1, len(want)):
        n, got = ops.sift_extrema(np.stack(s["dog"][0]), 0, cap=cap, ctx=gtx_ctx)
        assert n == len(want)
        got = as_set(got)
        assert len(got) == cap == len(set(got)) and set(got) <= set(want)


# --------------------------------------------------------------------------- refine
def check_refine(ctx, stack, octave, cands):
    """Per candidate: both reject or both accept, and then every field bit for bit (size: rtol 1e-6). -> the oracle's results"""
    from geotrax_amd import ops

    got = ops.sift_refine(stack, cands, octave, ctx=ctx)
    by_key = {(int(g["key_o"]), int(g["key_layer"]), int(g["key_r"]), int(g["key_c"])): g for g in got}
    assert len(by_key) == len(got)
    res = {}
    for key in map(tuple, np.asarray(cands).reshape(-1, 4).tolist()):
        want = R().refine(list(stack), octave, *key[1:])
        res[key] = want
        assert (want is None) == (key not in by_key), (key, want)
        if want is None:
            continue
        g, (x, y, word, size, resp, layer, r, c) = by_key[key], want
        assert (g["x"], g["y"], g["response"]) == (F(x), F(y), F(resp)), (key, g, want)
        assert (int(g["word"]), int(g["o"]), int(g["layer"]), int(g["r"]), int(g["c"])) == (word, octave, layer, r, c), (key, g, want)
        np.testing.assert_allclose(g["size"], F(size), rtol=1e-6)
    return res


@pytest.mark.parametrize("k", range(len(SCENES)))
def test_refine_of_every_scene_candidate_equals_the_oracle(gtx_ctx, k):
    s = scene(k)
    moved = 0
    for o, d in enumerate(s["dog"]):
        cands = [c for c in as_set(s["cand"]) if c[0] == o]
        res = check_refine(gtx_ctx, np.stack(d), o, np.array(cands, np.int32).reshape(-1, 4))
        moved += sum(1 for key, w in res.items() if w is not None and (w[5], w[6], w[7]) != key[1:])
    assert sum(1 for key in as_set(s["cand"]) if key in s["refined"]) == len(s["refined"])
    if k == 0:
        assert len(s["refined"]) >= 40 and moved >= 3


def quad_stack(c0, r0, l0, axx, ayy, ass, peak, axy=0.0):
    """D(l, r, c) = peak + (axx (c - c0)^2 + ayy (r - r0)^2 + ass (l - l0)^2) / 2 + axy (c - c0)(r - r0) on 5 x 16 x 20."""
    l, r, c = np.mgrid[0:5, 0:16, 0:20].astype(np.float64)
    return (peak + 0.5 * (axx * (c - c0) ** 2 + ayy * (r - r0) ** 2 + ass * (l - l0) ** 2) + axy * (c - c0) * (r - r0)).astype(F)


def refine_hand_cases():
    """name -> (stack, candidate (layer, r, c), the oracle trace it must give)"""
    cases = {}
    cases["singular"] = (np.full((5, 16, 20), 3.0, F), (2, 8, 10), ["singular"])
    d = np.zeros((5, 16, 20), F)
    d[2, 8, 11], d[2, 8, 9], d[2, 8, 10] = 2.0 ** 20, -2.0 ** 20, -2.0 ** -12
    cases["offset"] = (d, (2, 8, 10), ["offset"])
    cases["border"] = (quad_stack(3.8, 8, 2, -2, -2, -2, 60), (2, 8, 5), [("move", 0, 0, -1), "border"])
    cases["layer4"] = (quad_stack(10, 8, 4.3, -2, -2, -2, 60), (3, 8, 10), [("move", 1, 0, 0), "layer"])
    cases["layer0"] = (quad_stack(10, 8, -0.3, -2, -2, -2, 60), (1, 8, 10), [("move", -1, 0, 0), "layer"])
    l, r, c = np.mgrid[0:5, 0:16, 0:20].astype(np.float64)
    cases["steps"] = ((np.exp(c - 14) + 0.5 * ((r - 8) ** 2 + (l - 2) ** 2)).astype(F), (2, 8, 14), [("move", 0, 0, -1)] * 5 + ["steps"])
    cases["contrast"] = (quad_stack(10.2, 8, 2, -1, -1, -1, 3.0), (2, 8, 10), ["contrast"])
    cases["contrast_ok"] = (quad_stack(10.2, 8, 2, -1, -1, -1, 3.6), (2, 8, 10), ["accept"])
    cases["det"] = (quad_stack(10, 8, 2, 2, -2, -2, 40), (2, 8, 10), ["det"])
    cases["edge_reject"] = (quad_stack(10.1, 8.2, 2, -10.03, -1, -2, 60), (2, 8, 10), ["edge"])
    cases["edge_accept"] = (quad_stack(10.1, 8.2, 2, -9.97, -1, -2, 60), (2, 8, 10), ["accept"])
    cases["move_then_converge"] = (quad_stack(10.8, 8, 2, -2, -2, -2, 60), (2, 8, 10), [("move", 0, 0, 1), "accept"])
    cases["move_row_and_layer"] = (quad_stack(10, 7.3, 2.7, -2, -2, -2, 60), (2, 8, 10), [("move", 1, -1, 0), "accept"])
    return cases


@pytest.mark.parametrize("name", sorted(refine_hand_cases()))
def test_refine_exits_on_hand_made_stacks(gtx_ctx, name):
    stack, cand, want_trace = refine_hand_cases()[name]
    trace = []
    R().refine(list(stack), 1, *cand, trace=trace)
    assert trace == want_trace                           # the input reaches the exit it is there for
    res = check_refine(gtx_ctx, stack, 1, np.array([(1,) + cand], np.int32))
    assert (res[(1,) + cand] is not None) == (want_trace[-1] == "accept")


# --------------------------------------------------------------------------- orientation
def check_orient(ctx, g, octave):
    """Histogram within the computed bound per bin; peaks and angles of the decided keypoints. -> (keypoints, undecided, multi-peak)"""
    from geotrax_amd import ops

    n, out, hist = ops.sift_orient(g["img"], g["rec"], octave, ctx=ctx)
    assert n == len(out)
    peaks = {}
    for o in out:
        peaks.setdefault((int(o["key_o"]), int(o["key_layer"]), int(o["key_r"]), int(o["key_c"])), {})[int(o["bin"])] = o
    undecided = multi = 0
    for rec, h, hg in zip(g["rec"], g["hists"], hist):
        B = hist_bound(h)
        dev = np.abs(hg.astype(np.float64) - h["h64"])
        print(f"orient o={octave} r={h['r']} c={h['c']} radius={h['radius']} max dev/bound {np.max(dev / np.maximum(B, 1e-300)):.3f} "
              f"dev/max {dev.max() / max(h['h64'].max(), 1e-300):.2e}")
        assert (dev <= B).all(), (h["r"], h["c"], dev.max(), B[np.argmax(dev - B)])
        st = peak_status(h["h64"], B)
        key = (int(rec["key_o"]), int(rec["key_layer"]), int(rec["key_r"]), int(rec["key_c"]))
        mine = peaks.get(key, {})
        for j, o in mine.items():                        # the record carries its keypoint through unchanged
            assert all(o[f] == rec[f] for f in ("x", "y", "size", "response", "word", "o", "layer"))
        if (st < 0).any():
            undecided += 1
            continue
        assert sorted(mine) == list(np.nonzero(st == 1)[0]), (key, sorted(mine), np.nonzero(st == 1)[0])
        multi += len(mine) >= 2
        for j, o in mine.items():
            mid, half = angle_interval(h["h64"], B, j)
            a = float(o["angle"])
            assert 0.0 <= a < 360.0
            assert abs((a - mid + 540.0) % 360.0 - 180.0) <= half + 2 * float(np.spacing(F(360.0))), (key, j, a, mid, half)
    return len(g["rec"]), undecided, multi


@pytest.mark.parametrize("k", range(len(SCENES)))
def test_orientation_of_the_scene_keypoints(gtx_ctx, k):
    cases = orient_cases(k)
    hs = [(g, h) for g in cases for h in g["hists"]]
    # the conditions, from the oracle alone
    rel = max(np.max(np.maximum(np.abs(h["h32"] - h["h64"]) - h["amb"], 0.0)) / h["h64"].max() for _, h in hs)
    assert rel <= REL_HIST, rel
    und = sum(1 for _, h in hs if (peak_status(h["h64"], hist_bound(h)) < 0).any())
    assert und <= 0.05 * len(hs), (und, len(hs))
    clipped = sum(1 for g, h in hs if h["r"] - h["radius"] <= 0 or h["c"] - h["radius"] <= 0 or h["r"] + h["radius"] >= g["img"].shape[0] - 1
                  or h["c"] + h["radius"] >= g["img"].shape[1] - 1)
    larger = sum(1 for g, h in hs if min(g["img"].shape) < 2 * h["radius"] + 1)
    multi = sum(1 for _, h in hs if len(R().keypoint_angles(h["h32"])) >= 2)
    assert len(hs) >= (40, 40, 5)[k] and clipped >= (5, 5, 1)[k] and multi >= (10, 10, 0)[k] and larger >= (0, 1, 1)[k], (len(hs), clipped, larger, multi)
    tot = und_gpu = 0
    for g in cases:
        n, u, _ = check_orient(gtx_ctx, g, g["o"])
        tot, und_gpu = tot + n, und_gpu + u
    assert und_gpu == und and tot == len(hs)


def ramp(angle_deg, h=41, w=41):
    """An image whose gradient (dx, -dy as the kernel takes them) points at angle_deg everywhere."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    a = math.radians(angle_deg)
    return (100.0 + 2.0 * (math.cos(a) * x - math.sin(a) * y)).astype(F)


def one_keypoint(img, size=4.0, octave=0):
    from geotrax_amd import ops

    rec = np.zeros(1, ops.SIFT_REFINED)
    r, c = img.shape[0] // 2, img.shape[1] // 2
    rec[0] = (c, r, size, 0.05, 1 << 8, octave, 1, r, c, octave, 1, r, c)
    radius, sigma = window(size, octave)
    h64, amb = R().orientation_hist64(img, r, c, radius, sigma, ambiguous=HALF_TOL)
    return dict(o=octave, layer=1, img=img, rec=rec, hists=[dict(h32=R().orientation_hist(img, r, c, radius, sigma), h64=h64, amb=amb, radius=radius, r=r, c=c)])


def test_orientation_of_hand_made_layers(gtx_ctx):
    from geotrax_amd import ops

    # a horizontal ramp: one peak at bin 0, and the angle 360 - 10 * 0 takes the |a - 360| < 1.19e-7 -> 0 branch
    g = one_keypoint(ramp(0.0))
    h = g["hists"][0]
    assert R().keypoint_angles(h["h32"]) == [0.0] and np.argmax(h["h64"]) == 0 and h["amb"].max() == 0
    assert check_orient(gtx_ctx, g, 0) == (1, 0, 0)
    _, out, _ = ops.sift_orient(g["img"], g["rec"], 0, ctx=gtx_ctx)
    assert len(out) == 1 and out["bin"][0] == 0 and out["angle"][0] == 0.0
    # 355 degrees is bin 35.5 exactly: every pixel sits on the boundary between bins 35 and 0, the bound is the whole histogram and
    # the keypoint is undecided by construction. What holds: the histogram stays within the bound, whichever side atan2f falls
    g = one_keypoint(ramp(355.0))
    h = g["hists"][0]
    assert (peak_status(h["h64"], hist_bound(h)) < 0).any() and h["amb"].max() >= h["h64"].max()
    assert check_orient(gtx_ctx, g, 0)[:2] == (1, 1)
    # 353 degrees (bin 35.3): the raw histogram is bin 35 alone, the smoothing spreads it over 33..1 across tmp[-2..-1] / tmp[n..n+1]
    g = one_keypoint(ramp(353.0))
    h = g["hists"][0]
    assert set(np.nonzero(h["h64"] > 0)[0]) == {33, 34, 35, 0, 1} and h["amb"].max() == 0
    assert check_orient(gtx_ctx, g, 0) == (1, 0, 0)
    _, out, _ = ops.sift_orient(g["img"], g["rec"], 0, ctx=gtx_ctx)
    assert len(out) == 1 and out["bin"][0] == 35 and abs(float(out["angle"][0]) - float(R().keypoint_angles(h["h32"])[0])) < 1e-3
    # an asymmetric pair: the wrap entries are not interchangeable (tmp[-2] = bin 34, tmp[-1] = bin 35)
    y, x = np.mgrid[0:41, 0:41]
    img = np.where(y < 20, ramp(338.0), ramp(4.0) + F(7.0)).astype(F)
    g = one_keypoint(img, size=6.0)
    h = g["hists"][0]
    assert abs(h["h64"][34] - h["h64"][35]) > 0.05 * h["h64"].max()
    assert check_orient(gtx_ctx, g, 0)[:2] == (1, 0)
    # flat: no gradient, no peak, no output
    g = one_keypoint(np.full((41, 41), 50.0, F))
    assert g["hists"][0]["h64"].max() == 0 and R().keypoint_angles(g["hists"][0]["h32"]) == []
    n, out, hist = ops.sift_orient(g["img"], g["rec"], 0, ctx=gtx_ctx)
    assert n == 0 and len(out) == 0 and (hist == 0).all()
    # two equal ramps crossing: two peaks
    img = (100.0 + 2.0 * np.maximum(x - 20, 20 - y)).astype(F)      # gradient at 0 degrees right of the diagonal through the centre, 90 left of it
    g = one_keypoint(img, size=6.0)
    assert len(R().keypoint_angles(g["hists"][0]["h32"])) >= 2
    n, und, multi = check_orient(gtx_ctx, g, 0)
    assert (n, und, multi) == (1, 0, 1)
    # a window larger than the image, in octave 2
    g = one_keypoint(ramp(120.0, 9, 13), size=40.0, octave=2)
    assert g["hists"][0]["radius"] * 2 + 1 > 13 and g["hists"][0]["h64"].max() > 0
    assert check_orient(gtx_ctx, g, 2)[:2] == (1, 0)


def test_orientation_count_is_the_true_total_when_the_list_is_full(gtx_ctx):
    from geotrax_amd import ops

    g = max(orient_cases(0), key=lambda g: len(g["rec"]))
    total = sum(len(R().keypoint_angles(h["h32"])) for h in g["hists"])
    und = sum(1 for h in g["hists"] if (peak_status(h["h64"], hist_bound(h)) < 0).any())
    assert total >= 4 and und == 0
    for cap in (1, total - 1, total):
        n, out, _ = ops.sift_orient(g["img"], g["rec"], g["o"], cap=cap, ctx=gtx_ctx)
        assert n == total and len(out) == cap
        assert len({(int(o["key_r"]), int(o["key_c"]), int(o["bin"])) for o in out}) == cap


# --------------------------------------------------------------------------- descriptor
def loose_bins(u64):
    """Bins whose float64 value lies within DELTA_DESC of a half-integer, or just below the clamp's knee. Clamped bins all hold
    the knee's value, the largest; they round like any other value and get no allowance of their own."""
    knee = u64.max(axis=-1, keepdims=True)
    return (np.abs(u64 - np.floor(u64) - 0.5) <= DELTA_DESC) | ((u64 < knee) & (knee - u64 <= DELTA_DESC))


def check_describe(ctx, img, rows):
    """root 0: each value within 1 of the oracle's and different only in loose bins; root 1: RootSIFT rows where the integers agree,
    unit norm everywhere. -> (bins, loose bins)"""
    from geotrax_amd import ops

    px, py, ori, scl = (np.array(v) for v in zip(*rows))
    want = np.stack([R().descriptor(img, float(a), float(b), float(o), float(s)) for a, b, o, s in rows])
    u32 = np.stack([R().descriptor_unrounded(img, float(a), float(b), float(o), float(s)) for a, b, o, s in rows])
    u64 = np.stack([R().descriptor_unrounded64(img, float(a), float(b), float(o), float(s)) for a, b, o, s in rows])
    dev = np.abs(u32 - u64).max()
    print(f"describe {img.shape} n={len(rows)} oracle float32 vs float64: {dev:.3e}")
    assert dev <= DELTA_DESC
    loose = loose_bins(u64)
    got = ops.sift_describe(img, px, py, ori, scl, root=False, ctx=ctx)
    assert (got == np.rint(got)).all() and got.min() >= 0 and got.max() <= 255
    diff = np.abs(got - want)
    print(f"describe differing bins {int((diff > 0).sum())} of {diff.size}, loose {int(loose.sum())}")
    assert diff.max() <= 1
    assert not ((diff > 0) & ~loose).any(), np.argwhere((diff > 0) & ~loose)[:5]
    rs = ops.sift_describe(img, px, py, ori, scl, root=True, eps=1e-8, ctx=ctx)
    same = (diff == 0).all(1)
    root_want = np.sqrt(want / (want.astype(np.float64).sum(1).astype(F) + F(1e-8))[:, None]).astype(F)
    np.testing.assert_allclose(rs[same], root_want[same], rtol=1e-6)
    nz = want.sum(1) > 0
    assert (np.abs(np.linalg.norm(rs[nz].astype(np.float64), axis=1) - 1) < 1e-3).all()
    return loose.size, int(loose.sum())


@pytest.mark.parametrize("k", range(len(SCENES)))
def test_descriptors_of_the_scene_keypoints(gtx_ctx, k):
    bins = loose = n = 0
    for g in describe_cases(k):
        b, l = check_describe(gtx_ctx, g["img"], g["rows"])
        bins, loose, n = bins + b, loose + l, n + len(g["rows"])
    assert n >= (50, 50, 5)[k]
    assert loose <= 0.02 * bins, (loose, bins)


def test_descriptors_of_hand_placed_keypoints(gtx_ctx):
    """Windows cut by the image on every side, a radius clamped by the diagonal, and orientations at and next to the wrap."""
    s = scene(0)
    img = s["gauss"][1][2]
    h, w = img.shape
    rows = []
    for px, py in ((1.0, h / 2), (w - 2.0, h / 2), (1.0, 1.0), (w - 1.0, h - 1.0), (w / 2 + 0.5, 2.0), (w / 2 - 0.5, h / 2 + 0.5)):
        for ori in (0.0, 359.9999, 45.0):
            rows.append((F(px), F(py), ori, F(2.5)))
    rows.append((F(w / 2), F(h / 2), 45.0, F(200.0)))    # radius 2121 clamped to the diagonal
    rows.append((F(w / 2), F(h / 2), 359.9999, F(60.0)))
    assert R().cv_round(3 * 200.0 * 1.4142135623730951 * 2.5) > int(math.sqrt(h * h + w * w))
    bins, loose = check_describe(gtx_ctx, img, rows)
    assert loose <= 0.02 * bins
    small = s["gauss"][4][1]                             # a coarse octave: every window is larger than the image
    assert max(small.shape) <= 20
    bins, loose = check_describe(gtx_ctx, small, [(F(small.shape[1] / 2), F(small.shape[0] / 2), o, F(2.0)) for o in (0.0, 45.0, 200.0)])
    assert loose <= 0.02 * bins


def test_descriptor_of_a_flat_image_is_zero(gtx_ctx):
    """No gradient: the plain descriptor is all zeros, and so is the RootSIFT row with eps = 1e-8 (0 / 1e-8 = 0). With eps = 0 the
    oracle's 0 / 0 is NaN, and the kernel's as well."""
    from geotrax_amd import ops

    img = np.full((30, 30), 77.0, F)
    want = R().descriptor(img, 15.0, 15.0, 30.0, 2.0)
    assert (want == 0).all()
    for root, eps in ((False, 1e-8), (True, 1e-8)):
        got = ops.sift_describe(img, [15.0], [15.0], [30.0], [2.0], root=root, eps=eps, ctx=gtx_ctx)
        assert got.shape == (1, 128) and (got == 0).all()
    with np.errstate(invalid="ignore"):
        root_want = np.sqrt(want / F(F(want.astype(np.float64).sum()) + F(0.0)))
    assert np.isnan(root_want).all()
    got = ops.sift_describe(img, [15.0], [15.0], [30.0], [2.0], root=True, eps=0.0, ctx=gtx_ctx)
    assert np.isnan(got).all()
