"""`gmc_method: orb` as a stream-ordered chain (gtx_fgmc_*, csrc/gmc_feat.hip): the match-filter kernel against a host
restatement, frames submitted ahead against frame-by-frame calls and against oracle/gmc_ref.py, priming with a BGR frame in HBM
(orb and sift), restart with frames in flight. Scene and frame size of tests/test_gmc_gpu.py's feature test."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HW = (360, 640)
SHIFT = (6, 4)                     # pixels per frame (x, y) of the shifted sequence


@pytest.fixture(scope="module")
def scene_frames():
    from geotrax_amd.synth import make_scene

    sc = make_scene(seed=3, h=HW[0], w=HW[1])
    return [sc.render(t) for t in (0, 50, 100, 150)]


@pytest.fixture(scope="module")
def shifted_frames(scene_frames):
    """Four frames, each the one before it moved by SHIFT (the strip that wraps round lies inside ORB's 31-pixel border at level 0)."""
    return [np.roll(scene_frames[0], (k * SHIFT[1], k * SHIFT[0]), (0, 1)) for k in range(4)]


def _gray_half(f):
    from oracle.yolov8_ref import bgr2gray_half

    return bgr2gray_half(f)


def _restate(raw, hw):
    """ratio 0.9 + geotrax_amd.gmc.filter_matches on the matcher's raw output, numpy float64 -> (prev, cur) kept, in match
    order, and the smallest relative distance of any tested quantity from its threshold."""
    bi, d1, d2 = raw["best_idx"], raw["best_d"].astype(np.float64), raw["second_d"].astype(np.float64)
    if len(raw["prev_xy"]) < 2 or len(bi) == 0:
        return np.zeros((0, 2), np.float32), np.zeros((0, 2), np.float32), np.inf
    good = (bi >= 0) & (d1 < 0.9 * d2)
    p, q = raw["prev_xy"][bi[good]], raw["cur_xy"][good]
    d = p.astype(np.float64) - q.astype(np.float64)
    lim = np.array([0.25 * hw[1], 0.25 * hw[0]])
    margin = np.min(np.abs(np.abs(d) - lim) / lim) if len(d) else np.inf
    keep = (np.abs(d) < lim).all(1)
    if keep.sum() == 0:
        return p[:0], q[:0], margin
    dk = d[keep]
    dev, bound = dk - dk.mean(0), 2.5 * dk.std(0)
    if (bound > 0).all():
        margin = min(margin, np.min(np.abs(dev - bound) / bound))
    inl = (dev < bound).all(1)
    return p[keep][inl], q[keep][inl], margin


def test_filter_kernel_keeps_the_pairs_of_the_host_restatement(gtx_ctx, shifted_frames):
    from geotrax_amd.gmc import FeatureGMC

    g = FeatureGMC(HW, method="orb", ctx=gtx_ctx)
    assert np.array_equal(g.apply(shifted_frames[0]), np.eye(2, 3)) and not g.valid
    assert len(g.kept_pairs()[0]) == 0 and len(g.raw_matches()["best_idx"]) == 0         # a sequence's first frame: nothing was matched
    for k in (1, 2, 3):
        A = g.apply(shifted_frames[k])
        raw = g.raw_matches()
        assert len(raw["best_idx"]) > 100 and len(raw["prev_xy"]) > 100       # ORB finds ~200 keypoints on this scene at this size
        p, q, margin = _restate(raw, HW)
        print(f"frame {k}: {len(raw['best_idx'])} queries, {len(p)} kept, margin {margin:.3e}, A {A.ravel()}")
        assert margin > 1e-9                                                             # no displacement sits on a threshold: the kept set is decided
        gp, gq = g.kept_pairs()
        assert len(p) > 50
        np.testing.assert_array_equal(gp, p)
        np.testing.assert_array_equal(gq, q)
        assert g.valid and g.stats[0] == len(raw["prev_xy"]) and g.stats[1] == len(p) and g.stats[2] > 0.5 * len(p)
        assert abs(A[0, 2] - SHIFT[0]) < 1.0 and abs(A[1, 2] - SHIFT[1]) < 1.0 and abs(A[0, 0] - 1) < 0.01 and abs(A[0, 1]) < 0.01
    # an empty previous set: a flat frame has no keypoints, the frame after it nothing to match against
    flat = np.full((HW[0], HW[1], 3), 100, np.uint8)
    g.apply(flat)
    assert not g.valid and g.stats[1] == 0
    A = g.apply(shifted_frames[1])
    raw = g.raw_matches()
    assert len(raw["prev_xy"]) == 0 and len(raw["cur_xy"]) > 100
    assert np.array_equal(A, np.eye(2, 3)) and not g.valid and list(g.stats) == [0, 0, 0] and len(g.kept_pairs()[0]) == 0
    # fewer than 5 survivors: a frame with a single bright dot has a handful of keypoints at most
    dot = flat.copy()
    dot[176:182, 316:322] = 255
    A = g.apply(dot)
    raw = g.raw_matches()
    p, q, margin = _restate(raw, HW)
    print(f"dot frame: {len(raw['best_idx'])} queries, {len(p)} kept")
    assert 1 <= len(raw["best_idx"]) and len(p) < 5
    gp, gq = g.kept_pairs()
    np.testing.assert_array_equal(gp, p)
    np.testing.assert_array_equal(gq, q)
    assert np.array_equal(A, np.eye(2, 3)) and not g.valid and g.stats[1] == len(p) and g.stats[2] == 0
    g.close()


def test_frames_submitted_ahead_equal_frame_by_frame_calls_and_the_oracle(gtx_ctx, scene_frames):
    from geotrax_amd.gmc import FeatureGMC
    from oracle.gmc_ref import GmcFeatureRef

    a, b, o = FeatureGMC(HW, method="orb", ctx=gtx_ctx), FeatureGMC(HW, method="orb", ctx=gtx_ctx), GmcFeatureRef(HW, method="orb")
    grays = [_gray_half(f) for f in scene_frames]
    for gimg in grays:                                       # all frames queued before the first is collected
        a.submit_gray(gimg)
    for k, (f, gimg) in enumerate(zip(scene_frames, grays)):
        A = a.collect()
        va, sa = a.valid, a.stats.copy()
        B = b.apply(f)                                       # the same chain, one frame at a time, on a fresh object
        assert A.tobytes() == B.tobytes() and va == b.valid and np.array_equal(sa, b.stats)
        Ao = o.apply(gimg)
        assert va == (k > 0)
        if k:
            assert sa[1] == int(o.last["keep"].sum())
            np.testing.assert_allclose(A, Ao, rtol=0, atol=1e-9)     # the bound tests/test_gmc_gpu.py holds FeatureGMC to
    a.close(); b.close()


@pytest.mark.parametrize("method", ["orb", "sift"])
def test_priming_with_the_frame_before_gives_the_continuous_sequences_warps(gtx_ctx, scene_frames, method):
    from geotrax_amd.gmc import FeatureGMC

    hw = HW
    c = FeatureGMC(hw, method=method, ctx=gtx_ctx)
    want = [(c.apply(f), c.valid, c.stats.copy()) for f in scene_frames]
    c.close()
    g = FeatureGMC(hw, method=method, ctx=gtx_ctx)
    n = hw[0] * hw[1] * 3
    d_prev, d_gray = gtx_ctx.dev_alloc(n), gtx_ctx.dev_alloc(hw[0] // 2 * (hw[1] // 2))
    k = 2
    gtx_ctx.dev_upload(d_prev, np.ascontiguousarray(scene_frames[k - 1]))
    g.submit_frame_dev(d_prev, hw[0], hw[1], restart=True)   # frame k - 1 primes; its own warp is the identity
    A0 = g.collect()
    assert np.array_equal(A0, np.eye(2, 3)) and not g.valid
    for j in (k, k + 1):                                     # ... then frames k.. as the detector would hand them over
        gtx_ctx.dev_upload(d_gray, _gray_half(scene_frames[j]))
        g.submit_gray_dev(d_gray, hw[0] // 2, hw[1] // 2)
        A = g.collect()
        assert A.tobytes() == want[j][0].tobytes() and g.valid == want[j][1] and np.array_equal(g.stats, want[j][2])
    g.close()
    gtx_ctx.dev_free(d_prev); gtx_ctx.dev_free(d_gray)


def test_restart_with_frames_in_flight_order_and_errors(gtx_ctx, scene_frames):
    from geotrax_amd._lib import GtxError
    from geotrax_amd.gmc import FeatureGMC

    g = FeatureGMC(HW, method="orb", ctx=gtx_ctx)
    with pytest.raises(GtxError):
        g.collect()                                          # nothing submitted
    grays = [_gray_half(f) for f in scene_frames]
    ref = FeatureGMC(HW, method="orb", ctx=gtx_ctx)
    w01 = (ref.apply(scene_frames[0]), ref.apply(scene_frames[1]))[1]
    ref.reset_params()
    w23 = (ref.apply(scene_frames[2]), ref.apply(scene_frames[3]))[1]
    g.submit_gray(grays[0]); g.submit_gray(grays[1])
    g.reset_sequence()                                       # two frames in flight: only what is submitted from here on restarts
    g.submit_gray(grays[2]); g.submit_gray(grays[3])
    got = [(g.collect(), g.valid) for _ in range(4)]
    assert [v for _, v in got] == [False, True, False, True]
    assert np.array_equal(got[0][0], np.eye(2, 3)) and np.array_equal(got[2][0], np.eye(2, 3))
    assert got[1][0].tobytes() == w01.tobytes() and got[3][0].tobytes() == w23.tobytes()
    with pytest.raises(GtxError):
        g.collect()
    with pytest.raises(ValueError):
        g.submit_gray(np.zeros((10, 10), np.uint8))          # wrong size
    g.close(); ref.close()
