"""The resident sift / rsift stabilizer (csrc/sift_stab.cpp, Sift::extract_async, the select_* kernels, ratio_pairs) on the GPU:
  - the selection stage (gtx_op_sift_select) against a numpy restatement, exactly;
  - the stream-ordered extraction against the synchronous detector (gtx_sift_detect), bit for bit;
  - the chain against gtx_register_images (pairs, counters, matrix), bit for bit;
  - the engine against one SiftStabilizer driven frame by frame, byte for byte, and against the known camera.
Nothing here has a tolerance except the 1 px bar on the known camera, which is the one
tests/test_stabilizer_gpu.py::test_sift_detectors_recover_the_ground_truth_homography sets for the blocking path."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F = np.float32


# --------------------------------------------------------------------------- selection stage
def _key(rec):
    return ((rec["key_o"].astype(np.uint64) << np.uint64(56)) | (rec["key_layer"].astype(np.uint64) << np.uint64(48))
            | (rec["key_r"].astype(np.uint64) << np.uint64(28)) | (rec["key_c"].astype(np.uint64) << np.uint64(8)) | rec["bin"].astype(np.uint64))


def _records(n, seed, responses=(0.031, 0.07, 0.12)):
    """n oriented records with one key each, in a seeded random order; responses drawn from `responses` only."""
    from geotrax_amd import ops

    rng = np.random.default_rng(seed)
    rec = np.zeros(n, ops.SIFT_ORIENTED)
    cell = rng.permutation(4 * 40 * 60)[:n]                       # (octave, row, column) cells, each used once
    o = (cell // 2400).astype(np.int32)
    rec["o"] = rec["key_o"] = o
    rec["key_r"], rec["key_c"] = (cell % 2400) // 60 + 5, cell % 60 + 5
    rec["layer"] = rec["key_layer"] = rng.integers(1, 4, n)
    rec["bin"] = rng.integers(0, 36, n)
    scale = (1 << o).astype(F)
    rec["x"] = (rec["key_c"] + rng.uniform(-0.5, 0.5, n)).astype(F) * scale
    rec["y"] = (rec["key_r"] + rng.uniform(-0.5, 0.5, n)).astype(F) * scale
    rec["size"] = rng.uniform(2.0, 9.0, n).astype(F) * scale
    rec["angle"] = rng.uniform(0.0, 360.0, n).astype(F)
    rec["angle"][::7] = 0.0                                       # 360 - 0 = 360 -> the snap to 0
    rec["response"] = F(responses)[rng.integers(0, len(responses), n)]
    rec["word"] = o + (rec["layer"] << 8) + (rng.integers(0, 256, n).astype(np.int32) << 16)
    return rec


def _masked(rec, rects):
    x = (rec["x"].astype(np.float64) * 0.5).astype(F)
    y = (rec["y"].astype(np.float64) * 0.5).astype(F)
    ix, iy = (x + F(0.5)).astype(np.int32), (y + F(0.5)).astype(np.int32)        # (int)(v + 0.5f)
    hit = np.zeros(len(rec), bool)
    for x1, y1, x2, y2 in rects:
        hit |= (ix >= x1) & (ix <= x2) & (iy >= y1) & (iy <= y2)
    return hit


def _select_ref(rec, k, rects=()):
    """lexsort on (-response, key), cut, sort by key, mask -> the records kept, in output order, and their output rows."""
    from geotrax_amd import ops

    key = _key(rec)
    order = np.lexsort((key, -rec["response"].astype(np.float64)))[:k]
    order = order[np.argsort(key[order], kind="stable")]
    order = order[~_masked(rec[order], rects)]
    r = rec[order]
    scale = 1.0 / (1 << r["o"]).astype(np.float64)
    fin = np.zeros(len(r), ops.SIFT_FINAL)
    fin["px"], fin["py"] = r["x"].astype(np.float64) * scale, r["y"].astype(np.float64) * scale
    a = 360.0 - r["angle"].astype(np.float64)
    a[np.abs(a - 360.0) < 1.19e-7] = 0.0
    fin["ori"], fin["scl"], fin["o"], fin["layer"] = a, r["size"].astype(np.float64) * scale * 0.5, r["o"], r["layer"]
    kp5 = np.stack([(r["x"].astype(np.float64) * 0.5).astype(F), (r["y"].astype(np.float64) * 0.5).astype(F),
                    (r["size"].astype(np.float64) * 0.5).astype(F), r["angle"], r["response"]], 1).astype(F)
    octave = (r["word"] & ~np.int32(255)) | ((r["o"] - 1) & 255)
    return dict(n=len(r), final=fin, xy=kp5[:, :2].copy(), kp5=kp5, octave=octave.astype(np.int32))


def _same(got, want):
    assert got["n"] == want["n"]
    for f in ("final", "xy", "kp5", "octave"):
        assert got[f].tobytes() == want[f].tobytes(), f


@pytest.mark.parametrize("n,k", [(0, 5), (1, 5), (199, 200), (200, 200), (201, 200), (5000, 2000)])
def test_select_keeps_the_strongest_in_key_order(gtx_ctx, n, k):
    """Three distinct responses only, so the cut falls inside a tie whenever it cuts at all; two list orders, the same bytes."""
    from geotrax_amd import ops

    rec = _records(n, seed=n + 1)
    want = _select_ref(rec, k)
    assert want["n"] == min(n, k)
    got = ops.sift_select(rec, k, ctx=gtx_ctx)
    _same(got, want)
    again = ops.sift_select(rec[np.random.default_rng(5).permutation(n)], k, ctx=gtx_ctx)
    _same(again, got)


def test_select_with_all_responses_equal_is_a_cut_by_key(gtx_ctx):
    from geotrax_amd import ops

    rec = _records(1500, seed=9, responses=(0.05,))
    want = _select_ref(rec, 700)
    got = ops.sift_select(rec, 700, ctx=gtx_ctx)
    _same(got, want)
    _same(ops.sift_select(rec[::-1].copy(), 700, ctx=gtx_ctx), got)


def test_select_mask_edges_rounding_and_order(gtx_ctx):
    """The mask is tested on (int)(v + 0.5f) of the working-resolution position, on inclusive edges, after the cut."""
    from geotrax_amd import ops

    rec = _records(6, seed=2, responses=(0.05,))
    rec["o"] = rec["key_o"] = 0
    rec["key_r"], rec["key_c"] = 10, np.arange(6) + 10
    rec["y"] = 40.0                                                # working y = 20
    rec["x"] = [21.0, 20.98, 19.0, 60.0, 61.0, 80.0]               # working x = 10.5 -> 11, 10.49 -> 10, 9.5 -> 10, 30 -> 30, 30.5 -> 31, 40 -> 40
    rounded = [11, 10, 10, 30, 31, 40]
    assert ((rec["x"].astype(np.float64) * 0.5).astype(F) + F(0.5)).astype(np.int32).tolist() == rounded
    for rects, dropped in (([[0, 0, 10, 100]], [1, 2]),            # x2 = 10 inclusive: 10.49 and 9.5 go, 10.5 (-> 11) stays
                           ([[11, 20, 30, 20]], [0, 3]),           # x1 = 11 and x2 = 30 inclusive, y1 = y2 = 20 inclusive
                           ([[11, 21, 30, 40]], []),               # one row below: nobody
                           ([[31, 0, 39, 100], [0, 0, 9, 100]], [4]),
                           ([[0, 0, 1000, 1000]], [0, 1, 2, 3, 4, 5])):    # everything: 0 keypoints
        want = _select_ref(rec, 6, rects)
        assert want["n"] == 6 - len(dropped)
        got = ops.sift_select(rec, 6, np.array(rects, np.int32), ctx=gtx_ctx)
        _same(got, want)
    # the mask comes after retainBest: of the 3 strongest one is masked, and no fourth takes its place
    rec["response"] = [0.9, 0.8, 0.7, 0.1, 0.1, 0.1]
    got = ops.sift_select(rec, 3, np.array([[11, 0, 11, 100]], np.int32), ctx=gtx_ctx)
    _same(got, _select_ref(rec, 3, [[11, 0, 11, 100]]))
    assert got["n"] == 2 and got["kp5"][:, 4].tolist() == [F(0.8), F(0.7)]


# --------------------------------------------------------------------------- scenes
def _blob_field(h, w, seed, n=None):
    rng = np.random.default_rng(seed)
    n = n or (h * w) // 160
    return dict(cx=rng.uniform(0, w, n), cy=rng.uniform(0, h, n), s=rng.uniform(1.2, 5.0, n), a=rng.uniform(-90, 90, n))


def _render(field, h, w, Hinv=None):
    """u8 gray view [h, w] of the blob field; Hinv maps this view's pixels to the field's coordinates."""
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    if Hinv is not None:
        d = Hinv[2, 0] * xs + Hinv[2, 1] * ys + Hinv[2, 2]
        xs, ys = (Hinv[0, 0] * xs + Hinv[0, 1] * ys + Hinv[0, 2]) / d, (Hinv[1, 0] * xs + Hinv[1, 1] * ys + Hinv[1, 2]) / d
    img = np.full((h, w), 120.0)
    for cx, cy, s, a in zip(field["cx"], field["cy"], field["s"], field["a"]):
        img += a * np.exp(-((xs - cx) ** 2 + (ys - cy) ** 2) / (2 * s * s))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _gray(kind):
    if kind == "small":
        return _render(_blob_field(96, 128, 11), 96, 128)
    if kind == "wide":
        return _render(_blob_field(180, 320, 12), 180, 320)
    if kind == "tiled":                                           # 2 x 2 tiling of one patch: equal responses really occur
        return np.tile(_render(_blob_field(48, 64, 13, n=40), 48, 64), (2, 2))
    if kind == "flat":
        return np.full((96, 128), 90, np.uint8)
    if kind == "view":                                            # the "wide" scene under a small known homography
        return _render(_blob_field(180, 320, 12), 180, 320, _VIEW_H)
    raise KeyError(kind)


_VIEW_H = np.array([[1.01, 0.012, -3.0], [-0.01, 0.995, 2.5], [1.5e-5, -1e-5, 1.0]])      # view pixels -> scene ("wide") pixels


class _DevGray:
    def __init__(self, ctx, img):
        self.ctx, self.h, self.w = ctx, img.shape[0], img.shape[1]
        self.p = ctx.dev_alloc(img.nbytes)
        ctx.dev_upload(self.p, np.ascontiguousarray(img))

    def args(self):
        return self.p, self.h, self.w

    def free(self):
        self.ctx.dev_free(self.p)


def _stab(ctx, gray_hw, **kw):
    from geotrax_amd.sift_stabilizer import SiftStabilizer

    base = dict(detector_name="rsift", max_features=2000, ref_multiplier=1.0, filter_ratio=0.75, ransac_epipolar_threshold=2.0, ransac_max_iter=5000,
                seed=0, sift_enable_precise_upscale=True, ctx=ctx)
    base.update(kw)
    return SiftStabilizer((2 * gray_hw[0], 2 * gray_hw[1]), **base)


def _bgr(gray):
    return np.repeat(gray[..., None], 3, 2)


# --------------------------------------------------------------------------- extraction against the synchronous detector
@pytest.mark.parametrize("root", [1, 0])
@pytest.mark.parametrize("kind", ["small", "wide", "tiled", "flat"])
def test_extract_async_equals_the_synchronous_detector(gtx_ctx, kind, root):
    from geotrax_amd.registration import Sift

    gray = _gray(kind)
    sift = Sift(gray.shape, ctx=gtx_ctx)
    full = sift.detect_and_compute(_bgr(gray), max_features=60000, root=bool(root))
    n_all = full["count"]
    assert (n_all == 0) == (kind == "flat")
    if kind == "tiled":
        assert len(np.unique(full["response"])) < n_all          # equal responses do occur
    dev = _DevGray(gtx_ctx, gray)
    try:
        for k in ([8] if n_all == 0 else [n_all + 50, max(n_all // 3, 4)]):
            want = sift.detect_and_compute(_bgr(gray), max_features=k, root=bool(root))
            st = _stab(gtx_ctx, gray.shape, detector_name="rsift" if root else "sift", max_features=k)
            try:
                st.set_ref_gray_dev(*dev.args())
                st.stabilize_gray_dev(*dev.args())
                cnt = st.counters()
                assert cnt[2] == n_all and cnt[3] == min(n_all, k) == want["count"]      # k below n_all: the selection really cuts
                for which in ("ref", "cur"):
                    got = st.keypoints(which)
                    assert len(got["kp5"]) == want["count"]
                    w5 = np.concatenate([want["xy"], want["size"][:, None], want["angle"][:, None], want["response"][:, None]], 1).astype(F)
                    assert got["kp5"].tobytes() == w5.tobytes()
                    assert got["octave"].tobytes() == want["octave"].tobytes()
                    assert got["desc"].tobytes() == want["desc"].tobytes()
                assert st.get_cur_num_keypoints() == (want["count"], want["count"])
            finally:
                st.close()
    finally:
        dev.free()
        sift.close()


# --------------------------------------------------------------------------- chain against gtx_register_images
def test_chain_equals_register_images(gtx_ctx):
    from geotrax_amd import ops
    from geotrax_amd.registration import Sift, register_once

    ref, cur = _gray("wide"), _gray("view")
    K, ratio = 2000, 0.75
    dref, dcur, dflat = _DevGray(gtx_ctx, ref), _DevGray(gtx_ctx, cur), _DevGray(gtx_ctx, np.full_like(ref, 77))
    st = _stab(gtx_ctx, ref.shape, max_features=K, filter_ratio=ratio)
    sift = Sift(ref.shape, ctx=gtx_ctx)
    try:
        st.set_ref_gray_dev(*dref.args())
        st.stabilize_gray_dev(*dcur.args())
        # the pair list, rebuilt from the synchronous detector, the matcher hook and the ratio rule
        kq = sift.detect_and_compute(_bgr(cur), max_features=K, root=True)
        kt = sift.detect_and_compute(_bgr(ref), max_features=K, root=True)
        i1, i2, d1, d2 = ops.match_2nn(kq["desc"], kt["desc"], ctx=gtx_ctx)[:4]
        ok = (i1 >= 0) & (i2 >= 0) & (d1 < F(ratio) * d2)
        want_pairs = np.concatenate([kq["xy"][ok], kt["xy"][i1[ok]]], 1).astype(F)
        assert len(want_pairs) > 50
        assert st.pairs().tobytes() == want_pairs.tobytes()
        H, stats, _ = register_once(_bgr(cur), _bgr(ref), max_features=K, filter_ratio=ratio, ransac_epipolar_threshold=2.0, ransac_max_iter=5000,
                                    ransac_confidence=0.999999, rsift_eps=1e-8, seed=0, ctx=gtx_ctx)
        assert H is not None and st.registered
        # gtx_register_images counts (source = current, destination = reference, pairs, inliers)
        assert (st.get_cur_num_keypoints()[1], st.get_cur_num_keypoints()[0], st.get_cur_num_matches(), st.get_cur_inliers_count()) == tuple(int(v) for v in stats)
        assert st.working_matrix().tobytes() == H.tobytes()
        # and it is the camera: scene = _VIEW_H(view), to a fraction of a pixel of the working image
        g = np.array([[0, 0, 1], [319, 0, 1], [0, 179, 1], [319, 179, 1.0]]).T
        a, b = st.working_matrix() @ g, _VIEW_H @ g
        assert np.abs(a[:2] / a[2] - b[:2] / b[2]).max() < 0.5
        last = st.get_cur_trans_matrix()
        st.stabilize_gray_dev(*dflat.args())                          # nothing to register: counters filled, no error, last known transform
        assert not st.registered and st.get_cur_num_keypoints() == (len(kt["xy"]), 0) and st.get_cur_num_matches() == 0
        assert st.get_cur_inliers_count() == 0 and len(st.pairs()) == 0
        assert np.array_equal(st.get_cur_trans_matrix(), last) and st.get_cur_trans_matrix(raw=True) is None
    finally:
        st.close()
        sift.close()
        for d in (dref, dcur, dflat):
            d.free()


def test_vehicle_mask_drops_kept_keypoints_only(gtx_ctx):
    gray = _gray("wide")
    dev = _DevGray(gtx_ctx, gray)
    boxes = np.array([[200.0, 120.0, 90.0, 60.0], [500.0, 250.0, 120.0, 100.0], [630.0, 350.0, 60.0, 40.0]], F)     # xywh, frame pixels (2 x working)
    margin, K = 0.15, 150
    rects = []
    for cx, cy, w, h in boxes.astype(np.float64):
        w, h = F(w) * (F(1) + F(margin)), F(h) * (F(1) + F(margin))
        x1, y1 = int(np.floor((F(cx) - w / 2) * F(0.5))), int(np.floor((F(cy) - h / 2) * F(0.5)))
        x2, y2 = int(np.ceil((F(cx) + w / 2) * F(0.5))), int(np.ceil((F(cy) + h / 2) * F(0.5)))
        rects.append([max(x1, 0), max(y1, 0), min(x2, gray.shape[1] - 1), min(y2, gray.shape[0] - 1)])
    st = _stab(gtx_ctx, gray.shape, max_features=K, mask_use=True, mask_margin_ratio=margin)
    try:
        st.set_ref_gray_dev(*dev.args())
        st.stabilize_gray_dev(*dev.args())
        plain = st.keypoints("cur")
        assert st.counters()[2] > K == len(plain["kp5"])              # the selection cuts
        st.stabilize_gray_dev(*dev.args(), boxes)
        got = st.keypoints("cur")
        ix, iy = (plain["kp5"][:, 0] + F(0.5)).astype(np.int32), (plain["kp5"][:, 1] + F(0.5)).astype(np.int32)
        hit = np.zeros(K, bool)
        for x1, y1, x2, y2 in rects:
            hit |= (ix >= x1) & (ix <= x2) & (iy >= y1) & (iy <= y2)
        assert 0 < hit.sum() < K
        for f in ("kp5", "octave", "desc"):
            assert got[f].tobytes() == plain[f][~hit].tobytes(), f    # the unmasked run's set minus the masked ones, in order
        assert st.get_cur_num_keypoints()[1] == K - hit.sum()
        st.set_ref_gray_dev(*dev.args(), boxes)                       # the reference is masked by the same rule
        assert st.keypoints("ref")["kp5"].tobytes() == plain["kp5"][~hit].tobytes()
    finally:
        st.close()
        dev.free()


# --------------------------------------------------------------------------- engine
HW = (720, 1280)


def _grid_err(Ha, Hb, hw):
    ys, xs = np.meshgrid(np.linspace(0, hw[0] - 1, 9), np.linspace(0, hw[1] - 1, 16), indexing="ij")
    p = np.stack([xs.ravel(), ys.ravel(), np.ones(xs.size)])
    a, b = Ha @ p, Hb @ p
    return np.abs(a[:2] / a[2] - b[:2] / b[2]).max()


def test_engine_runs_rsift_pipelined_with_the_results_of_the_serial_loop(gtx_ctx):
    from geotrax_amd.detector import Detector
    from geotrax_amd.engine import ExtractEngine
    from geotrax_amd.sift_stabilizer import SiftStabilizer
    from geotrax_amd.synth import make_scene
    from geotrax_amd.weights import calibrate_cls_bias, synthetic_yolov8

    sc = make_scene(seed=3, h=HW[0], w=HW[1])
    times = [0, 10, 20, 30, None, 40, 50, 60]                          # None: a flat frame
    frames = [np.full((HW[0], HW[1], 3), 90, np.uint8) if t is None else sc.render(t) for t in times]
    kw = dict(imgsz=640, conf=0.25, iou=0.7, max_det=300, classes=[0, 1, 2, 3], agnostic_nms=True, half=True, rect=True)
    w = synthetic_yolov8(seed=2, nc=4)
    det = Detector(w, HW, ctx=gtx_ctx, **kw)
    det.detect(frames[0])
    w = calibrate_cls_bias(w, det.raw_output(logits=True)[:, 4:], 0.25, 40)
    det.close()
    stab_kw = dict(detector_name="rsift", downsample_ratio=0.5, max_features=3000, ref_multiplier=2.0, filter_ratio=0.75, ransac_epipolar_threshold=2.0,
                   ransac_max_iter=5000, mask_use=True, mask_margin_ratio=0.15, matcher_name="bf", filter_type="ratio",
                   transformation_type="projective", clahe=False, sift_enable_precise_upscale=True)
    batches = [frames[i:i + 2] for i in range(0, len(frames), 2)]

    def run(stab_streams):
        eng = ExtractEngine(w, HW, kw, None, stab_kw, batch=2, det_streams=2, stab_streams=stab_streams)
        try:
            assert all(isinstance(s, SiftStabilizer) for s in eng.stabs) and len(eng.stabs) == stab_streams
            return [(r.index, None if r.xywh is None else r.xywh.copy(), None if r.H is None else r.H.copy(),
                     None if r.xywh_stab is None else r.xywh_stab.copy()) for r in eng.run(batches)]
        finally:
            eng.close()

    def same(a, b):
        return (a is None and b is None) or (a is not None and b is not None and a.dtype == b.dtype and a.tobytes() == b.tobytes())

    four, one = run(4), run(1)
    # a block SiftStabilizer does not run keeps Stabilizer (rsift at ratio 1.0: its host-frame path), as does an explicit stab_cls
    from geotrax_amd.stabilizer import Stabilizer

    for over, kwargs in ((dict(downsample_ratio=1.0), {}), ({}, dict(stab_cls=Stabilizer))):
        eng = ExtractEngine(w, HW, kw, None, dict(stab_kw, **over), batch=2, det_streams=1, stab_streams=2, **kwargs)
        try:
            assert [type(s) for s in eng.stabs] == [Stabilizer, Stabilizer]
        finally:
            eng.close()
    assert [r[0] for r in four] == list(range(len(frames)))
    for a, b in zip(four, one):
        assert same(a[1], b[1]) and same(a[2], b[2]) and same(a[3], b[3])
    # the known camera on the 9 x 16 grid, the flat frame on the last known transform
    assert four[0][2] is None
    for (i, _, H, _), t in zip(four, times):
        if i == 0:
            continue
        if t is None:
            assert same(H, four[i - 1][2])
        else:
            assert _grid_err(H, np.linalg.inv(sc.camera(t)), HW) < 1.0, (i, t)
    # one SiftStabilizer, frame by frame, on the same gray images and boxes
    det = Detector(w, HW, ctx=gtx_ctx, **kw)
    st = SiftStabilizer(HW, ctx=gtx_ctx, **stab_kw)
    try:
        for (i, xywh, H, xywh_stab), f in zip(four, frames):
            det.detect(f)
            g = det.gray_dptr(0)
            if i == 0:
                st.set_ref_gray_dev(g[0], g[1], g[2], xywh)
                continue
            st.stabilize_gray_dev(g[0], g[1], g[2], xywh)
            assert st.registered == (times[i] is not None)
            assert same(st.get_cur_trans_matrix(), H)
            if xywh is not None:
                assert same(st.transform_cur_boxes(), xywh_stab)
        assert st.last_ms() > 0
    finally:
        st.close()
        det.close()
