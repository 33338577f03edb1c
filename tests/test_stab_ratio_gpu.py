"""ORB stabilization at any downsample_ratio on the GPU: the BGR -> working-gray kernel alone (gtx_op_gray_resize) bit for bit
against oracle/yolov8_ref.py::resize_linear_u8 over oracle/stabilo_ref.py::bgr2gray, the stabilizer at ratios 0.75 and 0.4 against
the oracle chain composed here (StabilizerRef with that gray image), the device-gray entries against the host-frame ones, the
engine fed with device batches against the blocking per-frame calls, and the `stable` preset through the read-ahead feeder."""
import ctypes as C
import logging

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
logger = logging.getLogger("test_stab_ratio")

CFG = dict(max_features=600, ref_multiplier=2.0, filter_ratio=0.9, ransac_threshold=2.0, mask_use=True, mask_margin_ratio=0.15,
           fast_threshold=20, n_levels=8, scale_factor=1.2, seed=0)
HW = (720, 1280)                      # tests/test_stabilizer_gpu.py's scene and frame size


def working_gray_ref(frame, ratio):
    """cv2.cvtColor(BGR2GRAY) then cv2.resize(fx = fy = ratio, INTER_LINEAR) as the project restates them, composed: gray rounded to
    u8 first, then the 11-bit fixed-point bilinear resize to the working size."""
    from oracle.stabilo_ref import bgr2gray
    from oracle.yolov8_ref import resize_linear_u8

    from geotrax_amd.stabilizer import working_size

    gh, gw = working_size(frame.shape[:2], ratio)
    return resize_linear_u8(bgr2gray(frame, False)[..., None], gh, gw)[..., 0]


def _inputs(h, w, seed):
    rng = np.random.default_rng(seed)
    ramp_x = np.broadcast_to((np.arange(w) * 255 // max(w - 1, 1)).astype(np.uint8)[None, :, None], (h, w, 3))
    ramp_y = np.broadcast_to((np.arange(h) * 255 // max(h - 1, 1)).astype(np.uint8)[:, None, None], (h, w, 3))
    return dict(noise=rng.integers(0, 256, (h, w, 3), dtype=np.uint8), white=np.full((h, w, 3), 255, np.uint8),
                ramp_x=np.ascontiguousarray(ramp_x), ramp_y=np.ascontiguousarray(ramp_y))


# frame (h, w), ratio, working (gh, gw): odd sizes with gw no multiple of 4; a ragged tail inside a row; more than one 256-lane
# block along x and the source pixels bilinear skips at 1/4; every tap clamped at a border
KERNEL_CASES = [((37, 50), 0.6, (22, 30)), ((37, 50), 0.3, (11, 15)), ((37, 50), 0.9, (33, 45)), ((64, 260), 0.75, (48, 195)),
                ((130, 1030), 0.25, (32, 258)), ((9, 9), 0.2, (2, 2))]


@pytest.mark.parametrize("hw,ratio,ghw", KERNEL_CASES)
def test_gray_resize_kernel_equals_the_oracle_bit_for_bit(gtx_ctx, hw, ratio, ghw):
    from geotrax_amd import ops

    for name, f in _inputs(hw[0], hw[1], seed=hw[1]).items():
        want = working_gray_ref(f, ratio)
        assert want.shape == ghw
        got = ops.gray_resize(f, ratio, ctx=gtx_ctx)
        np.testing.assert_array_equal(got, want, err_msg=name)
        if name == "white":
            assert (got == 255).all()                        # the two weights of a tap pair sum to 2048


def _gray_resize_at_offset(ctx, f, ratio, off):
    """gtx_op_gray_resize_dev into a device buffer that starts `off` bytes behind its allocation, between guard bytes; returns the
    image and checks that nothing beside it was written."""
    from geotrax_amd import _lib
    from geotrax_amd.stabilizer import working_size

    h, w = f.shape[:2]
    gh, gw = working_size((h, w), ratio)
    pad = np.full(gh * gw + off + 8, 0xA5, np.uint8)
    src, dst = ctx.dev_alloc(f.nbytes), ctx.dev_alloc(pad.nbytes)
    try:
        ctx.dev_upload(src, f)
        ctx.dev_upload(dst, pad)
        _lib.check(ctx.lib.gtx_op_gray_resize_dev(ctx.handle, C.c_void_p(src), h, w, float(ratio), C.c_void_p(dst + off), gh, gw))
        ctx.synchronize()
        ctx.dev_download(pad, dst)
    finally:
        ctx.dev_free(src)
        ctx.dev_free(dst)
    assert (pad[:off] == 0xA5).all() and (pad[off + gh * gw:] == 0xA5).all(), "bytes beside the image were written"
    return pad[off:off + gh * gw].reshape(gh, gw).copy()


@pytest.mark.parametrize("hw,ratio", [((64, 260), 0.75), ((37, 50), 0.6), ((130, 1030), 0.25)])
def test_gray_resize_into_an_unaligned_buffer(gtx_ctx, hw, ratio):
    """The output starts one, two and three bytes behind an allocation: no row start is dword-aligned where the kernel would like
    it, the scalar path writes the same bytes and nothing beside the image."""
    f = _inputs(hw[0], hw[1], seed=7)["noise"]
    want = working_gray_ref(f, ratio)
    for off in (1, 2, 3):
        np.testing.assert_array_equal(_gray_resize_at_offset(gtx_ctx, f, ratio, off), want)


def test_gray_resize_keeps_the_kernels_of_one_half_and_one(gtx_ctx):
    from oracle.stabilo_ref import bgr2gray

    from geotrax_amd import ops

    f = _inputs(37, 51, seed=1)["noise"]
    np.testing.assert_array_equal(ops.gray_resize(f, 1.0, ctx=gtx_ctx), bgr2gray(f, False))
    np.testing.assert_array_equal(ops.gray_resize(f, 0.5, ctx=gtx_ctx), bgr2gray(f[:36, :50], True))
    np.testing.assert_array_equal(_gray_resize_at_offset(gtx_ctx, f, 1.0, 1), bgr2gray(f, False))


@pytest.fixture(scope="module")
def seq():
    from geotrax_amd.synth import make_scene

    sc = make_scene(seed=3, h=HW[0], w=HW[1])
    return sc, {t: sc.render(t) for t in (0, 40)}


def _grid_err(Ha, Hb, hw):
    ys, xs = np.meshgrid(np.linspace(0, hw[0] - 1, 9), np.linspace(0, hw[1] - 1, 16), indexing="ij")
    p = np.stack([xs.ravel(), ys.ravel(), np.ones(xs.size)])
    a, b = Ha @ p, Hb @ p
    return np.abs(a[:2] / a[2] - b[:2] / b[2]).max()


def _make(gtx_ctx, ratio, **over):
    from geotrax_amd.stabilizer import Stabilizer

    kw = dict(downsample_ratio=ratio, max_features=CFG["max_features"], ref_multiplier=CFG["ref_multiplier"], filter_ratio=CFG["filter_ratio"],
              ransac_epipolar_threshold=CFG["ransac_threshold"], mask_use=CFG["mask_use"], mask_margin_ratio=CFG["mask_margin_ratio"],
              seed=CFG["seed"], ctx=gtx_ctx)
    kw.update(over)
    return Stabilizer(HW, **kw)


@pytest.mark.parametrize("ratio", [0.75, 0.4])
def test_stabilizer_equals_the_oracle_chain_at_other_ratios(gtx_ctx, seq, ratio):
    """Keypoints, descriptors and matches are integer work on the working gray image: the oracle's, bit for bit (the mask
    rectangles and the 1 / ratio keypoint rescale included). The homography is the oracle's within the bound
    tests/test_stabilizer_gpu.py uses. Against the scene's true camera the GPU estimate may be at most 1e-3 px worse than the
    oracle's own error at that ratio, which is printed (nobody had measured it)."""
    from oracle.stabilo_ref import StabilizerRef

    class RatioRef(StabilizerRef):
        def _gray(self, frame_bgr):
            return working_gray_ref(frame_bgr, self.cfg["downsample_ratio"])

    sc, fr = seq
    st = _make(gtx_ctx, ratio)
    ref = RatioRef(dict(CFG, downsample_ratio=ratio), HW, n_hyp=2048)
    b0, b1 = sc.boxes(0), sc.boxes(40)
    st.set_ref_frame(fr[0], b0)
    ref.set_ref_frame(fr[0], b0)
    st.stabilize(fr[40], b1)
    H_ref, n_inl = ref.stabilize(fr[40], b1)
    for which, o in (("ref", ref.ref), ("cur", ref.cur)):
        g = st.keypoints(which)
        assert len(g["bin"]) == len(o["bin"]) > 200, which
        np.testing.assert_array_equal(g["level"], o["level"])
        np.testing.assert_array_equal(g["xy"], o["xy"])
        np.testing.assert_array_equal(g["desc"], o["desc"])
    q, t, d = st.matches()
    np.testing.assert_array_equal(q, ref.m[0])
    np.testing.assert_array_equal(t, ref.m[1])
    np.testing.assert_array_equal(d, ref.m[2])
    assert len(q) > 50
    H = st.get_cur_trans_matrix()
    assert H is not None and H_ref is not None
    assert _grid_err(H, H_ref, HW) < 1e-3
    assert abs(st.get_cur_inliers_count() - n_inl) <= 2
    truth = np.linalg.inv(sc.camera(40))
    e_gpu, e_ref = _grid_err(H, truth, HW), _grid_err(H_ref, truth, HW)
    print(f"ratio {ratio}: grid error against the true camera: GPU {e_gpu:.4f} px, oracle {e_ref:.4f} px; {len(q)} matches, {n_inl} inliers")
    assert e_gpu <= e_ref + 1e-3


def test_device_gray_equals_host_frames(gtx_ctx, seq):
    """Ratio 0.75: gtx_op_gray_resize_dev into a buffer, then set_ref_gray_dev / stabilize_gray_dev, against set_ref_frame / stabilize
    on the host frames: the same transform bytes and the same matches. A gray image of another size is refused."""
    from geotrax_amd import _lib
    from geotrax_amd.stabilizer import working_size

    sc, fr = seq
    ratio = 0.75
    gh, gw = working_size(HW, ratio)
    b0, b1 = sc.boxes(0), sc.boxes(40)
    host = _make(gtx_ctx, ratio)
    host.set_ref_frame(fr[0], b0)
    host.stabilize(fr[40], b1)
    dev = _make(gtx_ctx, ratio)
    d_frame, d_gray = gtx_ctx.dev_alloc(fr[0].nbytes), gtx_ctx.dev_alloc(gh * gw)
    try:
        def gray_of(f):
            gtx_ctx.dev_upload(d_frame, f)
            _lib.check(gtx_ctx.lib.gtx_op_gray_resize_dev(gtx_ctx.handle, C.c_void_p(d_frame), HW[0], HW[1], ratio, C.c_void_p(d_gray), gh, gw))
            gtx_ctx.synchronize()

        gray_of(fr[0])
        for bad in ((gh - 1, gw), (gh, gw + 1), (HW[0] // 2, HW[1] // 2), HW):
            with pytest.raises(_lib.GtxError, match="expected"):
                dev.set_ref_gray_dev(d_gray, bad[0], bad[1], b0)
        dev.set_ref_gray_dev(d_gray, gh, gw, b0)
        gray_of(fr[40])
        with pytest.raises(_lib.GtxError, match="expected"):
            dev.stabilize_gray_dev(d_gray, gh, gw - 1, b1)
        with pytest.raises(_lib.GtxError, match="expected"):
            dev.submit_gray_dev(d_gray, gh + 1, gw, b1)
        dev.stabilize_gray_dev(d_gray, gh, gw, b1)
    finally:
        gtx_ctx.dev_free(d_frame)
        gtx_ctx.dev_free(d_gray)
    assert host.get_cur_trans_matrix() is not None
    assert dev.get_cur_trans_matrix().tobytes() == host.get_cur_trans_matrix().tobytes()
    for a, b in zip(dev.matches(), host.matches()):
        np.testing.assert_array_equal(a, b)
    assert dev.get_cur_num_keypoints() == host.get_cur_num_keypoints()
    with pytest.raises(_lib.GtxError, match=r"\(0, 1\]"):
        _make(gtx_ctx, 1.5)
    with pytest.raises(_lib.GtxError, match=r"\(0, 1\]"):
        _make(gtx_ctx, 0.0)
    with pytest.raises(_lib.GtxError, match="too small"):
        _make(gtx_ctx, 0.05)                                 # 36 x 64 working pixels: below the keypoint border


@pytest.mark.parametrize("ratio,container", [(1.0, "y4m"), (0.75, "npy")])
def test_engine_device_batches_equal_blocking_calls(gtx_ctx, tmp_path, ratio, container):
    """ExtractEngine fed with the read-ahead feeder's DeviceBatches (no frame ever on the host side of the engine) against the
    blocking loop that detects each frame and calls Stabilizer.set_ref_frame / stabilize with host frames: xywh, H and xywh_stab
    byte for byte, the last-known-transform rule on the flat frame included."""
    from test_extract_gpu import H, IMGSZ, W

    from geotrax_amd.detector import Detector
    from geotrax_amd.engine import ExtractEngine, gray_route
    from geotrax_amd.feeder import FrameFeeder
    from geotrax_amd.frames import open_source, write_y4m
    from geotrax_amd.stabilizer import Stabilizer
    from geotrax_amd.synth import make_scene
    from geotrax_amd.weights import calibrate_cls_bias, synthetic_yolov8

    scene = make_scene(seed=6, h=H, w=W)
    frames = [scene.render(10 * k, 150) for k in range(7)]
    frames.insert(5, np.full((H, W, 3), 127, np.uint8))         # no texture: no transform of its own, the last known one is reported
    if container == "y4m":
        src = tmp_path / "clip.y4m"
        write_y4m(src, frames)
        r = open_source(src)
        frames = [r.read()[1].bgr() for _ in range(len(frames))]    # what the decoder hands on (I420 -> BGR: device = host, tests/test_y4m*.py)
        r.release()
    else:
        src = tmp_path / "clip.npy"
        np.save(src, np.stack(frames))
    kw = dict(imgsz=IMGSZ, conf=0.25, iou=0.7, max_det=300, classes=[0, 1, 2, 3], agnostic_nms=True, half=True, rect=True)
    w = synthetic_yolov8(seed=1, nc=4)
    det = Detector(w, (H, W), ctx=gtx_ctx, **kw)
    det.detect(frames[0])
    w = calibrate_cls_bias(w, det.raw_output(logits=True)[:, 4:], 0.25, 60)
    det.close()
    stab_kw = dict(max_features=500, downsample_ratio=ratio)
    assert gray_route(stab_kw) == "frame"
    det, st = Detector(w, (H, W), ctx=gtx_ctx, **kw), Stabilizer((H, W), ctx=gtx_ctx, **stab_kw)
    want = []
    for i, f in enumerate(frames):
        d = det.detect(f)
        xywh = d.xywh if len(d) else None
        if i == 0:
            st.set_ref_frame(f, xywh)
            want.append((xywh, None, None if xywh is None else xywh.copy()))
        else:
            st.stabilize(f, xywh)
            want.append((xywh, st.get_cur_trans_matrix(), None if xywh is None else st.transform_cur_boxes()))
    assert st.registered                                         # the last frame registered; the flat one did not:
    det.close()
    st.close()
    eng = ExtractEngine(w, (H, W), kw, None, stab_kw, batch=2, det_streams=2, stab_streams=3, feeder_stream=True)
    reader = open_source(src)
    path, kind, off = reader.raw_layout()
    fd = FrameFeeder((H, W), kind=kind, batch=2, ring=6, device=eng.device, ctx=eng.feeder_ctx)
    try:
        assert eng.gray_route == "frame" and eng.stab_dev_gray
        fd.open_file(path, off, n_threads=2)
        got = list(eng.run(fd.batches(len(eng.dets))))
        assert not eng._host_frames                              # no host copies of frames were kept
        # set_reference() ahead of a run (what the frame-sharded loop does), then host frames: frames 1 and 2 come back with the
        # transforms of the blocking calls (same reference image and boxes, the gray image made in HBM either way)
        eng.reset()
        eng.set_reference(frames[0])
        again = list(eng.run([frames[1:3]]))
        assert not eng._host_frames and [r.H.tobytes() for r in again] == [want[1][1].tobytes(), want[2][1].tobytes()]
    finally:
        fd.close()
        reader.release()
        eng.close()
    assert [r.index for r in got] == list(range(len(frames)))
    for r, (xywh, Hm, stab) in zip(got, want):
        assert (r.xywh is None) == (xywh is None) and (r.H is None) == (Hm is None) and (r.xywh_stab is None) == (stab is None), r.index
        if xywh is not None:
            assert r.xywh.tobytes() == xywh.tobytes(), r.index
            assert r.xywh_stab.tobytes() == np.asarray(stab, np.float32).tobytes(), r.index
        if Hm is not None:
            assert r.H.tobytes() == Hm.tobytes(), r.index
    assert got[5].H_fallback and got[5].H.tobytes() == got[4].H.tobytes()
    assert sum(r.H_fallback for r in got) == 1 and sum(len(r.xywh) for r in got if r.xywh is not None) > 20


def test_the_stable_preset_runs_through_the_read_ahead_feeder(gtx_ctx, tmp_path, monkeypatch):
    """`--cfg stable` (ORB at downsample_ratio 1.0, CLAHE) on a small .y4m: the run takes the read-ahead feeder, and its two result
    files are the bytes of the same command with `engine: {read_ahead: false, pipelined: false}` (the frame-at-a-time loop on host
    frames)."""
    from test_extract_gpu import H, W, _weights_file

    from geotrax_amd import extract as ex
    from geotrax_amd.frames import write_y4m
    from geotrax_amd.synth import make_scene

    sc = make_scene(seed=4, h=H, w=W)
    frames = [sc.render(5 * t) for t in range(6)]
    src = tmp_path / "U_clip.y4m"
    write_y4m(src, frames)
    wpath, _ = _weights_file(tmp_path, gtx_ctx, frames[0], half=False)
    (tmp_path / "blocking.yaml").write_text("_base: stable\nengine: {read_ahead: false, pipelined: false}\n")
    fed = []
    inner = ex._read_ahead_batches

    def spy(*a, **k):
        out = inner(*a, **k)
        fed.append(out[1])
        return out

    monkeypatch.setattr(ex, "_read_ahead_batches", spy)
    outs = {}
    for name, cfg in (("feeder", "stable"), ("blocking", str(tmp_path / "blocking.yaml"))):
        ex.main([str(src), "--cfg", cfg, "--model", str(wpath), "--output-folder", str(tmp_path / name)])
        outs[name] = ((tmp_path / name / "U_clip.txt").read_bytes(), (tmp_path / name / "U_clip_vid_transf.txt").read_bytes())
    assert len(fed) == 1 and fed[0] is not None                  # the pipelined run asked once and got a feeder; the blocking run never asks
    assert outs["feeder"] == outs["blocking"]
    tr = np.loadtxt(tmp_path / "feeder" / "U_clip_vid_transf.txt", delimiter=",", ndmin=2)
    assert tr.shape == (5, 10) and len(outs["feeder"][0]) > 0


def test_the_frame_at_a_time_loop_reads_y4m_sources(gtx_ctx, tmp_path):
    """`engine: {pipelined: false}` on a .y4m source (I420 frames, converted on the host with the device conversion's arithmetic):
    the two result files are the bytes of the pipelined run on the same clip, at the default downsample_ratio 0.5."""
    from test_extract_gpu import H, W, _cfg_file, _weights_file

    import yaml

    from geotrax_amd import extract as ex
    from geotrax_amd.frames import write_y4m
    from geotrax_amd.synth import make_scene

    sc = make_scene(seed=5, h=H, w=W)
    frames = [sc.render(4 * t, 150) for t in range(5)]
    src = tmp_path / "U_clip.y4m"
    write_y4m(src, frames)
    wpath, _ = _weights_file(tmp_path, gtx_ctx, frames[0])
    cfg_path, cfg = _cfg_file(tmp_path, wpath)
    cfg["engine"] = dict(pipelined=False, read_ahead=False)
    (tmp_path / "blocking.yaml").write_text(yaml.safe_dump(cfg))
    outs = {}
    for name, c in (("piped", cfg_path), ("blocking", tmp_path / "blocking.yaml")):
        ex.main([str(src), "--cfg", str(c), "--output-folder", str(tmp_path / name)])
        outs[name] = ((tmp_path / name / "U_clip.txt").read_bytes(), (tmp_path / name / "U_clip_vid_transf.txt").read_bytes())
    assert outs["piped"] == outs["blocking"] and len(outs["piped"][0]) > 0 and len(outs["piped"][1].splitlines()) == 4
