"""The JPEG frame sink on the GPU (csrc/jpeg_enc.hip): gtx_op_jpeg_encode against the numpy twin byte for byte (integer arithmetic
on both sides: any difference is a bug), one encoder object over several frames, MjpegWriter.write_dev keeping the order with its
ring and its thread pool, and the stabilized-video stage on a small .y4m clip."""
import re

import numpy as np
import pytest
from test_jpeg import ROOT
from test_jpeg_encode import inputs

pytestmark = pytest.mark.gpu

SCAN_TILE = int(re.search(r"kJpegScanTile\s*=\s*(\d+)", (ROOT / "geo-trax_amd" / "csrc" / "jpeg_enc.hpp").read_text()).group(1))
# three scan tiles and a ragged tail in 4:2:0 (6 blocks per 16x16 MCU), six and a tail in 4:4:4, neither side a multiple of 16
_mcus = (3 * SCAN_TILE + SCAN_TILE // 2) // 6 + 1
SCAN_SIZE = (16 * 24 - 5, 16 * -(-_mcus // 24) - 3)
SIZES = [(1, 1), (8, 8), (16, 16), (17, 23), (33, 15), (250, 130), SCAN_SIZE]      # width x height


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_kernels_equal_the_twin_byte_for_byte(gtx_ctx, size):
    """Noise at quality 100 makes the blocks 64 long (the stream's capacity), flat 128 makes every block empty, the scene lies
    between; both samplings, qualities 5, 90 and 100."""
    from geotrax_amd import jpeg

    w, h = size
    frames = inputs(w, h)
    for s in ("4:2:0", "4:4:4"):
        if size == SCAN_SIZE:
            nb = jpeg.record_fields(jpeg.bgr_to_record(frames["flat128"], 90, s))[0]["n_blocks"]
            assert nb >= 3 * SCAN_TILE and nb % SCAN_TILE
        for name in ("noise", "flat128", "scene"):
            for q in (5, 90, 100):
                want = jpeg.bgr_to_record(frames[name], q, s)
                got = jpeg.encode_dev(gtx_ctx, frames[name], q, s)
                where = f"{w}x{h} {name} q{q} {s}"
                assert got.nbytes == want.nbytes, where
                fg, qg, og, cg = jpeg.record_fields(got)
                fw, qw, ow, cw = jpeg.record_fields(want)
                assert fg == fw, where
                np.testing.assert_array_equal(qg, qw, err_msg=where)
                np.testing.assert_array_equal(og, ow, err_msg=where)
                np.testing.assert_array_equal(cg, cw, err_msg=where)
                assert got.tobytes() == want.tobytes(), where


def test_short_record_buffer_reports_the_size(gtx_ctx):
    import ctypes as C

    from geotrax_amd import _lib, jpeg

    a = inputs(33, 15)["noise"]
    want = jpeg.bgr_to_record(a, 90)
    n = C.c_size_t()
    small = np.full(want.nbytes // 4, 0xA5A5A5A5, np.uint32).view(np.uint8)[:want.nbytes - 4]
    assert gtx_ctx.lib.gtx_op_jpeg_encode(gtx_ctx.handle, _lib.ptr(a), 15, 33, 90, 2, _lib.ptr(small), small.nbytes, C.byref(n)) == 1
    assert n.value == want.nbytes and (small == 0xA5).all()


def test_one_encoder_object_over_six_frames(gtx_ctx):
    """No state leaks from frame to frame: busy, empty and in-between frames in a row through one object, each record the twin's."""
    import ctypes as C

    from geotrax_amd import _lib, jpeg

    w, h = 250, 130
    fr = inputs(w, h)
    rng = np.random.default_rng(9)
    frames = [fr["noise"], fr["flat128"], fr["scene"], rng.integers(0, 256, (h, w, 3), dtype=np.uint8), fr["flat0"], fr["ramp"]]
    lib = gtx_ctx.lib
    enc = C.c_void_p()
    _lib.check(lib.gtx_jpeg_enc_create(gtx_ctx.handle, h, w, 100, 2, C.byref(enc)))
    dptr = gtx_ctx.dev_alloc(h * w * 3)
    try:
        rec = np.zeros(lib.gtx_jpeg_record_bound(h, w) // 4 + 1, np.uint32).view(np.uint8)
        n, ms = C.c_size_t(), C.c_float()
        assert lib.gtx_jpeg_enc_collect(enc, _lib.ptr(rec), rec.nbytes, C.byref(n)) == -1          # nothing submitted yet
        for i, f in enumerate(frames):
            gtx_ctx.dev_upload(dptr, f)
            _lib.check(lib.gtx_jpeg_enc_submit_dev(enc, C.c_void_p(dptr)))
            if i == 0:
                assert lib.gtx_jpeg_enc_submit_dev(enc, C.c_void_p(dptr)) == -1                       # one frame in flight per object
            _lib.check(lib.gtx_jpeg_enc_collect(enc, _lib.ptr(rec), rec.nbytes, C.byref(n)))
            assert rec[:n.value].tobytes() == jpeg.bgr_to_record(f, 100).tobytes(), i
            _lib.check(lib.gtx_jpeg_enc_last_ms(enc, C.byref(ms)))
            assert 0.0 < ms.value < 1000.0
    finally:
        lib.gtx_jpeg_enc_destroy(enc)
        gtx_ctx.dev_free(dptr)


def test_writer_keeps_the_order_through_its_ring_and_pool(gtx_ctx, tmp_path):
    """12 frames of 250x130 through write_dev with 4 encode threads: frame i of the file decodes to the twin's decode of the twin's
    encode of frame i."""
    from geotrax_amd import jpeg
    from geotrax_amd.frames import AviMjpegReader
    from geotrax_amd.synth import make_scene
    from geotrax_amd.video_writer import MjpegWriter

    w, h = 250, 130
    scene = make_scene(seed=3, h=h, w=w)
    frames = [np.ascontiguousarray(scene.render(5 * i)) for i in range(12)]
    assert len({f.tobytes() for f in frames}) == 12
    dptrs = [gtx_ctx.dev_alloc(h * w * 3) for _ in frames]
    try:
        for p, f in zip(dptrs, frames):
            gtx_ctx.dev_upload(p, f)
        path = tmp_path / "out.avi"
        wr = MjpegWriter(path, 25.0, (w, h), quality=90, encode_threads=4, ctx=gtx_ctx)
        for p in dptrs:
            wr.write_dev(p)
        wr.release()
        assert wr.frames == 12
    finally:
        for p in dptrs:
            gtx_ctx.dev_free(p)
    rd = AviMjpegReader(path)
    assert rd.frame_count == 12 and rd.frame_hw == (h, w) and rd.fps == 25.0
    for i, f in enumerate(frames):
        want = jpeg.record_to_bgr(jpeg.bgr_to_record(f, 90))
        np.testing.assert_array_equal(jpeg.decode_host(rd._bytes(i), i), want, err_msg=f"frame {i}")
    rd.release()
    # host frames through write(): the same file
    path2 = tmp_path / "out2.avi"
    wr = MjpegWriter(path2, 25.0, (w, h), quality=90, encode_threads=4, ctx=gtx_ctx)
    for f in frames:
        wr.write(f)
    wr.release()
    assert path2.read_bytes() == path.read_bytes()


def test_stabilized_video_stage(gtx_ctx, tmp_path):
    """An 8-frame 256x144 .y4m and a transforms file that leaves frame 3 out: every picture of the output is the emitter's bytes for
    the twin's record of the warped frame, frame 3's of the frame as it is. The warped frame is the oracle's (oracle/warp_ref.py on
    the matrix as the transforms file holds it, with the library's own inverse), not the warp kernel's."""
    from geotrax_amd import jpeg, stabilized_video
    from geotrax_amd.frames import AviMjpegReader, Y4mReader, write_y4m
    from geotrax_amd.synth import make_scene
    from geotrax_amd.warp import inverse_homography, warp_perspective
    from oracle.warp_ref import warp_perspective as warp_ref

    w, h = 256, 144
    scene = make_scene(seed=1, h=h, w=w)
    clip = tmp_path / "clip.y4m"
    write_y4m(clip, [scene.render(4 * i) for i in range(8)])
    rd = Y4mReader(clip)
    frames = [rd.read()[1] for _ in range(8)]
    frames = [f.bgr() if hasattr(f, "bgr") else f for f in frames]
    rd.release()
    Hs = {i: np.array([[1 + 0.004 * i, 0.002 * i, 1.5 * i], [-0.003 * i, 1 - 0.002 * i, -0.75 * i], [1e-6 * i, -2e-6 * i, 1.0]]) for i in range(8) if i != 3}
    (tmp_path / "results").mkdir()
    np.savetxt(tmp_path / "results" / "clip_vid_transf.txt", np.array([[i, *H.ravel()] for i, H in Hs.items()]), fmt="%.16g", delimiter=",")
    on_file = {int(r[0]): r[1:].reshape(3, 3) for r in np.loadtxt(tmp_path / "results" / "clip_vid_transf.txt", delimiter=",")}
    assert sorted(on_file) == sorted(Hs) and all(np.allclose(on_file[i], Hs[i], rtol=1e-15, atol=0) for i in Hs)
    warped = {i: warp_ref(frames[i], on_file[i], M_inv=inverse_homography(on_file[i])) for i in Hs}
    for i in (1, 7):                                                 # (and the kernel on its own agrees, so a difference below is the stage's)
        np.testing.assert_array_equal(warp_perspective(frames[i], on_file[i], gtx_ctx), warped[i])
        assert (warped[i] != frames[i]).any()
    assert stabilized_video.main([str(clip), "--quality", "85"]) == 0
    out = tmp_path / "results" / "clip_mode_1.avi"
    got = AviMjpegReader(out)
    assert got.frame_count == 8 and got.frame_hw == (h, w)
    for i, f in enumerate(frames):
        src = warped[i] if i in Hs else f
        assert got._bytes(i) == jpeg.record_to_bytes(jpeg.bgr_to_record(src, 85)), f"frame {i}"
    got.release()
    # the frame range: cut_frame_left .. cut_frame_right - 1, numbered as in the clip
    assert stabilized_video.main([str(clip), "-cfl", "2", "-cfr", "5", "-o", str(tmp_path / "cut.mjpeg")]) == 0
    from geotrax_amd.frames import MjpegReader

    cut = MjpegReader(tmp_path / "cut.mjpeg")
    assert cut.frame_count == 3
    for k, i in enumerate((2, 3, 4)):
        src = warped[i] if i in Hs else frames[i]
        assert cut._bytes(k) == jpeg.record_to_bytes(jpeg.bgr_to_record(src, 90)), f"frame {i}"
    cut.release()
