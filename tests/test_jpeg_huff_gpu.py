"""The JPEG frame sink with the entropy coder on the GPU, whole chain (csrc/jpeg_enc.hip + csrc/jpeg_huff.hip): the picture an
encoder on the GPU route hands over equals, byte for byte, the host emitter's bytes for the twin's record of the same frame; one
encoder object over several frames; MjpegWriter(entropy="gpu") writing the file the host route writes; the stabilized-video stage
with --entropy gpu."""
import ctypes as C

import numpy as np
import pytest
from test_jpeg_encode import inputs
from test_jpeg_encode_gpu import SCAN_SIZE, SIZES

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_chain_equals_the_host_route_byte_for_byte(gtx_ctx, size):
    from geotrax_amd import jpeg

    w, h = size
    frames = inputs(w, h)
    for s in ("4:2:0", "4:4:4"):
        for name in ("noise", "flat128", "scene"):
            for q in (5, 90, 100):
                want = jpeg.record_to_bytes(jpeg.bgr_to_record(frames[name], q, s))
                got = jpeg.encode_jpeg_dev(gtx_ctx, frames[name], q, s)
                where = f"{w}x{h} {name} q{q} {s}"
                assert len(got) == len(want), where
                assert got == want, where
    assert SCAN_SIZE in SIZES


def test_one_gpu_route_encoder_over_six_frames_and_the_first_again(gtx_ctx):
    """Nothing is left over from the frame before (the bit buffer is zeroed as far as each frame's scan reaches, a long scan is
    followed by a short one); the wrong collect call for the route is refused and leaves the frame collectable."""
    from geotrax_amd import _lib, jpeg

    w, h = 250, 130
    fr = inputs(w, h)
    rng = np.random.default_rng(9)
    frames = [fr["noise"], fr["flat128"], fr["scene"], rng.integers(0, 256, (h, w, 3), dtype=np.uint8), fr["flat0"], fr["ramp"], fr["noise"]]
    lib = gtx_ctx.lib
    enc, host = C.c_void_p(), C.c_void_p()
    _lib.check(lib.gtx_jpeg_enc_create(gtx_ctx.handle, h, w, 100, 2, C.byref(enc)))
    _lib.check(lib.gtx_jpeg_enc_create(gtx_ctx.handle, h, w, 100, 2, C.byref(host)))
    dptr = gtx_ctx.dev_alloc(h * w * 3)
    try:
        _lib.check(lib.gtx_jpeg_enc_set_entropy(enc, 1))
        _lib.check(lib.gtx_jpeg_enc_set_entropy(host, 0))
        bound = lib.gtx_jpeg_picture_bound(h, w)
        assert bound > 0
        out = np.zeros(bound, np.uint8)
        rec = np.zeros(lib.gtx_jpeg_record_bound(h, w) // 4 + 1, np.uint32).view(np.uint8)
        n, ms, ems = C.c_size_t(), C.c_float(), C.c_float()
        assert lib.gtx_jpeg_enc_collect_jpeg(enc, _lib.ptr(out), out.nbytes, C.byref(n)) == -1     # nothing submitted yet
        for i, f in enumerate(frames):
            want = jpeg.record_to_bytes(jpeg.bgr_to_record(f, 100))
            gtx_ctx.dev_upload(dptr, f)
            _lib.check(lib.gtx_jpeg_enc_submit_dev(enc, C.c_void_p(dptr)))
            if i == 0:
                assert lib.gtx_jpeg_enc_submit_dev(enc, C.c_void_p(dptr)) == -1                   # one frame in flight per object
                assert lib.gtx_jpeg_enc_set_entropy(enc, 0) == -1                                  # only before the first submit
                assert lib.gtx_jpeg_enc_collect(enc, _lib.ptr(rec), rec.nbytes, C.byref(n)) == -1  # the host route's call
                assert lib.gtx_jpeg_enc_collect_jpeg(enc, _lib.ptr(out), len(want) - 1, C.byref(n)) == 1 and n.value == len(want)
                # the host route's encoder refuses the GPU route's call and keeps its frame too
                _lib.check(lib.gtx_jpeg_enc_submit_dev(host, C.c_void_p(dptr)))
                assert lib.gtx_jpeg_enc_collect_jpeg(host, _lib.ptr(out), out.nbytes, C.byref(n)) == -1
                _lib.check(lib.gtx_jpeg_enc_collect(host, _lib.ptr(rec), rec.nbytes, C.byref(n)))
                assert rec[:n.value].tobytes() == jpeg.bgr_to_record(f, 100).tobytes()
                assert lib.gtx_jpeg_enc_set_entropy(host, 1) == -1
            _lib.check(lib.gtx_jpeg_enc_collect_jpeg(enc, _lib.ptr(out), out.nbytes, C.byref(n)))
            assert n.value == len(want) <= bound, i
            assert out[:n.value].tobytes() == want, i
            _lib.check(lib.gtx_jpeg_enc_last_ms(enc, C.byref(ms)))
            _lib.check(lib.gtx_jpeg_enc_entropy_ms(enc, C.byref(ems)))
            assert 0.0 < ems.value < ms.value < 1000.0
    finally:
        lib.gtx_jpeg_enc_destroy(enc)
        lib.gtx_jpeg_enc_destroy(host)
        gtx_ctx.dev_free(dptr)


def test_writer_on_the_gpu_route_writes_the_host_routes_file(gtx_ctx, tmp_path):
    """ring = 3 over 10 distinct frames through write_dev and through write, to .avi and to .mjpeg: the same bytes as
    entropy="host", in submission order; the readers read them back."""
    from geotrax_amd import jpeg
    from geotrax_amd.frames import AviMjpegReader, MjpegReader
    from geotrax_amd.synth import make_scene
    from geotrax_amd.video_writer import MjpegWriter

    w, h = 250, 130
    scene = make_scene(seed=3, h=h, w=w)
    frames = [np.ascontiguousarray(scene.render(5 * i)) for i in range(10)]
    assert len({f.tobytes() for f in frames}) == 10
    dptrs = [gtx_ctx.dev_alloc(h * w * 3) for _ in frames]
    try:
        for p, f in zip(dptrs, frames):
            gtx_ctx.dev_upload(p, f)
        for suffix, reader in ((".avi", AviMjpegReader), (".mjpeg", MjpegReader)):
            files = {}
            for entropy in ("host", "gpu"):
                for how in ("dev", "host_frames"):
                    path = tmp_path / f"{entropy}_{how}{suffix}"
                    wr = MjpegWriter(path, 25.0, (w, h), quality=90, encode_threads=4, ctx=gtx_ctx, ring=3, entropy=entropy)
                    for p, f in zip(dptrs, frames):
                        if how == "dev":
                            wr.write_dev(p)
                        else:
                            wr.write(f)
                    wr.release()
                    assert wr.frames == 10
                    files[entropy, how] = path.read_bytes()
                    if entropy == "gpu":                                # what left the GPU: the pictures themselves
                        assert wr.record_bytes == sum(len(jpeg.record_to_bytes(jpeg.bgr_to_record(f, 90))) for f in frames)
            assert files["gpu", "dev"] == files["host", "dev"] == files["gpu", "host_frames"] == files["host", "host_frames"], suffix
            rd = reader(tmp_path / f"gpu_dev{suffix}")
            assert rd.frame_count == 10 and rd.frame_hw == (h, w)
            for i, f in enumerate(frames):
                assert rd._bytes(i) == jpeg.record_to_bytes(jpeg.bgr_to_record(f, 90)), f"frame {i}"
            rd.release()
    finally:
        for p in dptrs:
            gtx_ctx.dev_free(p)


def test_stabilized_video_stage_with_gpu_entropy(gtx_ctx, tmp_path):
    """The 8-frame 256x144 .y4m of test_stabilized_video_stage (a transforms file that leaves frame 3 out): --entropy gpu writes the
    file --entropy host writes."""
    from geotrax_amd import stabilized_video
    from geotrax_amd.frames import AviMjpegReader, write_y4m
    from geotrax_amd.synth import make_scene

    w, h = 256, 144
    scene = make_scene(seed=1, h=h, w=w)
    clip = tmp_path / "clip.y4m"
    write_y4m(clip, [scene.render(4 * i) for i in range(8)])
    Hs = {i: np.array([[1 + 0.004 * i, 0.002 * i, 1.5 * i], [-0.003 * i, 1 - 0.002 * i, -0.75 * i], [1e-6 * i, -2e-6 * i, 1.0]]) for i in range(8) if i != 3}
    (tmp_path / "results").mkdir()
    np.savetxt(tmp_path / "results" / "clip_vid_transf.txt", np.array([[i, *H.ravel()] for i, H in Hs.items()]), fmt="%.16g", delimiter=",")
    outs = {}
    for entropy in ("host", "gpu"):
        outs[entropy] = tmp_path / f"{entropy}.avi"
        assert stabilized_video.main([str(clip), "--quality", "85", "--entropy", entropy, "-o", str(outs[entropy])]) == 0
    assert outs["gpu"].read_bytes() == outs["host"].read_bytes()
    rd = AviMjpegReader(outs["gpu"])
    assert rd.frame_count == 8 and rd.frame_hw == (h, w)
    rd.release()
