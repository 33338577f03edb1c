"""The restart-interval route on the GPU: gtx_op_jpeg_restart against the numpy twin and the host parser, and the route through
the feeder and through extract's loop: same records, same pixels, same error messages and result tables as the host route.
Records and pixels are compared for equality."""
import numpy as np
import pytest
from jpeg_entropy_cases import fixture_bytes
from jpeg_restart_cases import damaged, frames

pytestmark = pytest.mark.gpu

H, W, N = 45, 70, 6


@pytest.mark.parametrize("label", sorted(frames()))
def test_the_hook_returns_the_twins_and_the_parsers_record(gtx_ctx, label):
    from geotrax_amd import jpeg

    rec, blob = frames()[label]
    plan = jpeg.restart_plan(blob)
    status, got = jpeg.restart_plan_dev(gtx_ctx, plan)
    t_status, t_rec = jpeg.restart_decode_twin(plan)
    assert status == t_status == 0
    assert got.tobytes() == t_rec.tobytes() == rec.tobytes()


def test_one_640x360_frame_at_one_mcu_row_per_interval(gtx_ctx):
    from geotrax_amd import jpeg

    b = fixture_bytes("w640x360_420")
    want = jpeg.parse(b)[0]
    for r in (jpeg.mcus_per_row(b), 8, 1):                       # 23, 115 and 920 lanes: one workgroup, two, fifteen
        plan = jpeg.restart_plan(jpeg.recode_with_restarts(b, r))
        status, got = jpeg.restart_plan_dev(gtx_ctx, plan)
        assert status == 0 and got.tobytes() == want.tobytes(), r
    np.testing.assert_array_equal(jpeg.decode_dev(gtx_ctx, got, 360, 640), jpeg.decode_host(b))


@pytest.mark.parametrize("label", ("truncated_last", "stray_byte"))   # the others never become a plan (tests/test_jpeg_restart.py)
def test_damaged_plans_get_the_twins_status_and_never_a_wrong_record(gtx_ctx, label):
    from geotrax_amd import jpeg

    plan = jpeg.restart_plan(damaged()[label])
    status, got = jpeg.restart_plan_dev(gtx_ctx, plan)
    t_status, _ = jpeg.restart_decode_twin(plan)
    assert status == t_status != 0 and got is None


def test_corrupted_streams_get_the_twins_status_and_record(gtx_ctx):
    """Seeded single-byte changes inside the clean stream and the tables of a good plan: whatever they do to the decode, the
    kernel and the twin agree on the status, and on the record where the status is 0."""
    from geotrax_amd import jpeg

    good = jpeg.restart_plan(frames()["420_70x45_r3"][1])
    f = jpeg.restart_plan_fields(good)[0]
    at = jpeg.interval_stream_offset(f["n_intervals"])
    rng = np.random.default_rng(11)
    seen = set()
    for k in range(24):
        plan = good.copy()
        lo, hi = (at, at + f["stream_bytes"]) if k % 3 else (jpeg.PLAN_HUFF_OFFSET, jpeg.PLAN_STREAM_OFFSET)
        plan[int(rng.integers(lo, hi))] ^= int(rng.integers(1, 256))
        status, got = jpeg.restart_plan_dev(gtx_ctx, plan)
        t_status, t_rec = jpeg.restart_decode_twin(plan)
        assert status == t_status, k
        assert (got is None) == (t_rec is None) and (got is None or got.tobytes() == t_rec.tobytes()), k
        seen.add(status)
    assert 1 in seen


def test_the_hook_refuses_a_bad_plan_before_any_launch(gtx_ctx):
    import ctypes as C

    from geotrax_amd import _lib, jpeg

    plan = jpeg.restart_plan(fixture_bytes("p70x45_420_rst3"))
    n, status = C.c_size_t(), C.c_int()
    rec = np.zeros(1 << 14, np.uint32).view(np.uint8)
    for bad, word in ((plan[:len(plan) - 4], "length"), (jpeg.entropy_plan(fixture_bytes("p70x45_420")), "magic")):
        p = np.frombuffer(bad.tobytes() + b"\0\0\0", np.uint8)[:len(bad)]
        rc = gtx_ctx.lib.gtx_op_jpeg_restart(gtx_ctx.handle, _lib.ptr(p), p.nbytes, _lib.ptr(rec), rec.nbytes, C.byref(n), C.byref(status))
        assert rc == -1 and word in gtx_ctx.lib.gtx_last_error().decode() and n.value == 0
    nonmono = plan.copy()
    nonmono[jpeg.PLAN_STREAM_OFFSET + 8:jpeg.PLAN_STREAM_OFFSET + 12].view(np.uint32)[0] = 5
    with pytest.raises(jpeg.JpegError, match="monotone"):
        jpeg.restart_plan_dev(gtx_ctx, nonmono)


# ---------------------------------------------------------------------------------------------------------------- the feeder

def _clip_blobs():
    """Six 70 x 45 frames: restart frames (one MCU per interval, one MCU row, Pillow's committed fixture) mixed with plain ones."""
    from geotrax_amd import jpeg

    rec = frames()["420_70x45_r1"][0]
    plain = jpeg.emit(rec, 0)
    return [jpeg.emit(rec, 1), plain, fixture_bytes("p70x45_420_rst3"), jpeg.emit(rec, 5), fixture_bytes("p70x45_420"), jpeg.emit(rec, 4)], (0, 2, 3, 5)


def _layout_of_clip(path, blobs):
    ln = np.array([len(b) for b in blobs], np.int64)
    off = np.concatenate([[0], np.cumsum(ln)[:-1]]).astype(np.int64)
    path.write_bytes(b"".join(blobs))
    return [str(path)], np.zeros(len(blobs), np.int32), off, ln


def _play(ctx, layout, entropy, restart):
    from geotrax_amd.feeder import FrameFeeder

    fd = FrameFeeder((H, W), kind="jpeg", batch=2, ring=3, device=ctx.device)
    got, err = [], None
    try:
        fd.set_jpeg_restart(restart)
        fd.open_jpeg(layout, n_threads=3, entropy=entropy)
        for b in fd.batches(in_flight=2):
            b.wait_on(ctx)
            out = np.empty((b.n, H, W, 3), np.uint8)
            ctx.dev_download(out, b.ptr)
            got.append(out)
    except Exception as e:                                       # noqa: BLE001 (compared with the other route's)
        err = e
    stats = fd.jpeg_stats(), fd.jpeg_restart_stats()
    fd.close()
    return got, err, stats


def test_clip_and_folder_with_mixed_frames_decode_to_the_host_routes_pixels(gtx_ctx, tmp_path):
    from geotrax_amd import jpeg

    blobs, with_restart = _clip_blobs()
    n_rst, n_other = len(with_restart), len(blobs) - len(with_restart)
    clip = _layout_of_clip(tmp_path / "clip.mjpeg", blobs)
    folder = tmp_path / "frames"
    folder.mkdir()
    paths = []
    for i, b in enumerate(blobs):
        paths.append(str(folder / f"f{i:03d}.jpg"))
        (folder / f"f{i:03d}.jpg").write_bytes(b)
    files = (paths, np.arange(N, dtype=np.int32), np.zeros(N, np.int64), np.array([len(b) for b in blobs], np.int64))
    host, err_h, stats_h = _play(gtx_ctx, clip, "host", "host")
    assert err_h is None and stats_h == ((0, 0, 0), (0, 0, 0)) and [len(g) for g in host] == [2, 2, 2]
    np.testing.assert_array_equal(host[0][0], jpeg.decode_host(blobs[0]))
    for layout in (clip, files):
        for entropy in ("host", "gpu"):
            got, err, (old, new) = _play(gtx_ctx, layout, entropy, "gpu")
            assert err is None, (entropy, err)
            np.testing.assert_array_equal(np.concatenate(got), np.concatenate(host))
            assert new == (n_rst, 0, 0)
            assert old == ((n_other, 0, 0) if entropy == "gpu" else (0, 0, 0))
    # the switch off: the restart frames go where they went (gtx_jpeg_plan hands them back)
    got, err, (old, new) = _play(gtx_ctx, clip, "gpu", "host")
    assert err is None and new == (0, 0, 0) and old == (n_other, n_rst, 0)
    np.testing.assert_array_equal(np.concatenate(got), np.concatenate(host))


def test_a_frame_the_kernel_refuses_is_redone_by_the_parser_or_reports_its_message(gtx_ctx, tmp_path):
    from geotrax_amd import jpeg

    blobs, _ = _clip_blobs()
    cut = list(blobs)
    cut[3] = damaged()["truncated_last"]                          # its markers are in place: the plan is written, the kernel sets the status
    assert jpeg.restart_plan(cut[3]) is not None
    layout = _layout_of_clip(tmp_path / "cut.mjpeg", cut)
    host, err_h, _ = _play(gtx_ctx, layout, "host", "host")
    got, err_g, (_, new) = _play(gtx_ctx, layout, "host", "gpu")
    assert err_h is not None and "JPEG frame 3" in str(err_h) and str(err_g) == str(err_h) and type(err_g) is type(err_h)
    assert [len(g) for g in got] == [len(g) for g in host] == [2]
    np.testing.assert_array_equal(np.concatenate(got), np.concatenate(host))
    assert new == (2, 0, 0)                                       # frames 0 and 2 were settled before frame 3, which is in no count
    # a marker out of sequence: the plan walk has the parser word it on the reader thread
    bad = list(blobs)
    bad[4] = damaged()["out_of_sequence"]
    layout = _layout_of_clip(tmp_path / "seq.mjpeg", bad)
    host, err_h, _ = _play(gtx_ctx, layout, "host", "host")
    got, err_g, _ = _play(gtx_ctx, layout, "gpu", "gpu")
    assert err_h is not None and "JPEG frame 4" in str(err_h) and "out of sequence" in str(err_h) and str(err_g) == str(err_h)
    assert [len(g) for g in got] == [len(g) for g in host] == [2, 2]
    np.testing.assert_array_equal(np.concatenate(got), np.concatenate(host))


def test_extract_on_a_recoded_clip_writes_the_host_routes_tables(gtx_ctx, tmp_path):
    import yaml
    from test_extract_gpu import H as EH, W as EW, _cfg_file, _weights_file

    from geotrax_amd import extract as ex
    from geotrax_amd import jpeg
    from geotrax_amd.feeder import FrameFeeder
    from geotrax_amd.synth import make_scene

    n = 12
    sc = make_scene(seed=4, h=EH, w=EW)
    shots = [sc.render(3 * t, 150) for t in range(n)]
    plain = [jpeg.record_to_bytes(jpeg.bgr_to_record(f, 90, "4:2:0")) for f in shots]
    clip = tmp_path / "U_clip.mjpeg"
    clip.write_bytes(b"".join(jpeg.recode_with_restarts(b, jpeg.mcus_per_row(b)) for b in plain))
    wpath, _ = _weights_file(tmp_path, gtx_ctx, shots[0])
    cfg_path, cfg = _cfg_file(tmp_path, wpath, tracker="botsort")
    stats = []
    real_close = FrameFeeder.close

    def close(self):                                             # who decoded the frames, read before the feeder goes
        if getattr(self, "handle", None) and self.kind == 2:
            stats.append((self.jpeg_stats(), self.jpeg_restart_stats()))
        real_close(self)

    FrameFeeder.close = close
    try:
        ex.main([str(clip), "--cfg", str(cfg_path), "--output-folder", str(tmp_path / "host")])
        cfg["engine"]["jpeg_restart"] = "gpu"
        cfg_path.write_text(yaml.safe_dump(cfg))
        ex.main([str(clip), "--cfg", str(cfg_path), "--output-folder", str(tmp_path / "gpu")])
    finally:
        FrameFeeder.close = real_close
    assert stats == [((0, 0, 0), (0, 0, 0)), ((0, 0, 0), (n, 0, 0))]
    for name in ("U_clip.txt", "U_clip_vid_transf.txt"):
        a, b = (tmp_path / "host" / name).read_bytes(), (tmp_path / "gpu" / name).read_bytes()
        assert a == b and len(a) > 0, name


def test_mjpeg_writer_with_restarts_reads_back_through_the_new_route_to_the_same_pixels(gtx_ctx, tmp_path):
    from geotrax_amd.frames import open_source
    from geotrax_amd.synth import make_scene
    from geotrax_amd.video_writer import MjpegWriter

    sc = make_scene(seed=3, h=H, w=W)
    shots = [sc.render(2 * t) for t in range(N)]
    layouts = {}
    for name, r in (("plain", 0), ("rst", 2)):
        wr = MjpegWriter(tmp_path / f"{name}.mjpeg", 25, (W, H), ctx=gtx_ctx, restart_interval=r)
        for f in shots:
            wr.write(f)
        wr.release()
        src = open_source(tmp_path / f"{name}.mjpeg")
        layouts[name] = src.jpeg_layout()
        src.release()
    want, err_w, _ = _play(gtx_ctx, layouts["plain"], "host", "host")
    got, err_g, (_, new) = _play(gtx_ctx, layouts["rst"], "host", "gpu")
    assert err_w is None and err_g is None and new == (N, 0, 0)
    np.testing.assert_array_equal(np.concatenate(got), np.concatenate(want))
