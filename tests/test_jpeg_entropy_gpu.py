"""The GPU entropy route through the feeder and through extract's loop: same pixels, same error messages and same result tables as
the host route, and the feeder's counts say who decoded what."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

H, W, N = 144, 256, 12


def _blobs():
    from geotrax_amd import jpeg
    from geotrax_amd.synth import make_scene

    sc = make_scene(seed=5, h=H, w=W)
    return [jpeg.record_to_bytes(jpeg.bgr_to_record(sc.render(2 * t), 90, "4:2:0")) for t in range(N)]


@pytest.fixture(scope="module")
def blobs():
    return _blobs()


def _with_dri(blob: bytes, interval: int) -> bytes:
    """The same picture with a DRI segment in front of its SOS: an interval of all its MCUs puts no marker into the scan."""
    at = blob.index(b"\xff\xda")
    return blob[:at] + b"\xff\xdd\x00\x04" + interval.to_bytes(2, "big") + blob[at:]


def _layout_of_clip(path, blobs):
    ln = np.array([len(b) for b in blobs], np.int64)
    off = np.concatenate([[0], np.cumsum(ln)[:-1]]).astype(np.int64)
    path.write_bytes(b"".join(blobs))
    return [str(path)], np.zeros(len(blobs), np.int32), off, ln


def _play(ctx, layout, entropy):
    from geotrax_amd.feeder import FrameFeeder

    fd = FrameFeeder((H, W), kind="jpeg", batch=2, ring=3, device=ctx.device)
    got, err = [], None
    try:
        fd.open_jpeg(layout, n_threads=3, entropy=entropy)
        for b in fd.batches(in_flight=2):
            b.wait_on(ctx)
            out = np.empty((b.n, H, W, 3), np.uint8)
            ctx.dev_download(out, b.ptr)
            got.append(out)
    except Exception as e:                                       # noqa: BLE001 (compared with the other route's)
        err = e
    stats = fd.jpeg_stats()
    fd.close()
    return got, err, stats


def test_clip_and_folder_decode_to_the_host_routes_bytes(gtx_ctx, tmp_path, blobs):
    from geotrax_amd import jpeg

    layout = _layout_of_clip(tmp_path / "clip.mjpeg", blobs)
    host, err_h, stats_h = _play(gtx_ctx, layout, "host")
    gpu, err_g, stats_g = _play(gtx_ctx, layout, "gpu")
    assert err_h is None and err_g is None and [len(g) for g in gpu] == [2] * 6
    np.testing.assert_array_equal(np.concatenate(gpu), np.concatenate(host))
    np.testing.assert_array_equal(gpu[0][0], jpeg.decode_host(blobs[0]))
    assert stats_g == (N, 0, 0) and stats_h == (0, 0, 0)
    folder = tmp_path / "frames"
    folder.mkdir()
    paths = []
    for i, b in enumerate(blobs):
        paths.append(str(folder / f"f{i:03d}.jpg"))
        (folder / f"f{i:03d}.jpg").write_bytes(b)
    layout = (paths, np.arange(N, dtype=np.int32), np.zeros(N, np.int64), np.array([len(b) for b in blobs], np.int64))
    gpu, err_g, stats_g = _play(gtx_ctx, layout, "gpu")
    assert err_g is None and stats_g == (N, 0, 0)
    np.testing.assert_array_equal(np.concatenate(gpu), np.concatenate(host))


def test_a_frame_with_a_restart_interval_is_decoded_by_the_host(gtx_ctx, tmp_path, blobs):
    from geotrax_amd import jpeg

    mixed = list(blobs)
    mixed[5] = _with_dri(blobs[5], (W // 16) * (H // 16))
    assert jpeg.entropy_plan(mixed[5]) is None and jpeg.parse(mixed[5])[0].tobytes() == jpeg.parse(blobs[5])[0].tobytes()
    layout = _layout_of_clip(tmp_path / "dri.mjpeg", mixed)
    host, err_h, _ = _play(gtx_ctx, layout, "host")
    gpu, err_g, stats = _play(gtx_ctx, layout, "gpu")
    assert err_h is None and err_g is None and stats == (N - 1, 1, 0)
    np.testing.assert_array_equal(np.concatenate(gpu), np.concatenate(host))


def test_a_truncated_frame_reports_the_host_routes_message_after_the_batches_before_it(gtx_ctx, tmp_path, blobs):
    cut = list(blobs)
    cut[7] = blobs[7][:len(blobs[7]) * 2 // 3]
    layout = _layout_of_clip(tmp_path / "cut.mjpeg", cut)
    host, err_h, _ = _play(gtx_ctx, layout, "host")
    gpu, err_g, stats = _play(gtx_ctx, layout, "gpu")
    assert err_h is not None and "JPEG frame 7" in str(err_h) and str(err_g) == str(err_h) and type(err_g) is type(err_h)
    assert [len(g) for g in gpu] == [len(g) for g in host] == [2, 2, 2]
    np.testing.assert_array_equal(np.concatenate(gpu), np.concatenate(host))
    assert stats == (7, 0, 0)                                     # frames 0..6 were settled before frame 7, which is in no count


def test_extract_with_the_gpu_route_writes_the_host_routes_tables(gtx_ctx, tmp_path):
    import yaml
    from test_extract_gpu import H as EH, W as EW, _cfg_file, _weights_file

    from geotrax_amd import extract as ex
    from geotrax_amd import jpeg
    from geotrax_amd.feeder import FrameFeeder
    from geotrax_amd.synth import make_scene

    sc = make_scene(seed=4, h=EH, w=EW)
    frames = [sc.render(3 * t, 150) for t in range(N)]
    clip = tmp_path / "U_clip.mjpeg"
    clip.write_bytes(b"".join(jpeg.record_to_bytes(jpeg.bgr_to_record(f, 90, "4:2:0")) for f in frames))
    wpath, _ = _weights_file(tmp_path, gtx_ctx, frames[0])
    cfg_path, cfg = _cfg_file(tmp_path, wpath, tracker="botsort")
    routes, stats = [], []
    real, real_close = FrameFeeder.set_jpeg_entropy, FrameFeeder.close
    FrameFeeder.set_jpeg_entropy = lambda self, entropy: (routes.append(entropy), real(self, entropy))[1]

    def close(self):                                             # who decoded the frames, read before the feeder goes
        if getattr(self, "handle", None) and self.kind == 2:
            stats.append(self.jpeg_stats())
        real_close(self)

    FrameFeeder.close = close
    try:
        ex.main([str(clip), "--cfg", str(cfg_path), "--output-folder", str(tmp_path / "host")])
        cfg["engine"]["jpeg_entropy"] = "gpu"
        cfg_path.write_text(yaml.safe_dump(cfg))
        ex.main([str(clip), "--cfg", str(cfg_path), "--output-folder", str(tmp_path / "gpu")])
    finally:
        FrameFeeder.set_jpeg_entropy, FrameFeeder.close = real, real_close
    assert routes == ["host", "gpu"]
    assert stats == [(0, 0, 0), (N, 0, 0)]                       # every frame of the second run was decoded by the kernels, none fell back
    for name in ("U_clip.txt", "U_clip_vid_transf.txt"):
        a, b = (tmp_path / "host" / name).read_bytes(), (tmp_path / "gpu" / name).read_bytes()
        assert a == b and len(a) > 0, name
