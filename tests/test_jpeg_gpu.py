"""The JPEG frame source on the GPU (csrc/jpeg.hip): gtx_jpeg_decode_dev against the numpy twin byte for byte on every accepted
fixture; a feeder of kind "jpeg" over a Motion-JPEG clip whose tables change from frame to frame; the extract CLI on a .mjpeg
clip producing exactly what it produces on the same decoded frames given as .npy. Corrupt inputs never reach a kernel: they are
rejected on the host (tests/test_jpeg.py shows that without a GPU)."""
import logging

import numpy as np
import pytest
from test_jpeg import ACCEPTED, CLIP, expected, fixture, write_mjpeg

pytestmark = pytest.mark.gpu
logger = logging.getLogger("jpeg-gpu")


@pytest.mark.parametrize("name", ACCEPTED)
def test_device_decode_equals_the_host_twin(gtx_ctx, name):
    from geotrax_amd import jpeg

    rec, info = jpeg.parse(fixture(name))
    want = jpeg.record_to_bgr(rec)
    got = jpeg.decode_dev(gtx_ctx, rec, info["h"], info["w"])
    np.testing.assert_array_equal(got, want)                    # integer arithmetic on both sides: any difference is a bug
    np.testing.assert_array_equal(got, expected(name))          # ... and both are Pillow's bytes


def _download(ctx, ptr, n, h, w):
    out = np.empty((n, h, w, 3), np.uint8)
    ctx.dev_download(out, ptr)
    return out


def test_feeder_decodes_a_clip_whose_tables_change_every_frame(gtx_ctx, tmp_path):
    """Six 70x45 frames (plain, optimised Huffman tables, restart intervals, twice) through batches of 2 and a ring of 3; then the
    same clip with a seventh frame cut short: the three full batches arrive, the error after them."""
    from geotrax_amd import _lib, jpeg
    from geotrax_amd.feeder import FrameFeeder
    from geotrax_amd.frames import open_source

    frames = [fixture(n) for n in CLIP] * 2
    want = np.stack([jpeg.decode_host(f) for f in frames])
    path = tmp_path / "clip.mjpeg"
    write_mjpeg(path, frames)
    reader = open_source(path)
    layout = reader.jpeg_layout()
    reader.release()
    fd = FrameFeeder((45, 70), kind="jpeg", batch=2, ring=3, device=gtx_ctx.device)
    paths, idx, off, ln = layout
    fd.open_jpeg((paths, idx[:5], off[:5], ln[:5]), n_threads=3)            # five frames: the last batch is partial
    got = []
    for b in fd.batches(in_flight=2):
        b.wait_on(gtx_ctx)
        got.append((b.index, b.n, _download(gtx_ctx, b.ptr, b.n, 45, 70)))
    fd.close()
    assert [(j, n) for j, n, _ in got] == [(0, 2), (1, 2), (2, 1)]
    np.testing.assert_array_equal(np.concatenate([g for _, _, g in got]), want[:5])

    cut = tmp_path / "cut.mjpeg"
    write_mjpeg(cut, frames + [frames[0][:900]])
    off7 = np.append(off, off[-1] + ln[-1]).astype(np.int64)
    ln7 = np.append(ln, 900).astype(np.int64)
    fd = FrameFeeder((45, 70), kind="jpeg", batch=2, ring=3, device=gtx_ctx.device)
    fd.open_jpeg(([str(cut)], np.zeros(7, np.int32), off7, ln7), n_threads=3)
    got = []
    with pytest.raises(_lib.GtxError, match="frame 6"):
        for b in fd.batches(in_flight=2):
            b.wait_on(gtx_ctx)
            got.append(_download(gtx_ctx, b.ptr, b.n, 45, 70))
    fd.close()
    assert [len(g) for g in got] == [2, 2, 2]
    np.testing.assert_array_equal(np.concatenate(got), want)


def test_feeder_push_takes_compressed_frames_and_refuses_another_size(gtx_ctx):
    from geotrax_amd import _lib, jpeg
    from geotrax_amd.feeder import FrameFeeder

    frames = [fixture(n) for n in CLIP]
    fd = FrameFeeder((45, 70), kind="jpeg", batch=2, ring=3, device=gtx_ctx.device)
    fd.open_reader(iter(frames + [fixture("m16x16_420")]))                 # the fourth frame is 16 x 16
    got = []
    with pytest.raises(_lib.GtxError, match="differs from the feeder's"):
        for b in fd.batches(in_flight=2):
            b.wait_on(gtx_ctx)
            got.append(_download(gtx_ctx, b.ptr, b.n, 45, 70))
    fd.close()
    assert len(got) == 1                                                   # the full batch before the bad frame's batch
    np.testing.assert_array_equal(got[0], np.stack([jpeg.decode_host(f) for f in frames[:2]]))


def test_extract_on_mjpeg_equals_extract_on_the_decoded_frames(gtx_ctx, tmp_path, monkeypatch):
    from test_extract_gpu import H, W, _cfg_file, _weights_file

    from geotrax_amd import extract as ex
    from geotrax_amd import jpeg

    import io

    from geotrax_amd.feeder import FrameFeeder
    from geotrax_amd.synth import make_scene

    try:
        from PIL import Image
    except ImportError:                                                     # no encoder: a committed fixture, repeated
        blobs = [fixture("w640x360_420")] * 6
    else:
        sc = make_scene(seed=4, h=H, w=W)
        blobs = []
        for t in range(6):
            buf = io.BytesIO()
            Image.fromarray(np.ascontiguousarray(sc.render(3 * t, 150)[..., ::-1]), "RGB").save(buf, "JPEG", quality=90, subsampling=2)
            blobs.append(buf.getvalue())
    clip = tmp_path / "U_clip.mjpeg"
    write_mjpeg(clip, blobs)
    frames = [jpeg.decode_host(b) for b in blobs]
    npy = tmp_path / "npy" / "U_clip.npy"
    npy.parent.mkdir()
    np.save(npy, np.stack(frames))
    wpath, _ = _weights_file(tmp_path, gtx_ctx, frames[0])
    cfg_path, _ = _cfg_file(tmp_path, wpath, tracker="botsort")
    opened = []
    real_open = FrameFeeder.open_jpeg
    monkeypatch.setattr(FrameFeeder, "open_jpeg", lambda self, layout, n_threads=8: (opened.append(len(layout[2])), real_open(self, layout, n_threads))[1])
    ex.main([str(clip), "--cfg", str(cfg_path), "--output-folder", str(tmp_path / "a")])
    assert opened == [6]                                                    # the clip went through the feeder's GPU decode, not the host twin
    ex.main([str(npy), "--cfg", str(cfg_path), "--output-folder", str(tmp_path / "b")])
    a, b = (tmp_path / "a" / "U_clip.txt").read_text(), (tmp_path / "b" / "U_clip.txt").read_text()
    assert a == b and len(a.splitlines()) > (30 if len(set(blobs)) > 1 else 0)   # GPU decode == host decode, byte for byte downstream
    assert (tmp_path / "a" / "U_clip_vid_transf.txt").read_text() == (tmp_path / "b" / "U_clip_vid_transf.txt").read_text()


_NOFILE_CHILD = """
import os, resource, sys
import numpy as np
sys.path[:0] = {paths!r}
from geotrax_amd import _lib, jpeg
from geotrax_amd.feeder import FrameFeeder
from geotrax_amd.frames import open_source
ctx = _lib.default_context(0)
reader = open_source({folder!r})
layout = reader.jpeg_layout()
assert layout is not None and len(layout[0]) == {n}
fd = FrameFeeder((8, 8), kind="jpeg", batch=2, ring=3, device=ctx.device)
soft, hard = resource.getrlimit(resource.RLIMIT_NOFILE)
limit = max(int(x) for x in os.listdir("/proc/self/fd")) + 1 + {spare}         # room for {spare} more descriptors: far fewer than the frames
resource.setrlimit(resource.RLIMIT_NOFILE, (min(limit, soft), hard))
fd.open_jpeg(layout, n_threads=4)
want = jpeg.decode_host(open(layout[0][0], "rb").read())
k = 0
for b in fd.batches(in_flight=2):
    b.wait_on(ctx)
    out = np.empty((b.n, 8, 8, 3), np.uint8)
    ctx.dev_download(out, b.ptr)
    assert all(np.array_equal(o, want) for o in out)
    k += b.n
fd.close()
print("frames", k)
"""


def test_a_folder_longer_than_the_descriptor_limit_plays(tmp_path):
    """One file per frame: the feeder opens a frame's file when it reads it, so a folder with more frames than the process may
    hold descriptors plays like it did through Pillow. A child process lowers its own soft RLIMIT_NOFILE to 24 descriptors above those it holds, with 200 frames to play."""
    import subprocess
    import sys

    folder = tmp_path / "frames"
    folder.mkdir()
    for k in range(200):
        (folder / f"f{k:04d}.jpg").write_bytes(fixture("b8x8_444"))
    code = _NOFILE_CHILD.format(paths=[p for p in sys.path if p], folder=str(folder), n=200, spare=24)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "frames 200" in r.stdout, r.stdout + r.stderr
