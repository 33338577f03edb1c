"""Figures of the JPEG frame sink at 4K; raw output: profiles/jpeg_encode_time.txt.

    python tools/jpeg_encode_time.py [--frames 60] [--distinct 6] [--out FILE]

3840 x 2160, quality 90, 4:2:0, the synthetic scene:
  * GPU time per frame of the encoder's chain (events around the launches, gtx_jpeg_enc_last_ms), three passes
  * bytes per frame: the record, the .jpg, the BGR frame
  * gtx_jpeg_emit: ms per frame on one thread
  * the stage (MjpegWriter.write_dev on frames resident in HBM -> .mjpeg in a temporary directory): frames/s at 4, 8 and 12
    encode threads, three passes each
  * the GPU entropy route (csrc/jpeg_huff.hip, entropy="gpu") in the same session: GPU time per frame of the whole chain and of
    the entropy launches alone (gtx_jpeg_enc_entropy_ms), bytes per frame off the GPU on both routes, and the stage's frames/s
    next to the host route's 4 / 8 / 12-thread figures
  * in the same process, for comparison: the 25 MB download FrameWarper.__call__ does per frame today, and Pillow encoding the
    same frame on one host thread
"""
import argparse
import io
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "geo-trax_amd"))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--distinct", type=int, default=6)
    ap.add_argument("--h", type=int, default=2160)
    ap.add_argument("--w", type=int, default=3840)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import ctypes as C

    from PIL import Image

    from geotrax_amd import _lib, jpeg
    from geotrax_amd.synth import make_scene
    from geotrax_amd.video_writer import MjpegWriter

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    h, w = a.h, a.w
    ctx = _lib.default_context()
    lib = ctx.lib
    sc = make_scene(seed=0, h=h, w=w)
    frames = [np.ascontiguousarray(sc.render(5 * t, 150)) for t in range(a.distinct)]
    dptrs = [ctx.dev_alloc(h * w * 3) for _ in frames]
    for p, f in zip(dptrs, frames):
        ctx.dev_upload(p, f)
    say(f"frame {w} x {h}, quality 90, 4:2:0, {a.distinct} distinct frames of the synthetic scene")

    enc = C.c_void_p()
    _lib.check(lib.gtx_jpeg_enc_create(ctx.handle, h, w, 90, 2, C.byref(enc)))
    rec = np.zeros(lib.gtx_jpeg_record_bound(h, w) // 4 + 1, np.uint32).view(np.uint8)
    n, ms = C.c_size_t(), C.c_float()
    recs = []
    for k in range(4):                                      # pass 0 warms up
        t_gpu, t_collect = [], []
        for p in dptrs * 5:
            _lib.check(lib.gtx_jpeg_enc_submit_dev(enc, C.c_void_p(p)))
            t0 = time.perf_counter()
            _lib.check(lib.gtx_jpeg_enc_collect(enc, _lib.ptr(rec), rec.nbytes, C.byref(n)))
            t_collect.append(time.perf_counter() - t0)
            _lib.check(lib.gtx_jpeg_enc_last_ms(enc, C.byref(ms)))
            t_gpu.append(ms.value)
            if k == 0 and len(recs) < len(frames):
                recs.append(rec[:n.value].copy())
        if k:
            say(f"GPU time per frame, pass {k} (events around the six launches, {len(t_gpu)} frames): mean {np.mean(t_gpu):.4f} ms, median {np.median(t_gpu):.4f}, "
                f"min {np.min(t_gpu):.4f}; submit-to-record on the host (wait + copy of the record): median {1e3 * np.median(t_collect):.3f} ms")
    lib.gtx_jpeg_enc_destroy(enc)
    assert recs[0].tobytes() == jpeg.bgr_to_record(frames[0], 90).tobytes(), "the GPU record differs from the twin's"
    jpgs = [jpeg.record_to_bytes(r) for r in recs]
    say(f"bytes per frame: record {np.mean([r.nbytes for r in recs]):.0f}, jpg {np.mean([len(j) for j in jpgs]):.0f}, record bound "
        f"{lib.gtx_jpeg_record_bound(h, w)}, BGR {h * w * 3}")
    t = []
    for _ in range(3):
        for r in recs:
            t0 = time.perf_counter()
            jpeg.record_to_bytes(r)
            t.append(time.perf_counter() - t0)
    say(f"gtx_jpeg_emit: {1e3 * np.median(t):.2f} ms per frame on one thread (median of {len(t)}, min {1e3 * np.min(t):.2f})")

    # the GPU entropy route: the same frames through an encoder that Huffman-codes on the GPU
    _lib.check(lib.gtx_jpeg_enc_create(ctx.handle, h, w, 90, 2, C.byref(enc)))
    _lib.check(lib.gtx_jpeg_enc_set_entropy(enc, 1))
    pic = np.zeros(lib.gtx_jpeg_picture_bound(h, w), np.uint8)
    ems = C.c_float()
    pics = []
    for k in range(4):                                      # pass 0 warms up
        t_gpu, t_ent, t_collect = [], [], []
        for p in dptrs * 5:
            _lib.check(lib.gtx_jpeg_enc_submit_dev(enc, C.c_void_p(p)))
            t0 = time.perf_counter()
            _lib.check(lib.gtx_jpeg_enc_collect_jpeg(enc, _lib.ptr(pic), pic.nbytes, C.byref(n)))
            t_collect.append(time.perf_counter() - t0)
            _lib.check(lib.gtx_jpeg_enc_last_ms(enc, C.byref(ms)))
            _lib.check(lib.gtx_jpeg_enc_entropy_ms(enc, C.byref(ems)))
            t_gpu.append(ms.value)
            t_ent.append(ems.value)
            if k == 0 and len(pics) < len(frames):
                pics.append(pic[:n.value].tobytes())
        if k:
            say(f"GPU entropy route, GPU time per frame, pass {k} ({len(t_gpu)} frames): whole chain mean {np.mean(t_gpu):.4f} ms, median {np.median(t_gpu):.4f}, "
                f"min {np.min(t_gpu):.4f}; the entropy launches alone mean {np.mean(t_ent):.4f} ms, median {np.median(t_ent):.4f}, min {np.min(t_ent):.4f}; "
                f"submit-to-picture on the host (wait + copy of the picture): median {1e3 * np.median(t_collect):.3f} ms")
    lib.gtx_jpeg_enc_destroy(enc)
    assert pics == jpgs, "the GPU route's pictures differ from the emitter's"
    say(f"bytes per frame off the GPU: host route (the record) {np.mean([r.nbytes for r in recs]):.0f}, GPU route (the picture) {np.mean([len(j) for j in pics]):.0f}, "
        f"picture bound {lib.gtx_jpeg_picture_bound(h, w)}")

    with tempfile.TemporaryDirectory() as d:
        for k in range(3):
            path = Path(d) / f"gpu_{k}.mjpeg"
            t0 = time.perf_counter()
            wr = MjpegWriter(path, 30.0, (w, h), quality=90, ctx=ctx, entropy="gpu")
            for i in range(a.frames):
                wr.write_dev(dptrs[i % len(dptrs)])
            wr.release()
            dt = time.perf_counter() - t0
            say(f"stage (write_dev -> .mjpeg), entropy on the GPU (no encode threads), pass {k}: {a.frames} frames in {dt:.3f} s = {a.frames / dt:.0f} frames/s "
                f"({path.stat().st_size} bytes, {wr.record_bytes // a.frames} bytes per frame off the GPU)")
            path.unlink()
        for threads in (4, 8, 12):
            for k in range(3):
                path = Path(d) / f"t{threads}_{k}.mjpeg"
                t0 = time.perf_counter()
                wr = MjpegWriter(path, 30.0, (w, h), quality=90, encode_threads=threads, ctx=ctx)
                for i in range(a.frames):
                    wr.write_dev(dptrs[i % len(dptrs)])
                wr.release()
                dt = time.perf_counter() - t0
                say(f"stage (write_dev -> .mjpeg), {threads} encode threads, pass {k}: {a.frames} frames in {dt:.3f} s = {a.frames / dt:.0f} frames/s "
                    f"({path.stat().st_size} bytes)")
                path.unlink()

    out = np.empty_like(frames[0])
    t = []
    for _ in range(3):
        for p in dptrs:
            t0 = time.perf_counter()
            ctx.dev_download(out, p)
            t.append(time.perf_counter() - t0)
    say(f"for comparison, the download of the BGR frame (FrameWarper.__call__ today): {1e3 * np.median(t):.2f} ms per frame (median of {len(t)}, min {1e3 * np.min(t):.2f})")
    t = []
    for _ in range(2):
        for f in frames:
            im = Image.fromarray(np.ascontiguousarray(f[..., ::-1]), "RGB")
            t0 = time.perf_counter()
            buf = io.BytesIO()
            im.save(buf, "JPEG", quality=90, subsampling=2)
            t.append(time.perf_counter() - t0)
    say(f"for comparison, Pillow (libjpeg-turbo) encoding the frame on one host thread: {1e3 * np.median(t):.2f} ms per frame (median of {len(t)}, min {1e3 * np.min(t):.2f})")
    for p in dptrs:
        ctx.dev_free(p)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
