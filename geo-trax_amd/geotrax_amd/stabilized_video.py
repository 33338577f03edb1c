"""The stabilized clip: `geotrax visualize --viz-mode 1`'s frame source (geotrax/visualize.py:268-298) without the drawing.

Every frame of the clip is warped into the reference frame with its row of `<stem>_vid_transf.txt`
(cv2.warpPerspective(frame, transforms[frame_num], (w, h)), visualize.py:289; a frame without a row -- the reference frame,
an unregistered frame -- passes through unchanged, :285) and written as Motion-JPEG. The frames never visit the host: the
read-ahead feeder puts them into HBM, gtx_warp_frame_dev and the JPEG encoder (geotrax_amd.video_writer) run there, and only
the packed coefficient records come back for Huffman coding.

    python -m geotrax_amd.stabilized_video <clip> [--quality Q] [--entropy host|gpu] [--restart-interval N] [--cut-frame-left N] [--cut-frame-right N] [-o PATH]
"""
from __future__ import annotations

import argparse
import ctypes as C
import logging
import sys
from pathlib import Path

import numpy as np

from . import _lib
from .extract import get_output_dir
from .feeder import FrameFeeder
from .frames import Y4mReader, open_source
from .georef_stage import DEFAULT_FPS, build_result_path, detect_delimiter
from .video_writer import MjpegWriter, check_restart_interval


def visualized_path(source: Path, out_cfg: dict | None = None, viz_mode: int = 1, ext: str = "avi") -> Path:
    """file_utils.build_result_path(source, 'visualized', cfg, viz_mode, ext) (:69-70)."""
    cfg = out_cfg or {}
    return get_output_dir(source, cfg) / f"{Path(source).stem}{cfg.get('visualization_postfix', '')}_mode_{viz_mode}.{ext}"


def load_transforms(path: Path) -> dict[int, np.ndarray]:
    """visualize.py:550-570: rows of frame number + 9 matrix entries -> {frame: 3x3}; determinants must be positive."""
    t = np.loadtxt(path, delimiter=detect_delimiter(path), ndmin=2)
    if t.shape[1] != 10:
        raise ValueError(f"'{path}': {t.shape[1]} columns, a transforms file has 10")
    mats = t[:, 1:].reshape(-1, 3, 3)
    if not np.all(np.linalg.det(mats) > 0):
        raise ValueError(f"'{path}': a transform with a determinant that is not positive")
    return {int(n): m for n, m in zip(t[:, 0], mats)}


def _open_feeder(reader, first: int, stop: int, batch: int, ring: int, ctx: _lib.Context) -> FrameFeeder:
    """The clip's frames first..stop-1 through the read-ahead feeder, whichever way the reader lets them be read."""
    raw = reader.raw_layout() if hasattr(reader, "raw_layout") else None
    jl = reader.jpeg_layout() if raw is None and hasattr(reader, "jpeg_layout") else None
    if raw is not None:
        path, kind, offsets = raw
        fd = FrameFeeder(reader.frame_hw, kind=kind, batch=batch, ring=ring, device=ctx.device)
        fd.open_file(path, offsets[first:stop])
    elif jl is not None:
        paths, findex, offsets, lengths = jl
        fd = FrameFeeder(reader.frame_hw, kind="jpeg", batch=batch, ring=ring, device=ctx.device)
        fd.open_jpeg((paths, findex[first:stop], offsets[first:stop], lengths[first:stop]))
    else:
        fd = FrameFeeder(reader.frame_hw, kind="i420" if isinstance(reader, Y4mReader) else "bgr", batch=batch, ring=ring, device=ctx.device)

        def frames():
            k = 0
            while k < stop:
                ok, f = reader.read()
                if not ok:
                    return
                if k >= first:
                    yield f
                k += 1

        fd.open_reader(frames())
    return fd


def write_stabilized(source, out_path=None, transforms_path=None, quality: int = 90, subsampling: str = "4:2:0", cut_frame_left: int = 0,
                     cut_frame_right: int | None = None, out_cfg: dict | None = None, encode_threads: int = 8, ctx: _lib.Context | None = None,
                     logger: logging.Logger | None = None, entropy: str = "host", restart_interval: int = 0) -> tuple[Path, int]:
    """Writes the stabilized clip; returns (path, frames written). Frames cut_frame_left .. cut_frame_right - 1 are written
    (visualize.py:272-279: the loop breaks when it reaches cut_frame_right). restart_interval > 0: a restart marker every that
    many MCUs (host emitter only), so that the clip reads back one GPU lane per interval (`engine: {jpeg_restart: gpu}`)."""
    check_restart_interval(entropy, restart_interval)
    log = logger or logging.getLogger(__name__)
    source = Path(source)
    ctx = ctx or _lib.default_context()
    tpath = Path(transforms_path) if transforms_path else build_result_path(source, "video_transformations", out_cfg)
    transforms = load_transforms(tpath)
    out = Path(out_path) if out_path else visualized_path(source, out_cfg)
    reader = open_source(source)
    fd = None
    try:
        h, w = reader.frame_hw
        first = max(int(cut_frame_left or 0), 0)
        stop = reader.frame_count if cut_frame_right is None else min(reader.frame_count, max(int(cut_frame_right), first))
        fps = getattr(reader, "fps", 0.0) or DEFAULT_FPS
        out.parent.mkdir(parents=True, exist_ok=True)
        batch, n_written = 2, 0
        writer = MjpegWriter(out, fps, (w, h), quality=quality, subsampling=subsampling, encode_threads=encode_threads, ctx=ctx, entropy=entropy,
                             restart_interval=restart_interval)
        # a frame is read by its encoder's launches until the writer's ring has come round: that many batches stay with us
        keep = writer.ring // batch + 2
        warped = [ctx.dev_alloc(h * w * 3) for _ in range(writer.ring)]
        try:
            fd = _open_feeder(reader, first, stop, batch, keep + 3, ctx)
            for b in fd.batches(keep):
                b.wait_on(ctx)                             # the context's stream runs behind the batch's upload
                for k in range(b.n):
                    frame_num = first + n_written
                    src = b.ptr + k * h * w * 3
                    H = transforms.get(frame_num)
                    if H is not None:
                        dst = warped[n_written % writer.ring]
                        Hm = np.ascontiguousarray(H, dtype=np.float64).reshape(9)
                        _lib.check(ctx.lib.gtx_warp_frame_dev(ctx.handle, C.c_void_p(src), h, w, _lib.ptr(Hm), C.c_void_p(dst)))
                        src = dst
                    writer.write_dev(src)
                    n_written += 1
        finally:
            writer.release()
            for p in warped:
                ctx.dev_free(p)
        log.info(f"'{out}': {n_written} frames, {len(transforms)} transforms, {writer.record_bytes / max(n_written, 1) / 1e6:.2f} MB of record per frame")
        return out, n_written
    finally:
        if fd is not None:
            fd.close()
        reader.release()


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m geotrax_amd.stabilized_video", description=__doc__.split("\n\n")[0])
    ap.add_argument("source", type=Path, help="the clip (its transforms are read from <output folder>/<stem>_vid_transf.txt)")
    ap.add_argument("--quality", type=int, default=90, help="JPEG quality, 1..100 (libjpeg's scale)")
    ap.add_argument("--subsampling", choices=["4:2:0", "4:4:4"], default="4:2:0")
    ap.add_argument("--cut-frame-left", "-cfl", type=int, default=0, help="skip the first N frames")
    ap.add_argument("--cut-frame-right", "-cfr", type=int, default=None, help="stop when this frame is reached")
    ap.add_argument("--transforms", type=Path, default=None, help="another transforms file")
    ap.add_argument("--encode-threads", type=int, default=8)
    ap.add_argument("--entropy", choices=["host", "gpu"], default="host", help="where the pictures are Huffman-coded: host threads, or the GPU")
    ap.add_argument("--restart-interval", type=int, default=0, metavar="N",
                    help="a restart marker every N MCUs (0: none), so that the clip is read back one GPU lane per interval; needs --entropy host")
    ap.add_argument("-o", "--output", type=Path, default=None, help="the file to write (.avi, .mjpeg); default <output folder>/<stem>_mode_1.avi")
    args = ap.parse_args(argv)
    check_restart_interval(args.entropy, args.restart_interval)   # ValueError: the GPU coder and restart markers do not go together
    logging.basicConfig(level=logging.INFO, format="%(message)s")
    try:
        write_stabilized(args.source, args.output, args.transforms, args.quality, args.subsampling, args.cut_frame_left, args.cut_frame_right,
                         encode_threads=args.encode_threads, entropy=args.entropy, restart_interval=args.restart_interval)
    except (OSError, ValueError, _lib.GtxError) as e:
        logging.getLogger(__name__).error(str(e))
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
