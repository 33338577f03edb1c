"""Recodes a Motion-JPEG clip or a folder of .jpg frames with restart markers, once, so that later runs Huffman-decode it on the
GPU one lane per restart interval (`engine: {jpeg_restart: gpu}`, csrc/jpeg_restart.hip). Lossless on coefficients: every frame
is parsed into its record and emitted again with the Annex K.3 tables (geotrax_amd.jpeg.recode_with_restarts), so the decoded
pixels do not change. Host only: no GPU is touched.

    python -m geotrax_amd.jpeg_restart IN.mjpeg|IN.avi|DIR OUT (--rows K | --mcus N) [--threads T]

  --rows K   a restart marker every K MCU rows of the frame (K = 1: one interval per MCU row)
  --mcus N   a restart marker every N MCUs (1..65535)

OUT is a .avi / .mjpeg / .mjpg file for a clip, a folder (created; the frames keep their names) for a folder. Short intervals
decode faster and cost more bytes: DESIGN.md 7f has the figures."""
from __future__ import annotations

import argparse
import logging
import sys
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

from . import _lib, jpeg
from .frames import open_source
from .georef_stage import DEFAULT_FPS
from .video_writer import MjpegWriter, check_restart_interval


def interval_of(blob, rows: int | None, mcus: int | None) -> int:
    """The restart interval in MCUs that --rows / --mcus ask for on this frame; ValueError outside 1..65535."""
    if (rows is None) == (mcus is None):
        raise ValueError("give one of --rows K and --mcus N")
    if rows is not None and rows < 1:
        raise ValueError(f"--rows {rows}: at least 1")
    n = int(mcus) if mcus is not None else int(rows) * jpeg.mcus_per_row(blob)
    if n < 1:
        raise ValueError(f"--mcus {n}: at least 1")
    return check_restart_interval("host", n)


def _frame_bytes(layout, i: int) -> bytes:
    paths, findex, offsets, lengths = layout
    with open(paths[int(findex[i])], "rb") as f:
        f.seek(int(offsets[i]))
        return f.read(int(lengths[i]))


def recode(source, out, rows: int | None = None, mcus: int | None = None, threads: int = 8, logger: logging.Logger | None = None) -> tuple[int, int, int]:
    """Recodes `source` into `out`; returns (frames, bytes read, bytes written)."""
    log = logger or logging.getLogger(__name__)
    source, out = Path(source), Path(out)
    reader = open_source(source)
    try:
        layout = reader.jpeg_layout() if hasattr(reader, "jpeg_layout") else None
        if layout is None:
            raise ValueError(f"'{source}' is no Motion-JPEG clip (.mjpeg, .mjpg, MJPG .avi) and no folder of baseline .jpg frames")
        n = len(layout[1])
        if n == 0:
            raise ValueError(f"'{source}' has no frames")
        n_in = n_out = 0
        if source.is_dir():
            out.mkdir(parents=True, exist_ok=True)
            if out.resolve() == source.resolve():
                raise ValueError("OUT is the input folder")

            def one(i):
                blob = _frame_bytes(layout, i)
                new = jpeg.recode_with_restarts(blob, interval_of(blob, rows, mcus), i)
                (out / Path(layout[0][int(layout[1][i])]).name).write_bytes(new)
                return len(blob), len(new)

            with ThreadPoolExecutor(max_workers=max(int(threads), 1)) as pool:
                for a, b in pool.map(one, range(n)):
                    n_in, n_out = n_in + a, n_out + b
        else:
            h, w = reader.frame_hw
            interval = interval_of(_frame_bytes(layout, 0), rows, mcus)
            fps = getattr(reader, "fps", 0.0) or DEFAULT_FPS
            out.parent.mkdir(parents=True, exist_ok=True)
            writer = MjpegWriter(out, fps, (w, h), encode_threads=max(int(threads), 1), restart_interval=interval)
            try:
                for i in range(n):
                    blob = _frame_bytes(layout, i)
                    n_in += len(blob)
                    writer.write_record(jpeg.parse(blob, i)[0])
            finally:
                writer.release()
            n_out = out.stat().st_size
        log.info(f"'{out}': {n} frames, {n_in} bytes of pictures read, {n_out} bytes written ({100 * (n_out / max(n_in, 1) - 1):+.2f} %)")
        return n, n_in, n_out
    finally:
        reader.release()


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m geotrax_amd.jpeg_restart", description=__doc__.split("\n\n")[0])
    ap.add_argument("source", type=Path, help="a .mjpeg / .mjpg / MJPG .avi clip, or a folder of .jpg frames")
    ap.add_argument("out", type=Path, help="the clip (.avi, .mjpeg, .mjpg) or folder to write")
    g = ap.add_mutually_exclusive_group(required=True)
    g.add_argument("--rows", type=int, default=None, metavar="K", help="a restart marker every K MCU rows")
    g.add_argument("--mcus", type=int, default=None, metavar="N", help="a restart marker every N MCUs")
    ap.add_argument("--threads", type=int, default=8, help="host threads that Huffman-code the frames")
    args = ap.parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(message)s")
    try:
        recode(args.source, args.out, args.rows, args.mcus, args.threads)
    except (OSError, ValueError, RuntimeError, _lib.GtxError) as e:
        logging.getLogger(__name__).error(str(e))
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
