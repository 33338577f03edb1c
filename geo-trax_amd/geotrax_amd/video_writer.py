"""Motion-JPEG video writer over the C ABI (gtx_jpeg_enc_* / gtx_jpeg_emit): the cv2.VideoWriter of the reference's
visualisation loop (geotrax/visualize.py:131, :298), for frames that are already in HBM.

The GPU turns a BGR frame into a packed record of quantised coefficients (csrc/jpeg_enc.hip, a few MB instead of the frame's
25 MB at 4K), host threads Huffman-code the records into baseline JPEG pictures (csrc/jpeg_emit.cpp; the calls release the
GIL; with entropy="gpu" the GPU codes the pictures itself, csrc/jpeg_huff.hip, and only the finished picture leaves it), and
this module stores the pictures: suffix .avi -> RIFF AVI with one `vids` / `MJPG` stream, `00dc` chunks and an
`idx1` index, continued in `RIFF AVIX` lists before a RIFF would pass `riff_limit` bytes (OpenDML); suffix .mjpeg / .mjpg ->
the pictures one after the other. frames.AviMjpegReader / MjpegReader read both back.
"""
from __future__ import annotations

import ctypes as C
import struct
from collections import deque
from concurrent.futures import ThreadPoolExecutor
from fractions import Fraction
from pathlib import Path

import numpy as np

from . import _lib, jpeg
from ._lib import check


class _RawSink:
    """.mjpeg / .mjpg: the concatenated pictures."""

    def __init__(self, path, fps, size, riff_limit):
        self.f = open(path, "wb")

    def add(self, data: bytes) -> None:
        self.f.write(data)

    def close(self) -> None:
        self.f.close()


class _AviSink:
    """RIFF AVI, one MJPG video stream. Sizes and frame counts are patched when a RIFF list, and the file, is closed."""

    def __init__(self, path, fps, size, riff_limit):
        self.f = open(path, "wb")
        self.w, self.h = size
        self.limit = int(riff_limit)
        fr = Fraction(float(fps)).limit_denominator(100000)
        self.rate, self.scale = fr.numerator, fr.denominator
        self.total = 0                                     # frames in the file
        self.largest = 0
        self.index = []                                    # (offset from the first movi list's 'movi', length) of the first RIFF's frames
        f = self.f
        usec = round(1e6 * self.scale / self.rate) if self.rate else 0
        f.write(b"RIFF\0\0\0\0AVI ")
        f.write(b"LIST" + struct.pack("<I", 4 + 64 + (12 + 64 + 48) + (12 + 12)) + b"hdrl")
        self.avih_at = f.tell()
        f.write(b"avih" + struct.pack("<I14I", 56, usec, 0, 0, 0x10, 0, 0, 1, 0, self.w, self.h, 0, 0, 0, 0))
        f.write(b"LIST" + struct.pack("<I", 4 + 64 + 48) + b"strl")
        self.strh_at = f.tell()
        f.write(b"strh" + struct.pack("<I4s4sIHHIIIIIIII4H", 56, b"vids", b"MJPG", 0, 0, 0, 0, self.scale, self.rate, 0, 0, 0, 0xFFFFFFFF, 0,
                                      0, 0, self.w, self.h))
        f.write(b"strf" + struct.pack("<IIiiHH4sIiiII", 40, 40, self.w, self.h, 1, 24, b"MJPG", self.w * self.h * 3, 0, 0, 0, 0))
        f.write(b"LIST" + struct.pack("<I", 4 + 12) + b"odml")
        self.dmlh_at = f.tell()
        f.write(b"dmlh" + struct.pack("<II", 4, 0))
        self.riff_at, self.first = 0, True
        self._open_movi()

    def _open_movi(self) -> None:
        self.movi_at = self.f.tell()
        self.f.write(b"LIST\0\0\0\0movi")
        self.in_riff = 0

    def _close_riff(self) -> None:
        f = self.f
        end = f.tell()
        f.seek(self.movi_at + 4)
        f.write(struct.pack("<I", end - self.movi_at - 8))
        f.seek(end)
        if self.first:                                     # the index of the first RIFF's frames, offsets from the 'movi' tag
            f.write(b"idx1" + struct.pack("<I", 16 * len(self.index)))
            for off, n in self.index:
                f.write(b"00dc" + struct.pack("<III", 0x10, off, n))
            self.first_frames = self.in_riff
            end = f.tell()
        f.seek(self.riff_at + 4)
        f.write(struct.pack("<I", end - self.riff_at - 8))
        f.seek(end)
        self.first = False

    def add(self, data: bytes) -> None:
        f = self.f
        n = len(data)
        after = f.tell() + 8 + n + (n & 1) - self.riff_at + (8 + 16 * (self.in_riff + 1) if self.first else 0)
        if after > self.limit and self.in_riff > 0:        # this RIFF would pass the limit: go on in a RIFF AVIX list
            self._close_riff()
            self.riff_at = f.tell()
            f.write(b"RIFF\0\0\0\0AVIX")
            self._open_movi()
        if self.first:
            self.index.append((f.tell() - (self.movi_at + 8), n))
        f.write(b"00dc" + struct.pack("<I", n))
        f.write(data)
        if n & 1:
            f.write(b"\0")
        self.in_riff += 1
        self.total += 1
        self.largest = max(self.largest, n)

    def close(self) -> None:
        f = self.f
        self._close_riff()
        end = f.tell()
        f.seek(self.avih_at + 8 + 16)
        f.write(struct.pack("<I", self.first_frames))     # dwTotalFrames: the first RIFF's (OpenDML keeps the file's in dmlh)
        f.seek(self.avih_at + 8 + 28)
        f.write(struct.pack("<I", self.largest))          # dwSuggestedBufferSize
        f.seek(self.strh_at + 8 + 32)
        f.write(struct.pack("<II", self.total, self.largest))   # dwLength, dwSuggestedBufferSize
        f.seek(self.dmlh_at + 8)
        f.write(struct.pack("<I", self.total))
        f.seek(end)
        f.close()


class _Slot:
    __slots__ = ("enc", "dbuf", "busy")


def check_restart_interval(entropy: str, restart_interval: int) -> int:
    """The restart interval a writer may use with this entropy route, or ValueError: 0..65535 MCUs (what a DRI segment holds), and
    above 0 only with the host emitter (the GPU Huffman coder writes one unbroken scan). The stages' command lines call it as
    soon as their arguments are parsed, before any file or GPU is touched."""
    n = int(restart_interval)
    if not 0 <= n <= 65535:
        raise ValueError(f"restart interval {restart_interval} is outside 0..65535 MCUs")
    if entropy == "gpu" and n > 0:
        raise ValueError(f"a restart interval ({n} MCUs) needs the host emitter (--entropy host, entropy='host'): the GPU Huffman coder writes one unbroken scan")
    return n


class MjpegWriter:
    """cv2.VideoWriter's shape: MjpegWriter(path, fps, (w, h)); write(frame) / write_dev(dptr); release().

    A ring of `ring` encoder objects keeps submit and collect apart: write_dev() enqueues the frame's launches and returns, the
    record is collected when the slot comes round again (or at release()), then Huffman-coded on one of `encode_threads` pool
    threads (a parameter, never the machine's CPU count: the engine has threads of its own). Pictures reach the file strictly
    in submission order. A frame given to write_dev() is read on the context's stream: it must stay unchanged until `ring`
    further frames have been written or release() has returned, unless what overwrites it is ordered on that stream.

    entropy="gpu" (default "host") puts the ring's encoders on the GPU entropy route: a collected slot hands over the finished
    picture, which goes straight to the file; the thread pool is not used. write_record() is host coding on either setting.

    restart_interval=N (default 0: none) has the host emitter put a restart marker after every N MCUs (jpeg.emit), so that the
    file reads back one GPU lane per interval (`engine: {jpeg_restart: gpu}`); the same coefficients either way. It needs
    entropy="host": the GPU Huffman coder writes one unbroken scan."""

    ENTROPY = ("host", "gpu")

    def __init__(self, path, fps: float, size: tuple[int, int], quality: int = 90, subsampling: str = "4:2:0", encode_threads: int = 8,
                 ctx: _lib.Context | None = None, ring: int = 3, riff_limit: int = 1 << 30, entropy: str = "host", restart_interval: int = 0):
        if entropy not in self.ENTROPY:
            raise ValueError(f"entropy {entropy!r}: one of {list(self.ENTROPY)}")
        check_restart_interval(entropy, restart_interval)
        self.restart_interval = int(restart_interval)
        self.entropy = entropy
        self.path = Path(path)
        self.w, self.h = int(size[0]), int(size[1])
        self.quality = int(quality)
        jpeg.quality_tables(self.quality)                  # refuses the quality
        if subsampling not in jpeg.SUBSAMPLINGS:
            raise ValueError(f"JPEG subsampling {subsampling!r}: one of {sorted(jpeg.SUBSAMPLINGS)}")
        if not (1 <= self.w <= 16384 and 1 <= self.h <= 16384):
            raise ValueError(f"a {self.w} x {self.h} frame is outside 1..16384")
        if not 1 <= int(encode_threads) <= 64:
            raise ValueError(f"encode_threads {encode_threads} is outside 1..64")
        self.subsampling = subsampling
        sink = {".avi": _AviSink, ".mjpeg": _RawSink, ".mjpg": _RawSink}.get(self.path.suffix.lower())
        if sink is None:
            raise ValueError(f"'{path}': the suffix decides the container: .avi, .mjpeg or .mjpg")
        self.lib = _lib.load()
        self._ctx = ctx
        self.ring = max(int(ring), 1)
        self._slots: list[_Slot] = []
        self._next = 0
        self._guess = 1 << 16                              # record bytes of the frame before, the size of the next buffer
        self._pool = ThreadPoolExecutor(max_workers=int(encode_threads), thread_name_prefix="gtx-jpeg-emit")
        self._max_pending = 2 * int(encode_threads) + self.ring
        self._pending: deque = deque()
        self.frames = 0
        self.record_bytes = 0                              # of all frames: what left the GPU (records, or pictures with entropy="gpu")
        self._sink = sink(self.path, fps, (self.w, self.h), riff_limit)

    def isOpened(self) -> bool:  # noqa: N802 (cv2 naming)
        return self._sink is not None

    # ---- GPU side
    def _slot(self) -> _Slot:
        if not self._slots:
            self._ctx = self._ctx or _lib.default_context()
            for _ in range(self.ring):
                s = _Slot()
                h = C.c_void_p()
                check(self.lib.gtx_jpeg_enc_create(self._ctx.handle, self.h, self.w, self.quality, jpeg.SUBSAMPLINGS[self.subsampling][2], C.byref(h)))
                s.enc, s.dbuf, s.busy = h, None, False
                self._slots.append(s)
                if self.entropy == "gpu":
                    check(self.lib.gtx_jpeg_enc_set_entropy(h, 1))
        s = self._slots[self._next]
        self._next = (self._next + 1) % self.ring
        if s.busy:
            self._collect(s)
        return s

    def _collect(self, s: _Slot) -> None:
        n = C.c_size_t()
        if self.entropy == "gpu":                          # the finished picture: nothing left for the pool
            pic = np.empty(self._guess, np.uint8)
            rc = self.lib.gtx_jpeg_enc_collect_jpeg(s.enc, _lib.ptr(pic), pic.nbytes, C.byref(n))
            if rc == 1:
                pic = np.empty(n.value, np.uint8)
                rc = self.lib.gtx_jpeg_enc_collect_jpeg(s.enc, _lib.ptr(pic), pic.nbytes, C.byref(n))
            check(rc)
            s.busy = False
            self._guess = n.value + n.value // 8
            self.record_bytes += n.value
            self._drain(True)                              # records given to write_record() before this frame come first
            self._sink.add(pic[:n.value].tobytes())
            self.frames += 1
            return
        rec = np.empty((self._guess + 3) // 4, np.uint32).view(np.uint8)
        rc = self.lib.gtx_jpeg_enc_collect(s.enc, _lib.ptr(rec), rec.nbytes, C.byref(n))
        if rc == 1:                                        # larger than the frame before: its real length is known now
            rec = np.empty((n.value + 3) // 4, np.uint32).view(np.uint8)
            rc = self.lib.gtx_jpeg_enc_collect(s.enc, _lib.ptr(rec), rec.nbytes, C.byref(n))
        check(rc)
        s.busy = False
        self._guess = n.value + n.value // 8
        self.write_record(rec[:n.value], _ordered=True)

    def _flush_gpu(self) -> None:
        for k in range(self.ring):                         # oldest first: the slot that comes round next
            s = self._slots[(self._next + k) % self.ring] if self._slots else None
            if s is not None and s.busy:
                self._collect(s)

    def write_dev(self, dptr: int) -> None:
        """One BGR u8 [h][w][3] frame at device address `dptr`. Asynchronous."""
        s = self._slot()
        check(self.lib.gtx_jpeg_enc_submit_dev(s.enc, C.c_void_p(int(dptr))))
        s.busy = True

    def write(self, frame: np.ndarray) -> None:
        """One host BGR frame: uploaded into the slot's own HBM buffer, then as write_dev()."""
        f = np.ascontiguousarray(frame, dtype=np.uint8)
        if f.shape != (self.h, self.w, 3):
            raise ValueError(f"frame is {f.shape}, the writer was opened for {(self.h, self.w, 3)}")
        s = self._slot()
        if s.dbuf is None:
            s.dbuf = self._ctx.dev_alloc(f.nbytes)
        self._ctx.dev_upload(s.dbuf, f)
        check(self.lib.gtx_jpeg_enc_submit_dev(s.enc, C.c_void_p(s.dbuf)))
        s.busy = True

    # ---- host side
    def write_record(self, rec: np.ndarray, _ordered: bool = False) -> None:
        """One frame as a record (from the encoder, or from jpeg.bgr_to_record / jpeg.parse): Huffman-coded on the pool."""
        if not _ordered:
            self._flush_gpu()                              # frames still on the GPU were submitted before this one
        f = jpeg.record_fields(rec)[0]
        if (f["w"], f["h"]) != (self.w, self.h):
            raise ValueError(f"the record is of a {f['w']} x {f['h']} frame, the writer was opened for {self.w} x {self.h}")
        self.record_bytes += rec.nbytes
        self._pending.append(self._pool.submit(jpeg.emit, rec, self.restart_interval) if self.restart_interval else self._pool.submit(jpeg.record_to_bytes, rec))
        self._drain(False)

    def _drain(self, everything: bool) -> None:
        while self._pending and (everything or self._pending[0].done() or len(self._pending) > self._max_pending):
            self._sink.add(self._pending.popleft().result())
            self.frames += 1

    def release(self) -> None:
        if self._sink is None:
            return
        try:
            self._flush_gpu()
            self._drain(True)
        finally:
            self._pool.shutdown(wait=True)
            self._sink.close()
            self._sink = None
            for s in self._slots:
                self.lib.gtx_jpeg_enc_destroy(s.enc)
                if s.dbuf is not None:
                    self._ctx.dev_free(s.dbuf)
            self._slots = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.release()

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass
