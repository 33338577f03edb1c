"""Host twin of csrc/jpeg.hip: packed record -> sample planes -> BGR in numpy, with the kernels' arithmetic line for line
(libjpeg's default decode: slow-integer IDCT, fancy h2v1 / h2v2 upsampling, 16-bit YCbCr tables), the way
frames.yuv420_to_bgr_host twins csrc/yuv.hip. The record comes from the C parser (gtx_jpeg_parse: host only, no GPU). It makes
Pillow comparable with this build's decode on a machine without a GPU and serves callers that need an ndarray (reference-frame
consumers, tests); the pipeline's frames are decoded by the feeder (geotrax_amd.feeder, kind "jpeg").

Record layout: csrc/jpeg_parse.hpp."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib

MAGIC = 0x3152474A
HEADER_BYTES, QUANT_OFFSET, OFFSETS_OFFSET = 80, 80, 80 + 3 * 64 * 2
NATURAL = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])


class JpegError(_lib.GtxError):
    pass


def parse(data, frame: int = 0):
    """One compressed frame -> (record as a uint8 array, info dict). Raises JpegError (status -3: a variant outside the accepted
    set, the message names the marker; -1: damaged data)."""
    lib = _lib.load()
    raw = bytes(data)
    buf = np.frombuffer(raw or b"\0", dtype=np.uint8)              # (an empty frame still needs a pointer to hand over)
    out = [C.c_int() for _ in range(5)]
    needed = C.c_size_t()

    def call(rec, cap):
        rc = lib.gtx_jpeg_parse(_lib.ptr(buf), len(raw), int(frame), *[C.byref(v) for v in out], rec, cap, C.byref(needed))
        if rc < 0:
            raise JpegError(rc, lib.gtx_last_error().decode("utf-8", "replace"))
        return rc

    call(None, 0)
    rec = np.zeros((needed.value + 3) // 4, dtype=np.uint32).view(np.uint8)[:needed.value]
    if call(_lib.ptr(rec), rec.nbytes) != 0:
        raise JpegError(-5, f"JPEG frame {frame}: the record did not fit the size the parser asked for")
    h, w, ncomp, hs, vs = (v.value for v in out)
    return rec, dict(h=h, w=w, ncomp=ncomp, hs=hs, vs=vs)


def record_fields(rec: np.ndarray):
    """The record's header as a dict, its quantisation tables [3][64], block offsets and coefficient stream (views)."""
    hd = rec[:HEADER_BYTES].view(np.uint32)
    if int(hd[0]) != MAGIC or int(hd[1]) != rec.nbytes:
        raise ValueError("not a JPEG record")
    f = dict(w=int(hd[2]), h=int(hd[3]), ncomp=int(hd[4]), hs=int(hd[5]), vs=int(hd[6]), mcus_x=int(hd[7]), mcus_y=int(hd[8]),
             n_blocks=int(hd[9]), n_coef=int(hd[10]), bw=[int(v) for v in hd[11:14]], bh=[int(v) for v in hd[14:17]])
    quant = rec[QUANT_OFFSET:OFFSETS_OFFSET].view(np.uint16).reshape(3, 64)
    end = OFFSETS_OFFSET + 4 * (f["n_blocks"] + 1)
    offsets = rec[OFFSETS_OFFSET:end].view(np.uint32)
    coefs = rec[end:end + 2 * f["n_coef"]].view(np.int16)
    return f, quant, offsets, coefs


def _idct8(x: np.ndarray, rnd: int, shift: int) -> np.ndarray:
    """jidctint.c's 1-D pass over the last axis (8 long) of an int32 array; int32 arithmetic like the kernel's."""
    i = [x[..., k] for k in range(8)]
    z2, z3 = i[2], i[6]
    z1 = (z2 + z3) * np.int32(4433)
    tmp2 = z1 + z3 * np.int32(-15137)
    tmp3 = z1 + z2 * np.int32(6270)
    z2, z3 = i[0], i[4]
    tmp0, tmp1 = (z2 + z3) * np.int32(8192), (z2 - z3) * np.int32(8192)
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    t0, t1, t2, t3 = i[7], i[5], i[3], i[1]
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * np.int32(9633)
    t0, t1, t2, t3 = t0 * np.int32(2446), t1 * np.int32(16819), t2 * np.int32(25172), t3 * np.int32(12299)
    z1, z2, z3, z4 = z1 * np.int32(-7373), z2 * np.int32(-20995), z3 * np.int32(-16069), z4 * np.int32(-3196)
    z3, z4 = z3 + z5, z4 + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    r = np.int32(rnd)
    out = [tmp10 + t3, tmp11 + t2, tmp12 + t1, tmp13 + t0, tmp13 - t0, tmp12 - t1, tmp11 - t2, tmp10 - t3]
    return np.stack([(o + r) >> shift for o in out], -1)


def record_to_planes(rec: np.ndarray) -> tuple[dict, list[np.ndarray]]:
    """Stage 1 (jpeg_idct_kernel): dequantise, 8x8 inverse DCT, +128, clamp -> one u8 plane per component at block-grid size."""
    f, quant, offsets, coefs = record_fields(rec)
    nb = f["n_blocks"]
    off = offsets.astype(np.int64)
    lens = np.clip(off[1:] - off[:-1], 0, 64)
    luma = f["hs"] * f["vs"]
    bpm = 1 if f["ncomp"] == 1 else luma + 2
    b = np.arange(nb)
    mcu, k = b // bpm, b % bpm
    mx, my = mcu % f["mcus_x"], mcu // f["mcus_x"]
    is_luma = (k < luma) | (f["ncomp"] == 1)
    comp = np.where(is_luma, 0, 1 + (k - luma))
    bx = np.where(is_luma, mx * f["hs"] + k % f["hs"], mx)
    by = np.where(is_luma, my * f["vs"] + k // f["hs"], my)
    # scatter the zigzag runs into natural order, dequantised (DEQUANTIZE: coefficient * table entry, as int)
    ws = np.zeros((nb, 64), np.int32)
    z = np.arange(64)
    valid = z[None, :] < lens[:, None]
    src = np.minimum(off[:-1, None] + z[None, :], max(len(coefs) - 1, 0))
    vals = np.where(valid, coefs[src] if len(coefs) else 0, 0).astype(np.int32)
    ws[:, NATURAL] = vals * quant[comp][:, NATURAL].astype(np.int32)
    ws = ws.reshape(nb, 8, 8)
    ws = _idct8(ws.transpose(0, 2, 1), 1 << 10, 11).transpose(0, 2, 1)      # pass 1: columns, scaled up by 2^PASS1_BITS
    px = np.clip(_idct8(ws, 1 << 17, 18) + 128, 0, 255).astype(np.uint8)    # pass 2: rows, level shift, clamp
    planes = []
    for c in range(f["ncomp"]):
        pl = np.zeros((f["bh"][c], 8, f["bw"][c], 8), np.uint8)
        sel = comp == c
        pl[by[sel], :, bx[sel], :] = px[sel]
        planes.append(pl.reshape(f["bh"][c] * 8, f["bw"][c] * 8))
    return f, planes


def _upsample(pl: np.ndarray, hs: int, vs: int, h: int, w: int) -> np.ndarray:
    """jdsample.c: the chroma plane at full size, int32 [h][w]. Edges are those of the real chroma plane (ceil(w / 2) x
    ceil(h / 2) where subsampled), not of the MCU padding; at most 2 chroma columns: replication instead of the triangle filter."""
    if hs == 1:
        return pl[:h, :w].astype(np.int32)
    cw, ch = (w + 1) // 2, ((h + 1) // 2 if vs == 2 else h)
    p = pl[:ch, :cw].astype(np.int32)
    if cw <= 2:
        return np.repeat(np.repeat(p, vs, 0), 2, 1)[:h, :w]
    if vs == 1:                                                    # h2v1_fancy_upsample
        left, right = np.concatenate([p[:, :1], p[:, :-1]], 1), np.concatenate([p[:, 1:], p[:, -1:]], 1)
        even, odd = (3 * p + left + 1) >> 2, (3 * p + right + 2) >> 2
        even[:, 0], odd[:, -1] = p[:, 0], p[:, -1]
        return np.stack([even, odd], -1).reshape(ch, 2 * cw)[:h, :w]
    # h2v2_fancy_upsample: the nearer row weighs 3, the farther 1 (past the first / last real row: the row itself)
    up, down = np.concatenate([p[:1], p[:-1]], 0), np.concatenate([p[1:], p[-1:]], 0)
    rows = np.stack([3 * p + up, 3 * p + down], 1).reshape(2 * ch, cw)     # column sums of output rows 2r, 2r + 1
    left, right = np.concatenate([rows[:, :1], rows[:, :-1]], 1), np.concatenate([rows[:, 1:], rows[:, -1:]], 1)
    even, odd = (3 * rows + left + 8) >> 4, (3 * rows + right + 7) >> 4
    even[:, 0], odd[:, -1] = (4 * rows[:, 0] + 8) >> 4, (4 * rows[:, -1] + 7) >> 4
    return np.stack([even, odd], -1).reshape(2 * ch, 2 * cw)[:h, :w]


def planes_to_bgr(f: dict, planes: list[np.ndarray]) -> np.ndarray:
    """Stage 2 (jpeg_colour_kernel): chroma upsampling, jdcolor.c's YCbCr -> RGB at 16 fixed-point bits, packed as BGR."""
    h, w = f["h"], f["w"]
    y = planes[0][:h, :w].astype(np.int32)
    if f["ncomp"] == 1:
        return np.ascontiguousarray(np.repeat(y[..., None], 3, -1).astype(np.uint8))
    u = _upsample(planes[1], f["hs"], f["vs"], h, w) - 128
    v = _upsample(planes[2], f["hs"], f["vs"], h, w) - 128
    half = 1 << 15
    r = y + ((91881 * v + half) >> 16)
    g = y + ((-22554 * u + half - 46802 * v) >> 16)
    b = y + ((116130 * u + half) >> 16)
    return np.ascontiguousarray(np.clip(np.stack([b, g, r], -1), 0, 255).astype(np.uint8))


def record_to_bgr(rec: np.ndarray) -> np.ndarray:
    return planes_to_bgr(*record_to_planes(rec))


def decode_host(data, frame: int = 0) -> np.ndarray:
    """One compressed JPEG frame -> BGR u8 [h][w][3], the bytes the GPU decode produces."""
    rec, _ = parse(data, frame)
    return record_to_bgr(rec)


def decode_dev(ctx: _lib.Context, rec: np.ndarray, h: int, w: int) -> np.ndarray:
    """One record through gtx_jpeg_decode_dev, downloaded (tests, tools)."""
    dst = ctx.dev_alloc(h * w * 3)
    try:
        _lib.check(ctx.lib.gtx_jpeg_decode_dev(ctx.handle, _lib.ptr(rec), rec.nbytes, h, w, C.c_void_p(dst)))
        out = np.empty((h, w, 3), np.uint8)
        ctx.dev_download(out, dst)
    finally:
        ctx.dev_free(dst)
    return out
