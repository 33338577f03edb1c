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


# ---------------------------------------------------------------------------------------------------------------- encode
# The decode run backwards: BGR frame -> the same packed record (host twin of csrc/jpeg_enc.hip), libjpeg's integer definition
# step by step (jccolor.c, jcsample.c, jcprepct.c, jfdctint.c, jcdctmgr.c, jccoefct.c), so that the record equals the one the
# parser reads out of the file Pillow / libjpeg-turbo writes for the same pixels. record_to_bytes() is the host emitter
# (csrc/jpeg_emit.cpp): record -> baseline JFIF bytes.

SUBSAMPLINGS = {"4:4:4": (1, 1, 0), "4:2:0": (2, 2, 2)}            # name -> (hs, vs, the C ABI's number: libjpeg-turbo's TJSAMP)
# ITU T.81 Annex K.1 / K.2, natural (row-major) order
STD_LUMA_QUANT = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                           18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99])
STD_CHROMA_QUANT = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99]
                            + [99] * 32)


def quality_tables(quality: int) -> np.ndarray:
    """jpeg_set_quality(quality, force_baseline): jpeg_quality_scaling applied to the Annex K tables, clamped to 1..255.
    uint16 [2][64] (luma, chroma), natural order."""
    q = int(quality)
    if not 1 <= q <= 100:
        raise ValueError(f"JPEG quality {quality} is outside 1..100")
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return np.stack([np.clip((t * scale + 50) // 100, 1, 255) for t in (STD_LUMA_QUANT, STD_CHROMA_QUANT)]).astype(np.uint16)


def bgr_to_planes(bgr: np.ndarray, subsampling: str = "4:2:0") -> tuple[dict, list[np.ndarray]]:
    """Stage 1 (jpeg_planes_kernel): jccolor.c's RGB -> YCbCr at 16 fixed-point bits, edge replication, jcsample.c's h2v2
    downsampling. Returns the record's geometry and the u8 planes Y, Cb, Cr at their padded block-grid sizes.

    Edges as libjpeg pads them: columns repeat the last pixel (expand_right_edge) and input rows repeat the last row up to an
    even count before the chroma is formed; the rows below that repeat the last *downsampled* row (jcprepct.c pads its output)."""
    if subsampling not in SUBSAMPLINGS:
        raise ValueError(f"JPEG subsampling {subsampling!r}: one of {sorted(SUBSAMPLINGS)}")
    a = np.asarray(bgr)
    if a.ndim != 3 or a.shape[2] != 3 or a.dtype != np.uint8:
        raise ValueError(f"expected an [h, w, 3] uint8 frame, got {a.dtype} {a.shape}")
    h, w = a.shape[:2]
    if not (1 <= h <= 16384 and 1 <= w <= 16384):
        raise ValueError(f"a {w} x {h} frame is outside 1..16384")
    hs, vs, _ = SUBSAMPLINGS[subsampling]
    mcus_x, mcus_y = -(-w // (8 * hs)), -(-h // (8 * vs))
    f = dict(w=w, h=h, ncomp=3, hs=hs, vs=vs, mcus_x=mcus_x, mcus_y=mcus_y, n_blocks=mcus_x * mcus_y * (hs * vs + 2),
             bw=[mcus_x * hs, mcus_x, mcus_x], bh=[mcus_y * vs, mcus_y, mcus_y])
    b, g, r = (a[..., k].astype(np.int32) for k in range(3))
    half = 1 << 15
    y = (19595 * r + 38470 * g + 7471 * b + half) >> 16
    off = (128 << 16) + half - 1                                   # CBCR_OFFSET + ONE_HALF - 1
    cb = (-11059 * r - 21709 * g + 32768 * b + off) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + off) >> 16

    def pad(p, ph, pw):                                            # replicate the last column, then the last row
        return np.pad(p, ((0, ph - p.shape[0]), (0, pw - p.shape[1])), mode="edge")

    planes = [pad(y, 8 * f["bh"][0], 8 * f["bw"][0])]
    for c in (cb, cr):
        if hs == 2:                                                # h2v2_downsample: 2x2 box, bias 1, 2, 1, 2, ... along a row
            c = pad(c, h + (h & 1), 16 * mcus_x)
            bias = 1 + (np.arange(c.shape[1] // 2) & 1)
            c = (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + bias[None, :]) >> 2
        planes.append(pad(c, 8 * mcus_y, 8 * mcus_x))
    return f, [p.astype(np.uint8) for p in planes]


def _fdct8(x: np.ndarray, first: bool) -> np.ndarray:
    """jfdctint.c's 1-D pass over the last axis (8 long) of an int32 array. first: the row pass (results scaled up by
    2^PASS1_BITS), else the column pass (PASS1_BITS removed again; the output stays scaled by 8)."""
    d = [x[..., k] for k in range(8)]
    tmp0, tmp7, tmp1, tmp6 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6]
    tmp2, tmp5, tmp3, tmp4 = d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    sh = 11 if first else 15                                       # CONST_BITS -/+ PASS1_BITS
    rnd = np.int32(1 << (sh - 1))
    o = [None] * 8
    if first:
        o[0], o[4] = (tmp10 + tmp11) << 2, (tmp10 - tmp11) << 2
    else:
        o[0], o[4] = (tmp10 + tmp11 + 2) >> 2, (tmp10 - tmp11 + 2) >> 2
    z1 = (tmp12 + tmp13) * np.int32(4433)
    o[2] = (z1 + tmp13 * np.int32(6270) + rnd) >> sh
    o[6] = (z1 + tmp12 * np.int32(-15137) + rnd) >> sh
    z1, z2, z3, z4 = tmp4 + tmp7, tmp5 + tmp6, tmp4 + tmp6, tmp5 + tmp7
    z5 = (z3 + z4) * np.int32(9633)
    tmp4, tmp5, tmp6, tmp7 = tmp4 * np.int32(2446), tmp5 * np.int32(16819), tmp6 * np.int32(25172), tmp7 * np.int32(12299)
    z1, z2, z3, z4 = z1 * np.int32(-7373), z2 * np.int32(-20995), z3 * np.int32(-16069), z4 * np.int32(-3196)
    z3, z4 = z3 + z5, z4 + z5
    o[7], o[5] = (tmp4 + z1 + z3 + rnd) >> sh, (tmp5 + z2 + z4 + rnd) >> sh
    o[3], o[1] = (tmp6 + z2 + z3 + rnd) >> sh, (tmp7 + z1 + z4 + rnd) >> sh
    return np.stack(o, -1)


def _quantised_blocks(plane: np.ndarray, quant: np.ndarray) -> np.ndarray:
    """Every 8x8 block of a padded plane: -128, forward DCT, jcdctmgr.c's quantisation -> int32 [bh][bw][64], natural order."""
    bh, bw = plane.shape[0] // 8, plane.shape[1] // 8
    x = plane.reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3).astype(np.int32) - 128
    x = _fdct8(x, True)                                            # rows
    x = _fdct8(x.transpose(0, 1, 3, 2), False).transpose(0, 1, 3, 2)   # columns
    x = x.reshape(bh, bw, 64)
    div = quant.astype(np.int32)[None, None, :] << 3              # the DCT's output is scaled by 8
    mag = (np.abs(x) + (div >> 1)) // div                          # truncating division of the magnitude: rounds half away from zero
    return np.where(x < 0, -mag, mag).astype(np.int32)


def planes_to_record(f: dict, planes: list[np.ndarray], quality: int = 90) -> np.ndarray:
    """Stages 2-4 (jpeg_fdct_kernel, the prefix sum, the compaction): planes -> record. Blocks past a component's own block grid
    (ceil(w / 8) x ceil(h / 8) of its samples) that only fill up an MCU are jccoefct.c's dummy blocks: no AC, the DC of the
    block before them in the MCU (right edge: the last real block of the row; bottom row: the last block of the MCU's row above)."""
    qt = quality_tables(quality)
    quant = np.stack([qt[0], qt[1], qt[1]])
    hs, vs, mcus_x, mcus_y = f["hs"], f["vs"], f["mcus_x"], f["mcus_y"]
    comps = [_quantised_blocks(planes[c], quant[c]) for c in range(3)]
    rbw, rbh = -(-f["w"] // 8), -(-f["h"] // 8)                    # luma's own block grid
    lum = comps[0]
    if rbw < f["bw"][0]:                                           # hs == 2 and an odd count: the MCU's second column is dummy
        lum[:, rbw:, :] = 0
        lum[:, rbw:, 0] = lum[:, rbw - 1:rbw, 0]
    if rbh < f["bh"][0]:                                           # the MCU's second row is dummy: DC of the last block of its first row
        lum[rbh:, :, :] = 0
        src = lum[rbh - 1, :, 0].reshape(mcus_x, hs)[:, hs - 1]
        lum[rbh, :, 0] = np.repeat(src, hs)
    # scan order: MCU by MCU, hs x vs luma blocks row by row, Cb, Cr
    mcu_l = lum.reshape(mcus_y, vs, mcus_x, hs, 64).transpose(0, 2, 1, 3, 4).reshape(mcus_y, mcus_x, hs * vs, 64)
    blocks = np.concatenate([mcu_l, comps[1][:, :, None, :], comps[2][:, :, None, :]], 2).reshape(-1, 64)
    zz = blocks[:, NATURAL]
    nz = zz != 0
    lens = np.where(nz.any(1), 64 - np.argmax(nz[:, ::-1], 1), 0)
    nb = len(lens)
    offsets = np.zeros(nb + 1, np.uint32)
    np.cumsum(lens, out=offsets[1:])
    n_coef = int(offsets[-1])
    total = OFFSETS_OFFSET + 4 * (nb + 1) + 2 * n_coef
    rec = np.zeros((total + 3) // 4, np.uint32).view(np.uint8)[:total]
    rec[:HEADER_BYTES].view(np.uint32)[:17] = [MAGIC, total, f["w"], f["h"], 3, hs, vs, mcus_x, mcus_y, nb, n_coef, *f["bw"], *f["bh"]]
    rec[QUANT_OFFSET:OFFSETS_OFFSET].view(np.uint16)[:] = quant.ravel()
    end = OFFSETS_OFFSET + 4 * (nb + 1)
    rec[OFFSETS_OFFSET:end].view(np.uint32)[:] = offsets
    rec[end:].view(np.int16)[:] = zz[np.arange(64)[None, :] < lens[:, None]]
    return rec


def bgr_to_record(bgr: np.ndarray, quality: int = 90, subsampling: str = "4:2:0") -> np.ndarray:
    """One BGR u8 [h][w][3] frame -> the record libjpeg writes for it at this quality (its default tables and integer DCT),
    the bytes the GPU encoder produces (gtx_jpeg_enc_*)."""
    quality_tables(quality)                                        # refuses the quality before any work
    return planes_to_record(*bgr_to_planes(bgr, subsampling), quality)


def record_to_bytes(rec: np.ndarray) -> bytes:
    """Record -> baseline JFIF JPEG (gtx_jpeg_emit: SOI, APP0, DQT, SOF0, the Annex K.3 DHT, SOS, the Huffman-coded scan, EOI).
    Host only; the call releases the GIL."""
    lib = _lib.load()
    r = np.ascontiguousarray(rec, dtype=np.uint8)
    if r.ctypes.data & 3:
        r = np.concatenate([r, np.zeros(3, np.uint8)]).view(np.uint8)      # (a fresh allocation is aligned)
        r = r[:len(rec)]
    n = C.c_size_t()
    out = np.empty(r.nbytes + 1024, np.uint8)
    rc = lib.gtx_jpeg_emit(_lib.ptr(r), r.nbytes, _lib.ptr(out), out.nbytes, C.byref(n))
    if rc == 1:
        out = np.empty(n.value, np.uint8)
        rc = lib.gtx_jpeg_emit(_lib.ptr(r), r.nbytes, _lib.ptr(out), out.nbytes, C.byref(n))
    if rc != 0:
        raise JpegError(rc, lib.gtx_last_error().decode("utf-8", "replace"))
    return out[:n.value].tobytes()


def encode_dev(ctx: _lib.Context, bgr: np.ndarray, quality: int = 90, subsampling: str = "4:2:0") -> np.ndarray:
    """One host frame through gtx_op_jpeg_encode (upload, the encoder's launches, the record at its real length): tests, tools."""
    a = np.ascontiguousarray(bgr, dtype=np.uint8)
    h, w = a.shape[:2]
    if subsampling not in SUBSAMPLINGS:
        raise ValueError(f"JPEG subsampling {subsampling!r}: one of {sorted(SUBSAMPLINGS)}")
    lib = ctx.lib
    n = C.c_size_t()
    rec = np.zeros(1 << 16, np.uint32).view(np.uint8)
    for _ in range(2):
        rc = lib.gtx_op_jpeg_encode(ctx.handle, _lib.ptr(a), h, w, int(quality), SUBSAMPLINGS[subsampling][2], _lib.ptr(rec), rec.nbytes, C.byref(n))
        if rc != 1:
            break
        rec = np.zeros((n.value + 3) // 4, np.uint32).view(np.uint8)
    _lib.check(rc)
    return rec[:n.value]


# ------------------------------------------------------------------------------------------------- entropy coding on the GPU
# csrc/jpeg_huff.hip codes the record's blocks on the GPU, byte for byte what record_to_bytes() (the host emitter) writes.
# block_bits() is the numpy twin of its first kernel; blocks_to_record() builds records no real frame produces, for its tests.

def blocks_to_record(w: int, h: int, ncomp: int, hs: int, vs: int, runs, quant: np.ndarray | None = None) -> np.ndarray:
    """A record from hand-made blocks: runs[b] is block b's zigzag run (0..64 int16 values, DC first; scan order). ncomp 1
    (hs = vs = 1) or 3 with luma sampling 1x1, 2x1 or 2x2; quant: uint16 [3][64], default quality 90's tables."""
    mcus_x, mcus_y = -(-w // (8 * hs)), -(-h // (8 * vs))
    nb = mcus_x * mcus_y * (1 if ncomp == 1 else hs * vs + 2)
    if len(runs) != nb:
        raise ValueError(f"{len(runs)} runs for a frame of {nb} blocks")
    if quant is None:
        qt = quality_tables(90)
        quant = np.stack([qt[0], qt[1], qt[1]])
    lens = np.array([len(r) for r in runs], np.int64)
    if lens.max(initial=0) > 64:
        raise ValueError("a run is longer than 64")
    offsets = np.zeros(nb + 1, np.uint32)
    np.cumsum(lens, out=offsets[1:])
    n_coef = int(offsets[-1])
    total = OFFSETS_OFFSET + 4 * (nb + 1) + 2 * n_coef
    rec = np.zeros((total + 3) // 4, np.uint32).view(np.uint8)[:total]
    bw = [mcus_x * hs, mcus_x, mcus_x][:ncomp] + [0] * (3 - ncomp)
    bh = [mcus_y * vs, mcus_y, mcus_y][:ncomp] + [0] * (3 - ncomp)
    rec[:HEADER_BYTES].view(np.uint32)[:17] = [MAGIC, total, w, h, ncomp, hs, vs, mcus_x, mcus_y, nb, n_coef, *bw, *bh]
    rec[QUANT_OFFSET:OFFSETS_OFFSET].view(np.uint16)[:] = np.asarray(quant, np.uint16).ravel()
    end = OFFSETS_OFFSET + 4 * (nb + 1)
    rec[OFFSETS_OFFSET:end].view(np.uint32)[:] = offsets
    if n_coef:
        rec[end:].view(np.int16)[:] = np.concatenate([np.asarray(r, np.int16).ravel() for r in runs])
    return rec


def _aligned(rec: np.ndarray) -> np.ndarray:
    r = np.ascontiguousarray(rec, dtype=np.uint8)
    if r.ctypes.data & 3:
        r = np.concatenate([r, np.zeros(3, np.uint8)])[:len(rec)]  # (a fresh allocation is aligned)
    return r


def header_bytes(rec: np.ndarray) -> bytes:
    """The picture's header for this record (gtx_jpeg_header: SOI .. SOS, the one function both entropy routes call). Host only."""
    lib = _lib.load()
    r = _aligned(rec)
    n = C.c_size_t()
    out = np.empty(1024, np.uint8)
    rc = lib.gtx_jpeg_header(_lib.ptr(r), r.nbytes, _lib.ptr(out), out.nbytes, C.byref(n))
    if rc != 0:
        raise JpegError(rc, lib.gtx_last_error().decode("utf-8", "replace") if rc < 0 else "the JPEG header did not fit 1024 bytes")
    return out[:n.value].tobytes()


_HUFF_SIZES = None


def std_huff_sizes() -> tuple[np.ndarray, np.ndarray]:
    """Code lengths of the Annex K.3 tables, read out of the DHT segment the library itself writes: dc [2][12] by category,
    ac [2][256] by run << 4 | size (0: no code); index 0 luma, 1 chroma."""
    global _HUFF_SIZES
    if _HUFF_SIZES is None:
        data = header_bytes(blocks_to_record(8, 8, 3, 1, 1, [[]] * 3))
        at = 2
        while data[at + 1] != 0xC4:
            at += 2 + ((data[at + 2] << 8) | data[at + 3])
        end = at + 2 + ((data[at + 2] << 8) | data[at + 3])
        at += 4
        dc, ac = np.zeros((2, 12), np.int64), np.zeros((2, 256), np.int64)
        while at < end:
            cls, t = data[at] >> 4, data[at] & 15
            counts = data[at + 1:at + 17]
            at += 17
            for length, cnt in enumerate(counts, 1):
                for sym in data[at:at + cnt]:
                    (ac if cls else dc)[t][sym] = length
                at += cnt
        _HUFF_SIZES = (dc, ac)
    return _HUFF_SIZES


def _bit_length(x: np.ndarray) -> np.ndarray:
    return ((x[..., None] >> np.arange(17)) > 0).sum(-1)


def block_bits(rec: np.ndarray) -> np.ndarray:
    """Numpy twin of jpeg_huff_bits_kernel: the bits the emitter writes for every block, uint32 [n_blocks] -- the DC size code
    and amplitude (the difference against the block before it of the same component in scan order; a block of length 0 has DC
    0), per non-zero AC value a run/size code and its amplitude, a ZRL per 16 zeros of a run, and an EOB unless the run is 64
    long and position 63 is non-zero (zeros at the end of a run inside the record are dropped, as emit() drops them). Raises
    JpegError (-1) for a value the Annex K.3 tables cannot code."""
    f, _, offsets, coefs = record_fields(rec)
    nb = f["n_blocks"]
    off = offsets.astype(np.int64)
    lens = off[1:] - off[:-1]
    z = np.arange(64)
    inside = z[None, :] < lens[:, None]
    dense = np.zeros((nb, 64), np.int64)
    dense[inside] = coefs[:int(off[-1])]
    luma = f["hs"] * f["vs"]
    bpm = 1 if f["ncomp"] == 1 else luma + 2
    b = np.arange(nb)
    mcu, k = b // bpm, b % bpm
    if bpm == 1:
        chroma, before = np.zeros(nb, np.int64), b - 1
    else:
        chroma = (k >= luma).astype(np.int64)
        in_mcu = (k < luma) & (k > 0)
        before = np.where(in_mcu, b - 1, np.where(k == 0, b - bpm + luma - 1, b - bpm))
        before[(mcu == 0) & ~in_mcu] = -1
    dc = dense[:, 0]
    diff = dc - np.where(before >= 0, dc[np.maximum(before, 0)], 0)
    s = _bit_length(np.abs(diff))
    if (s > 11).any():
        raise JpegError(-1, "JPEG record: a DC difference beyond 11 bits (no Annex K.3 code)")
    dc_size, ac_size = std_huff_sizes()
    bits = dc_size[chroma, s] + s
    run = np.zeros(nb, np.int64)
    for p in range(1, 64):
        a = dense[:, p]
        nz = inside[:, p] & (a != 0)
        sa = _bit_length(np.abs(a))
        if (nz & (sa > 10)).any():
            raise JpegError(-1, "JPEG record: an AC coefficient beyond 10 bits (no Annex K.3 code)")
        sa = np.minimum(sa, 10)
        bits += np.where(nz, (run >> 4) * ac_size[chroma, 0xF0] + ac_size[chroma, ((run & 15) << 4) | sa] + sa, 0)
        run = np.where(nz, 0, np.where(inside[:, p], run + 1, run))
    eob = ~((lens == 64) & (dense[:, 63] != 0))
    return (bits + np.where(eob, ac_size[chroma, 0], 0)).astype(np.uint32)


def huff_dev(ctx: _lib.Context, rec: np.ndarray, want_bits: bool = False):
    """One record through gtx_op_jpeg_huff (upload of its dense runs, the GPU entropy coder's launches, the picture at its real
    length): the bytes, or (bytes, per-block bit counts as uint32 [n_blocks]). Tests, tools."""
    r = _aligned(rec)
    lib = ctx.lib
    n = C.c_size_t()
    nb = record_fields(r)[0]["n_blocks"]
    bits = np.zeros(nb, np.uint32) if want_bits else None
    out = np.empty(r.nbytes + 1024, np.uint8)
    for _ in range(2):
        rc = lib.gtx_op_jpeg_huff(ctx.handle, _lib.ptr(r), r.nbytes, _lib.ptr(out), out.nbytes, C.byref(n), _lib.ptr(bits) if want_bits else None)
        if rc != 1:
            break
        out = np.empty(n.value, np.uint8)
    if rc != 0:
        raise JpegError(rc, lib.gtx_last_error().decode("utf-8", "replace"))
    data = out[:n.value].tobytes()
    return (data, bits) if want_bits else data


def encode_jpeg_dev(ctx: _lib.Context, bgr: np.ndarray, quality: int = 90, subsampling: str = "4:2:0") -> bytes:
    """One host frame through an encoder on the GPU entropy route (gtx_jpeg_enc_set_entropy, _submit_dev, _collect_jpeg): the
    finished JPEG as it leaves the GPU. Tests, tools."""
    a = np.ascontiguousarray(bgr, dtype=np.uint8)
    h, w = a.shape[:2]
    if subsampling not in SUBSAMPLINGS:
        raise ValueError(f"JPEG subsampling {subsampling!r}: one of {sorted(SUBSAMPLINGS)}")
    lib = ctx.lib
    enc = C.c_void_p()
    _lib.check(lib.gtx_jpeg_enc_create(ctx.handle, h, w, int(quality), SUBSAMPLINGS[subsampling][2], C.byref(enc)))
    dptr = None
    try:
        _lib.check(lib.gtx_jpeg_enc_set_entropy(enc, 1))
        dptr = ctx.dev_alloc(a.nbytes)
        ctx.dev_upload(dptr, a)
        _lib.check(lib.gtx_jpeg_enc_submit_dev(enc, C.c_void_p(dptr)))
        n = C.c_size_t()
        out = np.empty(1 << 16, np.uint8)
        rc = lib.gtx_jpeg_enc_collect_jpeg(enc, _lib.ptr(out), out.nbytes, C.byref(n))
        if rc == 1:
            out = np.empty(n.value, np.uint8)
            rc = lib.gtx_jpeg_enc_collect_jpeg(enc, _lib.ptr(out), out.nbytes, C.byref(n))
        _lib.check(rc)
        return out[:n.value].tobytes()
    finally:
        lib.gtx_jpeg_enc_destroy(enc)
        if dptr is not None:
            ctx.dev_free(dptr)


# ----------------------------------------------------------------------------------------------- entropy decoding on the GPU
# csrc/jpeg_entropy.hip decodes the scan on the GPU from a plan (gtx_jpeg_plan: header walk and unstuffing on the host; layout in
# csrc/jpeg_parse.hpp). entropy_decode_twin() restates its kernels' rule -- the same state word, poison handling, workgroup
# structure and rounds -- so that the rule can be reasoned about and tested without a GPU.

ENTROPY_SUB_BITS, ENTROPY_ROUNDS, ENTROPY_MAX_ROUNDS = 1024, 8, 64     # the production choices (csrc/jpeg_entropy.hpp)
ENTROPY_SUB_BITS_SET = (256, 512, 1024, 2048)
ENTROPY_INVALID, ENTROPY_NOT_CONVERGED = 1, 2                          # status bits
PLAN_MAGIC = 0x3150474A
PLAN_QUANT_OFFSET, PLAN_HUFF_OFFSET, PLAN_HUFF_BYTES, PLAN_STREAM_OFFSET = 112, 112 + 384, 1432, 112 + 384 + 6 * 1432
_POISON = (1 << 64) - 1
_U32 = 0xFFFFFFFF


def entropy_lanes(sub_bits: int) -> int:
    """Lanes of one workgroup: its span of the stream (lanes * sub_bits / 8 bytes) is at most 32 KB."""
    return 128 if sub_bits == 2048 else 256


def entropy_plan(data, frame: int = 0):
    """One compressed frame -> its plan (uint8 array), or None for a frame the GPU route hands to the host parser (a restart
    interval). Raises JpegError where parse() refuses the header, with parse()'s message. Host only."""
    lib = _lib.load()
    raw = bytes(data)
    buf = np.frombuffer(raw or b"\0", dtype=np.uint8)
    out = [C.c_int() for _ in range(5)]
    needed = C.c_size_t()

    def call(dst, cap):
        rc = lib.gtx_jpeg_plan(_lib.ptr(buf), len(raw), int(frame), *[C.byref(v) for v in out], dst, cap, C.byref(needed))
        if rc < 0:
            raise JpegError(rc, lib.gtx_last_error().decode("utf-8", "replace"))
        return rc

    if call(None, 0) == 2:
        return None
    plan = np.zeros((needed.value + 3) // 4, dtype=np.uint32).view(np.uint8)[:needed.value]
    if call(_lib.ptr(plan), plan.nbytes) != 0:
        raise JpegError(-5, f"JPEG frame {frame}: the plan did not fit the size the parser asked for")
    return plan


def plan_fields(plan: np.ndarray):
    """The plan's header as a dict, its quantisation tables [3][64], its six Huffman tables (dicts: look, maxcode, valoff, vals,
    nvals; DC of component 0..2, then AC) and the clean stream (a view)."""
    hd = plan[:PLAN_QUANT_OFFSET].view(np.uint32)
    if int(hd[0]) != PLAN_MAGIC or int(hd[1]) != plan.nbytes:
        raise ValueError("not a JPEG plan")
    f = dict(w=int(hd[2]), h=int(hd[3]), ncomp=int(hd[4]), hs=int(hd[5]), vs=int(hd[6]), mcus_x=int(hd[7]), mcus_y=int(hd[8]), n_blocks=int(hd[9]),
             bw=[int(v) for v in hd[10:13]], bh=[int(v) for v in hd[13:16]], restart=int(hd[16]), td=[int(v) for v in hd[17:20]],
             ta=[int(v) for v in hd[20:23]], stream_bytes=int(hd[23]), stream_bits=int(hd[26]) | int(hd[27]) << 32)
    quant = plan[PLAN_QUANT_OFFSET:PLAN_HUFF_OFFSET].view(np.uint16).reshape(3, 64)
    tables = []
    for k in range(6):
        t = plan[PLAN_HUFF_OFFSET + k * PLAN_HUFF_BYTES:PLAN_HUFF_OFFSET + (k + 1) * PLAN_HUFF_BYTES]
        tables.append(dict(look=t[:1024].view(np.uint16).tolist(), maxcode=t[1024:1096].view(np.int32).tolist(), valoff=t[1096:1168].view(np.int32).tolist(),
                           vals=t[1168:1424].tolist(), nvals=int(t[1424:1428].view(np.uint32)[0])))
    stream = plan[PLAN_STREAM_OFFSET:PLAN_STREAM_OFFSET + f["stream_bytes"]]
    return f, quant, tables, stream


def _pack_state(p: int, k: int, z: int) -> int:
    return p | k << 40 | z << 44


class _WriteSink:
    """jpeg_entropy_write_kernel's side of a lane: b the block being decoded (at or past nb: dropped), next_b the next to begin."""

    def __init__(self, dense, aclen, nb, base):
        self.dense, self.aclen, self.nb, self.b, self.next_b, self.maxz, self.invalid = dense, aclen, nb, (base - 1) & _U32, base, 0, False

    def flush(self):
        if self.maxz and self.b < self.nb:
            assert 0 <= self.b < len(self.aclen)
            self.aclen[self.b] = max(int(self.aclen[self.b]), self.maxz)      # atomicMax
        self.maxz = 0

    def begin(self):
        self.flush()
        self.b, self.next_b = self.next_b, (self.next_b + 1) & _U32

    def dc(self, v):
        if self.b < self.nb:
            assert 0 <= self.b < self.dense.shape[0] and -32768 <= v <= 32767
            self.dense[self.b, 0] = v

    def ac(self, z, v):
        assert 1 <= z <= 63
        if self.b < self.nb:
            assert 0 <= self.b < self.dense.shape[0] and -32768 <= v <= 32767
            self.dense[self.b, z] = v
        self.maxz = z + 1

    end = flush

    def poisoned(self, at_dc):
        if (self.next_b if at_dc else self.b) < self.nb:
            self.invalid = True


def _decode_lane(cx, lane: int, entry: int, sink=None):
    """f_lane(entry) of csrc/jpeg_entropy.hip (decode_lane): the exit state and the blocks that began. cx: the frame's constants."""
    if entry >> 50:
        return _POISON, 0
    p, k, z = entry & ((1 << 40) - 1), (entry >> 40) & 15, (entry >> 44) & 63
    sub, bits, bpm, luma, tables, padded = cx["sub"], cx["bits"], cx["bpm"], cx["luma"], cx["tables"], cx["padded"]
    lo = lane * sub
    hi = lo + sub
    if p < lo or p >= hi or p > bits or k >= bpm:
        return _POISON, 0
    count = 0
    steps = 0
    while p < hi:
        steps += 1
        assert steps <= sub                                        # every step consumes at least one bit
        c = 0 if (bpm == 1 or k < luma) else 1 + (k - luma)
        assert 0 <= c <= 2
        t = tables[c if z == 0 else 3 + c]
        at = p >> 3
        assert 0 <= at and at + 8 <= len(padded)
        win = (int.from_bytes(padded[at:at + 8], "big") << (p & 7)) & ((1 << 64) - 1)       # bits past the stream read as zero
        top = win >> 48
        left = bits - p
        ln = sym = 0
        e = t["look"][top >> 7]
        if e:
            ln, sym = e >> 8, e & 255
        else:
            for l in range(10, 17):
                code = top >> (16 - l)
                if code <= t["maxcode"][l]:
                    idx = t["valoff"][l] + code
                    if 0 <= idx < min(t["nvals"], 256):
                        ln, sym = l, t["vals"][idx]
                    break
        if ln == 0 or ln > 16 or ln > left:
            if sink:
                sink.poisoned(z == 0)
            return _POISON, count
        if z == 0:
            s = sym
            if s > 15 or ln + s > left:
                if sink:
                    sink.poisoned(True)
                return _POISON, count
            v = 0
            if s:
                v = (win << ln & ((1 << 64) - 1)) >> (64 - s)
                v = v - (1 << s) + 1 if v < (1 << (s - 1)) else v
            if sink:
                sink.begin()
                sink.dc(v)
            count += 1
            p, z = p + ln + s, 1
            continue
        r, s = sym >> 4, sym & 15
        done = False
        if s == 0:
            p += ln
            if r != 15:
                done = True
            else:
                z += 16
                done = z >= 64
        else:
            z += r
            if z > 63 or ln + s > left:
                if sink:
                    sink.poisoned(False)
                return _POISON, count
            v = (win << ln & ((1 << 64) - 1)) >> (64 - s)
            v = v - (1 << s) + 1 if v < (1 << (s - 1)) else v
            if sink:
                sink.ac(z, v)
            p += ln + s
            z += 1
            done = z == 64
        if done:
            if sink:
                sink.end()
            k, z = (0 if k + 1 == bpm else k + 1), 0
    return _pack_state(p, k, z), count


def entropy_decode_plan_twin(plan: np.ndarray, sub_bits: int = 0, lanes: int = 0, rounds: int = 0):
    """The kernels of csrc/jpeg_entropy.hip on one plan, in numpy and plain Python: (status, record or None, rounds_used).
    sub_bits: bits of the clean stream per lane; lanes: lanes per workgroup; rounds: synchronisation rounds across workgroups
    (round 0 included); 0 = the production choice each."""
    sub = int(sub_bits) or ENTROPY_SUB_BITS
    if sub not in ENTROPY_SUB_BITS_SET:
        raise ValueError(f"sub_bits {sub_bits}: one of {ENTROPY_SUB_BITS_SET}")
    L = int(lanes) or entropy_lanes(sub)
    R = int(rounds) or ENTROPY_ROUNDS
    if L < 1 or not 1 <= R <= ENTROPY_MAX_ROUNDS:
        raise ValueError(f"lanes {lanes}, rounds {rounds}")
    f, quant, tables, stream = plan_fields(plan)
    nb, bits = f["n_blocks"], f["stream_bits"]
    luma = f["hs"] * f["vs"]
    bpm = 1 if f["ncomp"] == 1 else luma + 2
    cx = dict(sub=sub, bits=bits, bpm=bpm, luma=luma, tables=tables, padded=stream.tobytes() + bytes(16 + sub // 8))
    n_lanes = max(1, -(-bits // sub))
    n_wgs = -(-n_lanes // L)
    memo = {}

    def f_lane(lane, entry):
        key = (lane, entry)
        if key not in memo:
            memo[key] = _decode_lane(cx, lane, entry)
        return memo[key]

    # ---- jpeg_entropy_sync_kernel, `R` launches
    entry, exit_, count = [_POISON] * n_lanes, [_POISON] * n_lanes, [0] * n_lanes
    edge = [[_POISON] * n_wgs, [_POISON] * n_wgs]
    changed = [0] * R
    for r in range(R):
        for wg in range(n_wgs):
            first, last = wg * L, min((wg + 1) * L, n_lanes) - 1
            wg_entry = 0 if wg == 0 else (_pack_state(first * sub, 0, 0) if r == 0 else edge[(r - 1) & 1][wg - 1])
            if r > 0 and entry[first] == wg_entry:
                edge[r & 1][wg] = exit_[last]
                continue
            n = last - first + 1
            if r == 0:
                cur_entry = [wg_entry] + [_pack_state((first + t) * sub, 0, 0) for t in range(1, n)]
                got = [f_lane(first + t, cur_entry[t]) for t in range(n)]
                cur_exit, cur_count = [g[0] for g in got], [g[1] for g in got]
            else:
                cur_entry, cur_exit, cur_count = entry[first:last + 1], exit_[first:last + 1], count[first:last + 1]
            for _ in range(L):                                     # in LDS: until no lane of the workgroup changes
                want = [wg_entry] + cur_exit[:-1]
                again = [t for t in range(n) if want[t] != cur_entry[t]]
                if not again:
                    break
                for t in again:
                    cur_entry[t] = want[t]
                    cur_exit[t], cur_count[t] = f_lane(first + t, want[t])
            entry[first:last + 1], exit_[first:last + 1], count[first:last + 1] = cur_entry, cur_exit, cur_count
            edge[r & 1][wg] = cur_exit[-1]
            changed[r] = 1
    rounds_used = 1 + sum(changed[1:])
    # ---- blocks that begin in every lane -> the first of them (32-bit sums)
    blockoff = [0] * n_lanes
    run = 0
    for i in range(n_lanes):
        blockoff[i] = run
        run = (run + count[i]) & _U32
    # ---- jpeg_entropy_write_kernel
    status = 0
    dense = np.zeros((nb, 64), np.int16)
    aclen = np.zeros(nb, np.int64)
    for lane in range(n_lanes):
        if entry[lane] != (0 if lane == 0 else exit_[lane - 1]):
            status |= ENTROPY_NOT_CONVERGED
        sink = _WriteSink(dense, aclen, nb, blockoff[lane])
        x, _ = _decode_lane(cx, lane, entry[lane], sink)
        sink.flush()
        if sink.invalid:
            status |= ENTROPY_INVALID
        if lane == n_lanes - 1 and x != _POISON and ((sink.next_b - (1 if (x >> 44) & 63 else 0)) & _U32) < nb:
            status |= ENTROPY_INVALID                              # the data ends before the last block does
    # ---- the DC prefix sums by component (wrapping 32-bit sums), block lengths
    b = np.arange(nb)
    k = b % bpm
    comp = np.zeros(nb, np.int64) if bpm == 1 else np.where(k < luma, 0, 1 + (k - luma))
    diff = dense[:, 0].astype(np.int64)
    pred = np.zeros(nb, np.int64)
    for c in range(f["ncomp"]):
        vals = np.where(comp == c, diff, 0)
        pref = (np.cumsum(vals) - vals) & _U32                     # exclusive
        s32 = (pref + (diff & _U32)) & _U32
        s32 = np.where(s32 >= 1 << 31, s32 - (1 << 32), s32)
        pred = np.where(comp == c, s32, pred)
    if ((pred < -32768) | (pred > 32767)).any():
        status |= ENTROPY_INVALID
    dense[:, 0] = pred.astype(np.int16)                            # (truncated where invalid, as the kernel stores it)
    lens = np.maximum(np.minimum(aclen, 64), (pred != 0).astype(np.int64))
    if status:
        return status, None, rounds_used
    # ---- offsets, compaction, header
    offsets = np.zeros(nb + 1, np.uint32)
    np.cumsum(lens, out=offsets[1:])
    n_coef = int(offsets[-1])
    assert n_coef <= 64 * nb
    total = OFFSETS_OFFSET + 4 * (nb + 1) + 2 * n_coef
    rec = np.zeros((total + 3) // 4, np.uint32).view(np.uint8)[:total]
    rec[:HEADER_BYTES].view(np.uint32)[:17] = [MAGIC, total, f["w"], f["h"], f["ncomp"], f["hs"], f["vs"], f["mcus_x"], f["mcus_y"], nb, n_coef, *f["bw"], *f["bh"]]
    rec[QUANT_OFFSET:OFFSETS_OFFSET].view(np.uint16)[:] = quant.ravel()
    end = OFFSETS_OFFSET + 4 * (nb + 1)
    rec[OFFSETS_OFFSET:end].view(np.uint32)[:] = offsets
    rec[end:].view(np.int16)[:] = dense[np.arange(64)[None, :] < lens[:, None]]
    return 0, rec, rounds_used


def entropy_decode_twin(data, sub_bits: int = 0, lanes: int = 0, rounds: int = 0, frame: int = 0):
    """One compressed frame through entropy_plan() and the twin of the GPU entropy decoder: (status, record or None,
    rounds_used). A frame of the host route (entropy_plan() is None) raises ValueError."""
    plan = entropy_plan(data, frame)
    if plan is None:
        raise ValueError(f"JPEG frame {frame}: a frame of the host route (restart interval)")
    return entropy_decode_plan_twin(plan, sub_bits, lanes, rounds)


def entropy_dev(ctx: _lib.Context, data, sub_bits: int = 0, rounds: int = 0, frame: int = 0):
    """One compressed frame through gtx_jpeg_plan and gtx_op_jpeg_entropy (upload of the plan, the entropy chain, the record at
    its real length): (status, record or None, rounds_used). Tests, tools."""
    plan = entropy_plan(data, frame)
    if plan is None:
        raise ValueError(f"JPEG frame {frame}: a frame of the host route (restart interval)")
    return entropy_plan_dev(ctx, plan, sub_bits, rounds)


def entropy_plan_dev(ctx: _lib.Context, plan: np.ndarray, sub_bits: int = 0, rounds: int = 0):
    lib = ctx.lib
    n, status, used = C.c_size_t(), C.c_int(), C.c_int()
    rec = np.zeros(1 << 14, np.uint32).view(np.uint8)
    for _ in range(2):
        rc = lib.gtx_op_jpeg_entropy(ctx.handle, _lib.ptr(plan), plan.nbytes, int(sub_bits), int(rounds), _lib.ptr(rec), rec.nbytes, C.byref(n),
                                     C.byref(status), C.byref(used))
        if rc != 1:
            break
        rec = np.zeros((n.value + 3) // 4, np.uint32).view(np.uint8)
    if rc != 0:
        raise JpegError(rc, lib.gtx_last_error().decode("utf-8", "replace"))
    return status.value, (rec[:n.value] if status.value == 0 else None), used.value


# ------------------------------------------------------------------------------------- restart intervals, one lane per interval
# csrc/jpeg_restart.hip decodes a frame that has a restart interval from an interval plan (gtx_jpeg_plan_intervals: header walk,
# stuffing and RSTn markers removed, the start of every interval noted; layout in csrc/jpeg_parse.hpp). At every RSTn the stream is
# byte aligned, the DC predictors are zero and the MCU index is known, so a lane needs nothing from the others.
# restart_decode_twin() restates the kernel's rule with every index asserted; emit() is the host emitter with restart markers.

INTERVAL_PLAN_MAGIC = 0x3249474A
RESTART_INVALID = 1                                                    # status bit
NO_RESTART = 3                                                         # gtx_jpeg_plan_intervals: the frame has no restart interval


def interval_stream_offset(n_intervals: int) -> int:
    return (PLAN_STREAM_OFFSET + 4 * (n_intervals + 1) + 15) // 16 * 16


def restart_plan(data, frame: int = 0):
    """One compressed frame -> its interval plan (uint8 array), or None for a frame without a restart interval. Raises JpegError
    with parse()'s status and message where parse() refuses the header, or where a restart marker is missing or out of
    sequence. Host only."""
    lib = _lib.load()
    raw = bytes(data)
    buf = np.frombuffer(raw or b"\0", dtype=np.uint8)
    out = [C.c_int() for _ in range(5)]
    needed = C.c_size_t()

    def call(dst, cap):
        rc = lib.gtx_jpeg_plan_intervals(_lib.ptr(buf), len(raw), int(frame), *[C.byref(v) for v in out], dst, cap, C.byref(needed))
        if rc < 0:
            raise JpegError(rc, lib.gtx_last_error().decode("utf-8", "replace"))
        return rc

    if call(None, 0) == NO_RESTART:
        return None
    plan = np.zeros((needed.value + 3) // 4, dtype=np.uint32).view(np.uint8)[:needed.value]
    if call(_lib.ptr(plan), plan.nbytes) != 0:
        raise JpegError(-5, f"JPEG frame {frame}: the interval plan did not fit the size the parser asked for")
    return plan


def restart_plan_fields(plan: np.ndarray):
    """The interval plan's header as a dict (with n_intervals), its quantisation tables, its six Huffman tables (as plan_fields),
    start[n_intervals + 1] and the clean stream (views)."""
    hd = plan[:PLAN_QUANT_OFFSET].view(np.uint32)
    if int(hd[0]) != INTERVAL_PLAN_MAGIC or int(hd[1]) != plan.nbytes:
        raise ValueError("not a JPEG interval plan")
    f = dict(w=int(hd[2]), h=int(hd[3]), ncomp=int(hd[4]), hs=int(hd[5]), vs=int(hd[6]), mcus_x=int(hd[7]), mcus_y=int(hd[8]), n_blocks=int(hd[9]),
             bw=[int(v) for v in hd[10:13]], bh=[int(v) for v in hd[13:16]], restart=int(hd[16]), td=[int(v) for v in hd[17:20]],
             ta=[int(v) for v in hd[20:23]], stream_bytes=int(hd[23]), n_intervals=int(hd[24]), stream_bits=int(hd[26]) | int(hd[27]) << 32)
    quant = plan[PLAN_QUANT_OFFSET:PLAN_HUFF_OFFSET].view(np.uint16).reshape(3, 64)
    tables = []
    for k in range(6):
        t = plan[PLAN_HUFF_OFFSET + k * PLAN_HUFF_BYTES:PLAN_HUFF_OFFSET + (k + 1) * PLAN_HUFF_BYTES]
        tables.append(dict(look=t[:1024].view(np.uint16).tolist(), maxcode=t[1024:1096].view(np.int32).tolist(), valoff=t[1096:1168].view(np.int32).tolist(),
                           vals=t[1168:1424].tolist(), nvals=int(t[1424:1428].view(np.uint32)[0])))
    n_int = f["n_intervals"]
    start = plan[PLAN_STREAM_OFFSET:PLAN_STREAM_OFFSET + 4 * (n_int + 1)].view(np.uint32)
    at = interval_stream_offset(n_int)
    stream = plan[at:at + f["stream_bytes"]]
    return f, quant, tables, start, stream


def _symbol_step(t, win: int, left: int, z: int):
    """jpegsym::step of csrc/jpeg_symbol.hpp: (result, used bits, new z, event). result 0 bad, 1 the block goes on, 2 the block
    ends; event: None, ("dc", difference) or ("ac", z, value)."""
    top = win >> 48
    assert 0 <= top < 1 << 16
    ln = sym = 0
    e = t["look"][top >> 7]
    if e:
        ln, sym = e >> 8, e & 255
    else:
        for l in range(10, 17):
            code = top >> (16 - l)
            if code <= t["maxcode"][l]:
                idx = t["valoff"][l] + code
                if 0 <= idx < min(t["nvals"], 256):
                    ln, sym = l, t["vals"][idx]
                break
    if ln == 0 or ln > 16 or ln > left:
        return 0, 0, z, None
    m64 = (1 << 64) - 1

    def amplitude(s):
        v = ((win << ln) & m64) >> (64 - s)
        return v - (1 << s) + 1 if v < (1 << (s - 1)) else v

    if z == 0:
        s = sym
        if s > 15 or ln + s > left:
            return 0, 0, z, None
        return 1, ln + s, 1, ("dc", amplitude(s) if s else 0)
    r, s = sym >> 4, sym & 15
    if s == 0:
        if r != 15:
            return 2, ln, z, None
        z += 16
        return (2 if z >= 64 else 1), ln, z, None
    z += r
    if z > 63 or ln + s > left:
        return 0, 0, z, None
    ev = ("ac", z, amplitude(s))
    z += 1
    return (2 if z == 64 else 1), ln + s, z, ev


def restart_lane_twin(plan: np.ndarray, i: int):
    """Lane i of jpeg_restart_kernel alone: (bad, first block, dense int16 [blocks][64], lens [blocks]) for the blocks of
    interval i. It reads start[i], start[i + 1], the tables and its own bytes of the stream, nothing else."""
    f, _, tables, start, stream = restart_plan_fields(plan)
    n_int, nb = f["n_intervals"], f["n_blocks"]
    assert 0 <= i < n_int and i + 1 < len(start)
    luma = f["hs"] * f["vs"]
    bpm = 1 if f["ncomp"] == 1 else luma + 2
    n_mcus = f["mcus_x"] * f["mcus_y"]
    sb = f["stream_bytes"]
    byte1 = min(int(start[i + 1]), sb)
    byte0 = min(int(start[i]), byte1)
    bits = 8 * (byte1 - byte0)
    mcu0 = i * f["restart"]
    mcu1 = min(mcu0 + f["restart"], n_mcus)
    b0, b_end = min(mcu0 * bpm, nb), min(mcu1 * bpm, nb)
    own = stream[byte0:byte1].tobytes() + bytes(8)                 # bits at or past start[i + 1] read as zero
    dense = np.zeros((max(b_end - b0, 0), 64), np.int16)
    lens = np.zeros(max(b_end - b0, 0), np.int64)
    pred = [0, 0, 0]
    b, k, z, p, ln, bad = b0, 0, 0, 0, 0, False
    steps = 0
    while b < b_end:
        steps += 1
        assert steps <= bits + 1                                   # every step consumes at least one bit
        c = 0 if (bpm == 1 or k < luma) else min(1 + (k - luma), 2)
        at = p >> 3
        assert 0 <= at and at + 8 <= len(own)
        win = (int.from_bytes(own[at:at + 8], "big") << (p & 7)) & ((1 << 64) - 1)
        left = bits - p
        assert left >= 0
        if left < 64:
            assert win & ((1 << (64 - left)) - 1) == 0 or left == 0    # the zero padding is the mask the kernel applies
            win = win & ~((1 << (64 - left)) - 1) if left else 0
        r, used, z, ev = _symbol_step(tables[c if z == 0 else 3 + c], win, left, z)
        if r == 0:
            bad = True
            break
        assert 1 <= used <= left and b0 <= b < b_end and b < nb
        if ev and ev[0] == "dc":
            pred[c] += ev[1]
            if not -32768 <= pred[c] <= 32767:
                bad = True
                break
            dense[b - b0, 0] = pred[c]
            ln = 1 if pred[c] else 0
        elif ev:
            assert 1 <= ev[1] <= 63 and -32768 <= ev[2] <= 32767
            dense[b - b0, ev[1]] = ev[2]
            ln = ev[1] + 1
        p += used
        if r == 2:
            lens[b - b0] = ln
            b, k, z = b + 1, (0 if k + 1 == bpm else k + 1), 0
    if not bad and i + 1 < n_int and bits - p >= 8:                # a marker follows: one byte's pad bits at most stand before it
        bad = True
    return bad, b0, dense, lens


def restart_decode_twin(plan: np.ndarray):
    """jpeg_restart_kernel, the offset scan and the compaction on one interval plan, in numpy and plain Python with every index
    asserted: (status, record or None)."""
    f, quant, _, start, _ = restart_plan_fields(plan)
    nb, n_int = f["n_blocks"], f["n_intervals"]
    assert n_int == -(-(f["mcus_x"] * f["mcus_y"]) // f["restart"]) and int(start[0]) == 0 and int(start[n_int]) == f["stream_bytes"]
    assert (np.diff(start.astype(np.int64)) >= 0).all()
    dense = np.zeros((nb, 64), np.int16)
    lens = np.zeros(nb, np.int64)
    status = 0
    for i in range(n_int):
        bad, b0, d, l = restart_lane_twin(plan, i)
        assert b0 + len(l) <= nb
        dense[b0:b0 + len(l)], lens[b0:b0 + len(l)] = d, l
        if bad:
            status |= RESTART_INVALID
    if status:
        return status, None
    lens = np.minimum(lens, 64)
    offsets = np.zeros(nb + 1, np.uint32)
    np.cumsum(lens, out=offsets[1:])
    n_coef = int(offsets[-1])
    assert n_coef <= 64 * nb
    total = OFFSETS_OFFSET + 4 * (nb + 1) + 2 * n_coef
    rec = np.zeros((total + 3) // 4, np.uint32).view(np.uint8)[:total]
    rec[:HEADER_BYTES].view(np.uint32)[:17] = [MAGIC, total, f["w"], f["h"], f["ncomp"], f["hs"], f["vs"], f["mcus_x"], f["mcus_y"], nb, n_coef, *f["bw"], *f["bh"]]
    rec[QUANT_OFFSET:OFFSETS_OFFSET].view(np.uint16)[:] = quant.ravel()
    end = OFFSETS_OFFSET + 4 * (nb + 1)
    rec[OFFSETS_OFFSET:end].view(np.uint32)[:] = offsets
    rec[end:].view(np.int16)[:] = dense[np.arange(64)[None, :] < lens[:, None]]
    return 0, rec


def restart_plan_dev(ctx: _lib.Context, plan: np.ndarray):
    """One interval plan through gtx_op_jpeg_restart (upload, the interval launch, scan and compaction, the record at its real
    length): (status, record or None). Tests, tools."""
    lib = ctx.lib
    n, status = C.c_size_t(), C.c_int()
    p = _aligned(plan)
    rec = np.zeros(1 << 14, np.uint32).view(np.uint8)
    for _ in range(2):
        rc = lib.gtx_op_jpeg_restart(ctx.handle, _lib.ptr(p), p.nbytes, _lib.ptr(rec), rec.nbytes, C.byref(n), C.byref(status))
        if rc != 1:
            break
        rec = np.zeros((n.value + 3) // 4, np.uint32).view(np.uint8)
    if rc != 0:
        raise JpegError(rc, lib.gtx_last_error().decode("utf-8", "replace"))
    return status.value, (rec[:n.value] if status.value == 0 else None)


def emit(rec: np.ndarray, restart: int = 0) -> bytes:
    """Record -> baseline JFIF JPEG with a restart interval of `restart` MCUs (gtx_jpeg_emit_restart: record_to_bytes() plus a
    DRI segment, predictor resets, 1-bit padding and RSTn every `restart` MCUs). restart 0: record_to_bytes()'s bytes exactly.
    Raises JpegError where record_to_bytes() does, and for a restart outside 0..65535. Host only; the call releases the GIL."""
    lib = _lib.load()
    r = _aligned(rec)
    n = C.c_size_t()
    out = np.empty(r.nbytes + 1024, np.uint8)
    for _ in range(2):
        rc = lib.gtx_jpeg_emit_restart(_lib.ptr(r), r.nbytes, int(restart), _lib.ptr(out), out.nbytes, C.byref(n))
        if rc != 1:
            break
        out = np.empty(n.value, np.uint8)
    if rc != 0:
        raise JpegError(rc, lib.gtx_last_error().decode("utf-8", "replace"))
    return out[:n.value].tobytes()


def recode_with_restarts(data, restart: int, frame: int = 0) -> bytes:
    """One compressed frame -> the same coefficients coded again with a restart interval of `restart` MCUs (parse(), then emit()):
    lossless on coefficients, with the Annex K.3 tables. Refuses what parse() refuses and what gtx_jpeg_emit refuses."""
    rec, _ = parse(data, frame)
    return emit(rec, restart)


def mcus_per_row(data, frame: int = 0) -> int:
    """MCUs in one MCU row of the frame (the restart interval that gives one interval per row)."""
    lib = _lib.load()
    raw = bytes(data)
    buf = np.frombuffer(raw or b"\0", dtype=np.uint8)
    out = [C.c_int() for _ in range(5)]
    rc = lib.gtx_jpeg_probe(_lib.ptr(buf), len(raw), int(frame), *[C.byref(v) for v in out])
    if rc < 0:
        raise JpegError(rc, lib.gtx_last_error().decode("utf-8", "replace"))
    h, w, ncomp, hs, vs = (v.value for v in out)
    return -(-w // (8 * (hs if ncomp == 3 else 1)))
