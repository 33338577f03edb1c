"""The pixel rule of the plot stage's trajectory maps: the numpy twin of csrc/plot_draw.hip and the binding of gtx_plot_canvas_*.

What the reference draws with plt.plot / plt.scatter over plt.imshow(orthophoto) (geotrax/plot.py:419-488) is, here, a list of
semi-transparent strokes and discs painted into a BGR u8 canvas [h][w][3] that stays in HBM. This docstring is the
specification; `rasterize` / `reduce` below and the kernels compute it bit for bit. All of it is integer arithmetic: there is no
floating-point operation whose order or fusing could differ between the two.

Records. A primitive is 32 bytes: f32 x0, y0, x1, y1, width; i32 bgr, alpha, poly. (x0, y0) - (x1, y1) is a segment in canvas
pixels (pixel (x, y) has its centre AT (x, y), as under imshow), width is in pixels, bgr = b | g << 8 | r << 16, alpha is in
1/256 steps (1..256), poly names the polyline. A DISC of radius r is the zero-length segment of width 2 r (`disc`), so a
zero-length stroke and the disc of its width are the same record and the same pixels. A maximal run of consecutive records with
the same `poly` is one polyline; its records must agree in width, bgr and alpha.

Quantisation (host side, in float64, every step exact): X = floor(16 x + 0.5) (1/16 px), WQ = floor(256 width + 0.5)
(1/256 px), R = WQ + 256: w/2 + 1/2 in units of 1/512 px. Accepted: finite coordinates in [-32768, 32767], |x1 - x0| and
|y1 - y0| <= 2048 px (the bound that keeps every product below inside int64; a longer segment is split by whoever builds the
list, `split_long`), 0.25 <= width <= 64, 1 <= alpha <= 256.

Coverage of one segment at pixel (x, y), 0..256. With P = (16 x, 16 y), A, B the quantised endpoints, v = B - A, w = P - A,
L = v.v, s = w.v (int64):
    s <= 0 (a zero-length segment always lands here):  num = w.w,           den = 1
    s >= L:                                            num = |P - B|^2,     den = 1
    otherwise:                                         num = (wx vy - wy vx)^2, den = L
so num / den is the squared distance in (1/16 px)^2 and the caps are round. The coverage is the linear ramp
clamp(floor((w/2 + 1/2 - d) 256 + 1/2), 0, 256) of the distance d, evaluated exactly: with e = the smallest integer whose
square times den is >= 1024 num (e = ceil(512 d)),
    cov = 0                               if 1024 num > (R - 1)^2 den   (tested as num > ((R - 1)^2 den) >> 10)
    cov = min((R + 1 - e) >> 1, 256)      otherwise.
That is: 256 inside w/2 - 1/2, one pixel of ramp, 0 from w/2 + 1/2 on. e is an integer defined by two integer inequalities, so
however a side estimates the square root, the value is the same.

A polyline's coverage at a pixel is the MAXIMUM over its segments (joints and self-crossings of one track do not darken, as
one Agg path does not). Polylines are blended in list order, every channel
    c = c + (((src - c) * alpha * cov + 32768) >> 16)           (arithmetic shift: floor)
so alpha 256 with coverage 256 writes the colour and coverage 0 leaves the byte. The result is a function of list order only.

Bounding box (inclusive pixels): [floor((min - pad) / 16), floor((max + pad) / 16)] per axis with pad = (R + 31) // 32 in 1/16 px
(cov > 0 needs 512 d <= R - 1), clamped to int16. No pixel outside it is covered: what lets both sides cull.

reduce: the exact box average of an [H][W] gray, [H][W][3] RGB or [H][W][4] RGBA u8 image by an integer factor k (1..256) into BGR
[ceil(H/k)][ceil(W/k)][3]: out = (2 sum + n) // (2 n) over the n pixels the block really has (round half up; alpha ignored).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

PRIM_DTYPE = np.dtype([("x0", "<f4"), ("y0", "<f4"), ("x1", "<f4"), ("y1", "<f4"), ("width", "<f4"), ("bgr", "<i4"), ("alpha", "<i4"), ("poly", "<i4")])
COORD_MIN, COORD_MAX = -32768.0, 32767.0
MAX_SPAN = 2048.0                                     # |x1 - x0|, |y1 - y0| of one record, pixels
MIN_WIDTH, MAX_WIDTH = 0.25, 64.0
MAX_PRIMS = 1 << 22                                   # per draw call (csrc/plot_draw.hpp kPlotMaxPrims)
MAX_SIDE = 16384                                      # canvas sides: what the JPEG encoder accepts (csrc/jpeg_parse.hpp kMaxDim)
MAX_FACTOR = 256


def pack_bgr(color) -> int:
    b, g, r = (int(v) for v in color)
    return b | g << 8 | r << 16


def as_prims(prims) -> np.ndarray:
    """A list of (x0, y0, x1, y1, width, bgr, alpha, poly) tuples, or an array of PRIM_DTYPE, as a contiguous PRIM_DTYPE array."""
    if isinstance(prims, np.ndarray) and prims.dtype == PRIM_DTYPE:
        return np.ascontiguousarray(prims.reshape(-1))
    rows = list(prims)
    out = np.zeros(len(rows), PRIM_DTYPE)
    for k, name in enumerate(PRIM_DTYPE.names):
        out[name] = [r[k] for r in rows]
    return out


def stroke(x0, y0, x1, y1, width, color, alpha: int = 256, poly: int = 0) -> tuple:
    return (x0, y0, x1, y1, width, pack_bgr(color), int(alpha), int(poly))


def disc(cx, cy, radius, color, alpha: int = 256, poly: int = 0) -> tuple:
    return (cx, cy, cx, cy, 2.0 * radius, pack_bgr(color), int(alpha), int(poly))


def polyline(xs, ys, width, color, alpha: int = 256, poly: int = 0) -> np.ndarray:
    """The records of one polyline through the points (one point: the disc of the stroke's width), long segments split."""
    xs, ys = np.asarray(xs, np.float64), np.asarray(ys, np.float64)
    if len(xs) == 1:
        xs, ys = np.repeat(xs, 2), np.repeat(ys, 2)
    out = np.zeros(max(len(xs) - 1, 0), PRIM_DTYPE)
    out["x0"], out["y0"], out["x1"], out["y1"] = xs[:-1], ys[:-1], xs[1:], ys[1:]
    out["width"], out["bgr"], out["alpha"], out["poly"] = width, pack_bgr(color), alpha, poly
    return split_long(out)


def split_long(prims) -> np.ndarray:
    """Every record whose span exceeds MAX_SPAN replaced by equal pieces that do not (same polyline, so the maximum rule makes
    the pieces one stroke again, up to the quantisation of the split points)."""
    p = as_prims(prims)
    span = np.maximum(np.abs(p["x1"].astype(np.float64) - p["x0"]), np.abs(p["y1"].astype(np.float64) - p["y0"]))
    if not (span > MAX_SPAN - 1).any():
        return p
    parts = []
    for rec, s in zip(p, span):
        m = int(np.ceil(s / (MAX_SPAN - 1))) if s > MAX_SPAN - 1 else 1
        t = np.linspace(0.0, 1.0, m + 1)
        q = np.repeat(rec[None], m)
        xa, ya, xb, yb = (np.float64(rec[k]) for k in ("x0", "y0", "x1", "y1"))
        q["x0"], q["y0"], q["x1"], q["y1"] = xa + (xb - xa) * t[:-1], ya + (yb - ya) * t[:-1], xa + (xb - xa) * t[1:], ya + (yb - ya) * t[1:]
        parts.append(q)
    return np.concatenate(parts)


def validate(prims) -> None:
    """The checks of csrc/plot_draw.cpp, in its order; ValueError names the first bad record's index."""
    p = as_prims(prims)
    if len(p) > MAX_PRIMS:
        raise ValueError(f"{len(p)} primitives, a call takes {MAX_PRIMS}")
    prev = None
    for i, r in enumerate(p.tolist()):
        x0, y0, x1, y1, width, bgr, alpha, poly = r
        if not all(np.isfinite(v) and COORD_MIN <= v <= COORD_MAX for v in (x0, y0, x1, y1)):
            raise ValueError(f"primitive {i}: a coordinate is not finite or outside [-32768, 32767]")
        if abs(x1 - x0) > MAX_SPAN or abs(y1 - y0) > MAX_SPAN:
            raise ValueError(f"primitive {i}: the segment spans more than {MAX_SPAN:.0f} pixels")
        if not (MIN_WIDTH <= width <= MAX_WIDTH):
            raise ValueError(f"primitive {i}: width {width}")
        if not (1 <= alpha <= 256):
            raise ValueError(f"primitive {i}: alpha {alpha}")
        if bgr < 0 or bgr > 0xFFFFFF:
            raise ValueError(f"primitive {i}: colour {bgr:#x}")
        if prev is not None and prev[3] == poly and prev[:3] != (width, bgr, alpha):
            raise ValueError(f"primitive {i}: width, colour or alpha differ from the polyline's first record")
        prev = (width, bgr, alpha, poly)


def quantise(prims) -> np.ndarray:
    """[n][8] int64: X0, Y0, X1, Y1 (1/16 px), R (1/512 px), bgr, alpha, run (the index of the record's polyline, 0, 1, ...)."""
    p = as_prims(prims)
    q = np.zeros((len(p), 8), np.int64)
    for k, name in enumerate(("x0", "y0", "x1", "y1")):
        q[:, k] = np.floor(p[name].astype(np.float64) * 16.0 + 0.5).astype(np.int64)
    q[:, 4] = np.floor(p["width"].astype(np.float64) * 256.0 + 0.5).astype(np.int64) + 256
    q[:, 5], q[:, 6] = p["bgr"], p["alpha"]
    if len(p):
        q[:, 7] = np.concatenate([[0], np.cumsum(p["poly"][1:] != p["poly"][:-1])])
    return q


def bounding_boxes(q: np.ndarray) -> np.ndarray:
    """[n][4] int64 x_lo, y_lo, x_hi, y_hi (inclusive pixels) of quantised records: the box of the module docstring."""
    pad = (q[:, 4] + 31) // 32
    lo_x, hi_x = (np.minimum(q[:, 0], q[:, 2]) - pad) // 16, (np.maximum(q[:, 0], q[:, 2]) + pad) // 16
    lo_y, hi_y = (np.minimum(q[:, 1], q[:, 3]) - pad) // 16, (np.maximum(q[:, 1], q[:, 3]) + pad) // 16
    return np.clip(np.stack([lo_x, lo_y, hi_x, hi_y], axis=1), -32768, 32767)


def _ceil_sqrt_ratio(n: np.ndarray, den: np.ndarray) -> np.ndarray:
    """The smallest integer e >= 0 with e * e * den >= n (int64 arrays, den >= 1)."""
    e = np.floor(np.sqrt(n.astype(np.float64) / den.astype(np.float64))).astype(np.int64)
    for _ in range(4):
        e = np.where((e > 0) & ((e - 1) * (e - 1) * den >= n), e - 1, e)
    for _ in range(4):
        e = np.where(e * e * den < n, e + 1, e)
    return e


def _coverage(ax, ay, bx, by, R, px, py) -> np.ndarray:
    """The rule of the module docstring on int64 arrays that broadcast against each other (px, py: 16 x the pixel coordinates)."""
    vx, vy = bx - ax, by - ay
    wx, wy = px - ax, py - ay
    L = vx * vx + vy * vy
    s = wx * vx + wy * vy
    ex, ey = px - bx, py - by
    c = wx * vy - wy * vx
    first, mid = s <= 0, (s > 0) & (s < L)
    num = np.where(first, wx * wx + wy * wy, np.where(mid, c * c, ex * ex + ey * ey))
    den = np.where(mid, L, 1).astype(np.int64)
    live = num <= (((R - 1) * (R - 1)) * den >> 10)
    n = np.where(live, num, 0) << 10
    e = _ceil_sqrt_ratio(n, den)
    return np.where(live, np.minimum((R + 1 - e) >> 1, 256), 0).astype(np.int64)


def coverage(rec, xs: np.ndarray, ys: np.ndarray) -> np.ndarray:
    """cov (int64, 0..256) of one quantised record at the pixels xs x ys (1-D integer arrays) -> [len(ys)][len(xs)]. The pixels
    must lie within the record's bounding box grown by a tile (64 pixels), where every product stays inside int64."""
    ax, ay, bx, by, R = (np.int64(v) for v in rec[:5])
    px = 16 * np.asarray(xs, np.int64)[None, :]
    py = 16 * np.asarray(ys, np.int64)[:, None]
    return np.broadcast_to(_coverage(ax, ay, bx, by, R, px, py), (py.shape[0], px.shape[1]))


def rasterize(canvas: np.ndarray, prims) -> np.ndarray:
    """The canvas with the list painted: per polyline the maximum coverage of its records, then one blend."""
    out = np.array(canvas, dtype=np.uint8, copy=True)
    if out.ndim != 3 or out.shape[2] != 3:
        raise ValueError(f"expected an [h, w, 3] uint8 canvas, got {out.shape}")
    validate(prims)
    h, w = out.shape[:2]
    q = quantise(prims)
    boxes = np.stack([np.maximum(bounding_boxes(q)[:, 0], 0), np.maximum(bounding_boxes(q)[:, 1], 0),
                      np.minimum(bounding_boxes(q)[:, 2], w - 1), np.minimum(bounding_boxes(q)[:, 3], h - 1)], axis=1) if len(q) else np.zeros((0, 4), np.int64)
    i, n = 0, len(q)
    while i < n:
        j = i
        while j < n and q[j, 7] == q[i, 7]:
            j += 1
        b = boxes[i:j]
        seen = (b[:, 0] <= b[:, 2]) & (b[:, 1] <= b[:, 3])
        if seen.any():
            X0, Y0, X1, Y1 = b[seen, 0].min(), b[seen, 1].min(), b[seen, 2].max(), b[seen, 3].max()
            cov = np.zeros((Y1 - Y0 + 1, X1 - X0 + 1), np.int64)
            live = np.nonzero(seen)[0]
            if len(live) > 1 and cov.shape[0] <= 64 and cov.shape[1] <= 64:
                # a short polyline: all its records at once over its window, each masked to its own box (the same values, fewer calls)
                r = q[i + live][:, :5, None, None]
                xs, ys = np.arange(X0, X1 + 1)[None, None, :], np.arange(Y0, Y1 + 1)[None, :, None]
                bb = b[live][:, :, None, None]
                own = (xs >= bb[:, 0]) & (xs <= bb[:, 2]) & (ys >= bb[:, 1]) & (ys <= bb[:, 3])
                cov = np.where(own, _coverage(r[:, 0], r[:, 1], r[:, 2], r[:, 3], r[:, 4], 16 * xs, 16 * ys), 0).max(axis=0)
            else:
                for k in live:
                    bx0, by0, bx1, by1 = (int(v) for v in b[k])
                    sub = cov[by0 - Y0:by1 - Y0 + 1, bx0 - X0:bx1 - X0 + 1]
                    np.maximum(sub, coverage(q[i + k], np.arange(bx0, bx1 + 1), np.arange(by0, by1 + 1)), out=sub)
            col = np.array([q[i, 5] & 255, q[i, 5] >> 8 & 255, q[i, 5] >> 16 & 255], np.int64)
            win = out[Y0:Y1 + 1, X0:X1 + 1].astype(np.int64)
            out[Y0:Y1 + 1, X0:X1 + 1] = (win + (((col - win) * (int(q[i, 6]) * cov[:, :, None]) + 32768) >> 16)).astype(np.uint8)
        i = j
    return out


def _as_image(image) -> np.ndarray:
    a = np.asarray(image)
    if a.dtype != np.uint8 or a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] not in (1, 3, 4)) or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"expected a uint8 image [h, w], [h, w, 3] (RGB) or [h, w, 4] (RGBA), got {a.dtype} {a.shape}")
    return np.ascontiguousarray(a.reshape(a.shape[0], a.shape[1], -1))


def reduced_size(h: int, w: int, k: int) -> tuple[int, int]:
    return -(-h // k), -(-w // k)


def reduce(image, k: int) -> np.ndarray:
    """The box average of the module docstring: gray / RGB / RGBA u8 -> BGR u8 [ceil(h/k)][ceil(w/k)][3]."""
    a = _as_image(image)
    if not (1 <= int(k) <= MAX_FACTOR):
        raise ValueError(f"factor {k} is outside 1..{MAX_FACTOR}")
    h, w, ch = a.shape
    src = (a[:, :, [0, 0, 0]] if ch == 1 else a[:, :, [2, 1, 0]]).astype(np.int64)
    ho, wo = reduced_size(h, w, k)
    pad = np.zeros((ho * k, wo * k, 3), np.int64)
    pad[:h, :w] = src
    ones = np.zeros((ho * k, wo * k), np.int64)
    ones[:h, :w] = 1
    total = pad.reshape(ho, k, wo, k, 3).sum(axis=(1, 3))
    n = ones.reshape(ho, k, wo, k).sum(axis=(1, 3))[:, :, None]
    return ((2 * total + n) // (2 * n)).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------- the GPU side

def draw_dev(ctx, canvas: np.ndarray, prims) -> np.ndarray:
    """gtx_op_plot_draw: a host canvas through the kernels (upload, bin, paint, download); returns the painted canvas."""
    from . import _lib

    p = as_prims(prims)
    f = np.array(canvas, dtype=np.uint8, copy=True, order="C")
    if f.ndim != 3 or f.shape[2] != 3:
        raise ValueError(f"expected an [h, w, 3] uint8 canvas, got {f.shape}")
    h, w = f.shape[:2]
    _lib.check(ctx.lib.gtx_op_plot_draw(ctx.handle, _lib.ptr(f), f.size, h, w, 3 * w, _lib.ptr(p) if len(p) else None, len(p)))
    return f


def draw_dev_pitched(ctx, buf: np.ndarray, h: int, w: int, pitch: int, prims) -> np.ndarray:
    """gtx_op_plot_draw on a raw byte buffer: rows of `pitch` bytes whose first 3 w are the canvas's, any bytes after row h - 1."""
    from . import _lib

    p = as_prims(prims)
    b = np.array(buf, dtype=np.uint8, copy=True, order="C").reshape(-1)
    _lib.check(ctx.lib.gtx_op_plot_draw(ctx.handle, _lib.ptr(b), b.size, int(h), int(w), int(pitch), _lib.ptr(p) if len(p) else None, len(p)))
    return b


def reduce_dev(ctx, image, k: int) -> np.ndarray:
    """gtx_op_plot_reduce: a host image through the reduce kernel."""
    from . import _lib

    a = _as_image(image)
    h, w, ch = a.shape
    ho, wo = reduced_size(h, w, max(int(k), 1))
    out = np.zeros((ho, wo, 3), np.uint8)
    _lib.check(ctx.lib.gtx_op_plot_reduce(ctx.handle, _lib.ptr(a), h, w, ch, int(k), _lib.ptr(out)))
    return out


STATS = ("upload_ms", "reduce_ms", "bin_ms", "paint_ms", "tiles", "entries", "max_per_tile", "prims")


class PlotCanvas:
    """gtx_plot_canvas_*: an image reduced by k into a BGR canvas in HBM, primitive lists painted into it, read back or handed
    to the JPEG encoder where it lies."""

    def __init__(self, ctx, image, k: int = 1):
        from . import _lib

        self._lib, self.ctx = _lib, ctx
        a = _as_image(image)
        h = C.c_void_p()
        _lib.check(ctx.lib.gtx_plot_canvas_create(ctx.handle, _lib.ptr(a), a.shape[0], a.shape[1], a.shape[2], int(k), C.byref(h)))
        self.handle = h
        self.h, self.w = reduced_size(a.shape[0], a.shape[1], int(k))

    def draw(self, prims) -> None:
        p = as_prims(prims)
        self._lib.check(self.ctx.lib.gtx_plot_canvas_draw(self.handle, self._lib.ptr(p) if len(p) else None, len(p)))

    def read(self) -> np.ndarray:
        out = np.zeros((self.h, self.w, 3), np.uint8)
        self._lib.check(self.ctx.lib.gtx_plot_canvas_read(self.handle, self._lib.ptr(out)))
        return out

    @property
    def dptr(self) -> int:
        p = C.c_void_p()
        self._lib.check(self.ctx.lib.gtx_plot_canvas_dptr(self.handle, C.byref(p)))
        return p.value

    def stats(self) -> dict:
        """Milliseconds of the creation's upload and reduce and of the last draw()'s binning and paint launches (between events;
        waits for them), and that draw's tile-list figures."""
        v = (C.c_double * len(STATS))()
        self._lib.check(self.ctx.lib.gtx_plot_canvas_stats(self.handle, v))
        return dict(zip(STATS, list(v)))

    def encode_jpeg(self, quality: int = 90, subsampling: str = "4:2:0") -> bytes:
        """The canvas as a baseline JPEG through the frame sink's encoder (gtx_jpeg_enc_*), from where it lies in HBM."""
        from . import jpeg

        lib, enc = self.ctx.lib, C.c_void_p()
        self._lib.check(lib.gtx_jpeg_enc_create(self.ctx.handle, self.h, self.w, int(quality), jpeg.SUBSAMPLINGS[subsampling][2], C.byref(enc)))
        try:
            self._lib.check(lib.gtx_jpeg_enc_submit_dev(enc, C.c_void_p(self.dptr)))
            n = C.c_size_t()
            rec = np.zeros(1 << 16, np.uint32).view(np.uint8)
            rc = lib.gtx_jpeg_enc_collect(enc, self._lib.ptr(rec), rec.nbytes, C.byref(n))
            if rc == 1:
                rec = np.zeros((n.value + 3) // 4, np.uint32).view(np.uint8)
                rc = lib.gtx_jpeg_enc_collect(enc, self._lib.ptr(rec), rec.nbytes, C.byref(n))
            self._lib.check(rc)
            return jpeg.record_to_bytes(rec[:n.value])
        finally:
            lib.gtx_jpeg_enc_destroy(enc)

    def close(self) -> None:
        if getattr(self, "handle", None):
            self.ctx.lib.gtx_plot_canvas_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
