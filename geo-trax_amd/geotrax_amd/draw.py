"""The drawing rule of the visualize stage: the numpy twin of csrc/draw.hip, the glyph atlas and the binding of gtx_drawer_*.

What the reference draws with cv2.rectangle / cv2.line / cv2.polylines / cv2.circle / cv2.putText in annotate_frame and
draw_oriented_box (geotrax/visualize.py:662-940) is, here, a list of primitives painted into a BGR u8 frame [h][w][3] that
stays in HBM. This docstring is the specification; `rasterize` below and the kernel compute it bit for bit.

A primitive is eight int32: kind, x0, y0, x1, y1, p0, p1, bgr. bgr = b | g << 8 | r << 16. x0, y0, x1, y1 lie in
[-32768, 32767]. Primitives are applied in index order: a later one paints over an earlier one.

A primitive gives the pixel (x, y) a coverage a in 0..256, and every channel becomes

    out = (dst * (256 - a) + col * a + 128) >> 8

so a = 0 leaves the byte and a = 256 writes the colour.

  kind 0 FILL     cv2.rectangle(..., -1): the corners (x0, y0), (x1, y1) inclusive, in any order. a = 256 inside.
  kind 1 SEGMENT  every anti-aliased line of the reference: endpoints (x0, y0), (x1, y1), p0 = thickness t >= 1, round caps.
                  Integers vx = x1 - x0, vy = y1 - y0, wx = x - x0, wy = y - y0; int64 L = vx^2 + vy^2, s = wx vx + wy vy.
                  The squared distance D2 as float64: s <= 0 -> wx^2 + wy^2 (a zero-length segment always lands here);
                  s >= L -> (x - x1)^2 + (y - y1)^2; otherwise (double)c * (double)c / (double)L with c = wx vy - wy vx.
                  d = sqrt(D2); a = clamp(floor(((0.5 t + 0.5) - d) * 256 + 0.5), 0, 256). Every float64 operation is rounded
                  once, in this order (the kernel's file is compiled with -ffp-contract=off).
  kind 2 RING     cv2.circle(..., r, color, t) as the tail uses it (not anti-aliased): centre (x0, y0), x1 = r >= 0, p0 = t >= 1.
                  With the integer D = 4 ((x - x0)^2 + (y - y0)^2): a = 256 iff max(2r - t, 0)^2 <= D <= (2r + t)^2.
  kind 3 GLYPH    one character cell: top-left (x0, y0), x1, y1 = the cell's width and height, p0 = byte offset of the cell in
                  the coverage atlas, p1 = its row pitch. Inside the cell the atlas byte c = atlas[p0 + (y - y0) p1 + (x - x0)]
                  gives a = c + (c >> 7) (255 -> 256); an offset outside the atlas gives a = 0 (`validate` refuses such a record).

Bounding boxes (inclusive, clamped to int16): no pixel outside a primitive's box has a > 0, which is what lets the kernel cull.
FILL: its corners. SEGMENT: the endpoints' hull grown by (t + 1) // 2 + 1 (a > 0 needs d < t / 2 + 1/2, and a pixel k columns
or rows outside the hull has d >= k). RING: the centre +- (r + (t + 1) // 2) (a > 0 needs d <= r + t / 2). GLYPH: the cell.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

FILL, SEGMENT, RING, GLYPH = 0, 1, 2, 3
COORD_MIN, COORD_MAX = -32768, 32767
MAX_PRIMS = 1 << 20                                    # what one drawer may be created for (csrc/draw.hpp kDrawMaxPrims)


def pack_bgr(color) -> int:
    b, g, r = (int(v) for v in color)
    return b | g << 8 | r << 16


def as_prims(prims) -> np.ndarray:
    p = np.asarray(prims, dtype=np.int64).reshape(-1, 8)
    if p.size and ((p < -2**31) | (p > 2**31 - 1)).any():
        raise ValueError("a primitive field does not fit int32")
    return np.ascontiguousarray(p.astype(np.int32))


def validate(prims, atlas_bytes: int = 0, max_prims: int | None = None) -> None:
    """The checks of csrc/draw.cpp, in its order; ValueError names the first bad record's index."""
    p = as_prims(prims).astype(np.int64)
    if max_prims is not None and len(p) > max_prims:
        raise ValueError(f"{len(p)} primitives, the drawer holds {max_prims}")
    for i, (kind, x0, y0, x1, y1, p0, p1, _) in enumerate(p.tolist()):
        if kind not in (FILL, SEGMENT, RING, GLYPH):
            raise ValueError(f"primitive {i}: kind {kind}")
        if not all(COORD_MIN <= v <= COORD_MAX for v in (x0, y0, x1, y1)):
            raise ValueError(f"primitive {i}: a coordinate outside [-32768, 32767]")
        if kind in (SEGMENT, RING) and p0 < 1:
            raise ValueError(f"primitive {i}: thickness {p0}")
        if kind == RING and x1 < 0:
            raise ValueError(f"primitive {i}: radius {x1}")
        if kind == GLYPH and not (x1 > 0 and y1 > 0 and p1 > 0 and p0 >= 0 and p0 + (y1 - 1) * p1 + x1 <= atlas_bytes):
            raise ValueError(f"primitive {i}: the glyph cell leaves the atlas of {atlas_bytes} bytes")


def bounding_boxes(prims) -> np.ndarray:
    """[n][4] int16 x_lo, y_lo, x_hi, y_hi (inclusive): the conservative boxes of the module docstring."""
    p = as_prims(prims).astype(np.int64)
    kind, x0, y0, x1, y1, p0 = (p[:, k] for k in range(6))
    g = np.where(kind == SEGMENT, (p0 + 1) // 2 + 1, 0)
    lo_x, hi_x = np.minimum(x0, x1) - g, np.maximum(x0, x1) + g
    lo_y, hi_y = np.minimum(y0, y1) - g, np.maximum(y0, y1) + g
    ring, glyph = kind == RING, kind == GLYPH
    e = x1 + (p0 + 1) // 2
    lo_x, hi_x = np.where(ring, x0 - e, lo_x), np.where(ring, x0 + e, hi_x)
    lo_y, hi_y = np.where(ring, y0 - e, lo_y), np.where(ring, y0 + e, hi_y)
    lo_x, hi_x = np.where(glyph, x0, lo_x), np.where(glyph, x0 + x1 - 1, hi_x)
    lo_y, hi_y = np.where(glyph, y0, lo_y), np.where(glyph, y0 + y1 - 1, hi_y)
    return np.clip(np.stack([lo_x, lo_y, hi_x, hi_y], axis=1), COORD_MIN, COORD_MAX).astype(np.int16)


def coverage(prim, xs: np.ndarray, ys: np.ndarray, atlas: np.ndarray | None = None) -> np.ndarray:
    """a (int64, 0..256) of one primitive at the pixels xs x ys (1-D integer arrays) -> [len(ys)][len(xs)]."""
    kind, x0, y0, x1, y1, p0, p1, _ = (int(v) for v in prim)
    x = np.asarray(xs, np.int64)[None, :]
    y = np.asarray(ys, np.int64)[:, None]
    shape = (y.shape[0], x.shape[1])
    if kind == FILL:
        inside = (x >= min(x0, x1)) & (x <= max(x0, x1)) & (y >= min(y0, y1)) & (y <= max(y0, y1))
        return np.where(inside, 256, 0).astype(np.int64)
    if kind == SEGMENT:
        vx, vy = x1 - x0, y1 - y0
        wx, wy = np.broadcast_to(x - x0, shape), np.broadcast_to(y - y0, shape)
        L = vx * vx + vy * vy
        s = wx * vx + wy * vy
        c = (wx * vy - wy * vx).astype(np.float64)
        first = (wx * wx + wy * wy).astype(np.float64)
        ex, ey = np.broadcast_to(x - x1, shape), np.broadcast_to(y - y1, shape)
        second = (ex * ex + ey * ey).astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            mid = c * c / np.float64(L)
        d2 = np.where(s <= 0, first, np.where(s >= L, second, mid))
        v = np.floor(((0.5 * p0 + 0.5) - np.sqrt(d2)) * 256.0 + 0.5)
        return np.clip(v, 0.0, 256.0).astype(np.int64)
    if kind == RING:
        dx, dy = np.broadcast_to(x - x0, shape), np.broadcast_to(y - y0, shape)
        D = 4 * (dx * dx + dy * dy)
        lo, hi = max(2 * x1 - p0, 0) ** 2, (2 * x1 + p0) ** 2
        return np.where((D >= lo) & (D <= hi), 256, 0).astype(np.int64)
    if kind == GLYPH:
        cx, cy = np.broadcast_to(x - x0, shape), np.broadcast_to(y - y0, shape)
        inside = (cx >= 0) & (cx < x1) & (cy >= 0) & (cy < y1)
        off = p0 + cy * p1 + cx
        n = 0 if atlas is None else int(atlas.size)
        ok = inside & (off >= 0) & (off < n)
        cval = np.zeros(shape, np.int64)
        if ok.any():
            cval[ok] = np.asarray(atlas, np.uint8).reshape(-1)[off[ok]]
        return cval + (cval >> 7)
    raise ValueError(f"kind {kind}")


def rasterize(frame: np.ndarray, prims, atlas: np.ndarray | None = None, cull: bool = True) -> np.ndarray:
    """The frame with the primitives painted in index order. cull=False evaluates every primitive at every pixel; the two agree."""
    out = np.array(frame, dtype=np.uint8, copy=True)
    if out.ndim != 3 or out.shape[2] != 3:
        raise ValueError(f"expected an [h, w, 3] uint8 frame, got {out.shape}")
    h, w = out.shape[:2]
    p = as_prims(prims)
    boxes = bounding_boxes(p).astype(np.int64)
    for prim, (bx0, by0, bx1, by1) in zip(p.tolist(), boxes.tolist()):
        if cull:
            bx0, by0, bx1, by1 = max(bx0, 0), max(by0, 0), min(bx1, w - 1), min(by1, h - 1)
            if bx0 > bx1 or by0 > by1:
                continue
        else:
            bx0, by0, bx1, by1 = 0, 0, w - 1, h - 1
        a = coverage(prim, np.arange(bx0, bx1 + 1), np.arange(by0, by1 + 1), atlas)[:, :, None]
        col = np.array([prim[7] & 255, prim[7] >> 8 & 255, prim[7] >> 16 & 255], np.int64)
        win = out[by0:by1 + 1, bx0:bx1 + 1].astype(np.int64)
        out[by0:by1 + 1, bx0:bx1 + 1] = ((win * (256 - a) + col * a + 128) >> 8).astype(np.uint8)
    return out


# ---------------------------------------------------------------------------------------------------------------- glyph atlas

class GlyphAtlas:
    """Coverage cells of ASCII 32..126 from Pillow's default FreeType font, built once per run. The reference writes its labels with
    cv2.putText(FONT_HERSHEY_SIMPLEX, fontScale = line_width / 3); here the text height is round(22 * line_width / 3) pixels (Hershey
    simplex's cap height at that scale) and the font size is the smallest whose capital H is that tall. A character outside
    32..126 is drawn as '?'. No kerning: a label is its cells side by side on one baseline."""

    def __init__(self, line_width: int = 2):
        from PIL import Image, ImageDraw, ImageFont

        self.text_height = max(int(round(22 * line_width / 3)), 1)
        font = None
        try:
            for size in range(self.text_height, 4 * self.text_height + 8):
                f = ImageFont.load_default(size=size)
                box = f.getbbox("H")
                if box[3] - box[1] >= self.text_height:
                    font = f
                    break
        except (TypeError, OSError, AttributeError) as e:
            raise RuntimeError(f"Pillow cannot produce its default font at a given size ({e}): labels cannot be drawn; --hide-labels still works") from e
        if font is None:
            raise RuntimeError("Pillow's default font never reaches the label height: labels cannot be drawn; --hide-labels still works")
        self.ascent, descent = font.getmetrics()
        self.cell_h = self.ascent + descent
        self.cells: dict[int, tuple[int, int]] = {}        # code -> (byte offset, width = pitch)
        self.blank: set[int] = set()
        parts, off = [], 0
        for code in range(32, 127):
            ch = chr(code)
            cw = max(int(np.ceil(font.getlength(ch))), 1)
            img = Image.new("L", (cw, self.cell_h), 0)
            ImageDraw.Draw(img).text((0, 0), ch, font=font, fill=255)
            cell = np.asarray(img, np.uint8)
            if not cell.any():
                self.blank.add(code)
            self.cells[code] = (off, cw)
            parts.append(cell.reshape(-1))
            off += cell.size
        self.data = np.ascontiguousarray(np.concatenate(parts))

    def _code(self, ch: str) -> int:
        return ord(ch) if 32 <= ord(ch) <= 126 else ord("?")

    def text_size(self, label: str) -> tuple[int, int]:
        """(width, height) as cv2.getTextSize(label, ...)[0] is used: the cells' widths, the nominal text height."""
        return sum(self.cells[self._code(ch)][1] for ch in label), self.text_height

    def layout(self, label: str, x: int, y: int, color) -> list[tuple]:
        """GLYPH records of `label` with its baseline's left end at (x, y), cv2.putText's origin. Empty cells (the space) are left out."""
        out, bgr = [], pack_bgr(color)
        for ch in label:
            code = self._code(ch)
            off, cw = self.cells[code]
            if code not in self.blank:
                out.append((GLYPH, x, y - self.ascent, cw, self.cell_h, off, cw, bgr))
            x += cw
        return out


# ---------------------------------------------------------------------------------------------------------------- the GPU side

def _blob(atlas):
    a = np.zeros(0, np.uint8) if atlas is None else np.ascontiguousarray(atlas, dtype=np.uint8).reshape(-1)
    return a, (a.ctypes.data_as(C.c_void_p) if a.size else None)


def draw_dev(ctx, frame: np.ndarray, prims, atlas: np.ndarray | None = None) -> np.ndarray:
    """gtx_op_draw: a host frame through the kernel (upload, one drawer, download); returns the painted frame."""
    from . import _lib

    f = np.array(frame, dtype=np.uint8, copy=True, order="C")
    if f.ndim != 3 or f.shape[2] != 3:
        raise ValueError(f"expected an [h, w, 3] uint8 frame, got {f.shape}")
    p = as_prims(prims)
    a, ap = _blob(atlas)
    _lib.check(ctx.lib.gtx_op_draw(ctx.handle, _lib.ptr(f), f.shape[0], f.shape[1], _lib.ptr(p) if len(p) else None, len(p), ap, a.size))
    return f


class Drawer:
    """gtx_drawer_*: paints primitive lists into frames in HBM, on the context's stream, without waiting."""

    def __init__(self, ctx, frame_hw: tuple[int, int], max_prims: int, atlas: np.ndarray | None = None):
        from . import _lib

        self._lib, self.ctx = _lib, ctx
        self.h, self.w = int(frame_hw[0]), int(frame_hw[1])
        a, ap = _blob(atlas)
        h = C.c_void_p()
        _lib.check(ctx.lib.gtx_drawer_create(ctx.handle, self.h, self.w, int(max_prims), ap, a.size, C.byref(h)))
        self.handle = h

    def draw(self, frame_dptr: int, prims) -> None:
        p = as_prims(prims)
        self._lib.check(self.ctx.lib.gtx_drawer_draw_dev(self.handle, C.c_void_p(int(frame_dptr)), self._lib.ptr(p) if len(p) else None, len(p)))

    def last_ms(self) -> float:
        """The launch of the last draw() between two events (waits for it); 0 when that call launched nothing."""
        ms = C.c_float()
        self._lib.check(self.ctx.lib.gtx_drawer_last_ms(self.handle, C.byref(ms)))
        return ms.value

    def close(self) -> None:
        if getattr(self, "handle", None):
            self.ctx.lib.gtx_drawer_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
