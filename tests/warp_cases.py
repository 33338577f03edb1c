"""Shared by tests/test_warp_ops_gpu.py (GPU) and tests/test_geometry.py (CPU): the homographies the frame-warp kernel is held
against, the oracle's coordinate arithmetic with its intermediate values kept, and a plain restatement of the per-tile footprint
rule of csrc/warp.hip (corner coordinates, `pos`, the clamped box, `row_bytes`, `staged`).

The restatement is only ever used to show that a case is the edge it claims to be (which tiles are staged, which are not, where
the box is clamped). Expected pixels never come from it: they come from oracle/warp_ref.py alone."""
import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
_SRC = (ROOT / "geo-trax_amd" / "csrc" / "warp.hip").read_text()


def _const(name):
    m = re.search(rf"\b{name}\s*=\s*(\d+)(?:\s*\*\s*(\d+))?\s*[,;]", _SRC)
    return int(m.group(1)) * int(m.group(2) or 1)


TW, TH, LDS_CAP = _const("kTW"), _const("kTH"), _const("kLdsCap")
INT_MIN, INT_MAX = -2**31, 2**31 - 1


def hook_inverse(H):
    """The matrix the kernel is launched with for H: gtx_op_invert3x3 (host arithmetic)."""
    from geotrax_amd.warp import inverse_homography

    return inverse_homography(H)


def noise(seed, h, w):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def ramp(h, w):
    y, x, c = np.mgrid[0:h, 0:w, 0:3]
    return ((7 * x + 13 * y + 5 * c) & 255).astype(np.uint8)


# ---------------------------------------------------------------- the oracle's coordinates, intermediate values kept

def _src_coord(M, xi, yf):
    """saturate_cast<int>((X0 + M0*x1) * (32 / W)) for integer x (any shape) and float rows yf, operation by operation as
    oracle/warp_ref.py states it. Returns W before the division, the clamped products before rounding, and the rounded integers."""
    bx, x1 = (xi & ~63).astype(np.float64), (xi & 63).astype(np.float64)
    X0 = M[0] * bx + M[1] * yf + M[2]
    Y0 = M[3] * bx + M[4] * yf + M[5]
    W0 = M[6] * bx + M[7] * yf + M[8]
    W = W0 + M[6] * x1
    with np.errstate(divide="ignore", over="ignore"):
        Wi = np.where(W != 0.0, 32.0 / W, 0.0)
        pX, pY = (X0 + M[0] * x1) * Wi, (Y0 + M[3] * x1) * Wi
    assert not (np.isnan(pX).any() or np.isnan(pY).any()), "0 * inf in a coordinate: the case is outside what the oracle defines"
    fX = np.maximum(float(INT_MIN), np.minimum(float(INT_MAX), pX))
    fY = np.maximum(float(INT_MIN), np.minimum(float(INT_MAX), pY))
    return W, fX, fY, np.rint(fX).astype(np.int64), np.rint(fY).astype(np.int64)


def coords(h, w, Minv):
    """Per destination pixel: W, fX / fY (1/32-pixel units before rounding), X / Y (after), x0 / y0 / ax / ay."""
    M = np.asarray(Minv, np.float64).ravel()
    W, fX, fY, X, Y = _src_coord(M, np.arange(w)[None, :], np.arange(h, dtype=np.float64)[:, None])
    return SimpleNamespace(W=W, fX=fX, fY=fY, X=X, Y=Y, x0=X >> 5, y0=Y >> 5, ax=X & 31, ay=Y & 31)


# ---------------------------------------------------------------- the kernel's per-tile plan, restated

def plan(h, w, Minv):
    """Arrays over the tile grid [tiles in y, tiles in x]; corner arrays are [cj, ci, ty, tx] (cj: bottom row, ci: right column)."""
    M = np.asarray(Minv, np.float64).ravel()
    tx0, ty0 = np.arange(0, w, TW), np.arange(0, h, TH)
    cx = np.stack([tx0, np.minimum(tx0 + TW, w) - 1])[None, :, None, :]
    cy = np.stack([ty0, np.minimum(ty0 + TH, h) - 1])[:, None, :, None]
    cx, cy = np.broadcast_arrays(cx, cy)
    _, _, _, X, Y = _src_coord(M, cx, cy.astype(np.float64))
    lo_x, hi_x = (X >> 5).min((0, 1)), (X >> 5).max((0, 1))
    lo_y, hi_y = (Y >> 5).min((0, 1)), (Y >> 5).max((0, 1))
    Wc = M[6] * cx + M[7] * cy + M[8]
    pos = (Wc > 1e-9).all((0, 1))
    bx0, bx1 = np.clip(lo_x - 1, 0, w), np.clip(hi_x + 3, 0, w)
    by0, by1 = np.clip(lo_y - 1, 0, h), np.clip(hi_y + 3, 0, h)
    out_x, out_y = (lo_x > w) | (hi_x < -4), (lo_y > h) | (hi_y < -4)
    bx0, bx1 = np.where(out_x, 0, bx0), np.where(out_x, 0, bx1)
    by0, by1 = np.where(out_y, 0, by0), np.where(out_y, 0, by1)
    row_bytes = np.where(bx1 > bx0, ((bx1 * 3 + 15) & ~15) - ((bx0 * 3) & ~15), 0)
    nbytes = row_bytes * (by1 - by0)
    staged = pos & (row_bytes > 0) & (by1 > by0) & (nbytes <= LDS_CAP)
    return SimpleNamespace(h=h, w=w, X=X, Y=Y, Wc=Wc, lo_x=lo_x, hi_x=hi_x, lo_y=lo_y, hi_y=hi_y, pos=pos, bx0=bx0, bx1=bx1, by0=by0, by1=by1,
                           row_bytes=row_bytes, nbytes=nbytes, staged=staged, n_staged=int(staged.sum()), n_unstaged=int((~staged).sum()),
                           n_pos0=int((~pos).sum()))


def counts(p):
    return f"{p.staged.size} tiles: {p.n_staged} staged, {p.n_unstaged} unstaged (of them {p.n_pos0} with pos == 0)"


def staging(p, src_addr=0):
    """How the staged tiles of plan p are copied: `aligned` as the kernel decides it for a source at address src_addr (mod 16 is
    what matters), and the number of 16-byte chunks that take the image-tail branch (off + 16 > img_len)."""
    row_len = p.w * 3
    img_len = p.h * row_len
    aligned = row_len % 16 == 0 and src_addr % 16 == 0
    tail = chunks_total = 0
    for ty, tx in zip(*np.nonzero(p.staged)):
        a0 = (int(p.bx0[ty, tx]) * 3) & ~15
        chunks = int(p.row_bytes[ty, tx]) >> 4
        off = ((np.arange(p.by0[ty, tx], p.by1[ty, tx]) * row_len + a0)[:, None] + 16 * np.arange(chunks)[None, :])
        tail += int((off + 16 > img_len).sum())
        chunks_total += off.size
    return SimpleNamespace(aligned=aligned, tail_chunks=tail, chunks=chunks_total)


# ---------------------------------------------------------------- matrices (source -> destination, what the library is given)

def translation(tx, ty):
    return np.array([[1.0, 0.0, tx], [0.0, 1.0, ty], [0.0, 0.0, 1.0]])


def from_inverse(Minv):
    """H whose inverse is (to rounding) Minv, by the library's own adjugate: plain float64 arithmetic, the same on every machine.
    The tests always take the kernel's matrix from hook_inverse(H) again, never from Minv."""
    return hook_inverse(np.asarray(Minv, np.float64))


def scale_offset_inverse(sx, sy, ox, oy):
    """M = diag(sx, sy) + (ox, oy): destination (x, y) reads source (sx*x + ox, sy*y + oy)."""
    return from_inverse([[sx, 0.0, ox], [0.0, sy, oy], [0.0, 0.0, 1.0]])


TIES = translation(-1.0 / 64, -3.0 / 64)                     # M = translation (1/64, 3/64), exact
MIXED = scale_offset_inverse(2.25, 2.25, 0.3, 0.7)
ZOOM_IN = np.array([[4.0, 0.0, -10.5], [0.0, 4.0, -6.25], [0.0, 0.0, 1.0]])     # M = diag(1/4) + (2.625, 1.5625), exact
HORIZON = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [1.0 / 64, 0.0, 1.0]])    # M = [[1,0,0],[0,1,0],[-1/64,0,1]], exact
# W = 1 - x/200 + y/1000 vanishes between x = 200 and x = 205: tile column 0 lies before the horizon, column 1 across it, column 2 and 3 behind
HORIZON_GENERAL = from_inverse([[1.0, 0.03, 2.0], [-0.02, 1.0, 1.0], [-1.0 / 200, 1.0 / 1000, 1.0]])
PERSPECTIVE = np.array([[1.01, 0.02, 3.0], [-0.015, 0.99, -2.0], [1.1e-3, 0.9e-3, 1.0]])
ROT34 = np.array([[np.cos(0.6), -np.sin(0.6), 60.0], [np.sin(0.6), np.cos(0.6), -40.0], [1e-5, -1e-5, 1.0]])
OUTSIDE = (1e7, 3e9, -3e9)


def rot90(w):
    return np.array([[0.0, -1.0, w - 1.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])


def flips(h, w):
    return {"rot180": (np.array([[-1.0, 0.0, w - 1.0], [0.0, -1.0, h - 1.0], [0.0, 0.0, 1.0]]), lambda f: f[::-1, ::-1]),
            "flip-x": (np.array([[-1.0, 0.0, w - 1.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]), lambda f: f[:, ::-1]),
            "flip-y": (np.array([[1.0, 0.0, 0.0], [0.0, -1.0, h - 1.0], [0.0, 0.0, 1.0]]), lambda f: f[::-1])}


def clipped(h, w):
    """One translation per side of the source that the footprint runs over."""
    return {"left": translation(w / 2 + 0.37, 0.0), "right": translation(-(w / 2 + 0.37), 0.0),
            "top": translation(0.0, h / 2 + 0.61), "bottom": translation(0.0, -(h / 2 + 0.61))}


def camera(seed, strength=1.0):
    """A near-identity camera motion, as tests/test_warp_gpu.py draws them."""
    rng = np.random.default_rng(seed)
    a = 2e-3 * strength * rng.standard_normal()
    return np.array([[np.cos(a) * (1 + 1e-3 * strength), -np.sin(a), 6.0 * strength * rng.standard_normal()],
                     [np.sin(a), np.cos(a) * (1 - 1e-3 * strength), 6.0 * strength * rng.standard_normal()],
                     [1e-7 * strength * rng.standard_normal(), 1e-7 * strength * rng.standard_normal(), 1.0]])


CAP_HW = (48, 640)
_cap_found = []


def cap_scan():
    """Seeded scan for an anisotropic zoom-out M = diag(sx, sy) + offset on a 48 x 640 frame that holds, in one image, a staged tile
    with a footprint in (cap - 512, cap] bytes and an unstaged tile (W > 0 at its corners) with one in (cap, cap + 512]. Two
    families are tried in turn, around 1024 B x 16 rows and around 512 B x 32 rows; a candidate with a tile of exactly `cap`
    bytes is preferred, the first loose hit is the fallback. Returns (H, exact)."""
    if _cap_found:
        return _cap_found[0]
    h, w = CAP_HW
    rng = np.random.default_rng(11)
    loose = None
    for i in range(6000):
        if i & 1:
            sx, sy, ox, oy = rng.uniform(2.55, 2.75), rng.uniform(1.6, 1.9), rng.uniform(-300, 8), rng.uniform(0, 4)
        else:
            sx, sy, ox, oy = rng.uniform(1.25, 1.36), rng.uniform(3.8, 4.2), rng.uniform(0, 16), rng.uniform(1, 8)
        H = scale_offset_inverse(sx, sy, ox, oy)
        p = plan(h, w, hook_inverse(H))
        under = p.staged & (p.nbytes > LDS_CAP - 512)
        over = p.pos & ~p.staged & (p.nbytes > LDS_CAP) & (p.nbytes <= LDS_CAP + 512)
        if under.any() and over.any():
            if (p.staged & (p.nbytes == LDS_CAP)).any():
                _cap_found.append((H, True))
                return _cap_found[0]
            loose = loose if loose is not None else H
    assert loose is not None, "the scan found no matrix with tiles on both sides of the LDS cap"
    _cap_found.append((loose, False))
    return _cap_found[0]


def issue_matrices():
    """Every homography the GPU cases hand the library, by name (the CPU test of gtx_op_invert3x3 runs over them)."""
    m = {"identity": np.eye(3), "ties": TIES, "mixed": MIXED, "zoom-in": ZOOM_IN, "horizon": HORIZON, "horizon-general": HORIZON_GENERAL,
         "perspective": PERSPECTIVE, "rot34": ROT34, "rot90": rot90(200), "near-cap": cap_scan()[0], "camera": camera(5, 3.0)}
    for name, (H, _) in flips(21, 261).items():
        m[name] = H
    for name, H in clipped(21, 261).items():
        m["clipped-" + name] = H
    for t in OUTSIDE:
        m[f"outside-x{t:g}"], m[f"outside-y{t:g}"] = translation(t, 0.0), translation(0.0, t)
    return m
