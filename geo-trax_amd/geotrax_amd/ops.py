"""numpy-facing wrappers of the operator-level C ABI (gtx_op_*): host arrays in, host arrays out.

These exist so that every HIP kernel of the detector can be checked against oracle/ on the exact
layer shapes. Activations are NHWC; dtype float16 or float32.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import ConvDesc, check, ptr

GTX_F16, GTX_F32, GTX_F32S = 0, 1, 2


def _dt(a: np.ndarray) -> int:
    if a.dtype == np.float16:
        return GTX_F16
    if a.dtype == np.float32:
        return GTX_F32
    raise TypeError(f"activations must be float16 or float32, got {a.dtype}")


def conv2d(x: np.ndarray, w_ohwi: np.ndarray, bias: np.ndarray | None = None, *, stride: int = 1,
           act: bool = True, residual: np.ndarray | None = None, in_coff: int = 0, cin: int | None = None,
           out: np.ndarray | None = None, out_coff: int = 0, split: bool = False, ctx: _lib.Context | None = None) -> np.ndarray:
    """act(conv2d(x[..., in_coff:in_coff+cin], w) + b) (+ residual), written into
    out[..., out_coff:out_coff+cout]. x: [n,h,w,cs]; w_ohwi: [cout,k,k,cin] fp32. split=True (float32 arrays only):
    the split-f16x3 kernel (GTX_F32S) instead of the exact-fp32 MFMA."""
    ctx = ctx or _lib.default_context()
    x = np.ascontiguousarray(x)
    w = np.ascontiguousarray(w_ohwi, dtype=np.float32)
    cout, k, _, wcin = w.shape
    cin = wcin if cin is None else cin
    assert cin == wcin
    n, h, wd, cs = x.shape
    pad = k // 2
    ho, wo = (h + 2 * pad - k) // stride + 1, (wd + 2 * pad - k) // stride + 1
    if out is None:
        out = np.zeros((n, ho, wo, cout), dtype=x.dtype)
    out = np.ascontiguousarray(out)
    assert out.shape[:3] == (n, ho, wo) and out.dtype == x.dtype
    if split and x.dtype != np.float32:
        raise TypeError("split=True needs float32 activations")
    d = ConvDesc(dtype=GTX_F32S if split else _dt(x), n=n, h=h, w=wd, cin=cin, cout=cout, ksize=k, stride=stride, act=int(act),
                 in_cstride=cs, in_coff=in_coff, out_cstride=out.shape[3], out_coff=out_coff,
                 has_residual=int(residual is not None))
    b = None if bias is None else np.ascontiguousarray(bias, dtype=np.float32)
    r = None if residual is None else np.ascontiguousarray(residual, dtype=x.dtype)
    check(ctx.lib.gtx_op_conv2d(ctx.handle, C.byref(d), ptr(x), ptr(w), ptr(b), ptr(r), ptr(out)))
    return out


def conv2d_group(members, *, stride: int = 1, act: bool = True, split: bool = False, ctx: _lib.Context | None = None):
    """One grouped launch (the Detect stages' form). members: dicts with x [n,h,w,cs], w [cout,k,k,cin] and optionally bias,
    in_coff, out (the output buffer as it is before the launch), out_coff, ty_first, ty_count (compute only these 8-row output
    tile rows; the others keep what `out` holds). Returns the members' outputs."""
    ctx = ctx or _lib.default_context()
    m = len(members)
    descs = (ConvDesc * m)()
    keep, outs = [], []
    xs, ws, bs, ys = (C.c_void_p * m)(), (C.c_void_p * m)(), (C.c_void_p * m)(), (C.c_void_p * m)()
    tf, tc = (C.c_int * m)(), (C.c_int * m)()
    for i, mem in enumerate(members):
        x = np.ascontiguousarray(mem["x"])
        w = np.ascontiguousarray(mem["w"], dtype=np.float32)
        cout, k, _, cin = w.shape
        n, h, wd, cs = x.shape
        pad = k // 2
        ho, wo = (h + 2 * pad - k) // stride + 1, (wd + 2 * pad - k) // stride + 1
        out = mem.get("out")
        out = np.zeros((n, ho, wo, cout), dtype=x.dtype) if out is None else np.array(out, dtype=x.dtype, order="C")
        assert out.shape[:3] == (n, ho, wo)
        b = None if mem.get("bias") is None else np.ascontiguousarray(mem["bias"], dtype=np.float32)
        descs[i] = ConvDesc(dtype=GTX_F32S if split else _dt(x), n=n, h=h, w=wd, cin=cin, cout=cout, ksize=k, stride=stride, act=int(act),
                            in_cstride=cs, in_coff=mem.get("in_coff", 0), out_cstride=out.shape[3], out_coff=mem.get("out_coff", 0), has_residual=0)
        xs[i], ws[i], bs[i], ys[i] = x.ctypes.data, w.ctypes.data, (b.ctypes.data if b is not None else None), out.ctypes.data
        tf[i], tc[i] = mem.get("ty_first", 0), mem.get("ty_count", 0)
        keep += [x, w, b]
        outs.append(out)
    check(ctx.lib.gtx_op_conv2d_group(ctx.handle, m, descs, xs, ws, bs, ys, tf, tc))
    return outs


def conv2d_time(dtype, n, h, w, cin, cout, ksize, stride, iters=20, ctx=None):
    """Mean kernel time (ms) and algorithmic FLOPs of one conv launch on zero-filled data."""
    ctx = ctx or _lib.default_context()
    d = ConvDesc(dtype=dtype, n=n, h=h, w=w, cin=cin, cout=cout, ksize=ksize, stride=stride, act=1,
                 in_cstride=cin, in_coff=0, out_cstride=cout, out_coff=0, has_residual=0)
    ms, fl = C.c_float(), C.c_double()
    check(ctx.lib.gtx_op_conv2d_time(ctx.handle, C.byref(d), iters, C.byref(ms), C.byref(fl)))
    return ms.value, fl.value


def sppf_pool(x: np.ndarray, c: int, ctx=None, split: bool = False) -> np.ndarray:
    """x: [n,h,w,4c]; fills channels [c,4c) with the 5/9/13 window maxima of channels [0,c). split (float32 only): the
    device tensor is in the pair format of the default fp32 path (values come back as hi + lo, i.e. 22-bit rounded)."""
    ctx = ctx or _lib.default_context()
    x = np.ascontiguousarray(x).copy()
    n, h, w, cs = x.shape
    assert cs == 4 * c and (not split or x.dtype == np.float32)
    check(ctx.lib.gtx_op_sppf_pool(ctx.handle, GTX_F32S if split else _dt(x), n, h, w, c, ptr(x)))
    return x


def upsample2x(x: np.ndarray, c: int, in_coff: int, out: np.ndarray, out_coff: int, ctx=None) -> np.ndarray:
    ctx = ctx or _lib.default_context()
    x = np.ascontiguousarray(x)
    out = np.ascontiguousarray(out).copy()
    n, h, w, cs = x.shape
    check(ctx.lib.gtx_op_upsample2x(ctx.handle, _dt(x), n, h, w, c, ptr(x), cs, in_coff, ptr(out), out.shape[3], out_coff))
    return out


def psa_attention(qkv: np.ndarray, pe_w: np.ndarray, pe_b: np.ndarray, heads: int, *, n: int | None = None, in_coff: int = 0,
                  out: np.ndarray | None = None, out_coff: int = 0, split: bool = False, form: int = 0, iters: int = 0, ctx=None):
    """C2PSA's attention on maps: qkv [n_alloc, h, w, cs] with heads x [q 32 | k 32 | v 64] channels from in_coff; pe_w [64 heads, 1, 3, 3]
    (the depthwise conv's own layout), pe_b [64 heads]. The first n maps run (default all). form: 0 the library's choice, 1 / 2 the
    large- / small-map kernel. Returns (out [n, h, w, cs_out], saturated, ms per launch or None)."""
    ctx = ctx or _lib.default_context()
    qkv = np.ascontiguousarray(qkv)
    na, h, w, cs = qkv.shape
    n = na if n is None else n
    c = heads * 64
    if out is None:
        out = np.zeros((n, h, w, c), qkv.dtype)
    out = np.ascontiguousarray(out).copy()
    assert out.shape[:3] == (n, h, w) and out.dtype == qkv.dtype and (not split or qkv.dtype == np.float32)
    wt = np.ascontiguousarray(np.asarray(pe_w, np.float32).reshape(c, 9).T)     # tap-major
    b = np.ascontiguousarray(pe_b, dtype=np.float32)
    ms, sat = C.c_float(), C.c_int()
    check(ctx.lib.gtx_op_psa_attention(ctx.handle, GTX_F32S if split else _dt(qkv), n, na, h, w, heads, ptr(qkv), cs, in_coff, ptr(wt), ptr(b),
                                       ptr(out), out.shape[3], out_coff, form, iters, C.byref(ms), C.byref(sat)))
    return out, bool(sat.value), (ms.value if iters > 0 else None)


def dwconv(x: np.ndarray, w: np.ndarray, bias: np.ndarray, *, stride: int = 1, act: int = 1, residual: np.ndarray | None = None,
           split: bool = False, ctx=None):
    """Depthwise k x k convolution (k = 3, 5, 7; pad k / 2) + bias + activation (0 none, 1 SiLU, 2 ReLU) + residual after the
    activation. x [n, h, w, c]; w [c, 1, k, k] (the conv's own layout); residual [n, ho, wo, c]. split=True (float32 arrays): the
    pair format on the device (GTX_F32S). Returns (out, saturated)."""
    ctx = ctx or _lib.default_context()
    x = np.ascontiguousarray(x)
    n, h, wd, c = x.shape
    k = int(w.shape[-1])
    wt = np.ascontiguousarray(np.asarray(w, np.float32).reshape(c, k * k).T)     # tap-major
    b = np.ascontiguousarray(bias, dtype=np.float32)
    out = np.zeros((n, (h - 1) // stride + 1, (wd - 1) // stride + 1, c), x.dtype)
    r = None if residual is None else np.ascontiguousarray(residual, dtype=x.dtype)
    assert r is None or r.shape == out.shape
    sat = C.c_int()
    check(ctx.lib.gtx_op_dwconv(ctx.handle, GTX_F32S if split else _dt(x), n, h, wd, c, k, stride, ptr(x), ptr(wt), ptr(b), int(act), ptr(r), ptr(out),
                                C.byref(sat)))
    return out, bool(sat.value)


def preprocess(frame_bgr: np.ndarray, net_h: int, net_w: int, dtype=np.float32, want_gray: bool = True, ctx=None):
    """Letterbox + BGR->RGB + /255 into [net_h,net_w,4] (RGB0) and the half-res gray image."""
    ctx = ctx or _lib.default_context()
    frame = np.ascontiguousarray(frame_bgr, dtype=np.uint8)
    h, w, _ = frame.shape
    img = np.zeros((net_h, net_w, 4), dtype=dtype)
    gray = np.zeros((h // 2, w // 2), dtype=np.uint8) if want_gray else None
    check(ctx.lib.gtx_op_preprocess(ctx.handle, _dt(img), ptr(frame), h, w, net_h, net_w, ptr(img), ptr(gray),
                                    h // 2, w // 2))
    return img, gray


def match_2nn(query: np.ndarray, train: np.ndarray, iters: int = 0, ctx: _lib.Context | None = None):
    """2 nearest train rows (L2) of every query row; unit-norm [n,128] fp32 descriptors.
    -> (idx1, idx2, d1, d2[, ms_per_pass when iters > 0])."""
    ctx = ctx or _lib.default_context()
    q = np.ascontiguousarray(query, np.float32).reshape(-1, 128)
    t = np.ascontiguousarray(train, np.float32).reshape(-1, 128)
    nq, nt = len(q), len(t)
    i1, i2 = np.full(nq, -1, np.int32), np.full(nq, -1, np.int32)
    d1, d2 = np.zeros(nq, np.float32), np.zeros(nq, np.float32)
    ms = C.c_float()
    check(ctx.lib.gtx_op_match_2nn(ctx.handle, ptr(q), nq, ptr(t if nt else np.zeros((1, 128), np.float32)), nt, ptr(i1), ptr(i2),
                                   ptr(d1), ptr(d2), iters, C.byref(ms)))
    return (i1, i2, d1, d2, ms.value) if iters > 0 else (i1, i2, d1, d2)


def clahe(gray: np.ndarray, ctx=None) -> np.ndarray:
    """cv2.createCLAHE(clipLimit=2.0, tileGridSize=(8, 8)).apply(gray) on the GPU (the stabilizer's `clahe: true` step)."""
    ctx = ctx or _lib.default_context()
    g = np.ascontiguousarray(gray, dtype=np.uint8)
    out = np.empty_like(g)
    check(ctx.lib.gtx_op_clahe(ctx.handle, ptr(g), g.shape[0], g.shape[1], ptr(out)))
    return out


def conv_xcd_ranges(blocks, cin):
    """How a grouped convolution launch of len(blocks) members is cut over the 8 XCDs (host only).
    -> (xcd_begin [9] int32, grid_blocks)."""
    lib = _lib.load()
    b = np.ascontiguousarray(blocks, dtype=np.int32)
    c = np.ascontiguousarray(cin, dtype=np.int32)
    out = np.zeros(9, np.int32)
    grid = C.c_int()
    check(lib.gtx_op_conv_xcd_ranges(len(b), b.ctypes.data, c.ctypes.data, out.ctypes.data, C.addressof(grid)))
    return out, grid.value
