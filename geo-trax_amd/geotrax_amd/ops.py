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


def conv2d_fused(x: np.ndarray | None, w_ohwi: np.ndarray, bias: np.ndarray | None = None, *, stride: int = 1, act: bool = True,
                 residual: np.ndarray | None = None, in_coff: int = 0, cin: int | None = None, out: np.ndarray | None = None, out_coff: int = 0,
                 split: bool = True, in_shape=None, x2: np.ndarray | None = None, in2_coff: int = 0, c_split: int = 0, out_plain: bool = False,
                 want_sat: bool = False, post_w: np.ndarray | None = None, post_bias: np.ndarray | None = None, post_act: int = 1, post_separate: bool = False,
                 front_img: np.ndarray | None = None, front_w27: np.ndarray | None = None, front_bias: np.ndarray | None = None,
                 front_hw=None, ty_first: int = 0, ty_count: int = 0, force_kc: int = 0, members: int = 0,
                 res_coff: int | None = None, in_place: bool = False, ctx: _lib.Context | None = None):
    """conv2d with the extras of gtx_conv_fused (include/gtx.h), one launch. x2 [n,h/2,w/2,cs2]: the second source, whose channels
    [in2_coff, in2_coff + c_split) upsampled 2x are the layer's first c_split input channels. post_w [cout,cout] (or [cout,1,1,cout]),
    post_bias, post_act: the fused 1x1 layer (post_separate: the same two layers as two launches, the intermediate map staying in
    HBM in the pair format). front_img [n,H,W,4] RGB0 bytes, front_w27 [27,cin], front_bias: the fused stem; x may
    then be None and the layer's input map is in_shape = (n, h, w) (default: half of front_img's sides); front_hw overrides the image
    size told to the launcher. res_coff (not None): residual is [n,ho,wo,rcs] and the launch adds its channels [res_coff, res_coff + cout).
    in_place (stride 1): x is the one buffer [n,h,w,cs] behind input, residual (channels from res_coff, when given) and output (channels
    from out_coff); a copy of it is handed over once and comes back with the output slice written. Returns the output, or (output, sat)
    with want_sat."""
    ctx = ctx or _lib.default_context()
    w = np.ascontiguousarray(w_ohwi, dtype=np.float32)
    cout, k, _, wcin = w.shape
    cin = wcin if cin is None else cin
    assert cin == wcin
    dt = np.float32
    if x is not None:
        x = np.ascontiguousarray(x)
        n, h, wd, cs = x.shape
        dt = x.dtype
    else:
        assert front_img is not None, "only a front stage computes its own input"
        n, h, wd = in_shape if in_shape is not None else (front_img.shape[0], front_img.shape[1] // 2, front_img.shape[2] // 2)
        cs = cin
    if split and dt != np.float32:
        raise TypeError("split=True needs float32 activations")
    pad = k // 2
    ho, wo = (h + 2 * pad - k) // stride + 1, (wd + 2 * pad - k) // stride + 1
    if in_place:
        assert x is not None and out is None and residual is None, "in_place: x is the one buffer"
        x = out = np.array(x, order="C")                                   # the caller's array stays as it is
    elif out is None:
        out = np.zeros((n, ho, wo, cout), dtype=dt)
    else:
        out = np.array(out, dtype=dt, order="C")
    assert out.shape[:3] == (n, ho, wo)
    has_res = residual is not None or (in_place and res_coff is not None)
    d = ConvDesc(dtype=GTX_F32S if split else (GTX_F16 if dt == np.float16 else GTX_F32), n=n, h=h, w=wd, cin=cin, cout=cout, ksize=k,
                 stride=stride, act=int(act), in_cstride=cs, in_coff=in_coff, out_cstride=out.shape[3], out_coff=out_coff,
                 has_residual=int(has_res))
    f32 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float32)
    addr = lambda a: None if a is None else a.ctypes.data
    b, r = f32(bias), (None if residual is None else np.ascontiguousarray(residual, dtype=dt))
    if in_place and has_res:
        r = out
    assert r is None or r.shape[:3] == (n, ho, wo)
    assert res_coff is None or has_res, "res_coff needs a residual"
    x2a = None if x2 is None else np.ascontiguousarray(x2, dtype=dt)
    pw, pb, fw, fb = f32(post_w), f32(post_bias), f32(front_w27), f32(front_bias)
    fi = None if front_img is None else np.ascontiguousarray(front_img, dtype=np.uint8)
    assert pw is None or pw.size == cout * cout
    assert fi is None or (fi.ndim == 4 and fi.shape[3] == 4 and fw is not None and fw.shape == (27, cin) and fb is not None and fb.size == cin)
    assert x2a is None or x2a.shape[:3] == (n, h // 2, wd // 2)
    fh, fwp = front_hw if front_hw is not None else ((fi.shape[1], fi.shape[2]) if fi is not None else (0, 0))
    assert fi is None or fh * fwp <= fi.shape[1] * fi.shape[2]          # the launcher is told no more image than the array holds
    sat = C.c_int(0)
    f = _lib.ConvFused(x2=addr(x2a), in2_cstride=0 if x2a is None else x2a.shape[3], in2_coff=in2_coff, c_split=c_split, out_plain=int(out_plain),
                       sat=C.pointer(sat) if want_sat else None, post_w=addr(pw), post_bias=addr(pb), post_act=int(post_act), post_separate=int(post_separate),
                       front_img=addr(fi), front_w27=addr(fw), front_bias=addr(fb), front_h=fh, front_w_px=fwp, ty_first=ty_first,
                       ty_count=ty_count, force_kc=force_kc, members=members, res_cstride=0 if res_coff is None else r.shape[3],
                       res_coff=res_coff or 0, in_place=int(in_place))
    check(ctx.lib.gtx_op_conv2d_fused(ctx.handle, C.byref(d), C.byref(f), ptr(x), ptr(w), ptr(b), ptr(r), ptr(out)))
    return (out, sat.value) if want_sat else out


def stem(img: np.ndarray, w27: np.ndarray, bias: np.ndarray, *, dtype, packed: bool = True, ctx: _lib.Context | None = None) -> np.ndarray:
    """The stem launch (model.0) on img [n,h,w,4] RGB0 bytes: SiLU(conv 3x3 stride 2 of img / 255 + bias), w27 [27,c0] with row
    (ky * 3 + kx) * 3 + colour. dtype: GTX_F16 (packed: the matrix-core kernel, else the VALU one; fp16 out), GTX_F32 (the VALU
    kernel) or GTX_F32S (the split-f16x3 kernel; the values its pair-format output holds, as fp32)."""
    ctx = ctx or _lib.default_context()
    img = np.ascontiguousarray(img, dtype=np.uint8)
    w27 = np.ascontiguousarray(w27, dtype=np.float32)
    bias = np.ascontiguousarray(bias, dtype=np.float32)
    n, h, w, four = img.shape
    c0 = w27.shape[1]
    assert four == 4 and w27.shape == (27, c0) and bias.shape == (c0,)
    out = np.zeros((n, (h - 1) // 2 + 1, (w - 1) // 2 + 1, c0), np.float16 if dtype == GTX_F16 else np.float32)
    check(ctx.lib.gtx_op_stem(ctx.handle, int(dtype), int(packed), n, h, w, c0, ptr(img), ptr(w27), ptr(bias), ptr(out)))
    return out


def stem6(img: np.ndarray, w108: np.ndarray, bias: np.ndarray, *, dtype, iters: int = 0, ctx: _lib.Context | None = None):
    """yolov5.yaml's stem launch (model.0) on img [n,h,w,4] RGB0 bytes: SiLU(conv 6x6 stride 2 pad 2 of img / 255 + bias), w108 [108,c0]
    with row (ky * 6 + kx) * 3 + colour. dtype: GTX_F16 (the fp16 matrix-core kernel; fp16 out), GTX_F32 (the exact-fp32 kernel) or
    GTX_F32S (the split-f16x3 kernel; the values its pair-format output holds, as fp32). Returns the output [n,(h-2)//2+1,(w-2)//2+1,c0],
    or (output, milliseconds per launch over `iters` further launches) with iters > 0."""
    ctx = ctx or _lib.default_context()
    img = np.ascontiguousarray(img, dtype=np.uint8)
    w108 = np.ascontiguousarray(w108, dtype=np.float32)
    bias = np.ascontiguousarray(bias, dtype=np.float32)
    n, h, w, four = img.shape
    c0 = w108.shape[1]
    assert four == 4 and w108.shape == (108, c0) and bias.shape == (c0,)
    out = np.zeros((n, max((h - 2) // 2 + 1, 0), max((w - 2) // 2 + 1, 0), c0), np.float16 if dtype == GTX_F16 else np.float32)
    ms = C.c_float(0.0)
    check(ctx.lib.gtx_op_stem6(ctx.handle, int(dtype), n, h, w, c0, ptr(img), ptr(w108), ptr(bias), ptr(out), int(iters), C.byref(ms)))
    return (out, ms.value) if iters > 0 else out


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


def area_attention(qkv: np.ndarray, heads: int, area: int, *, planar: bool = False, in_coff: int = 0, out: np.ndarray | None = None,
                   out_coff: int = 0, split: bool = False, iters: int = 0, ctx=None):
    """YOLO12's area attention (AAttn) on maps: qkv [n, h, w, cs] with 96 heads channels from in_coff -- per head [q 32 | k 32 | v 32],
    or with planar [q of every head | k of every head | v of every head]. The h w positions, row-major, are cut into `area` equal runs
    and a position attends to its own run only. Returns (out [n, h, w, cs_out] with 32 heads channels written from out_coff, saturated,
    ms per launch or None). A map whose h w is no multiple of area is refused."""
    ctx = ctx or _lib.default_context()
    qkv = np.ascontiguousarray(qkv)
    n, h, w, cs = qkv.shape
    if out is None:
        out = np.zeros((n, h, w, heads * 32), qkv.dtype)
    out = np.ascontiguousarray(out).copy()
    assert out.shape[:3] == (n, h, w) and out.dtype == qkv.dtype and (not split or qkv.dtype == np.float32)
    ms, sat = C.c_float(), C.c_int()
    check(ctx.lib.gtx_op_area_attention(ctx.handle, GTX_F32S if split else _dt(qkv), n, h, w, heads, area, int(planar), ptr(qkv), cs, in_coff,
                                        ptr(out), out.shape[3], out_coff, iters, C.byref(ms), C.byref(sat)))
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


def pool_down(x: np.ndarray, c_avg: int, c_max: int = 0, *, n: int | None = None, in_coff: int = 0, avg: np.ndarray | None = None, avg_coff: int = 0,
              mx: np.ndarray | None = None, max_coff: int = 0, split: bool = False, iters: int = 0, ctx=None):
    """YOLOv9's AConv / ADown pools in one launch. x [n_alloc, h, w, cs] holds c_avg + c_max channels from in_coff. Returns (avg, max, ms):
    avg [n_alloc, h, w, .] = avg_pool2d(2, 1) of the first c_avg channels with a zero last row and column, max [n_alloc, h/2, w/2, .] =
    max_pool2d(3, 2, 1) of that average of the other c_max channels (None when c_max = 0). avg / mx given: the buffers as they are
    before the launch (written at avg_coff / max_coff; the first n images run, everything else comes back unchanged). split=True
    (float32 arrays): the pair format on the device (GTX_F32S)."""
    ctx = ctx or _lib.default_context()
    x = np.ascontiguousarray(x)
    na, h, w, cs = x.shape
    n = na if n is None else n
    avg = np.zeros((na, h, w, c_avg), x.dtype) if avg is None else np.array(avg, dtype=x.dtype, order="C")
    if c_max:
        mx = np.zeros((na, h // 2, w // 2, c_max), x.dtype) if mx is None else np.array(mx, dtype=x.dtype, order="C")
        assert mx.shape[:3] == (na, h // 2, w // 2)
    else:
        mx = None
    assert avg.shape[:3] == (na, h, w) and (not split or x.dtype == np.float32)
    ms = C.c_float()
    check(ctx.lib.gtx_op_pool_down(ctx.handle, GTX_F32S if split else _dt(x), n, na, h, w, c_avg, c_max, ptr(x), cs, in_coff, ptr(avg), avg.shape[3], avg_coff,
                                   ptr(mx), mx.shape[3] if c_max else 0, max_coff, iters, C.byref(ms)))
    return avg, mx, (ms.value if iters > 0 else None)


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


def georef_tracks(chain, x, y, bbox_unstab, veh_dim_px, frame_num, is_interpolated, plan: dict, quads, weights, *, frame_size,
                  visibility_margin: int, fps: float, conversion_factor: float = 3.6, boundary: int = 0, want=None, ctx=None) -> dict:
    """gtx_op_georef_tracks (include/gtx.h): the georeference stage's chain and every per-track column in one upload / download.
    chain: georeference.georef_chain(...); plan: georeference.track_plan(...) (order, seg, n_used, exp_off); quads [q, 8];
    weights: georeference.kinematics_weights(...). want: the output names to fetch (default all).
    -> dict(ortho_x, ortho_y, latitude, longitude, x_local, y_local, visibility, length_m, width_m, speed, accel, quad, ms)."""
    ctx = ctx or _lib.default_context()
    f64 = lambda a, shape: np.ascontiguousarray(a, np.float64).reshape(shape)
    i32 = lambda a: np.ascontiguousarray(a, np.int32).reshape(-1)
    x, y = f64(x, -1), f64(y, -1)
    n = len(x)
    frame_num = np.asarray(frame_num).reshape(-1)
    if len(frame_num) and (frame_num.dtype.kind not in "iu" or np.abs(frame_num.astype(np.int64)).max() >= 2 ** 31):
        raise ValueError("frame_num must be integers that fit 32 bits")
    bbox, dims, frames = f64(bbox_unstab, (-1, 4)), f64(veh_dim_px, (-1, 2)), i32(frame_num)
    interp = None if is_interpolated is None else i32(is_interpolated)
    for name, a in (("y", y), ("bbox_unstab", bbox), ("veh_dim_px", dims), ("frame_num", frames), ("is_interpolated", interp), ("order", plan["order"])):
        if a is not None and len(a) != n:
            raise ValueError(f"{name} has {len(a)} rows, x has {n}")
    order, seg, n_used = i32(plan["order"]), i32(plan["seg"]), i32(plan["n_used"])
    exp_off = np.ascontiguousarray(plan["exp_off"], np.int64).reshape(-1)
    if len(seg) != len(n_used) + 1 or len(exp_off) != len(seg):
        raise ValueError("plan: seg and exp_off need one entry more than n_used")
    quads = f64(quads if quads is not None else [], (-1, 8))
    weights = f64(weights, -1)
    cfg = _lib.GeorefTracksCfg(int(frame_size[0]), int(frame_size[1]), int(visibility_margin), float(fps), float(conversion_factor), int(boundary),
                               len(n_used))
    kinds = {"ortho_x": np.float64, "ortho_y": np.float64, "latitude": np.float64, "longitude": np.float64, "x_local": np.float64,
             "y_local": np.float64, "visibility": np.uint8, "length_m": np.float64, "width_m": np.float64, "speed": np.float64,
             "accel": np.float64, "quad": np.int32}
    out = {k: np.empty(n, dt) for k, dt in kinds.items() if want is None or k in want}
    check(ctx.lib.gtx_op_georef_tracks(ctx.handle, C.byref(chain), C.byref(cfg), ptr(x), ptr(y), ptr(bbox), ptr(dims), ptr(frames), ptr(interp), n,
                                       ptr(order), ptr(seg), ptr(n_used), ptr(exp_off), ptr(quads), len(quads), ptr(weights), len(weights),
                                       *[ptr(out.get(k)) for k in kinds]))
    ms = np.zeros(_lib.GEOREF_TRACKS_MS, np.float32)
    check(ctx.lib.gtx_georef_tracks_ms(ptr(ms)))
    out["ms"] = ms
    return out


def clahe(gray: np.ndarray, ctx=None) -> np.ndarray:
    """cv2.createCLAHE(clipLimit=2.0, tileGridSize=(8, 8)).apply(gray) on the GPU (the stabilizer's `clahe: true` step)."""
    ctx = ctx or _lib.default_context()
    g = np.ascontiguousarray(gray, dtype=np.uint8)
    out = np.empty_like(g)
    check(ctx.lib.gtx_op_clahe(ctx.handle, ptr(g), g.shape[0], g.shape[1], ptr(out)))
    return out


def gray_resize(frame_bgr: np.ndarray, ratio: float, ctx=None) -> np.ndarray:
    """The ORB stabilizer's working-resolution gray image of a BGR frame (cv2.cvtColor(BGR2GRAY), then cv2.resize(fx = fy = ratio,
    INTER_LINEAR)) [gh, gw] u8, gh, gw = stabilizer.working_size: gtx_op_gray_resize, one launch of the kernel the stabilizer and the
    engine's "frame" route run."""
    from .stabilizer import working_size

    ctx = ctx or _lib.default_context()
    f = np.ascontiguousarray(frame_bgr, dtype=np.uint8)
    if f.ndim != 3 or f.shape[2] != 3:
        raise ValueError("frame_bgr is [h, w, 3] u8")
    h, w = f.shape[:2]
    gh, gw = working_size((h, w), ratio)
    out = np.empty((gh, gw), np.uint8)
    check(ctx.lib.gtx_op_gray_resize(ctx.handle, ptr(f), h, w, float(ratio), ptr(out), gh, gw))
    return out


CONV_FORMS = ("Staged", "Split", "K32", "K32S2")      # gtx_op_conv_config's *form


def conv_config(dtype: int, ksize: int, stride: int, cin: int, cout: int, force_kc: int = 0):
    """The kernel a convolution of this shape is given (host only; the GTX_K32 / GTX_K32S2 switches as every launch reads them).
    dtype: GTX_F16, GTX_F32 or GTX_F32S. -> (form, one of CONV_FORMS; cout tile; K chunk; kernel name)."""
    lib = _lib.load()
    form, bn, kc = C.c_int(-1), C.c_int(), C.c_int()
    name = C.create_string_buffer(128)
    check(lib.gtx_op_conv_config(int(dtype), ksize, stride, cin, cout, force_kc, C.byref(form), C.byref(bn), C.byref(kc), name, len(name)))
    return CONV_FORMS[form.value], bn.value, kc.value, name.value.decode()


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


# ---------------------------------------------------------------------------- RT-DETR's token-side kernels (gtx_op_rt_*)
def _f32(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float32)


def _map_fmt(a: np.ndarray, split: bool) -> int:
    if split and a.dtype != np.float32:
        raise TypeError("split=True needs float32 maps")
    return GTX_F32S if split else _dt(a)


def _levels(maps, coff, split):
    """Level maps [n, h, w, cstride] -> the hooks' per-level arrays. Returns (kept arrays, fmt, n, L, ptrs, h, w, cstride, coff)."""
    maps = [np.ascontiguousarray(m) for m in maps]
    L = len(maps)
    coff = [coff] * L if np.isscalar(coff) else list(coff)
    assert 1 <= L <= 3 and len(coff) == L and all(m.ndim == 4 and m.dtype == maps[0].dtype and m.shape[0] == maps[0].shape[0] for m in maps)
    ptrs = (C.c_void_p * L)(*[m.ctypes.data for m in maps])
    ints = lambda v: (C.c_int * L)(*[int(i) for i in v])
    return (maps, _map_fmt(maps[0], split), maps[0].shape[0], L, ptrs, ints(m.shape[1] for m in maps), ints(m.shape[2] for m in maps),
            ints(m.shape[3] for m in maps), ints(coff))


def rt_linear(x: np.ndarray, w: np.ndarray, bias=None, *, k: int | None = None, x2=None, x2_cols: int = 0, res=None, act: int = 0,
              y: np.ndarray | None = None, ycol: int = 0, ctx=None) -> np.ndarray:
    """y[:, ycol:ycol + Nout] = act(x[:, :K] (+ x2[:, :K] for the output columns [0, x2_cols)) @ w.T + bias) (+ res[:, :Nout]).
    x [M, ldx >= K], w [Nout, K], res [M, ldr >= Nout]; y (optional) [M, ldy]: a copy comes back with only that block written.
    act: 0 none, 2 ReLU, 3 GELU."""
    ctx = ctx or _lib.default_context()
    x, w, x2, res, b = _f32(x), _f32(w), _f32(x2), _f32(res), _f32(bias)
    nout, kk = w.shape
    k = kk if k is None else k
    assert k == kk and x.ndim == 2
    m = x.shape[0]
    y = np.zeros((m, nout), np.float32) if y is None else np.array(y, dtype=np.float32, order="C")
    assert y.shape[0] == m and (x2 is None or x2.shape[0] == m) and (res is None or res.shape[0] == m)
    check(ctx.lib.gtx_op_rt_linear(ctx.handle, m, k, nout, ptr(x), x.shape[1], ptr(x2), 0 if x2 is None else x2.shape[1], int(x2_cols), ptr(w), ptr(b),
                                   ptr(res), 0 if res is None else res.shape[1], ptr(y), y.shape[1], int(ycol), int(act)))
    return y


def rt_layernorm(x: np.ndarray, gamma, beta, *, c: int | None = None, in_coff: int = 0, in_split: bool = False, out: np.ndarray | None = None,
                 out_coff: int = 0, out_dtype=None, out_split: bool = False, ctx=None):
    """LayerNorm (eps 1e-5) of x[:, in_coff:in_coff + c] into out[:, out_coff:out_coff + c] (a copy of `out` otherwise). Formats
    are the arrays' dtypes; *_split=True (float32 arrays): the pair format on the device. Returns (out, saturated)."""
    ctx = ctx or _lib.default_context()
    x = np.ascontiguousarray(x)
    rows, cs = x.shape
    c = cs if c is None else c
    if out is None:
        out = np.zeros((rows, c), out_dtype or x.dtype)
    out = np.array(out, order="C")
    assert out.shape[0] == rows
    sat = C.c_int()
    check(ctx.lib.gtx_op_rt_layernorm(ctx.handle, rows, c, _map_fmt(x, in_split), ptr(x), cs, in_coff, _map_fmt(out, out_split), ptr(out), out.shape[1],
                                      out_coff, ptr(_f32(gamma)), ptr(_f32(beta)), C.byref(sat)))
    return out, bool(sat.value)


def rt_mha(qkv: np.ndarray, c: int, heads: int, *, out: np.ndarray | None = None, form: int = 0, ctx=None) -> np.ndarray:
    """Multi-head attention on token rows: qkv [n, T, ld >= 3 c] (q | k | v at columns 0, c, 2 c) -> out [n, T, ldo >= c] (a copy of
    `out` with columns [0, c) written). form: 0 the library's rule, 1 the generic kernel."""
    ctx = ctx or _lib.default_context()
    qkv = _f32(qkv)
    n, t, ld = qkv.shape
    out = np.zeros((n, t, c), np.float32) if out is None else np.array(out, dtype=np.float32, order="C")
    assert out.shape[:2] == (n, t)
    check(ctx.lib.gtx_op_rt_mha(ctx.handle, n, t, c, heads, ptr(qkv), ld, ptr(out), out.shape[2], form))
    return out


def rt_topk(scores, nc: int, nq: int, *, coff=0, ctx=None) -> np.ndarray:
    """Query selection over up to three score maps [n, h, w, cstride] (float32 or float16; classes at [coff, coff + nc)) -> idx [n, nq]."""
    ctx = ctx or _lib.default_context()
    keep, fmt, n, L, ptrs, h, w, cs, co = _levels(scores, coff, False)
    idx = np.full((n, nq), -1, np.int32)
    check(ctx.lib.gtx_op_rt_topk(ctx.handle, fmt, n, L, ptrs, h, w, cs, co, nc, nq, ptr(idx)))
    return idx


def rt_gather_refer(enc, c: int, idx: np.ndarray, delta: np.ndarray, *, coff=0, split: bool = False, ctx=None):
    """The selected anchors' rows, anchor logits and first reference boxes: enc = level maps [n, h, w, cstride], idx [n, nq],
    delta [n * nq, ldd >= 4] -> (embed [n * nq, c], anchors [n * nq, 4], refer [n * nq, 16])."""
    ctx = ctx or _lib.default_context()
    keep, fmt, n, L, ptrs, h, w, cs, co = _levels(enc, coff, split)
    idx = np.ascontiguousarray(idx, dtype=np.int32)
    delta = _f32(delta)
    nq = idx.shape[1]
    m = n * nq
    assert idx.shape[0] == n and delta.shape[0] == m
    embed, anchors, refer = np.zeros((m, c), np.float32), np.zeros((m, 4), np.float32), np.zeros((m, 16), np.float32)
    check(ctx.lib.gtx_op_rt_gather_refer(ctx.handle, fmt, n, L, ptrs, h, w, cs, co, c, nq, ptr(idx), ptr(delta), delta.shape[1], 0, ptr(embed),
                                         ptr(anchors), ptr(refer)))
    return embed, anchors, refer


def rt_refer_update(refer: np.ndarray, delta: np.ndarray, ctx=None) -> np.ndarray:
    """refer[:, :4] = sigmoid(delta[:, :4] + inverse_sigmoid(refer[:, :4])) (rt_refer mode 1); refer [M, 16] comes back as a copy."""
    ctx = ctx or _lib.default_context()
    refer = np.array(refer, dtype=np.float32, order="C")
    delta = _f32(delta)
    m = refer.shape[0]
    assert refer.shape == (m, 16) and delta.shape[0] == m
    check(ctx.lib.gtx_op_rt_gather_refer(ctx.handle, GTX_F32, 1, 0, None, None, None, None, None, 0, m, None, ptr(delta), delta.shape[1], 1, None, None,
                                         ptr(refer)))
    return refer


def rt_deform(value, hd: int, nh: int, npts: int, offaw: np.ndarray, refer: np.ndarray, *, coff=0, split: bool = False, ctx=None) -> np.ndarray:
    """Multi-scale deformable attention sampling: value = level maps [n, h, w, cstride] (hd channels from coff), offaw
    [n, nq, nh * L * npts * 3], refer [n, nq, 16] -> out [n, nq, hd]."""
    ctx = ctx or _lib.default_context()
    keep, fmt, n, L, ptrs, h, w, cs, co = _levels(value, coff, split)
    offaw, refer = _f32(offaw), _f32(refer)
    nq = offaw.shape[1]
    assert offaw.shape == (n, nq, nh * L * npts * 3) and refer.shape == (n, nq, 16)
    out = np.zeros((n, nq, hd), np.float32)
    check(ctx.lib.gtx_op_rt_deform(ctx.handle, fmt, n, L, ptrs, h, w, cs, co, hd, nh, npts, nq, ptr(offaw), ptr(refer), ptr(out)))
    return out


def rt_post(logits: np.ndarray, nc: int, refer: np.ndarray, conf: float, frame_wh, max_det: int, *, class_mask=(2**64 - 1, 2**64 - 1),
            out_rows: np.ndarray | None = None, want_raw: bool = True, ctx=None):
    """RT-DETR's score / box stage: logits [n, nq, ldl >= nc], refer [n, nq, 16] -> (rows [n, max_det, 6] -- a copy of `out_rows`
    with the first out_n rows of each image written --, out_n [n], raw [n, nq, 4 + nc] or None). class_mask: two 64-bit words."""
    ctx = ctx or _lib.default_context()
    logits, refer = _f32(logits), _f32(refer)
    n, nq, ldl = logits.shape
    assert refer.shape == (n, nq, 16)
    rows = np.zeros((n, max_det, 6), np.float32) if out_rows is None else np.array(out_rows, dtype=np.float32, order="C")
    assert rows.shape == (n, max_det, 6)
    out_n = np.full(n, -1, np.int32)
    raw = np.zeros((n, nq, 4 + nc), np.float32) if want_raw else None
    check(ctx.lib.gtx_op_rt_post(ctx.handle, n, nq, nc, ptr(logits), ldl, ptr(refer), float(conf), int(class_mask[0]), int(class_mask[1]),
                                 int(frame_wh[0]), int(frame_wh[1]), max_det, ptr(rows), ptr(out_n), ptr(raw)))
    return rows, out_n, raw


# ---------------------------------------------------------------------------- RT-DETR's map-side kernels (gtx_op_rt_*)
# Maps are [n_alloc, h, w, cstride] arrays whose channels [coff, coff + c) a launch reads or writes; the first n images run
# (default all). An output map is given as it is before the launch; a copy comes back with only the launch's slice written.
def _rt_map(a, split):
    a = np.array(a, order="C")
    assert a.ndim == 4
    return a, _map_fmt(a, split)


def rt_stem1(img: np.ndarray, w27: np.ndarray, bias: np.ndarray, out: np.ndarray, *, n: int | None = None, out_coff: int = 0, split: bool = False,
             ctx=None):
    """HGStem.stem1 on img [n_alloc, H, W, 4] RGB0 bytes: ReLU(conv 3x3 stride 2 of img / 255 + bias) into out[..., out_coff:out_coff + c0],
    out [n_alloc, H / 2, W / 2, cstride]; w27 [27, c0] with row (ky * 3 + kx) * 3 + colour. Returns (out, saturated)."""
    ctx = ctx or _lib.default_context()
    img = np.ascontiguousarray(img, dtype=np.uint8)
    w27, bias = _f32(w27), _f32(bias)
    na, h, w, four = img.shape
    c0 = w27.shape[1]
    out, fmt = _rt_map(out, split)
    assert four == 4 and w27.shape == (27, c0) and bias.shape == (c0,) and out.shape[:3] == (na, h // 2, w // 2)
    sat = C.c_int()
    check(ctx.lib.gtx_op_rt_stem1(ctx.handle, fmt, na if n is None else n, na, h, w, c0, ptr(img), ptr(w27), ptr(bias), ptr(out), out.shape[3],
                                  out_coff, C.byref(sat)))
    return out, bool(sat.value)


def rt_pool2(x: np.ndarray, c: int, out: np.ndarray, *, n: int | None = None, in_coff: int = 0, out_coff: int = 0, split: bool = False, ctx=None):
    """max_pool2d(F.pad(x, [0, 1, 0, 1]), 2, 1) of x[..., in_coff:in_coff + c] into out[..., out_coff:out_coff + c]. Returns (out, saturated)."""
    ctx = ctx or _lib.default_context()
    x, fmt = _rt_map(x, split)
    out, _ = _rt_map(out, split)
    na, h, w, cs = x.shape
    assert out.shape[:3] == (na, h, w) and out.dtype == x.dtype
    sat = C.c_int()
    check(ctx.lib.gtx_op_rt_pool2(ctx.handle, fmt, na if n is None else n, na, h, w, c, ptr(x), cs, in_coff, ptr(out), out.shape[3], out_coff,
                                  C.byref(sat)))
    return out, bool(sat.value)


def rt_dwconv(x: np.ndarray, w: np.ndarray, bias, out: np.ndarray, *, stride: int = 1, act: int = 0, residual: np.ndarray | None = None,
              n: int | None = None, in_coff: int = 0, out_coff: int = 0, res_coff: int = 0, split: bool = False, ctx=None):
    """dwconv() on channel slices: x[..., in_coff:in_coff + c] -> out[..., out_coff:out_coff + c], the residual read from
    residual[..., res_coff:res_coff + c]; w [c, 1, k, k], bias [c] or None. Returns (out, saturated)."""
    ctx = ctx or _lib.default_context()
    x, fmt = _rt_map(x, split)
    out, _ = _rt_map(out, split)
    na, h, wd, cs = x.shape
    c, k = int(w.shape[0]), int(w.shape[-1])
    wt = np.ascontiguousarray(np.asarray(w, np.float32).reshape(c, k * k).T)     # tap-major
    b = _f32(bias)
    r = None if residual is None else np.ascontiguousarray(residual, dtype=x.dtype)
    assert out.shape[:3] == (na, (h - 1) // stride + 1, (wd - 1) // stride + 1) and out.dtype == x.dtype and (r is None or r.shape[:3] == out.shape[:3])
    sat = C.c_int()
    check(ctx.lib.gtx_op_rt_dwconv(ctx.handle, fmt, na if n is None else n, na, h, wd, c, k, stride, ptr(x), cs, in_coff, ptr(wt), ptr(b), int(act),
                                   ptr(r), 0 if r is None else r.shape[3], res_coff, ptr(out), out.shape[3], out_coff, C.byref(sat)))
    return out, bool(sat.value)


def rt_upsample2x(x: np.ndarray, c: int, out: np.ndarray, *, n: int | None = None, in_coff: int = 0, out_coff: int = 0, split: bool = False,
                  ctx=None) -> np.ndarray:
    """Nearest 2x upsampling of x[..., in_coff:in_coff + c] into out[..., out_coff:out_coff + c] (RT-DETR's kernel: raw 8-channel groups)."""
    ctx = ctx or _lib.default_context()
    x, fmt = _rt_map(x, split)
    out, _ = _rt_map(out, split)
    na, h, w, cs = x.shape
    assert out.shape[:3] == (na, 2 * h, 2 * w) and out.dtype == x.dtype
    check(ctx.lib.gtx_op_rt_upsample2x(ctx.handle, fmt, na if n is None else n, na, h, w, c, ptr(x), cs, in_coff, ptr(out), out.shape[3], out_coff))
    return out


def rt_tokens_in(x: np.ndarray, c: int, pos, src: np.ndarray, q: np.ndarray | None = None, *, n: int | None = None, in_coff: int = 0,
                 split: bool = False, ctx=None):
    """Map -> token rows: src [n_alloc * h * w, c] = x[..., in_coff:in_coff + c] as float32 and, with pos [h * w, c] and q given,
    q = src + pos. src and q are given as they are before the launch. Returns (src, q or None)."""
    ctx = ctx or _lib.default_context()
    x, fmt = _rt_map(x, split)
    na, h, w, cs = x.shape
    src = np.array(src, dtype=np.float32, order="C")
    q = None if q is None else np.array(q, dtype=np.float32, order="C")
    pos = _f32(pos)
    assert src.shape == (na * h * w, c) and (q is None or q.shape == src.shape) and (pos is None or pos.shape == (h * w, c))
    check(ctx.lib.gtx_op_rt_tokens_in(ctx.handle, fmt, na if n is None else n, na, h, w, c, ptr(x), cs, in_coff, ptr(pos), ptr(src), ptr(q)))
    return src, q


def rt_mask_invalid(m: np.ndarray, c: int, level: int, *, n: int | None = None, coff: int = 0, split: bool = False, ctx=None) -> np.ndarray:
    """RTDETRDecoder._generate_anchors' valid_mask applied to m[..., coff:coff + c] of a level's map (a copy comes back)."""
    ctx = ctx or _lib.default_context()
    m, fmt = _rt_map(m, split)
    na, h, w, cs = m.shape
    check(ctx.lib.gtx_op_rt_mask_invalid(ctx.handle, fmt, na if n is None else n, na, h, w, c, ptr(m), cs, coff, int(level)))
    return m


# ---------------------------------------------------------------------------- the detector's post-pass kernels
def head_levels(levels):
    """Detect levels for the post-pass hooks. levels: dicts with feat [n, h, w, cstride] (float16 / float32), cb, cc, stride and, as
    the hook needs them, wb [cb, 64], bb [64], wc [nc, cc], bc [nc]. -> (kept arrays, dtype, n, L, gtx_head_level array)."""
    L = len(levels)
    arr = (_lib.HeadLevel * max(L, 1))()
    keep = []
    feat0 = np.ascontiguousarray(levels[0]["feat"])
    for i, lv in enumerate(levels):
        f = np.ascontiguousarray(lv["feat"])
        assert f.ndim == 4 and f.dtype == feat0.dtype and f.shape[0] == feat0.shape[0]
        w = {k: _f32(lv.get(k)) for k in ("wb", "bb", "wc", "bc")}
        keep += [f, w]
        adr = lambda a: None if a is None else a.ctypes.data
        arr[i] = _lib.HeadLevel(f.ctypes.data, f.shape[1], f.shape[2], f.shape[3], int(lv["cb"]), int(lv["cc"]), adr(w["wb"]), adr(w["bb"]), adr(w["wc"]),
                                adr(w["bc"]), float(lv.get("stride", 8.0)))
    return keep, _dt(feat0), feat0.shape[0], L, arr


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def head_gate(levels, nc: int, conf: float, cap: int, *, class_mask=(2**64 - 1, 2**64 - 1), lvl_cap: int = 0, ctx=None):
    """The score gate. -> dict: count [n] (the true number that passed), score / anchor / cls [n, cap] (unwritten entries: NaN / -1),
    lvl_count [n, 4] and lvl_list [n, 4, lvl_cap] when lvl_cap > 0."""
    ctx = ctx or _lib.default_context()
    keep, dt, n, L, arr = head_levels(levels)
    count = np.full(n, -1, np.int32)
    score, anchor, cls = np.zeros((n, cap), np.float32), np.zeros((n, cap), np.int32), np.zeros((n, cap), np.int32)
    lc = np.zeros((n, 4), np.int32) if lvl_cap else None
    ll = np.zeros((n, 4, lvl_cap), np.int32) if lvl_cap else None
    check(ctx.lib.gtx_op_head_gate(ctx.handle, dt, n, L, arr, nc, float(conf), int(class_mask[0]), int(class_mask[1]), cap, lvl_cap, ptr(count),
                                   ptr(score), ptr(anchor), ptr(cls), ptr(lc), ptr(ll)))
    return dict(count=count, score=score, anchor=anchor, cls=cls, lvl_count=lc, lvl_list=ll)


def head_boxes(levels, count, cand_anchor, ctx=None) -> np.ndarray:
    """DFL decode of the first min(count, cap) candidates per image: cand_anchor [n, cap] -> boxes [n, cap, 4] (xyxy, network pixels;
    NaN where nothing was decoded)."""
    ctx = ctx or _lib.default_context()
    keep, dt, n, L, arr = head_levels(levels)
    count, cand_anchor = _i32(count), _i32(cand_anchor)
    cap = cand_anchor.shape[1]
    assert count.shape == (n,) and cand_anchor.shape == (n, cap)
    box = np.zeros((n, cap, 4), np.float32)
    check(ctx.lib.gtx_op_head_boxes(ctx.handle, dt, n, L, arr, cap, ptr(count), ptr(cand_anchor), ptr(box)))
    return box


def head_boxes_r1(levels, count, cand_anchor, ctx=None) -> np.ndarray:
    """head_boxes for a Detect layer with reg_max = 1 (yolo26.yaml): the levels' wb are [cb, 4] and bb [4], the four signed distances
    in strides; boxes [n, cap, 4] = the cell centre -/+ them, times the stride (NaN where nothing was decoded)."""
    ctx = ctx or _lib.default_context()
    keep, dt, n, L, arr = head_levels(levels)
    count, cand_anchor = _i32(count), _i32(cand_anchor)
    cap = cand_anchor.shape[1]
    assert count.shape == (n,) and cand_anchor.shape == (n, cap)
    assert all(np.shape(lv["wb"]) == (int(lv["cb"]), 4) and np.shape(lv["bb"]) == (4,) for lv in levels)
    box = np.zeros((n, cap, 4), np.float32)
    check(ctx.lib.gtx_op_head_boxes_r1(ctx.handle, dt, n, L, arr, cap, ptr(count), ptr(cand_anchor), ptr(box)))
    return box


def sparse_levels(levels):
    """Detect levels for the sparse box hook. levels: dicts with feat [n, h, w, cstride] float32, coff, cin, w1 [c1out, 3, 3, cin], b1
    [c1out], w2 [64, 3, 3, 64], b2 [64], wb [64, 4 * reg_max], bb [4 * reg_max], stride. -> (kept arrays, n, L, gtx_sparse_level array)."""
    L = len(levels)
    arr = (_lib.SparseLevel * max(L, 1))()
    keep = []
    n = np.shape(levels[0]["feat"])[0]
    for i, lv in enumerate(levels):
        f = _f32(lv["feat"])
        w = {k: _f32(lv[k]) for k in ("w1", "b1", "w2", "b2", "wb", "bb")}
        cin = int(lv.get("cin", w["w1"].shape[3]))
        assert f.ndim == 4 and f.shape[0] == n and w["w1"].shape[1:] == (3, 3, cin) and w["b1"].shape == (w["w1"].shape[0],)
        assert w["w2"].shape == (64, 3, 3, 64) and w["b2"].shape == (64,) and w["wb"].shape[0] == 64 and w["bb"].shape == (w["wb"].shape[1],)
        keep += [f, w]
        arr[i] = _lib.SparseLevel(f.ctypes.data, f.shape[1], f.shape[2], f.shape[3], int(lv.get("coff", 0)), cin, w["w1"].shape[0], w["w1"].ctypes.data,
                                  w["b1"].ctypes.data, w["w2"].ctypes.data, w["b2"].ctypes.data, w["wb"].ctypes.data, w["bb"].ctypes.data,
                                  float(lv.get("stride", 8.0)))
    return keep, n, L, arr


def head_sparse_box(levels, count, cand_anchor, lvl_count, lvl_list, *, reg_max: int = 16, ctx=None):
    """The sparse Detect box launch (head_sparse.hip) on given candidates: cand_anchor [n, cap], lvl_count [n, 4], lvl_list
    [n, 4, lvl_cap] (entry indices filed by level). -> (boxes [n, cap, 4] xyxy in network pixels, NaN where no list names the entry;
    sat: 1 when a first-layer value a candidate reads left the fp16 range)."""
    ctx = ctx or _lib.default_context()
    keep, n, L, arr = sparse_levels(levels)
    count, cand_anchor, lvl_count, lvl_list = _i32(count), _i32(cand_anchor), _i32(lvl_count), _i32(lvl_list)
    cap, lvl_cap = cand_anchor.shape[1], lvl_list.shape[2]
    assert count.shape == (n,) and cand_anchor.shape == (n, cap) and lvl_count.shape == (n, 4) and lvl_list.shape == (n, 4, lvl_cap)
    assert all(np.shape(lv["wb"]) == (64, 4 * reg_max) for lv in levels)
    box = np.zeros((n, cap, 4), np.float32)
    sat = C.c_int(-1)
    check(ctx.lib.gtx_op_head_sparse_box(ctx.handle, n, L, arr, int(reg_max), cap, lvl_cap, ptr(count), ptr(cand_anchor), ptr(lvl_count), ptr(lvl_list),
                                         ptr(box), C.byref(sat)))
    return box, sat.value


def _rows_io(n, max_det, out_rows, out_n, out_anchor):
    rows = np.zeros((n, max_det, 6), np.float32) if out_rows is None else np.array(out_rows, dtype=np.float32, order="C")
    on = np.full(n, -1, np.int32) if out_n is None else np.array(out_n, dtype=np.int32, order="C")
    oa = np.full((n, max_det), -1, np.int32) if out_anchor is None else np.array(out_anchor, dtype=np.int32, order="C")
    assert rows.shape == (n, max_det, 6) and on.shape == (n,) and oa.shape == (n, max_det)
    return rows, on, oa


def nms(count, score, anchor, cls, box, *, iou_thr: float, max_det: int, src_hw, net_hw, gain: float, agnostic: bool = False, max_nms: int = 30000,
        nms_cap: int = 4160, which: int = 0, out_rows=None, out_n=None, out_anchor=None, ctx=None):
    """launch_nms on given candidates (count [n], score / anchor / cls [n, cap], box [n, cap, 4]). which: 0 both paths, 1 the
    single-workgroup kernel, 2 the general kernels. -> (rows [n, max_det, 6], out_n [n], out_anchor [n, max_det]): copies of what is
    given (zeros / -1 / -1 otherwise) with only what the kernels wrote changed."""
    ctx = ctx or _lib.default_context()
    count, score, anchor, cls, box = _i32(count), _f32(score), _i32(anchor), _i32(cls), _f32(box)
    n, cap = score.shape
    assert count.shape == (n,) and anchor.shape == (n, cap) and cls.shape == (n, cap) and box.shape == (n, cap, 4)
    rows, on, oa = _rows_io(n, max_det, out_rows, out_n, out_anchor)
    check(ctx.lib.gtx_op_nms(ctx.handle, n, cap, ptr(count), ptr(score), ptr(anchor), ptr(cls), ptr(box), float(iou_thr), int(agnostic), max_nms, nms_cap,
                             max_det, int(src_hw[0]), int(src_hw[1]), int(net_hw[0]), int(net_hw[1]), float(gain), which, ptr(rows), ptr(on), ptr(oa)))
    return rows, on, oa


def v10_select(levels, nc: int, conf: float, count, cand_score, cand_anchor, *, sel_cap: int = 304, lvl_cap: int = 0, ctx=None):
    """YOLOv10's two-stage top-300 cut over the gate's candidates. -> dict: count [n], score / anchor / cls [n, sel_cap], lvl_count /
    lvl_list when lvl_cap > 0, scores [n, 300, nc] (the kernel's scratch: one row per anchor stage 1 kept, NaN rows past them) and
    score_anchor [n, 300] (the anchor of each row, -1 past them)."""
    ctx = ctx or _lib.default_context()
    keep, dt, n, L, arr = head_levels(levels)
    count, cand_score, cand_anchor = _i32(count), _f32(cand_score), _i32(cand_anchor)
    cap = cand_score.shape[1]
    assert count.shape == (n,) and cand_score.shape == (n, cap) and cand_anchor.shape == (n, cap)
    sc = np.full(n, -1, np.int32)
    ss, sa, sk = np.zeros((n, sel_cap), np.float32), np.zeros((n, sel_cap), np.int32), np.zeros((n, sel_cap), np.int32)
    lc = np.zeros((n, 4), np.int32) if lvl_cap else None
    ll = np.zeros((n, 4, lvl_cap), np.int32) if lvl_cap else None
    scores = np.zeros((n, 300, nc), np.float32)
    score_anchor = np.zeros((n, 300), np.int32)
    check(ctx.lib.gtx_op_v10_select(ctx.handle, dt, n, L, arr, nc, float(conf), cap, ptr(count), ptr(cand_score), ptr(cand_anchor), sel_cap, lvl_cap,
                                    ptr(sc), ptr(ss), ptr(sa), ptr(sk), ptr(lc), ptr(ll), ptr(scores), ptr(score_anchor)))
    return dict(count=sc, score=ss, anchor=sa, cls=sk, lvl_count=lc, lvl_list=ll, scores=scores, score_anchor=score_anchor)


def v10_rows(sel_count, sel_score, sel_anchor, sel_cls, sel_box, *, max_det: int, src_hw, net_hw, gain: float, class_mask=(2**64 - 1, 2**64 - 1),
             out_rows=None, out_n=None, out_anchor=None, ctx=None):
    """The rows of given selected entries (sel_* [n, sel_cap], sel_box [n, sel_cap, 4]): class mask, max_det cut, scale_boxes + clip.
    -> (rows, out_n, out_anchor) as nms()."""
    ctx = ctx or _lib.default_context()
    sel_count, sel_score, sel_anchor, sel_cls, sel_box = _i32(sel_count), _f32(sel_score), _i32(sel_anchor), _i32(sel_cls), _f32(sel_box)
    n, cap = sel_score.shape
    assert sel_count.shape == (n,) and sel_anchor.shape == (n, cap) and sel_cls.shape == (n, cap) and sel_box.shape == (n, cap, 4)
    rows, on, oa = _rows_io(n, max_det, out_rows, out_n, out_anchor)
    check(ctx.lib.gtx_op_v10_rows(ctx.handle, n, cap, ptr(sel_count), ptr(sel_score), ptr(sel_anchor), ptr(sel_cls), ptr(sel_box), int(class_mask[0]),
                                  int(class_mask[1]), max_det, int(src_hw[0]), int(src_hw[1]), int(net_hw[0]), int(net_hw[1]), float(gain), ptr(rows), ptr(on),
                                  ptr(oa)))
    return rows, on, oa


def obj_feats(maps, c, dim: int, out_n, out_anchor, *, coff=0, split: bool = False, out=None, ctx=None) -> np.ndarray:
    """Appearance vectors: maps = level maps [n, h, w, cstride] (c[l] channels from coff[l]; split=True: float32 arrays in the pair
    format on the device), out_n [n], out_anchor [n, max_det] -> out [n, max_det, dim] (a copy of `out` with rows [0, out_n) written)."""
    ctx = ctx or _lib.default_context()
    maps = [np.ascontiguousarray(m) for m in maps]
    L = len(maps)
    coff = [coff] * L if np.isscalar(coff) else list(coff)
    c = [c] * L if np.isscalar(c) else list(c)
    assert len(coff) == L and len(c) == L and all(m.ndim == 4 and m.dtype == maps[0].dtype and m.shape[0] == maps[0].shape[0] for m in maps)
    n = maps[0].shape[0]
    out_n, out_anchor = _i32(out_n), _i32(out_anchor)
    max_det = out_anchor.shape[1]
    assert out_n.shape == (n,) and out_anchor.shape == (n, max_det)
    out = np.zeros((n, max_det, dim), np.float32) if out is None else np.array(out, dtype=np.float32, order="C")
    assert out.shape == (n, max_det, dim)
    ptrs = (C.c_void_p * max(L, 1))(*[m.ctypes.data for m in maps])
    ints = lambda v: (C.c_int * max(L, 1))(*[int(i) for i in v])
    check(ctx.lib.gtx_op_obj_feats(ctx.handle, _map_fmt(maps[0], split), n, L, ptrs, ints(m.shape[1] for m in maps), ints(m.shape[2] for m in maps),
                                   ints(m.shape[3] for m in maps), ints(coff), ints(c), dim, max_det, ptr(out_n), ptr(out_anchor), ptr(out)))
    return out


def orb_match(desc_q, desc_t, ratio: float, *, keep_all: bool = False, xy_q=None, xy_t=None, slots_q: int | None = None, slots_t: int | None = None,
              ctx=None):
    """One launch of the stabilizer's matcher: desc_q [nq, 32], desc_t [nt, 32] u8 (xy_* [n, 2] f32, zeros when not given); slots_*: the
    keypoint slots the grid covers (default: the counts). -> dict: best_idx / best_d / second_d [nq], and the compacted q / t / d [m],
    pts [m, 4] of the queries that pass the ratio test (keep_all: that have a neighbour)."""
    ctx = ctx or _lib.default_context()
    dq = np.ascontiguousarray(desc_q, dtype=np.uint8).reshape(-1, 32)
    dt = np.ascontiguousarray(desc_t, dtype=np.uint8).reshape(-1, 32)
    nq, nt = len(dq), len(dt)
    xq = np.zeros((nq, 2), np.float32) if xy_q is None else _f32(xy_q)
    xt = np.zeros((max(nt, 1), 2), np.float32) if xy_t is None else _f32(xy_t)
    assert xq.shape == (nq, 2) and (xy_t is None or xt.shape == (nt, 2))
    if nt == 0:
        dt = np.zeros((1, 32), np.uint8)
    bi, bd, sd, mq, mt, md = (np.zeros(nq, np.int32) for _ in range(6))
    mp = np.zeros((nq, 4), np.float32)
    m = C.c_int(-1)
    check(ctx.lib.gtx_op_orb_match(ctx.handle, ptr(dq), nq, nq if slots_q is None else slots_q, ptr(dt), nt, max(nt, 1) if slots_t is None else slots_t,
                                   float(ratio), int(keep_all), ptr(xq), ptr(xt), ptr(bi), ptr(bd), ptr(sd), ptr(mq), ptr(mt), ptr(md), ptr(mp),
                                   C.byref(m)))
    k = m.value
    return dict(best_idx=bi, best_d=bd, second_d=sd, q=mq[:k].copy(), t=mt[:k].copy(), d=md[:k].copy(), pts=mp[:k].copy(), n=k,
                tail=(mq[k:], mt[k:], md[k:]))


def orb_ransac(pts, seed: int, n_hyp: int, frame_wh, thr: float, *, affine: bool = False, ctx=None):
    """One launch of the stabilizer's RANSAC kernel on pts [n, 4] f32 = (x, y) -> (z, w), no refit. -> (winner index or -1, its integer
    MSAC cost in 1/1024 px^2, its H [3, 3] f64 as sampled: all zero when there is no winner)."""
    ctx = ctx or _lib.default_context()
    p = np.ascontiguousarray(pts, dtype=np.float32).reshape(-1, 4)
    best, cost, H = C.c_int(-2), C.c_int64(-1), np.full(9, np.nan, np.float64)
    check(ctx.lib.gtx_op_orb_ransac(ctx.handle, ptr(p) if len(p) else None, len(p), int(seed) & 0xFFFFFFFF, int(n_hyp), int(frame_wh[0]), int(frame_wh[1]),
                                    float(thr), int(affine), C.byref(best), C.byref(cost), ptr(H)))
    return best.value, cost.value, H.reshape(3, 3)


def homography_refit(pts, H0, frame_wh, thr: float, *, affine: bool = False):
    """The host refit that ends every robust homography (csrc/homography_refit.cpp; no device): pts [n, 4] f32 = (x, y) -> (z, w), H0
    [3, 3] f64 the RANSAC winner as sampled. -> (H [3, 3] f64 with h33 = 1, the pairs within thr of it), or (None, 0): no model."""
    p = np.ascontiguousarray(pts, dtype=np.float32).reshape(-1, 4)
    h0 = np.ascontiguousarray(H0, dtype=np.float64).reshape(9)
    H, valid, inl = np.full(9, np.nan, np.float64), C.c_int(-1), C.c_int(-1)
    check(_lib.load().gtx_op_homography_refit(ptr(p) if len(p) else None, len(p), int(frame_wh[0]), int(frame_wh[1]), float(thr), int(affine), ptr(h0),
                                              ptr(H), C.byref(valid), C.byref(inl)))
    return (H.reshape(3, 3), inl.value) if valid.value else (None, 0)


def gmc_corners(gray, *, ctx=None):
    """The sparse-optical-flow GMC's corner step (response + nms + select kernels, one launch each) on a gray image [h, w] u8.
    -> (corners [n, 2] f32 (x, y), n <= 1000, strongest first, equal responses by larger pixel index first;
    dict(found, stored, gathered, passes): the step's record, see gtx_gmc_counts)."""
    ctx = ctx or _lib.default_context()
    g = np.ascontiguousarray(gray, dtype=np.uint8)
    assert g.ndim == 2
    n, xy, c = C.c_int(-1), np.full((1000, 2), np.nan, np.float32), np.full(4, -1, np.int32)
    check(ctx.lib.gtx_op_gmc_corners(ctx.handle, ptr(g), g.shape[0], g.shape[1], 1000, C.byref(n), ptr(xy), ptr(c)))
    return xy[:n.value].copy(), dict(zip(("found", "stored", "gathered", "passes"), (int(v) for v in c)))


def gmc_lk(prev, cur, pts, *, ctx=None):
    """The GMC's pyramid reductions on both gray images [h, w] u8 and its Lucas-Kanade kernel on pts [n, 2] f32 (n <= 1000,
    fractional, anywhere inside the image). -> (next [n, 2] f32, status [n] bool)."""
    ctx = ctx or _lib.default_context()
    a, b = np.ascontiguousarray(prev, dtype=np.uint8), np.ascontiguousarray(cur, dtype=np.uint8)
    assert a.ndim == 2 and a.shape == b.shape
    p = np.ascontiguousarray(pts, dtype=np.float32).reshape(-1, 2)
    n = len(p)
    nxt, st = np.full((max(n, 1), 2), np.nan, np.float32), np.full(max(n, 1), -1, np.int32)
    check(ctx.lib.gtx_op_gmc_lk(ctx.handle, ptr(a), ptr(b), a.shape[0], a.shape[1], ptr(p) if n else None, n, ptr(nxt), ptr(st)))
    assert n == 0 or set(np.unique(st[:n])) <= {0, 1}
    return nxt[:n], st[:n].astype(bool)


def gmc_ransac(pairs, seed: int = 0, *, ctx=None):
    """The GMC's hypothesis kernel and its arg-max on pairs [n, 4] f32 = (p.x, p.y, q.x, q.y), n <= 1024, no refit.
    -> dict(best_count, winner, model [4] f64 = (a, b, tx, ty), count [512] int32)."""
    ctx = ctx or _lib.default_context()
    p = np.ascontiguousarray(pairs, dtype=np.float32).reshape(-1, 4)
    best, win, model, count = C.c_int(-2), C.c_int(-2), np.full(4, np.nan, np.float64), np.full(512, -2, np.int32)
    check(ctx.lib.gtx_op_gmc_ransac(ctx.handle, ptr(p) if len(p) else None, len(p), int(seed) & 0xFFFFFFFF, C.byref(best), C.byref(win), ptr(model), ptr(count)))
    return dict(best_count=best.value, winner=win.value, model=model, count=count)


# ---- GMC method ecc (csrc/ecc.hip): the prepare kernel, and the gradient kernel with one round of the fit's four launches
def ecc_prepare(frame_bgr, *, ctx=None):
    """cvtColor -> GaussianBlur(3x3, 1.5) -> resize(1/2) of a BGR u8 frame [H, W, 3] (H, W >= 8) -> [H // 2, W // 2] f32."""
    ctx = ctx or _lib.default_context()
    f = np.ascontiguousarray(frame_bgr, dtype=np.uint8)
    assert f.ndim == 3 and f.shape[2] == 3
    out = np.full((f.shape[0] // 2, f.shape[1] // 2), np.nan, np.float32)
    check(ctx.lib.gtx_op_ecc_prepare(ctx.handle, ptr(f), f.shape[0], f.shape[1], ptr(out)))
    return out


def ecc_iterate(tmpl, img, M, *, exact: bool = True, rho: float = -1.0, last_rho: float | None = None, eps: float = 1e-6, iter_in: int = 0,
                max_iters: int = 5000, status_in: int = 0, done_in: int = 0, ctx=None):
    """The gradient kernel on img, then exactly one round of stats, stats-finish, accum and update on template and image [h, w] f32
    from the state given (M [2, 3] f32; the defaults are the state a fit starts from). -> dict(gx, gy [h, w] f32; partial_stats,
    partial_accum [512, 13] f64: the partial-sum buffer after the stats kernel (columns 0..4 written, the rest still the 0xFF fill:
    NaN) and after the accum kernel; map [2, 3] f32, iter, status, done, rho, last_rho, n, img_norm, tmp_norm, img_mean, tmp_mean)."""
    ctx = ctx or _lib.default_context()
    t, i = np.ascontiguousarray(tmpl, dtype=np.float32), np.ascontiguousarray(img, dtype=np.float32)
    assert t.ndim == 2 and t.shape == i.shape
    m = np.ascontiguousarray(M, dtype=np.float32).reshape(6)
    h, w = t.shape
    gx, gy = np.full((h, w), np.nan, np.float32), np.full((h, w), np.nan, np.float32)
    ps, pa = np.zeros((512, 13), np.float64), np.zeros((512, 13), np.float64)
    mo, si, sd, me = np.full(6, np.nan, np.float32), np.full(3, -9, np.int32), np.full(5, np.nan, np.float64), np.full(2, np.nan, np.float32)
    check(ctx.lib.gtx_op_ecc_iterate(ctx.handle, ptr(t), ptr(i), h, w, ptr(m), int(bool(exact)), float(rho), float(-eps if last_rho is None else last_rho),
                                     float(eps), int(iter_in), int(max_iters), int(status_in), int(done_in), ptr(gx), ptr(gy), ptr(ps), ptr(pa), ptr(mo),
                                     ptr(si), ptr(sd), ptr(me)))
    return dict(gx=gx, gy=gy, partial_stats=ps, partial_accum=pa, map=mo.reshape(2, 3), iter=int(si[0]), status=int(si[1]), done=int(si[2]),
                rho=float(sd[0]), last_rho=float(sd[1]), n=float(sd[2]), img_norm=float(sd[3]), tmp_norm=float(sd[4]), img_mean=me[0], tmp_mean=me[1])


# ---- the SIFT kernels one stage at a time (csrc/sift.hip; record layouts: include/gtx.h)
_KEY = [("key_o", "<i4"), ("key_layer", "<i4"), ("key_r", "<i4"), ("key_c", "<i4")]
SIFT_REFINED = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("response", "<f4"), ("word", "<i4"), ("o", "<i4"), ("layer", "<i4"),
                         ("r", "<i4"), ("c", "<i4")] + _KEY)
SIFT_ORIENTED = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("word", "<i4"), ("o", "<i4"),
                          ("layer", "<i4")] + _KEY + [("bin", "<i4")])
SIFT_FINAL = np.dtype([("ori", "<f8"), ("px", "<f4"), ("py", "<f4"), ("scl", "<f4"), ("o", "<i4"), ("layer", "<i4"), ("pad", "<i4")])
assert SIFT_REFINED.itemsize == 52 and SIFT_ORIENTED.itemsize == 52 and SIFT_FINAL.itemsize == 32


def sift_blur(src, sigma: float, form: int = 0, *, dog: bool = True, ctx=None):
    """One Gaussian blur of the SIFT scale space on src [h, w] f32 -> (dst, dst - src or None). form 0: as the pyramid dispatches
    it, 1: the generic tile kernel, 2: the row / column / subtraction passes. A radius above 16 raises."""
    ctx = ctx or _lib.default_context()
    a = np.ascontiguousarray(src, dtype=np.float32)
    assert a.ndim == 2
    dst = np.full(a.shape, np.nan, np.float32)
    d = np.full(a.shape, np.nan, np.float32) if dog else None
    check(ctx.lib.gtx_op_sift_blur(ctx.handle, ptr(a), a.shape[0], a.shape[1], float(sigma), int(form), ptr(dst), ptr(d)))
    return dst, d


def sift_extrema(dog5, octave: int = 0, cap: int | None = None, *, ctx=None):
    """The three extrema passes over the five DoG layers [5, h, w] f32 of one octave -> (true count, stored candidates
    [min(count, cap), 4] i32 = (octave, layer, row, column), in no particular order). cap defaults to every interior pixel."""
    ctx = ctx or _lib.default_context()
    d = np.ascontiguousarray(dog5, dtype=np.float32)
    assert d.ndim == 3 and d.shape[0] == 5
    h, w = d.shape[1:]
    cap = max(1, 3 * h * w) if cap is None else int(cap)
    n, cand = C.c_int(-1), np.full((cap, 4), -1, np.int32)
    check(ctx.lib.gtx_op_sift_extrema(ctx.handle, ptr(d), h, w, int(octave), cap, C.byref(n), ptr(cand)))
    return n.value, cand[:min(n.value, cap)].copy()


def sift_refine(dog5, cand, octave: int = 0, *, ctx=None):
    """refine_kernel on candidates [n, 4] i32 of one octave -> the accepted records (SIFT_REFINED), in no particular order."""
    ctx = ctx or _lib.default_context()
    d = np.ascontiguousarray(dog5, dtype=np.float32)
    assert d.ndim == 3 and d.shape[0] == 5
    c = np.ascontiguousarray(cand, dtype=np.int32).reshape(-1, 4)
    n, out = C.c_int(-1), np.zeros(max(len(c), 1), SIFT_REFINED)
    check(ctx.lib.gtx_op_sift_refine(ctx.handle, ptr(d), d.shape[1], d.shape[2], int(octave), ptr(c) if len(c) else None, len(c), C.byref(n), ptr(out)))
    return out[:n.value].copy()


def sift_orient(gauss_layer, refined, octave: int = 0, cap: int | None = None, *, ctx=None):
    """orient_kernel on refined records (SIFT_REFINED) over one Gaussian layer [h, w] f32 -> (true count of peaks, the stored
    records (SIFT_ORIENTED) in no particular order, hist [n, 36] f32: the smoothed histogram of every input record)."""
    ctx = ctx or _lib.default_context()
    g = np.ascontiguousarray(gauss_layer, dtype=np.float32)
    assert g.ndim == 2
    r = np.ascontiguousarray(refined, dtype=SIFT_REFINED).reshape(-1)
    cap = max(1, 36 * len(r)) if cap is None else int(cap)
    n, out, hist = C.c_int(-1), np.zeros(cap, SIFT_ORIENTED), np.full((max(len(r), 1), 36), np.nan, np.float32)
    check(ctx.lib.gtx_op_sift_orient(ctx.handle, ptr(g), g.shape[0], g.shape[1], int(octave), ptr(r) if len(r) else None, len(r), cap, C.byref(n), ptr(out),
                                     ptr(hist)))
    return n.value, out[:min(n.value, cap)].copy(), hist[:len(r)]


def sift_describe(gauss_layer, px, py, ori, scl, *, root: bool = False, eps: float = 1e-8, ctx=None):
    """describe_kernel over one Gaussian layer [h, w] f32 for keypoints at octave-local (px, py) with orientation ori (degrees,
    360 - angle) and scale scl -> desc [n, 128] f32 (0..255 integers; RootSIFT rows when root)."""
    ctx = ctx or _lib.default_context()
    g = np.ascontiguousarray(gauss_layer, dtype=np.float32)
    assert g.ndim == 2
    f = np.zeros(len(np.atleast_1d(px)), SIFT_FINAL)
    f["px"], f["py"], f["ori"], f["scl"] = px, py, ori, scl
    desc = np.full((max(len(f), 1), 128), np.nan, np.float32)
    check(ctx.lib.gtx_op_sift_describe(ctx.handle, ptr(g), g.shape[0], g.shape[1], ptr(f) if len(f) else None, len(f), int(root), float(eps), ptr(desc)))
    return desc[:len(f)]


def sift_select(oriented, max_features: int, rects=None, *, ctx=None):
    """The selection / finalisation / mask launches of the stream-ordered extraction on oriented records (SIFT_ORIENTED, any
    order): the max_features strongest (response descending, equal responses by key ascending), in key order, minus those whose
    rounded working-resolution position lies in one of rects [m, 4] i32 (x1, y1, x2, y2, inclusive).
    -> dict(n, final (SIFT_FINAL), xy [n, 2], kp5 [n, 5], octave [n])."""
    ctx = ctx or _lib.default_context()
    o = np.ascontiguousarray(oriented, dtype=SIFT_ORIENTED).reshape(-1)
    r = np.zeros((0, 4), np.int32) if rects is None else np.ascontiguousarray(rects, dtype=np.int32).reshape(-1, 4)
    room = max(min(len(o), int(max_features)), 1)
    n = C.c_int(-1)
    fin, xy, kp5, octv = np.zeros(room, SIFT_FINAL), np.zeros((room, 2), np.float32), np.zeros((room, 5), np.float32), np.zeros(room, np.int32)
    check(ctx.lib.gtx_op_sift_select(ctx.handle, ptr(o) if len(o) else None, len(o), int(max_features), ptr(r) if len(r) else None, len(r), C.byref(n),
                                     ptr(fin), ptr(xy), ptr(kp5), ptr(octv)))
    k = n.value
    return dict(n=k, final=fin[:k].copy(), xy=xy[:k].copy(), kp5=kp5[:k].copy(), octave=octv[:k].copy())


# ---- the plot stage's trajectory maps (csrc/plot_draw.hip; the rule and the PlotCanvas class live in geotrax_amd/plot_draw.py)

def plot_draw(ctx, canvas, prims):
    """gtx_op_plot_draw: a host BGR canvas [h][w][3] with the strokes / discs of `prims` blended in (plot_draw.PRIM_DTYPE records)."""
    from . import plot_draw as PD

    return PD.draw_dev(ctx, canvas, prims)


def plot_reduce(ctx, image, k: int):
    """gtx_op_plot_reduce: the exact box average of a gray / RGB / RGBA u8 image by the integer factor k, as BGR."""
    from . import plot_draw as PD

    return PD.reduce_dev(ctx, image, k)
