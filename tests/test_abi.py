"""The C-ABI library loads without a GPU and exports every symbol include/gtx.h declares (and
nothing in the ctypes table is missing from the header); host-only entry points behave."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent


def _header_symbols():
    text = (ROOT / "include" / "gtx.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(gtx_[a-z0-9_]+)\s*\(", text))


def test_library_exports_every_declared_symbol():
    from geotrax_amd import _lib

    lib = _lib.load()
    declared = _header_symbols()
    assert len(declared) > 40
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} declared in include/gtx.h but not exported by libgtx.so"
    assert declared == set(_lib._SIGNATURES), declared ^ set(_lib._SIGNATURES)
    assert lib.gtx_abi_version() == _lib.ABI_VERSION == 14


def test_errors_are_codes_with_messages_not_exceptions():
    from geotrax_amd import _lib

    lib = _lib.load()
    assert lib.gtx_last_error() is not None
    out = np.zeros(4, np.float32)
    rc = lib.gtx_warp_boxes(None, None, 1, _lib.ptr(out))          # NULL matrix
    assert rc == -1 and b"NULL" in lib.gtx_last_error()
    h = C.c_void_p()
    cfg = _lib.TrackerConfig(type=7)
    rc = lib.gtx_tracker_create(C.byref(cfg), C.byref(h))
    assert rc < 0 and b"tracker type" in lib.gtx_last_error()
    with pytest.raises(_lib.GtxError):
        _lib.check(rc)


def test_rtdetr_hooks_refuse_bad_sizes_before_any_launch():
    """Host only: what a launcher's own checks would refuse comes back as an error code from the operator hooks (no context is
    even given), and more than 128 classes -- the class mask of the score stage has two 64-bit words -- never reaches a detector."""
    from geotrax_amd import _lib

    lib = _lib.load()
    f = np.zeros(4096, np.float32)
    i = np.zeros(64, np.int32)
    p = _lib.ptr
    full = 2**64 - 1
    assert lib.gtx_op_rt_post(None, 1, 4, 129, p(f), 132, p(f), 0.5, full, full, 64, 64, 4, p(f), p(i), None) == -1
    assert b"128 classes" in lib.gtx_last_error()
    assert lib.gtx_op_rt_post(None, 1, 513, 4, p(f), 4, p(f), 0.5, full, full, 64, 64, 4, p(f), p(i), None) == -1
    assert b"512 queries" in lib.gtx_last_error()
    assert lib.gtx_op_rt_post(None, 1, 4, 128, p(f), 128, p(f), 0.5, full, full, 64, 64, 4, p(f), p(i), None) == -1
    assert b"ctx is NULL" in lib.gtx_last_error()                                   # the sizes were fine
    assert lib.gtx_op_rt_linear(None, 4, 24, 16, p(f), 24, None, 0, 0, p(f), None, None, 0, p(f), 16, 0, 0) == -1      # K % 16
    assert b"rt_linear" in lib.gtx_last_error()
    assert lib.gtx_op_rt_linear(None, 4, 16, 128, p(f), 16, p(f), 16, 32, p(f), None, None, 0, p(f), 128, 0, 0) == -1  # x2_cols % 64
    assert lib.gtx_op_rt_linear(None, 4, 16, 16, p(f), 16, None, 0, 0, p(f), None, None, 0, p(f), 24, 16, 0) == -1     # past ldy
    assert lib.gtx_op_rt_layernorm(None, 2, 1032, 1, p(f), 1032, 0, 1, p(f), 1032, 0, p(f), p(f), None) == -1          # C > 1024
    assert lib.gtx_op_rt_layernorm(None, 2, 64, 2, p(f), 64, 0, 1, p(f), 64, 0, p(f), p(f), None) == -1                # F32S -> F32
    assert lib.gtx_op_rt_mha(None, 1, 4, 48, 4, p(f), 144, p(f), 48, 0) == -1                                          # head dimension 12
    assert lib.gtx_op_rt_mha(None, 1, 4, 32, 1, p(f), 96, p(f), 32, 2) == -1                                           # form
    maps = (C.c_void_p * 1)(f.ctypes.data)
    one = lambda v: (C.c_int * 1)(v)
    assert lib.gtx_op_rt_topk(None, 1, 1, 1, maps, one(3), one(4), one(4), one(0), 4, 13, p(i)) == -1                  # 13 queries of 12 anchors
    assert b"rt_topk" in lib.gtx_last_error()
    assert lib.gtx_op_rt_topk(None, 2, 1, 1, maps, one(3), one(4), one(4), one(0), 4, 4, p(i)) == -1                   # pair-format scores
    i[:4] = [0, 5, 12, 3]
    assert lib.gtx_op_rt_gather_refer(None, 1, 1, 1, maps, one(3), one(4), one(8), one(0), 8, 4, p(i), p(f), 4, 0, p(f), p(f), p(f)) == -1
    assert b"outside the level set" in lib.gtx_last_error()
    assert lib.gtx_op_rt_deform(None, 1, 1, 1, maps, one(3), one(4), one(8), one(0), 8, 3, 4, 2, p(f), p(f), p(f)) == -1   # hd % nh
    h = C.c_void_p()
    cfg = _lib.DetConfig(imgsz=640, conf=0.25, iou=0.7, max_det=300, nc=129, frame_h=64, frame_w=64, arch=1)
    assert lib.gtx_detector_create(None, C.byref(cfg), C.byref(h)) == -3 and b"128 classes" in lib.gtx_last_error() and not h.value
    cfg.arch = 0
    assert lib.gtx_detector_create(None, C.byref(cfg), C.byref(h)) == -3 and not h.value


def test_rtdetr_map_hooks_refuse_bad_sizes_before_any_launch():
    """Host only: the six map-side hooks answer NULL arrays, non-positive sizes, channel counts, strides and offsets that are not whole
    8-channel groups (16 for stem1), a slice that does not fit its stride, an odd image and a level outside 0..5 with an error code,
    with no context given."""
    from geotrax_amd import _lib

    lib = _lib.load()
    f = np.zeros(8192, np.float32)
    img = np.zeros(2 * 8 * 8 * 4, np.uint8)
    p = _lib.ptr
    sat = C.c_int()
    opt = lambda a: None if a is None else p(a)
    err = lib.gtx_last_error

    def stem1(dtype=1, n=1, na=1, H=8, W=8, c0=16, im=img, w27=f, b=f, out=f, cs=16, co=0):
        return lib.gtx_op_rt_stem1(None, dtype, n, na, H, W, c0, opt(im), opt(w27), opt(b), opt(out), cs, co, C.byref(sat))

    assert stem1() == -1 and b"ctx is NULL" in err()                                                    # the sizes were fine
    assert stem1(n=2, na=2, H=2, W=4, c0=48, cs=64, co=16) == -1 and b"ctx is NULL" in err()
    for c0 in (0, 8, 24, -16):
        assert stem1(c0=c0, cs=32) == -1 and b"multiple of 16" in err(), c0
    assert stem1(c0=1040, cs=1040) == -1 and b"1024 channels" in err()
    for H, W in ((7, 8), (8, 7), (0, 8), (8, -2)):
        assert stem1(H=H, W=W) == -1 and b"even" in err(), (H, W)
    assert stem1(n=0) == -1 and b"n_alloc" in err()
    assert stem1(n=2) == -1 and b"n_alloc" in err()                                                     # more images than the arrays hold
    assert stem1(cs=20) == -1 and b"multiples of 8" in err()
    assert stem1(cs=32, co=4) == -1 and b"multiples of 8" in err()
    assert stem1(cs=32, co=-8) == -1 and b"multiples of 8" in err()
    assert stem1(cs=24, co=16) == -1 and b"does not fit" in err()
    assert stem1(dtype=3) == -1 and b"dtype" in err()
    for name in ("im", "w27", "b", "out"):
        assert stem1(**{name: None}) == -1 and b"is NULL" in err(), name

    def pool2(dtype=1, n=1, na=1, h=3, w=5, c=8, x=f, ics=8, ico=0, out=f, ocs=8, oco=0):
        return lib.gtx_op_rt_pool2(None, dtype, n, na, h, w, c, opt(x), ics, ico, opt(out), ocs, oco, C.byref(sat))

    assert pool2() == -1 and b"ctx is NULL" in err()
    assert pool2(h=1, w=1, c=24, ics=40, ico=16, ocs=32, oco=8) == -1 and b"ctx is NULL" in err()
    for c in (0, 4, 12, -8):
        assert pool2(c=c, ics=16, ocs=16) == -1 and b"multiple of 8" in err(), c
    for h, w in ((0, 5), (3, 0), (-1, 5)):
        assert pool2(h=h, w=w) == -1 and b"h and w" in err()
    assert pool2(ics=12) == -1 and b"multiples of 8" in err()
    assert pool2(ocs=16, oco=4) == -1 and b"multiples of 8" in err()
    assert pool2(ics=16, ico=16) == -1 and b"does not fit" in err()
    assert pool2(ocs=16, oco=16) == -1 and b"does not fit" in err()
    assert pool2(n=0) == -1 and b"n_alloc" in err()
    assert pool2(dtype=-1) == -1 and b"dtype" in err()
    assert pool2(x=None) == -1 and b"in is NULL" in err()
    assert pool2(out=None) == -1 and b"out is NULL" in err()

    def dw(dtype=2, n=1, na=1, h=3, w=5, c=8, k=5, stride=1, x=f, ics=8, ico=0, wt=f, b=f, act=0, res=None, rcs=0, rco=0, out=f, ocs=8, oco=0):
        return lib.gtx_op_rt_dwconv(None, dtype, n, na, h, w, c, k, stride, opt(x), ics, ico, opt(wt), opt(b), act, opt(res), rcs, rco, opt(out), ocs, oco,
                                    C.byref(sat))

    assert dw() == -1 and b"ctx is NULL" in err()
    assert dw(b=None) == -1 and b"ctx is NULL" in err()                                                 # a layer without bias is a case
    assert dw(res=f, rcs=24, rco=16, ics=16, ico=8, ocs=16, oco=8, stride=2, k=7) == -1 and b"ctx is NULL" in err()
    for k in (1, 4, 9):
        assert dw(k=k) == -1 and b"3, 5 or 7" in err()
    for stride in (0, 3):
        assert dw(stride=stride) == -1 and b"stride" in err()
    assert dw(act=3) == -1 and b"act" in err()
    for c in (0, 20):
        assert dw(c=c, ics=24, ocs=24) == -1 and b"multiple of 8" in err()
    assert dw(h=0) == -1 and b"h and w" in err()
    assert dw(ics=16, ico=12) == -1 and b"multiples of 8" in err()
    assert dw(ocs=16, oco=16) == -1 and b"does not fit" in err()
    assert dw(res=f, rcs=8, rco=8) == -1 and b"does not fit" in err()
    assert dw(res=f, rcs=12, rco=0) == -1 and b"multiples of 8" in err()
    assert dw(res=f, rcs=0, rco=0) == -1 and b"multiples of 8" in err()
    assert dw(n=3, na=2) == -1 and b"n_alloc" in err()
    for name in ("x", "wt", "out"):
        assert dw(**{name: None}) == -1 and b"is NULL" in err(), name

    def up(dtype=0, n=1, na=1, h=3, w=5, c=8, x=f, ics=8, ico=0, y=f, ocs=8, oco=0):
        return lib.gtx_op_rt_upsample2x(None, dtype, n, na, h, w, c, opt(x), ics, ico, opt(y), ocs, oco)

    assert up() == -1 and b"ctx is NULL" in err()
    assert up(c=4) == -1 and b"multiple of 8" in err()
    assert up(w=0) == -1 and b"h and w" in err()
    assert up(ics=10) == -1 and b"multiples of 8" in err()
    assert up(ocs=24, oco=20) == -1 and b"multiples of 8" in err()
    assert up(ocs=24, oco=24) == -1 and b"does not fit" in err()
    assert up(n=-1) == -1 and b"n_alloc" in err()
    assert up(x=None) == -1 and b"x is NULL" in err()
    assert up(y=None) == -1 and b"y is NULL" in err()

    def tok(dtype=1, n=1, na=1, h=3, w=5, c=8, x=f, ics=8, ico=0, pos=f, src=f, q=f):
        return lib.gtx_op_rt_tokens_in(None, dtype, n, na, h, w, c, opt(x), ics, ico, opt(pos), opt(src), opt(q))

    assert tok() == -1 and b"ctx is NULL" in err()
    assert tok(pos=None, q=None) == -1 and b"ctx is NULL" in err()                                      # src alone
    assert tok(pos=None) == -1 and b"together" in err()
    assert tok(q=None) == -1 and b"together" in err()
    assert tok(c=12, ics=16) == -1 and b"multiple of 8" in err()
    assert tok(h=0) == -1 and b"h and w" in err()
    assert tok(ics=16, ico=4) == -1 and b"multiples of 8" in err()
    assert tok(ics=16, ico=16) == -1 and b"does not fit" in err()
    assert tok(x=None) == -1 and b"in is NULL" in err()
    assert tok(src=None) == -1 and b"src is NULL" in err()

    def mask(dtype=1, n=1, na=1, h=3, w=5, c=8, m=f, cs=8, co=0, level=0):
        return lib.gtx_op_rt_mask_invalid(None, dtype, n, na, h, w, c, opt(m), cs, co, level)

    assert mask() == -1 and b"ctx is NULL" in err()
    assert mask(level=5) == -1 and b"ctx is NULL" in err()
    for level in (-1, 6, 31):
        assert mask(level=level) == -1 and b"level" in err()
    assert mask(c=4) == -1 and b"multiple of 8" in err()
    assert mask(w=-3) == -1 and b"h and w" in err()
    assert mask(cs=12) == -1 and b"multiples of 8" in err()
    assert mask(cs=16, co=16) == -1 and b"does not fit" in err()
    assert mask(n=0) == -1 and b"n_alloc" in err()
    assert mask(m=None) == -1 and b"m is NULL" in err()


def test_front_hooks_refuse_null_arguments_and_bad_sizes_before_any_launch():
    """Host only: gtx_op_stem and gtx_op_conv2d_fused check their arrays and the sizes they allocate by before they touch a context."""
    from geotrax_amd import _lib

    lib = _lib.load()
    f = np.zeros(4096, np.float32)
    img = np.zeros(4 * 8 * 8, np.uint8)
    p = _lib.ptr
    stem = lambda dtype, n, h, w, c0, im=img, w27=f, b=f, out=f: lib.gtx_op_stem(None, dtype, 1, n, h, w, c0, p(im) if im is not None else None,
                                                                               p(w27) if w27 is not None else None, p(b) if b is not None else None,
                                                                               p(out) if out is not None else None)
    for c0 in (0, 8, 24, 112, 128):
        assert stem(2, 1, 8, 8, c0) == -1 and b"c0 must be 16, 32, 48, 64, 80 or 96" in lib.gtx_last_error()
    assert stem(3, 1, 8, 8, 32) == -1 and b"dtype" in lib.gtx_last_error()
    for n, h, w in ((0, 8, 8), (1, 0, 8), (1, 8, 0), (1, -2, 8)):
        assert stem(2, n, h, w, 32) == -1 and b"at least 1" in lib.gtx_last_error()
    assert stem(2, 1, 8, 8, 32) == -1 and b"ctx is NULL" in lib.gtx_last_error()              # the sizes were fine

    d = _lib.ConvDesc(dtype=2, n=1, h=8, w=8, cin=32, cout=64, ksize=3, stride=2, act=1, in_cstride=32, in_coff=0, out_cstride=64, out_coff=0)
    fused = lambda ex, x=f, w=f, y=f, res=None, desc=d: lib.gtx_op_conv2d_fused(None, C.byref(desc) if desc is not None else None,
                                                                                C.byref(ex) if ex is not None else None, p(x) if x is not None else None,
                                                                                p(w) if w is not None else None, None, p(res) if res is not None else None,
                                                                                p(y) if y is not None else None)
    assert fused(_lib.ConvFused(), desc=None) == -1 and b"desc is NULL" in lib.gtx_last_error()
    assert fused(None) == -1 and b"fused is NULL" in lib.gtx_last_error()
    assert fused(_lib.ConvFused(), w=None) == -1 and b"w is NULL" in lib.gtx_last_error()
    assert fused(_lib.ConvFused(), y=None) == -1 and b"y is NULL" in lib.gtx_last_error()
    assert fused(_lib.ConvFused(), x=None) == -1 and b"x is NULL" in lib.gtx_last_error()     # only a front stage does without x
    dr = _lib.ConvDesc(dtype=2, n=1, h=8, w=8, cin=32, cout=64, ksize=3, stride=2, act=1, in_cstride=32, in_coff=0, out_cstride=64, out_coff=0,
                       has_residual=1)
    assert fused(_lib.ConvFused(), desc=dr) == -1 and b"residual is NULL" in lib.gtx_last_error()
    a = f.ctypes.data
    front = dict(front_img=img.ctypes.data, front_w27=a, front_bias=a, front_h=16, front_w_px=16)
    assert fused(_lib.ConvFused(**{**front, "front_w27": None}), x=None) == -1 and b"front_w27 is NULL" in lib.gtx_last_error()
    assert fused(_lib.ConvFused(**{**front, "front_bias": None}), x=None) == -1 and b"front_bias is NULL" in lib.gtx_last_error()
    assert fused(_lib.ConvFused(**{**front, "front_h": 0}), x=None) == -1 and b"front stage: bad sizes" in lib.gtx_last_error()
    assert fused(_lib.ConvFused(**{**front, "front_w_px": -4}), x=None) == -1 and b"front stage: bad sizes" in lib.gtx_last_error()
    assert fused(_lib.ConvFused(**front), x=None) == -1 and b"ctx is NULL" in lib.gtx_last_error()     # x may be NULL here
    for bad in (dict(in2_cstride=64, in2_coff=0, c_split=0), dict(in2_cstride=64, in2_coff=48, c_split=32), dict(in2_cstride=64, in2_coff=-8, c_split=32),
                dict(in2_cstride=68, in2_coff=0, c_split=32), dict(in2_cstride=64, in2_coff=4, c_split=32)):
        assert fused(_lib.ConvFused(x2=a, **bad)) == -1 and b"second source" in lib.gtx_last_error(), bad
    d1 = _lib.ConvDesc(dtype=2, n=1, h=1, w=8, cin=64, cout=64, ksize=1, stride=1, act=1, in_cstride=64, in_coff=0, out_cstride=64, out_coff=0)
    assert fused(_lib.ConvFused(x2=a, in2_cstride=64, in2_coff=0, c_split=32), desc=d1) == -1 and b"at least 2 x 2" in lib.gtx_last_error()
    assert fused(_lib.ConvFused(force_kc=-16)) == -1 and b"force_kc" in lib.gtx_last_error()
    assert fused(_lib.ConvFused(members=9)) == -1 and b"members" in lib.gtx_last_error()
    assert fused(_lib.ConvFused()) == -1 and b"ctx is NULL" in lib.gtx_last_error()                    # nothing asked for: gtx_op_conv2d
    # the residual as a channel slice: it needs a residual, fits its stride, and starts on 4 elements (whole 8-channel groups in the pair format)
    assert fused(_lib.ConvFused(res_cstride=192, res_coff=64)) == -1 and b"residual slice" in lib.gtx_last_error()
    for bad in (dict(res_cstride=0, res_coff=8), dict(res_cstride=-64), dict(res_cstride=64, res_coff=-8)):
        assert fused(_lib.ConvFused(**bad), res=f, desc=dr) == -1 and b"residual slice" in lib.gtx_last_error(), bad
    for bad in (dict(res_cstride=64, res_coff=8), dict(res_cstride=32, res_coff=0), dict(res_cstride=196, res_coff=64), dict(res_cstride=192, res_coff=4)):
        assert fused(_lib.ConvFused(**bad), res=f, desc=dr) == -1 and b"does not fit its stride" in lib.gtx_last_error(), bad
    assert fused(_lib.ConvFused(res_cstride=192, res_coff=64), res=f, desc=dr) == -1 and b"ctx is NULL" in lib.gtx_last_error()
    d16 = _lib.ConvDesc(dtype=0, n=1, h=8, w=8, cin=32, cout=64, ksize=3, stride=2, act=1, in_cstride=32, in_coff=0, out_cstride=64, out_coff=0, has_residual=1)
    assert fused(_lib.ConvFused(res_cstride=72, res_coff=4), res=f, desc=d16) == -1 and b"ctx is NULL" in lib.gtx_last_error()   # fp16: 4 elements do
    assert fused(_lib.ConvFused(res_cstride=72, res_coff=2), res=f, desc=d16) == -1 and b"does not fit its stride" in lib.gtx_last_error()
    # in place: one array behind x, residual and y, a plain stride-1 launch, one stride, input and residual clear of the output's channels
    ip = lambda res=0, **kw: _lib.ConvDesc(**{**dict(dtype=2, n=1, h=8, w=8, cin=32, cout=32, ksize=3, stride=1, act=0, in_cstride=96, in_coff=0,
                                                     out_cstride=96, out_coff=64, has_residual=res), **kw})
    slice1 = dict(in_place=1, res_cstride=96, res_coff=32)
    assert fused(_lib.ConvFused(in_place=1), desc=ip()) == -1 and b"ctx is NULL" in lib.gtx_last_error()
    assert fused(_lib.ConvFused(**slice1), res=f, desc=ip(1)) == -1 and b"ctx is NULL" in lib.gtx_last_error()
    assert fused(_lib.ConvFused(in_place=1), desc=ip(stride=2)) == -1 and b"in_place: a plain stride-1 launch" in lib.gtx_last_error()
    assert fused(_lib.ConvFused(in_place=2), desc=ip()) == -1 and b"in_place: a plain stride-1 launch" in lib.gtx_last_error()
    assert fused(_lib.ConvFused(in_place=1, out_plain=1), desc=ip()) == -1 and b"in_place: a plain stride-1 launch" in lib.gtx_last_error()
    assert fused(_lib.ConvFused(in_place=1), y=img, desc=ip()) == -1 and b"same array" in lib.gtx_last_error()
    assert fused(_lib.ConvFused(**slice1), res=img, desc=ip(1)) == -1 and b"same array" in lib.gtx_last_error()
    assert fused(_lib.ConvFused(in_place=1), desc=ip(out_cstride=128)) == -1 and b"one channel stride" in lib.gtx_last_error()
    assert fused(_lib.ConvFused(in_place=1), res=f, desc=ip(1)) == -1 and b"one channel stride" in lib.gtx_last_error()      # a [..][cout] residual
    for bad in (dict(in_coff=32, cin=64), dict(in_coff=64), dict(out_coff=24), dict(out_coff=0)):
        assert fused(_lib.ConvFused(in_place=1), desc=ip(**bad)) == -1 and b"must not overlap" in lib.gtx_last_error(), bad
    assert fused(_lib.ConvFused(in_place=1, res_cstride=96, res_coff=40), res=f, desc=ip(1)) == -1 and b"must not overlap" in lib.gtx_last_error()


def test_conv_config_hook_is_host_only_and_refuses_bad_arguments():
    """Host only: gtx_op_conv_config takes no context; it answers a class with its kernel's name, and NULL outputs, a dtype or sizes out
    of range and a shape no kernel takes with an error code."""
    from geotrax_amd import _lib

    lib = _lib.load()
    form, bn, kc = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    name = C.create_string_buffer(96)
    cfg = lambda dtype=2, ks=3, stride=1, cin=48, cout=64, force_kc=0, fo=form, nm=name, cap=96: lib.gtx_op_conv_config(
        dtype, ks, stride, cin, cout, force_kc, C.byref(fo) if fo is not None else None, C.byref(bn), C.byref(kc), nm, cap)
    assert cfg() == 0 and (form.value, bn.value, kc.value) == (1, 64, 16) and name.value == b"conv_igemm_split_kernel<3, 1, 2, 2, 1>"
    assert cfg(dtype=0, ks=1, cin=64) == 0 and (form.value, bn.value, kc.value) == (0, 64, 64) and name.value == b"conv_igemm_kernel<_Float16, 1, 1, 2, 8>"
    assert cfg(nm=None, cap=0) == 0
    assert cfg(cap=8) == 0 and name.value == b"conv_ig"                                                 # cut, and terminated
    assert cfg(fo=None) == -1 and b"form is NULL" in lib.gtx_last_error()
    assert cfg(dtype=3) == -1 and b"dtype" in lib.gtx_last_error()
    assert cfg(cin=0) == -1 and cfg(cout=-16) == -1 and cfg(force_kc=-1) == -1 and cfg(cap=0) == -1
    assert cfg(ks=5) < 0 and b"unsupported kernel" in lib.gtx_last_error()
    assert cfg(ks=1, stride=2) < 0 and b"unsupported kernel" in lib.gtx_last_error()
    assert cfg(cin=24) < 0 and b"K chunk" in lib.gtx_last_error()
    assert cfg(cout=24) < 0 and b"multiple of 16" in lib.gtx_last_error()


def test_head_hooks_refuse_bad_sizes_before_any_launch():
    """Host only: what the post-pass launchers would refuse, or their kernels would mishandle in silence, comes back as an error code
    from the operator hooks with no context given."""
    from geotrax_amd import _lib

    lib = _lib.load()
    f = np.zeros(8192, np.float32)
    i = np.zeros(4096, np.int32)
    p = _lib.ptr
    full = 2**64 - 1

    def levels(n_levels=1, h=2, w=2, cstride=32, cb=16, cc=16, cbs=None):
        arr = (_lib.HeadLevel * n_levels)()
        for l in range(n_levels):
            arr[l] = _lib.HeadLevel(f.ctypes.data, h, w, cstride, cb if cbs is None else cbs[l], cc, f.ctypes.data, f.ctypes.data, f.ctypes.data,
                                    f.ctypes.data, 8.0)
        return arr

    def gate(lv, n_levels=1, dtype=1, nc=4):
        return lib.gtx_op_head_gate(None, dtype, 1, n_levels, lv, nc, 0.25, full, full, 16, 0, p(i), p(f), p(i), p(i), None, None)

    assert gate(levels()) == -1 and b"ctx is NULL" in lib.gtx_last_error()                                # the sizes were fine
    assert gate(levels(cc=12)) == -1 and b"multiple of 8" in lib.gtx_last_error()                         # cc >> 3 chunks would drop channels
    assert gate(levels(cb=2, cstride=36)) == -1 and b"16-byte" in lib.gtx_last_error()                    # cb breaks load8's alignment (fp32)
    assert gate(levels(cb=4, cstride=36), dtype=0) == -1 and b"16-byte" in lib.gtx_last_error()           # fine in fp32, not in fp16
    assert gate(levels(cb=4, cstride=36)) == -1 and b"ctx is NULL" in lib.gtx_last_error()
    assert gate(levels(cstride=34)) == -1 and b"16-byte" in lib.gtx_last_error()                          # cstride does
    assert gate(levels(), nc=0) == -1 and b"128 classes" in lib.gtx_last_error()
    assert gate(levels(), nc=129) == -1 and b"128 classes" in lib.gtx_last_error()
    assert gate(levels(5), n_levels=5) == -1 and b"4 levels" in lib.gtx_last_error()
    assert gate(levels(cstride=24)) == -1 and b"do not fit" in lib.gtx_last_error()                       # cb + cc > cstride

    def boxes(lv, n_levels=1, anchor=0):
        i[:] = 0
        i[0] = 1                                                                                          # count = 1
        a = np.full(16, anchor, np.int32)
        return lib.gtx_op_head_boxes(None, 1, 1, n_levels, lv, 16, p(i), p(a), p(f))

    assert boxes(levels()) == -1 and b"ctx is NULL" in lib.gtx_last_error()
    assert boxes(levels(2, cstride=64, cbs=[16, 32]), 2) == -1 and b"level 0" in lib.gtx_last_error()                  # the LDS slices would overlap
    assert boxes(levels(cb=136, cstride=160)) == -1 and b"128 box channels" in lib.gtx_last_error()
    assert boxes(levels(), anchor=4) == -1 and b"outside the level set" in lib.gtx_last_error()           # 2 x 2 anchors

    def sparse(n_levels=1, h=2, w=2, cstride=40, coff=8, cin=32, c1out=64, reg_max=16, cap=16, lvl_cap=4, lvl_count=1, entry=0, anchor=0):
        arr = (_lib.SparseLevel * n_levels)()
        for l in range(n_levels):
            arr[l] = _lib.SparseLevel(f.ctypes.data, h, w, cstride, coff, cin, c1out, *([f.ctypes.data] * 6), 8.0)
        c = np.array([1], np.int32)
        a = np.full(cap if cap > 0 else 1, anchor, np.int32)
        lc = np.zeros((1, 4), np.int32)
        lc[0, :min(n_levels, 4)] = lvl_count
        ll = np.full((1, 4, max(lvl_cap, 1)), entry, np.int32)
        sat = C.c_int(0)
        return lib.gtx_op_head_sparse_box(None, 1, n_levels, arr, reg_max, cap, lvl_cap, p(c), p(a), p(lc), p(ll), p(f), C.byref(sat))

    assert sparse() == -1 and b"ctx is NULL" in lib.gtx_last_error()                                      # the sizes were fine
    assert sparse(cin=96, cstride=104) == -1 and b"ctx is NULL" in lib.gtx_last_error()
    assert sparse(lvl_count=9) == -1 and b"ctx is NULL" in lib.gtx_last_error()                           # lvl_count > lvl_cap: the kernel clamps
    assert sparse(cin=48, cstride=56) == -1 and b"multiple of 32" in lib.gtx_last_error()                 # the K chunk would run past the slice
    assert sparse(cin=16) == -1 and b"multiple of 32" in lib.gtx_last_error()
    assert sparse(cin=0) == -1 and b"multiple of 32" in lib.gtx_last_error()
    assert sparse(coff=4) == -1 and b"coff" in lib.gtx_last_error()                                       # half a pair-format group
    assert sparse(coff=-8) == -1 and b"coff" in lib.gtx_last_error()
    assert sparse(coff=16) == -1 and b"do not fit" in lib.gtx_last_error()                                # coff + cin > cstride
    assert sparse(cstride=44) == -1 and b"cstride" in lib.gtx_last_error()
    assert sparse(5) == -1 and b"4 levels" in lib.gtx_last_error()
    assert sparse(lvl_cap=0) == -1 and b"lvl_cap" in lib.gtx_last_error()
    assert sparse(lvl_count=-1) == -1 and b"negative lvl_count" in lib.gtx_last_error()
    assert sparse(entry=16) == -1 and b"outside [0, cap)" in lib.gtx_last_error()
    assert sparse(entry=-1) == -1 and b"outside [0, cap)" in lib.gtx_last_error()
    assert sparse(lvl_count=2, entry=16) == -1 and b"outside [0, cap)" in lib.gtx_last_error()
    assert sparse(lvl_count=0, entry=16) == -1 and b"ctx is NULL" in lib.gtx_last_error()                 # past the count: never followed
    assert sparse(anchor=4) == -1 and b"not inside the level" in lib.gtx_last_error()                     # 2 x 2 anchors
    assert sparse(anchor=-1) == -1 and b"not inside the level" in lib.gtx_last_error()
    assert sparse(2, anchor=0) == -1 and b"not inside the level" in lib.gtx_last_error()                  # level 1's list names an anchor of level 0
    assert sparse(c1out=96) == -1 and b"c1out" in lib.gtx_last_error()
    assert sparse(c1out=0) == -1 and b"c1out" in lib.gtx_last_error()
    assert sparse(reg_max=8) == -1 and b"reg_max" in lib.gtx_last_error()
    assert sparse(cap=0) == -1 and b"cap >= 1" in lib.gtx_last_error()
    assert sparse(cap=2**22 + 1) == -1 and b"cap >= 1" in lib.gtx_last_error()
    assert sparse(h=0) == -1 and b"a level's map" in lib.gtx_last_error()
    assert sparse(cstride=2**16 + 8, cin=32) == -1 and b"a level's map" in lib.gtx_last_error()
    assert sparse(h=2100, w=2100) == -1 and b"too many anchors" in lib.gtx_last_error()                   # > 2^22 (the check reads no array)

    def nms(anchor=0, nms_cap=64, which=0, score=0.5, count=1, max_det=4):
        c = np.array([count], np.int32)
        s = np.full(16, score, np.float32)
        a = np.full(16, anchor, np.int32)
        return lib.gtx_op_nms(None, 1, 16, p(c), p(s), p(a), p(i), p(f), 0.5, 0, 30000, nms_cap, max_det, 64, 64, 64, 64, 1.0, which, p(f), p(i), p(i))

    assert nms() == -1 and b"ctx is NULL" in lib.gtx_last_error()
    assert nms(anchor=2**20 - 1) == -1 and b"ctx is NULL" in lib.gtx_last_error()                         # the sort key's 20 anchor bits
    assert nms(anchor=2**20) == -1 and b"outside the level set" in lib.gtx_last_error()
    assert nms(nms_cap=100) == -1 and b"nms_cap" in lib.gtx_last_error()
    assert nms(nms_cap=32832) == -1 and b"nms_cap" in lib.gtx_last_error()
    assert nms(which=3) == -1 and b"which" in lib.gtx_last_error()
    assert nms(score=0.0) == -1 and b"positive" in lib.gtx_last_error()
    assert nms(count=-1) == -1 and b"negative count" in lib.gtx_last_error()
    assert nms(max_det=0) == -1

    def select(sel_cap=304, lvl_cap=0, anchor=0):
        c = np.array([1], np.int32)
        s = np.full(16, 0.5, np.float32)
        a = np.full(16, anchor, np.int32)
        return lib.gtx_op_v10_select(None, 1, 1, 1, levels(), 4, 0.25, 16, p(c), p(s), p(a), sel_cap, lvl_cap, p(i), p(f), p(i), p(i), p(i), p(i), p(f), p(i))

    assert select() == -1 and b"ctx is NULL" in lib.gtx_last_error()
    assert select(sel_cap=299) == -1 and b"sel_cap" in lib.gtx_last_error()
    assert select(sel_cap=513) == -1 and b"sel_cap" in lib.gtx_last_error()
    assert select(lvl_cap=299) == -1 and b"lvl_cap" in lib.gtx_last_error()
    assert select(anchor=4) == -1 and b"outside the level set" in lib.gtx_last_error()
    assert lib.gtx_op_v10_rows(None, 1, 513, p(i), p(f), p(i), p(i), p(f), full, full, 4, 64, 64, 64, 64, 1.0, p(f), p(i), p(i)) == -1
    assert b"sel_cap" in lib.gtx_last_error()
    assert lib.gtx_op_v10_rows(None, 1, 304, p(i), p(f), p(i), p(i), p(f), full, full, 4, 64, 64, 64, 64, 0.0, p(f), p(i), p(i)) == -1
    assert b"geometry" in lib.gtx_last_error()

    maps = (C.c_void_p * 1)(f.ctypes.data)
    one = lambda v: (C.c_int * 1)(v)

    def feats(dtype=1, cstride=32, coff=0, c=16, dim=8, anchor=0):
        n_out = np.array([1], np.int32)
        a = np.full(4, anchor, np.int32)
        return lib.gtx_op_obj_feats(None, dtype, 1, 1, maps, one(2), one(2), one(cstride), one(coff), one(c), dim, 4, p(n_out), p(a), p(f))

    assert feats() == -1 and b"ctx is NULL" in lib.gtx_last_error()
    assert feats(dim=12) == -1 and b"multiple of dim" in lib.gtx_last_error()
    assert feats(coff=24) == -1 and b"does not fit" in lib.gtx_last_error()
    assert feats(dtype=2, cstride=36) == -1 and b"multiples of 8" in lib.gtx_last_error()
    assert feats(dtype=3) == -1 and b"format" in lib.gtx_last_error()
    assert feats(anchor=4) == -1 and b"outside the level set" in lib.gtx_last_error()


def test_orb_hooks_refuse_bad_sizes_before_any_launch():
    """Host only: the matcher and RANSAC hooks and the stabilizer's read-backs answer bad sizes and missing arrays with an error
    code, with no context or object given."""
    from geotrax_amd import _lib

    lib = _lib.load()
    d = np.zeros((64, 32), np.uint8)
    f = np.zeros(4096, np.float32)
    i = np.zeros(4096, np.int32)
    p = _lib.ptr
    n = C.c_int()

    def match(nq=8, slots_q=8, nt=8, slots_t=8, ratio=0.9, dt=d, xt=f):
        return lib.gtx_op_orb_match(None, p(d), nq, slots_q, p(dt), nt, slots_t, ratio, 0, p(f), p(xt), p(i), p(i), p(i), p(i), p(i), p(i), p(f), C.byref(n))

    assert match() == -1 and b"ctx is NULL" in lib.gtx_last_error()                                     # the sizes were fine
    assert match(nt=0, slots_t=1, dt=None, xt=None) == -1 and b"ctx is NULL" in lib.gtx_last_error()    # no train keypoint is a case
    assert match(nq=0) == -1 and b"orb_match" in lib.gtx_last_error()
    assert match(slots_q=7) == -1 and b"orb_match" in lib.gtx_last_error()                              # fewer slots than keypoints
    assert match(nt=9) == -1 and b"orb_match" in lib.gtx_last_error()
    assert match(nt=0, slots_t=0) == -1 and b"orb_match" in lib.gtx_last_error()                        # an empty grid
    assert match(slots_q=(1 << 16) + 1) == -1 and b"orb_match" in lib.gtx_last_error()
    assert match(slots_q=1 << 16, slots_t=1 << 20) == -1 and b"partials" in lib.gtx_last_error()
    assert match(ratio=float("nan")) == -1 and b"ratio" in lib.gtx_last_error()
    assert match(dt=None) == -1 and b"desc_t is NULL" in lib.gtx_last_error()
    best, cost = C.c_int(), C.c_int64()
    H = np.zeros(9, np.float64)

    def ransac(n_pts=8, n_hyp=64, w=640, h=480, thr=2.0, affine=0, pts=f):
        return lib.gtx_op_orb_ransac(None, p(pts), n_pts, 0, n_hyp, w, h, thr, affine, C.byref(best), C.byref(cost), p(H))

    assert ransac() == -1 and b"ctx is NULL" in lib.gtx_last_error()
    assert ransac(n_pts=0, pts=None) == -1 and b"ctx is NULL" in lib.gtx_last_error()                   # no pair at all: no winner, not an error
    assert ransac(n_pts=-1) == -1 and b"orb_ransac" in lib.gtx_last_error()
    assert ransac(n_hyp=65537) == -1 and b"65536" in lib.gtx_last_error()                               # the key's 16 index bits
    assert ransac(n_hyp=0) == -1 and b"65536" in lib.gtx_last_error()
    assert ransac(w=0) == -1 and b"frame" in lib.gtx_last_error()
    assert ransac(thr=0.0) == -1 and b"threshold" in lib.gtx_last_error()
    assert ransac(affine=2) == -1 and b"affine" in lib.gtx_last_error()
    assert ransac(pts=None) == -1 and b"pts is NULL" in lib.gtx_last_error()
    assert lib.gtx_stabilizer_keep_pass(None, 1) == -1 and b"st is NULL" in lib.gtx_last_error()
    assert lib.gtx_stabilizer_level(None, 0, 0, C.byref(n), C.byref(n), None, 0) == -1 and b"st is NULL" in lib.gtx_last_error()
    assert lib.gtx_stabilizer_candidates(None, 0, 0, 0, C.byref(n), None, None, None, None, None) == -1 and b"st is NULL" in lib.gtx_last_error()


def test_homography_refit_hook_refuses_bad_arguments():
    """Host only: negative n, no pairs with n > 0, a frame without a size and missing outputs get an error code; n = 0 is a case (no model)."""
    from geotrax_amd import _lib

    lib = _lib.load()
    f = np.zeros((8, 4), np.float32)
    H0, H = np.eye(3).ravel(), np.full(9, 7.0)
    valid, inl = C.c_int(-1), C.c_int(-1)
    p = _lib.ptr

    def refit(n=8, w=640, h=480, pts=f, h0=H0, out=H):
        return lib.gtx_op_homography_refit(p(pts), n, w, h, 2.0, 0, p(h0), p(out), C.byref(valid), C.byref(inl))

    assert refit(n=-1) == -1 and b"homography_refit: n" in lib.gtx_last_error()
    assert refit(pts=None) == -1 and b"pairs is NULL" in lib.gtx_last_error()
    assert refit(w=0) == -1 and b"frame" in lib.gtx_last_error()
    assert refit(h=-480) == -1 and b"frame" in lib.gtx_last_error()
    assert refit(h0=None) == -1 and b"H0 is NULL" in lib.gtx_last_error()
    assert refit(out=None) == -1 and b"H is NULL" in lib.gtx_last_error()
    assert valid.value == -1 and inl.value == -1                                                       # nothing was written on the way out
    assert refit(n=0, pts=None) == 0 and valid.value == 0 and inl.value == 0
    np.testing.assert_array_equal(H, np.full(9, 7.0))


def test_gmc_hooks_refuse_bad_sizes_before_any_launch():
    """Host only: the sparse-optical-flow GMC's operator hooks and its counts read-back answer bad sizes, points outside the image
    and missing arrays with an error code, with no context or object given."""
    from geotrax_amd import _lib

    lib = _lib.load()
    g = np.zeros((64, 64), np.uint8)
    f = np.zeros(4096, np.float32)
    i = np.zeros(1024, np.int32)
    p = _lib.ptr
    n, w = C.c_int(), C.c_int()

    def corners(h=64, wd=64, cap=1000, gray=g):
        return lib.gtx_op_gmc_corners(None, p(gray), h, wd, cap, C.byref(n), p(f), p(i))

    assert corners() == -1 and b"ctx is NULL" in lib.gtx_last_error()                                   # the sizes were fine
    assert corners(h=15) == -1 and b"gmc_corners" in lib.gtx_last_error()
    assert corners(wd=8193) == -1 and b"gmc_corners" in lib.gtx_last_error()
    assert corners(cap=999) == -1 and b"1000 corners" in lib.gtx_last_error()
    assert corners(gray=None) == -1 and b"gray is NULL" in lib.gtx_last_error()

    def lk(h=64, wd=64, n_pts=2, pts=(10.0, 10.0, 63.0, 63.0), cur=g):
        xy = np.array(pts, np.float32)
        return lib.gtx_op_gmc_lk(None, p(g), p(cur), h, wd, p(xy), n_pts, p(f), p(i))

    assert lk() == -1 and b"ctx is NULL" in lib.gtx_last_error()                                        # the border pixel is inside
    assert lk(n_pts=0) == -1 and b"ctx is NULL" in lib.gtx_last_error()                                 # no point is a case
    assert lk(pts=(10.0, 10.0, 63.5, 10.0)) == -1 and b"outside the image" in lib.gtx_last_error()
    assert lk(pts=(10.0, 10.0, 10.0, -0.5)) == -1 and b"outside the image" in lib.gtx_last_error()
    assert lk(pts=(10.0, 10.0, float("nan"), 1.0)) == -1 and b"outside the image" in lib.gtx_last_error()
    assert lk(n_pts=1001) == -1 and b"1000 points" in lib.gtx_last_error()
    assert lk(n_pts=-1) == -1 and b"1000 points" in lib.gtx_last_error()
    assert lk(h=15) == -1 and b"gmc_lk" in lib.gtx_last_error()                                         # level 3 would be one pixel high
    assert lk(cur=None) == -1 and b"cur is NULL" in lib.gtx_last_error()
    model = np.zeros(4, np.float64)

    def ransac(n_pairs=8, pairs=f):
        return lib.gtx_op_gmc_ransac(None, p(pairs), n_pairs, 0, C.byref(n), C.byref(w), p(model), p(i))

    assert ransac() == -1 and b"ctx is NULL" in lib.gtx_last_error()
    assert ransac(n_pairs=0, pairs=None) == -1 and b"ctx is NULL" in lib.gtx_last_error()               # no pair: no winner, not an error
    assert ransac(n_pairs=1025) == -1 and b"1024 pairs" in lib.gtx_last_error()
    assert ransac(n_pairs=-1) == -1 and b"1024 pairs" in lib.gtx_last_error()
    assert ransac(pairs=None) == -1 and b"pairs is NULL" in lib.gtx_last_error()
    bad = np.zeros(32, np.float32)
    bad[5] = np.inf
    assert ransac(pairs=bad) == -1 and b"finite" in lib.gtx_last_error()
    assert lib.gtx_gmc_counts(None, p(i)) == -1 and b"gmc is NULL" in lib.gtx_last_error()


def test_ecc_hooks_refuse_bad_sizes_before_any_launch():
    """Host only: the two operator hooks of GMC method ecc answer bad sizes, a map or a state the kernels must not be started from and
    missing arrays with an error code, with no context given."""
    from geotrax_amd import _lib

    lib = _lib.load()
    fr = np.zeros((16, 16, 3), np.uint8)
    f = np.zeros(512 * 13 * 2, np.float32)
    d = np.zeros(512 * 13, np.float64)
    i = np.zeros(8, np.int32)
    p = _lib.ptr

    def prepare(H=16, W=16, frame=fr, out=f):
        return lib.gtx_op_ecc_prepare(None, p(frame), H, W, p(out))

    assert prepare() == -1 and b"ctx is NULL" in lib.gtx_last_error()                                   # the sizes were fine
    assert prepare(H=8, W=8) == -1 and b"ctx is NULL" in lib.gtx_last_error()                           # the object's own lower bound
    assert prepare(H=7) == -1 and b"ecc_prepare" in lib.gtx_last_error()
    assert prepare(W=7) == -1 and b"ecc_prepare" in lib.gtx_last_error()
    assert prepare(W=16385) == -1 and b"ecc_prepare" in lib.gtx_last_error()
    assert prepare(frame=None) == -1 and b"frame_bgr is NULL" in lib.gtx_last_error()
    assert prepare(out=None) == -1 and b"out is NULL" in lib.gtx_last_error()

    def iterate(h=8, w=8, m=(1, 0, 0, 0, 1, 0), exact=1, eps=1e-6, iter_in=0, max_iters=5, status_in=0, done_in=0, tmpl=f, img=f, ps=d, mo=f, none_map=False):
        mm = np.array(m, np.float32)
        return lib.gtx_op_ecc_iterate(None, p(tmpl), p(img), h, w, None if none_map else p(mm), exact, -1.0, -eps, eps, iter_in, max_iters, status_in, done_in,
                                      p(f), p(f), p(ps), p(d), p(mo), p(i), p(d), p(f))

    assert iterate() == -1 and b"ctx is NULL" in lib.gtx_last_error()
    assert iterate(h=2, w=2) == -1 and b"ctx is NULL" in lib.gtx_last_error()                           # the smallest REFLECT_101 can mirror
    assert iterate(iter_in=4, done_in=1, status_in=2, exact=0) == -1 and b"ctx is NULL" in lib.gtx_last_error()
    assert iterate(h=1) == -1 and b"ecc_iterate" in lib.gtx_last_error()
    assert iterate(w=8193) == -1 and b"ecc_iterate" in lib.gtx_last_error()
    assert iterate(m=(1, 0, float("nan"), 0, 1, 0)) == -1 and b"map entry" in lib.gtx_last_error()
    assert iterate(m=(1, 0, 0, 0, 1, float("inf"))) == -1 and b"map entry" in lib.gtx_last_error()
    assert iterate(m=(1, 0, 2e6, 0, 1, 0)) == -1 and b"map entry" in lib.gtx_last_error()
    assert iterate(none_map=True) == -1 and b"map is NULL" in lib.gtx_last_error()
    assert iterate(exact=2) == -1 and b"exact" in lib.gtx_last_error()
    assert iterate(eps=0.0) == -1 and b"eps" in lib.gtx_last_error()
    assert iterate(eps=float("nan")) == -1 and b"eps" in lib.gtx_last_error()
    assert iterate(iter_in=5) == -1 and b"iter_in" in lib.gtx_last_error()                              # the cap is already reached
    assert iterate(iter_in=-1) == -1 and b"iter_in" in lib.gtx_last_error()
    assert iterate(max_iters=0) == -1 and b"iter_in" in lib.gtx_last_error()
    assert iterate(status_in=3) == -1 and b"status_in" in lib.gtx_last_error()
    assert iterate(done_in=2) == -1 and b"status_in" in lib.gtx_last_error()
    assert iterate(tmpl=None) == -1 and b"tmpl is NULL" in lib.gtx_last_error()
    assert iterate(img=None) == -1 and b"img is NULL" in lib.gtx_last_error()
    assert iterate(ps=None) == -1 and b"partial_stats is NULL" in lib.gtx_last_error()
    assert iterate(mo=None) == -1 and b"map_out is NULL" in lib.gtx_last_error()


def test_sift_hooks_refuse_bad_sizes_before_any_launch():
    """Host only: the SIFT operator hooks answer bad sizes, a Gaussian wider than the kernels' 16-pixel radius, and records that
    would index outside their image with an error code, with no context given."""
    from geotrax_amd import _lib, ops

    lib = _lib.load()
    f = np.zeros(5 * 32 * 32, np.float32)
    i = np.zeros(4096, np.int32)
    p = _lib.ptr
    n = C.c_int()

    def blur(h=32, w=32, sigma=1.6, form=0, src=f):
        return lib.gtx_op_sift_blur(None, p(src), h, w, sigma, form, p(f), None)

    assert blur() == -1 and b"ctx is NULL" in lib.gtx_last_error()                                      # the sizes were fine
    assert blur(sigma=4.0) == -1 and b"ctx is NULL" in lib.gtx_last_error()                             # radius 16: the largest
    assert blur(sigma=4.25) == -3 and b"radius 17 exceeds 16" in lib.gtx_last_error()                   # make_taps, not a launch
    assert blur(sigma=0.0) == -1 and b"sigma" in lib.gtx_last_error()
    assert blur(sigma=float("nan")) == -1 and b"sigma" in lib.gtx_last_error()
    assert blur(form=3) == -1 and b"form" in lib.gtx_last_error()
    assert blur(h=0) == -1 and b"sift_blur" in lib.gtx_last_error()
    assert blur(w=4097) == -1 and b"sift_blur" in lib.gtx_last_error()
    assert blur(src=None) == -1 and b"src is NULL" in lib.gtx_last_error()

    def extrema(h=32, w=32, octave=0, cap=16, dog=f):
        return lib.gtx_op_sift_extrema(None, p(dog), h, w, octave, cap, C.byref(n), p(i))

    assert extrema() == -1 and b"ctx is NULL" in lib.gtx_last_error()
    assert extrema(h=10, w=30) == -1 and b"ctx is NULL" in lib.gtx_last_error()                         # no interior is a case, not an error
    assert extrema(cap=0) == -1 and b"cap" in lib.gtx_last_error()
    assert extrema(octave=16) == -1 and b"octave" in lib.gtx_last_error()
    assert extrema(dog=None) == -1 and b"dog5 is NULL" in lib.gtx_last_error()

    def refine(cand=(0, 1, 5, 5), n_cand=1, octave=0, h=32, w=32):
        c = np.array(cand, np.int32)
        return lib.gtx_op_sift_refine(None, p(f), h, w, octave, p(c), n_cand, C.byref(n), p(i))

    assert refine() == -1 and b"ctx is NULL" in lib.gtx_last_error()
    assert refine(n_cand=0) == -1 and b"ctx is NULL" in lib.gtx_last_error()                            # no candidate is a case
    assert refine(cand=(0, 3, 26, 26)) == -1 and b"ctx is NULL" in lib.gtx_last_error()                 # the last interior pixel and layer
    assert refine(cand=(0, 0, 5, 5)) == -1 and b"border" in lib.gtx_last_error()                        # layer 0 has no layer below
    assert refine(cand=(0, 4, 5, 5)) == -1 and b"border" in lib.gtx_last_error()
    assert refine(cand=(0, 1, 4, 5)) == -1 and b"border" in lib.gtx_last_error()
    assert refine(cand=(0, 1, 5, 27)) == -1 and b"border" in lib.gtx_last_error()
    assert refine(cand=(1, 1, 5, 5)) == -1 and b"another octave" in lib.gtx_last_error()
    assert refine(h=10) == -1 and b"border" in lib.gtx_last_error()                                     # an image without interior has no candidate
    assert refine(n_cand=-1) == -1 and b"sift_refine" in lib.gtx_last_error()

    def orient(octave=0, cap=36, **fields):
        r = np.zeros(1, ops.SIFT_REFINED)
        r["size"], r["layer"], r["r"], r["c"] = 4.0, 1, 5, 5
        for k, v in fields.items():
            r[k] = v
        return lib.gtx_op_sift_orient(None, p(f), 32, 32, octave, p(r), 1, cap, C.byref(n), p(i), p(f))

    assert orient() == -1 and b"ctx is NULL" in lib.gtx_last_error()
    assert orient(r=32) == -1 and b"outside the image" in lib.gtx_last_error()
    assert orient(c=-1) == -1 and b"outside the image" in lib.gtx_last_error()
    assert orient(layer=6) == -1 and b"outside the image" in lib.gtx_last_error()
    assert orient(o=1) == -1 and b"another octave" in lib.gtx_last_error()
    assert orient(size=0.0) == -1 and b"size" in lib.gtx_last_error()
    assert orient(size=float("nan")) == -1 and b"size" in lib.gtx_last_error()
    assert orient(size=1000.0) == -1 and b"radius" in lib.gtx_last_error()                              # a 2251-pixel radius
    assert orient(size=1000.0, octave=1, o=1) == -1 and b"ctx is NULL" in lib.gtx_last_error()          # half that in octave 1
    assert orient(cap=0) == -1 and b"cap" in lib.gtx_last_error()

    def describe(root=0, **fields):
        k = np.zeros(1, ops.SIFT_FINAL)
        k["px"], k["py"], k["scl"], k["ori"] = 5.0, 5.0, 2.0, 45.0
        for name, v in fields.items():
            k[name] = v
        return lib.gtx_op_sift_describe(None, p(f), 32, 32, p(k), 1, root, 1e-8, p(f))

    assert describe() == -1 and b"ctx is NULL" in lib.gtx_last_error()
    assert describe(px=-3.0, py=40.0, scl=1e6, ori=360.0) == -1 and b"ctx is NULL" in lib.gtx_last_error()   # the kernel clips the window itself
    assert describe(o=1) == -1 and b"octave 0" in lib.gtx_last_error()
    assert describe(layer=6) == -1 and b"octave 0" in lib.gtx_last_error()
    assert describe(ori=360.5) == -1 and b"ori" in lib.gtx_last_error()
    assert describe(ori=float("nan")) == -1 and b"ori" in lib.gtx_last_error()
    assert describe(px=float("inf")) == -1 and b"position" in lib.gtx_last_error()
    assert describe(scl=0.0) == -1 and b"scl" in lib.gtx_last_error()
    assert describe(root=2) == -1 and b"root" in lib.gtx_last_error()


def test_invert3x3_hook_needs_no_context_and_refuses_null_and_singular():
    """Host only: gtx_op_invert3x3 takes no context; NULL arrays and a singular matrix come back as -1 with a message."""
    from geotrax_amd import _lib

    lib = _lib.load()
    H, inv = np.array([1.0, 0, 5, 0, 2, -3, 0, 0, 1]), np.zeros(9)
    assert lib.gtx_op_invert3x3(_lib.ptr(H), _lib.ptr(inv)) == 0
    np.testing.assert_array_equal(inv, [1, 0, -5, 0, 0.5, 1.5, 0, 0, 1])
    assert lib.gtx_op_invert3x3(None, _lib.ptr(inv)) == -1 and b"H is NULL" in lib.gtx_last_error()
    assert lib.gtx_op_invert3x3(_lib.ptr(H), None) == -1 and b"inv is NULL" in lib.gtx_last_error()
    assert lib.gtx_op_invert3x3(_lib.ptr(np.zeros(9)), _lib.ptr(inv)) == -1 and b"singular" in lib.gtx_last_error()


def test_no_gpu_means_loud_failure_not_fallback():
    """Without a GPU the compute entry points must fail with a message; nothing falls back to CPU."""
    from geotrax_amd import _lib

    lib = _lib.load()
    if lib.gtx_device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(_lib.GtxError):
        _lib.Context(0)


def test_brief_table_equals_the_oracles_own():
    """The steered-BRIEF sampling table is generated independently by the oracle (published recipe: Gaussian pairs,
    sigma = patch/5, 256 orientation bins) and by the library; they must be the same bytes. Host only."""
    import sys

    sys.path.insert(0, str(ROOT))
    from geotrax_amd import _lib
    from oracle.stabilo_ref import brief_pattern

    lib = _lib.load()
    out = np.zeros((256, 256, 4), np.int8)
    _lib.check(lib.gtx_stabilizer_pattern(None, _lib.ptr(out)))
    want = brief_pattern()
    np.testing.assert_array_equal(out, want)
    assert np.abs(want.astype(int)).max() <= 17 and len(np.unique(want[0].reshape(256, 4), axis=0)) > 250


def test_graft_entry_build_runs():
    """The driver's build check: make (a no-op when the library is up to date), load, ABI version, package import."""
    import importlib
    import sys
    from pathlib import Path

    root = Path(__file__).resolve().parent.parent
    sys.path.insert(0, str(root))
    g = importlib.import_module("__graft_entry__")
    g.build()
