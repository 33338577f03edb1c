"""The plot entry points refuse every bad size, count, width, alpha and coordinate with GTX_ERR_INVALID before anything is uploaded:
host only, no context is even given."""
import ctypes as C

import numpy as np
import pytest

from geotrax_amd import plot_draw as P

INVALID = -1
WHITE = (255, 255, 255)


@pytest.fixture(scope="module")
def lib():
    from geotrax_amd import _lib

    return _lib.load()


def draw(lib, prims, h=8, w=8, pitch=None, buf_bytes=None, n=None, null_buf=False):
    from geotrax_amd import _lib

    p = P.as_prims(prims)
    pitch = 3 * w if pitch is None else pitch
    buf = np.zeros(max(h, 1) * max(pitch, 1) + 64, np.uint8)
    return lib.gtx_op_plot_draw(None, None if null_buf else _lib.ptr(buf), buf.size if buf_bytes is None else buf_bytes, h, w, pitch,
                                _lib.ptr(p) if len(p) else None, len(p) if n is None else n)


def test_a_good_call_gets_as_far_as_the_missing_context(lib):
    assert draw(lib, [P.stroke(1, 1, 5, 5, 0.5, WHITE)]) == INVALID and b"ctx is NULL" in lib.gtx_last_error()
    assert draw(lib, []) == INVALID and b"ctx is NULL" in lib.gtx_last_error()


@pytest.mark.parametrize("kw,word", [(dict(h=0), b"canvas"), (dict(w=0), b"canvas"), (dict(h=16385), b"canvas"), (dict(w=16385), b"canvas"), (dict(pitch=23), b"pitch"),
                                     (dict(buf_bytes=7 * 24 + 23), b"rows"), (dict(n=-1), b"n = -1"), (dict(n=(1 << 22) + 1), b"primitives"), (dict(null_buf=True), b"buf is NULL")])
def test_bad_sizes_and_counts(lib, kw, word):
    assert draw(lib, [P.stroke(1, 1, 5, 5, 0.5, WHITE)], **kw) == INVALID
    assert word in lib.gtx_last_error(), lib.gtx_last_error()


def test_null_list_with_a_count(lib):
    assert draw(lib, [], n=3) == INVALID and b"prims is NULL" in lib.gtx_last_error()


@pytest.mark.parametrize("bad,word", [(P.stroke(1, 1, 5, 5, 0.2, WHITE), b"width"), (P.stroke(1, 1, 5, 5, 64.5, WHITE), b"width"), (P.stroke(1, 1, 5, 5, np.nan, WHITE), b"width"),
                                      (P.stroke(1, 1, 5, 5, 0.5, WHITE, 0), b"alpha"), (P.stroke(1, 1, 5, 5, 0.5, WHITE, 257), b"alpha"),
                                      (P.stroke(np.inf, 1, 5, 5, 0.5, WHITE), b"coordinate"), (P.stroke(1, np.nan, 5, 5, 0.5, WHITE), b"coordinate"),
                                      (P.stroke(1, 1, 32768, 5, 0.5, WHITE), b"coordinate"), (P.stroke(1, -32769, 5, 5, 0.5, WHITE), b"coordinate"),
                                      (P.stroke(0, 0, 2049, 0, 0.5, WHITE), b"spans"), (P.stroke(0, 0, 0, -2049, 0.5, WHITE), b"spans"),
                                      (P.stroke(1, 1, 5, 5, 0.5, (255, 255, 255), 256, 0)[:5] + (1 << 24, 256, 0), b"colour"),
                                      (P.stroke(1, 1, 5, 5, 0.6, WHITE), b"polyline"), (P.stroke(1, 1, 5, 5, 0.5, (1, 2, 3)), b"polyline"),
                                      (P.stroke(1, 1, 5, 5, 0.5, WHITE, 100), b"polyline")])
def test_bad_records_are_named_by_index(lib, bad, word):
    good = P.stroke(1, 1, 5, 5, 0.5, WHITE)
    assert draw(lib, [good, bad]) == INVALID
    msg = lib.gtx_last_error()
    assert b"primitive 1" in msg and word in msg, msg
    with pytest.raises(ValueError, match="primitive 1"):
        P.validate([good, bad])                                      # the twin refuses the same record


@pytest.mark.parametrize("h,w,ch,k,word", [(0, 5, 3, 1, b"image"), (5, 0, 3, 1, b"image"), (5, 5, 2, 1, b"channels"), (5, 5, 5, 1, b"channels"), (5, 5, 3, 0, b"factor"),
                                           (5, 5, 3, 257, b"factor"), (16385, 5, 1, 1, b"canvas"), (5, 32770, 1, 2, b"canvas")])
def test_reduce_and_canvas_refuse_bad_sizes(lib, h, w, ch, k, word):
    from geotrax_amd import _lib

    img, out = np.zeros(16, np.uint8), np.zeros(16, np.uint8)
    assert lib.gtx_op_plot_reduce(None, _lib.ptr(img), h, w, ch, k, _lib.ptr(out)) == INVALID and word in lib.gtx_last_error()
    handle = C.c_void_p()
    assert lib.gtx_plot_canvas_create(None, _lib.ptr(img), h, w, ch, k, C.byref(handle)) == INVALID and word in lib.gtx_last_error()
    assert not handle.value


def test_null_arguments(lib):
    from geotrax_amd import _lib

    img = np.zeros(75, np.uint8)
    handle = C.c_void_p()
    assert lib.gtx_plot_canvas_create(None, None, 5, 5, 3, 1, C.byref(handle)) == INVALID and b"image is NULL" in lib.gtx_last_error()
    assert lib.gtx_plot_canvas_create(None, _lib.ptr(img), 5, 5, 3, 1, None) == INVALID and b"out is NULL" in lib.gtx_last_error()
    assert lib.gtx_plot_canvas_create(None, _lib.ptr(img), 5, 5, 3, 1, C.byref(handle)) == INVALID and b"ctx is NULL" in lib.gtx_last_error()
    assert lib.gtx_plot_canvas_draw(None, None, 0) == INVALID and lib.gtx_plot_canvas_read(None, _lib.ptr(img)) == INVALID
    assert lib.gtx_plot_canvas_dptr(None, C.byref(handle)) == INVALID and lib.gtx_plot_canvas_stats(None, None) == INVALID
    assert lib.gtx_plot_canvas_size(None, None, None) == INVALID
    assert lib.gtx_op_plot_reduce(None, None, 5, 5, 3, 1, _lib.ptr(img)) == INVALID and b"image is NULL" in lib.gtx_last_error()
