"""csrc/pool_down.hip alone, through gtx_op_pool_down, against float64 (tests/yolov9_ref.py's pooling, itself held against
torch.nn.functional in tests/test_yolov9.py): AConv's average with its zero border and ADown's fused average + 3x3 stride-2 maximum, in
the three activation formats. Shapes: the smallest at which the kernel can go wrong -- one output, narrow maps, both borders, a channel
split that is no power of two, a map that crosses the row strips (8 / 4 output rows) and a workgroup (256 lanes) in both directions,
and the 184 channels of yolov9m's model.16.

Bounds. Exact fp32, against float64: three additions, each within 2^-24 of a partial sum <= 4 max|x|, then an exact x 0.25: <= 3 * 2^-24
max|x|, plus the one rounding of the reference's own fp32 store: 4 * 2^-24 max|x|. fp16 and the pair format: against the reference
file's emulation of the same format -- fp32 sums in the kernel's order, rounded once where the map is stored -- within one unit in
the last place of that format at the value; and against float64 within the fp32 bound above plus that unit (the sums are fp32 in
every format, so under cancellation the distance to float64 is set by max|x|, not by the result)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FMTS = ["f32", "split", "f16"]
#          h   w   c_avg c_max
SHAPES = [(2, 2, 8, 8), (2, 8, 8, 8), (8, 2, 8, 8), (4, 6, 8, 8), (6, 4, 8, 8), (16, 16, 8, 0), (16, 16, 8, 16), (34, 66, 8, 8), (6, 4, 184, 0)]


def _values(rng, shape, fmt, scale=1.0):
    from yolov9_ref import store

    return store(rng.normal(0, scale, shape), fmt)          # values the format holds exactly


def _run(gtx_ctx, x64, c_avg, c_max, fmt, **kw):
    from geotrax_amd import ops

    x = x64.astype(np.float16 if fmt == "f16" else np.float32)
    return ops.pool_down(x, c_avg, c_max, split=fmt == "split", ctx=gtx_ctx, **kw)


def _compare(got, want, fmt, xmax, what):
    from yolov9_ref import ulp

    got = got.astype(np.float64)
    if isinstance(want, tuple):                              # (the format's emulation, float64 rounded into the format)
        want, want64 = want
        assert np.all(np.abs(got - want64) <= 4 * 2.0 ** -24 * xmax + ulp(want64, fmt)), f"{what}: against float64"
    tol = 4 * 2.0 ** -24 * xmax if fmt == "f32" else ulp(want, fmt)
    err = np.abs(got - want)
    print(f"{what} {fmt}: max error {err.max():.3e}, bound {np.max(tol):.3e}")
    assert np.all(err <= tol), f"{what}: {err.max():.3e}"


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("h,w,c_avg,c_max", SHAPES)
def test_pool_down_against_float64(gtx_ctx, fmt, h, w, c_avg, c_max):
    from yolov9_ref import pool_down_nhwc

    rng = np.random.default_rng(h * 1000 + w * 10 + c_avg + c_max)
    x = _values(rng, (2, h, w, c_avg + c_max), fmt)
    avg, mx, _ = _run(gtx_ctx, x, c_avg, c_max, fmt)
    want_avg, want_mx = pool_down_nhwc(x, c_avg, fmt)
    if fmt != "f32":
        e_avg, e_mx = pool_down_nhwc(x, c_avg, fmt, exact=True)
        want_avg, want_mx = (want_avg, e_avg), (want_mx, e_mx)
    xmax = np.abs(x).max()
    _compare(avg, want_avg, fmt, xmax, "avg")
    assert not avg[:, -1].any() and not avg[:, :, -1].any()                        # the zero border, bit-zero
    assert not np.signbit(avg[:, -1].astype(np.float32)).any() and not np.signbit(avg[:, :, -1].astype(np.float32)).any()
    if c_max:
        assert mx.shape == (2, h // 2, w // 2, c_max)
        _compare(mx, want_mx, fmt, xmax, "max")
    else:
        assert mx is None


@pytest.mark.parametrize("fmt", FMTS)
def test_maximum_at_every_window_position_and_all_negative(gtx_ctx, fmt):
    """An 8 x 8 map whose interior output (1, 1) covers input rows and columns 1..4: the largest value of the map is put at each of
    the window's 16 input positions in turn (channel by channel: 16 channels). Then all-negative data: zero padding in place of -inf
    would win every border window."""
    from yolov9_ref import pool_down_nhwc

    rng = np.random.default_rng(11)
    x = _values(rng, (1, 8, 8, 24), fmt)                     # 8 averaged + 16 pooled channels
    for k in range(16):
        x[0, 1 + k // 4, 1 + k % 4, 8 + k] = 16.0
    _, mx, _ = _run(gtx_ctx, x, 8, 16, fmt)
    _, want = pool_down_nhwc(x, 8, fmt)
    _compare(mx, want, fmt, 16.0, "max, peak at every tap")
    assert np.all(want[0, 1, 1] > 1.0)                       # every channel's window saw its peak: a quarter of 16 and three normal values
    from yolov9_ref import store

    neg = store(-np.abs(rng.normal(0, 1, (1, 6, 6, 16))) - 0.5, fmt)
    _, mx, _ = _run(gtx_ctx, neg, 8, 8, fmt)
    _, want = pool_down_nhwc(neg, 8, fmt)
    assert np.all(want < 0) and np.all(mx.astype(np.float64) < 0)
    _compare(mx, want, fmt, np.abs(neg).max(), "max, all negative")


@pytest.mark.parametrize("fmt", FMTS)
def test_nothing_outside_the_declared_maps_is_touched(gtx_ctx, fmt):
    """Channel slices inside wider buffers, and one image more than the launch runs: the guard values around the written slices, and the
    whole of the image that does not run, come back as given."""
    from yolov9_ref import pool_down_nhwc

    rng = np.random.default_rng(5)
    h, w, ca, cb = 6, 10, 8, 16
    xin = np.full((3, h, w, 40), 99.0)
    xin[..., 8:8 + ca + cb] = _values(rng, (3, h, w, ca + cb), fmt)
    avg0, mx0 = np.full((3, h, w, 24), 7.0), np.full((3, h // 2, w // 2, 32), -3.0)
    dt = np.float16 if fmt == "f16" else np.float32
    avg, mx, _ = _run(gtx_ctx, xin, ca, cb, fmt, n=2, in_coff=8, avg=avg0.astype(dt), avg_coff=8, mx=mx0.astype(dt), max_coff=8)
    want_avg, want_mx = pool_down_nhwc(xin[:2, ..., 8:8 + ca + cb], ca, fmt)
    _compare(avg[:2, ..., 8:16], want_avg, fmt, np.abs(xin[..., 8:32]).max(), "avg slice")
    _compare(mx[:2, ..., 8:24], want_mx, fmt, np.abs(xin[..., 8:32]).max(), "max slice")
    assert np.all(avg[..., :8] == 7.0) and np.all(avg[..., 16:] == 7.0) and np.all(avg[2] == 7.0)
    assert np.all(mx[..., :8] == -3.0) and np.all(mx[..., 24:] == -3.0) and np.all(mx[2] == -3.0)
