"""The detector's stem and fused front-end launches, one launch at a time against float64 (ops.stem, ops.conv2d_fused): the three
stem kernels, the front stage (ConvProblem::front_img), the post stage (post_w), the neck's second source (in2 / c_split), the plain
output (out_plain) and the saturation flag (sat_flag). Inputs, references and the bars with their sources: tests/front_cases.py.
Every measured error is printed with its case id (pytest -s); the figures of an MI355X run: profiles/front_ops_errors.txt."""
import numpy as np
import pytest

import front_cases as fc
from front_cases import F64_BAR, FORMS_BAR, pairs, rel

pytestmark = pytest.mark.gpu

F16, F32, F32S = 0, 1, 2
# kernel form -> (dtype, packed, the format its values live in, (rtol, atol) or None for the split bar)
STEM_FORMS = {"valu_f16": (F16, False, "f16", fc.TOL_F16), "valu_f32": (F32, False, "f32", fc.TOL_F32),
              "mfma_f16": (F16, True, "f16", fc.TOL_F16), "split": (F32S, True, "split", None)}
STEM_CASES = ([("valu_f16", c) for c in (16, 32, 48, 64, 80, 96)] + [("valu_f32", c) for c in (16, 32, 48, 64, 80, 96)] +
              [("mfma_f16", c) for c in (16, 32, 48, 80)] + [("split", c) for c in (16, 32, 48, 80)])


def _refused(fn, *needles):
    from geotrax_amd._lib import GtxError

    with pytest.raises(GtxError) as e:
        fn()
    assert e.value.code < 0 and any(s in str(e.value) for s in needles), str(e.value)


# ---------------------------------------------------------------------------------------------------- the stem kernels

@pytest.mark.parametrize("form,c0", STEM_CASES)
def test_stem_forms_against_float64(gtx_ctx, form, c0):
    """Batch 2 (random bytes; a frame inside a 255 and a 0 ring) on one exact tile, odd sides with a partial tile, four tiles per
    row (the `interior` fast path), odd sides whose last row must not take it, and a single output pixel. The split form's output
    is legal pair format (re-splitting it changes nothing); a batch of two equals two single launches bit for bit."""
    from geotrax_amd import ops

    dtype, packed, fmt, tol = STEM_FORMS[form]
    w27, bias = fc.stem_weights(100 + c0, c0)
    for h, w in fc.STEM_SIZES:
        img = fc.images(7 * h + w, h, w)
        got = ops.stem(img, w27, bias, dtype=dtype, packed=packed, ctx=gtx_ctx)
        ref = fc.stem64(img, w27, bias, fmt, packed)
        assert got.shape == ref.shape == (2, (h - 1) // 2 + 1, (w - 1) // 2 + 1, c0)
        err = rel(got, ref, np.abs(ref).max())
        if tol is None:
            print(f"stem {form} c0={c0} {h}x{w}: float64 {err:.2e} (bar {F64_BAR:.0e})")
            assert err < F64_BAR
            np.testing.assert_array_equal(pairs(got), got.astype(np.float64))
        else:
            ratio = fc.tol_ratio(got, ref, tol)
            print(f"stem {form} c0={c0} {h}x{w}: float64 {err:.2e} of max, {ratio:.3f} of rtol/atol {tol[0]:.0e}")
            np.testing.assert_allclose(got.astype(np.float64), ref, rtol=tol[0], atol=tol[1])
        for i in range(2):
            np.testing.assert_array_equal(ops.stem(img[i:i + 1], w27, bias, dtype=dtype, packed=packed, ctx=gtx_ctx)[0], got[i])


@pytest.mark.parametrize("form", list(STEM_FORMS))
def test_stem_tap_map(gtx_ctx, form):
    """One-hot weights: channel c must be SiLU of exactly the neighbour (tap c % 9, colour (c // 9) % 3), or of 0 beyond the border, on an
    image whose 27 values under any window all differ (a swapped tap or colour cannot pass). 21 x 193: border, interior and partial tiles."""
    from geotrax_amd import ops

    dtype, packed, fmt, tol = STEM_FORMS[form]
    img, w27, sel = fc.tap_map_case(21, 193)
    got = ops.stem(img, w27, np.zeros(32, np.float32), dtype=dtype, packed=packed, ctx=gtx_ctx)
    ref = fc.tap_map64(img, sel, fmt)
    err = rel(got, ref, np.abs(ref).max())
    print(f"stem tap map {form}: float64 {err:.2e}")
    if tol is None:
        assert err < F64_BAR
    else:
        np.testing.assert_allclose(got.astype(np.float64), ref, rtol=tol[0], atol=tol[1])


# ---------------------------------------------------------------------------------------------------- the front stage

def _front_data(cin, cout, h, w):
    img = fc.images(h + w + cin, h, w)
    w27, b0 = fc.stem_weights(200 + cin, cin)
    w1, b1 = fc.conv_weights(300 + cin, cout, 3, cin)
    return img, w27, b0, w1, b1


_chain_cache = {}


def _front_chain64(cin, cout, h, w):
    """float64: stem on the pair values of the pixels -> held as pairs -> 3x3 stride 2 + SiLU. Computed once per case."""
    key = (cin, cout, h, w)
    if key not in _chain_cache:
        img, w27, b0, w1, b1 = _front_data(cin, cout, h, w)
        _chain_cache[key] = fc.conv64(fc.held(fc.stem64(img, w27, b0, "split")), w1, b1, stride=2)
    return _chain_cache[key]


@pytest.mark.parametrize("h,w", fc.FRONT_SIZES)
@pytest.mark.parametrize("cin,cout", [(16, 32), (32, 64)])
def test_front_stage(gtx_ctx, cin, cout, h, w):
    """Both instantiations (16 -> 32, 32 -> 64), batch 2: one exact 8 x 16 tile whose patch hangs over every border, two partial
    tiles each way, a stem output with odd sides, and 3 x 3 tiles (the centre tile's image window wholly inside)."""
    from geotrax_amd import ops

    img, w27, b0, w1, b1 = _front_data(cin, cout, h, w)
    fused = ops.conv2d_fused(None, w1, b1, stride=2, front_img=img, front_w27=w27, front_bias=b0, ctx=gtx_ctx)
    two = ops.conv2d(ops.stem(img, w27, b0, dtype=F32S, ctx=gtx_ctx), w1, b1, stride=2, act=True, split=True, ctx=gtx_ctx)
    y = _front_chain64(cin, cout, h, w)
    scale = np.abs(y).max()
    assert fused.shape == y.shape == (2, (h // 2 - 1) // 2 + 1, (w // 2 - 1) // 2 + 1, cout)
    e_f64, e_forms, e_two = rel(fused, y, scale), rel(fused, two, scale), rel(two, y, scale)
    print(f"front {cin}->{cout} {h}x{w}: float64 {e_f64:.2e} (bar {F64_BAR:.0e}) two launches {e_forms:.2e} (bar {FORMS_BAR:.0e}); "
          f"the two launches against float64 {e_two:.2e}")
    assert not np.array_equal(fused, two)               # the fused kernel did run
    assert e_f64 < F64_BAR and e_forms < FORMS_BAR


@pytest.mark.parametrize("cin,cout", [(16, 32), (32, 64)])
def test_front_stage_tile_rows(gtx_ctx, cin, cout):
    """96 x 192 -> 24 x 48 = three tile rows: ty_first = 1, ty_count = 1 computes rows 8..15 as the full launch does, bit for bit,
    and the other rows keep what the buffer held."""
    from geotrax_amd import ops

    img, w27, b0, w1, b1 = _front_data(cin, cout, 96, 192)
    kw = dict(stride=2, front_img=img, front_w27=w27, front_bias=b0, ctx=gtx_ctx)
    before = fc.exact_pairs(np.random.default_rng(5), (2, 24, 48, cout))
    full = ops.conv2d_fused(None, w1, b1, **kw)
    part = ops.conv2d_fused(None, w1, b1, out=before, ty_first=1, ty_count=1, **kw)
    np.testing.assert_array_equal(part[:, 8:16], full[:, 8:16])
    np.testing.assert_array_equal(part[:, :8], before[:, :8])
    np.testing.assert_array_equal(part[:, 16:], before[:, 16:])
    assert not np.array_equal(full[:, :8], before[:, :8])


def test_front_stage_refusals(gtx_ctx, monkeypatch):
    """What conv_split_launch refuses comes back as an error, with nothing launched."""
    from geotrax_amd import ops

    img, w27, b0, w1, b1 = _front_data(32, 64, 38, 70)
    kw = dict(stride=2, front_img=img, front_w27=w27, front_bias=b0, ctx=gtx_ctx)
    need = "half the image size"
    _refused(lambda: ops.conv2d_fused(None, w1, b1, in_shape=(2, 19, 35), front_hw=(37, 70), **kw), need)        # odd front_h
    _refused(lambda: ops.conv2d_fused(None, w1, b1, in_shape=(2, 18, 35), front_hw=(38, 70), **kw), need)        # front_h != 2 H
    _refused(lambda: ops.conv2d_fused(None, w1, b1, in_shape=(2, 19, 34), front_hw=(38, 70), **kw), need)        # front_w_px != 2 W
    _refused(lambda: ops.conv2d_fused(None, w1, b1, members=2, **kw), need)                                        # two members
    w27c, b0c = fc.stem_weights(1, 48)
    w1c, b1c = fc.conv_weights(2, 64, 3, 48)
    _refused(lambda: ops.conv2d_fused(None, w1c, b1c, stride=2, front_img=img, front_w27=w27c, front_bias=b0c, ctx=gtx_ctx),
             "no front-stage kernel")                                                                              # Cin = 48
    _refused(lambda: ops.conv2d_fused(None, w1, b1, split=False, **kw), "need the split-f16x3 path")              # the exact-fp32 kernel
    w1s, _ = fc.conv_weights(3, 64, 3, 32)
    for k32, why in (("0", "half the image size"), ("1", "a plain 3x3 layer")):                                    # a stride-1 launch, either form
        monkeypatch.setenv("GTX_K32", k32)
        _refused(lambda: ops.conv2d_fused(None, w1s, b1, stride=1, in_shape=(2, 19, 35), front_img=img, front_w27=w27, front_bias=b0, ctx=gtx_ctx), why)


# ---------------------------------------------------------------------------------------------------- the post stage

def _post_data(cin, cout, h, w):
    rng = np.random.default_rng(cin + cout + h)
    x = (rng.standard_normal((2, h, w, cin)) * np.exp(rng.uniform(-2, 2, (2, h, w, cin)))).astype(np.float32)
    w1, b1 = fc.conv_weights(400 + cout, cout, 3, cin)
    w2, b2 = fc.conv_weights(500 + cout, cout, 1, cout)
    return x, w1, b1, w2, b2


def _fp16_ties(v):
    """Where an fp32 value lies exactly half way between two fp16 numbers: hi + lo split again may give the other hi."""
    hi = v.astype(np.float16)
    lo = np.abs(v - hi.astype(np.float32)).astype(np.float64)
    ulp = np.spacing(np.abs(hi)).astype(np.float64)
    return (lo > 0) & ((2 * lo == ulp) | (4 * lo == ulp))


@pytest.mark.parametrize("h,w", [(17, 33), (48, 96)])
@pytest.mark.parametrize("cin,cout", [(16, 32), (32, 64)])
def test_post_stage(gtx_ctx, cin, cout, h, w):
    """The 1x1 layer fused behind the 3x3 stride-2 one (Cout = the cout tile), outputs 9 x 17 and 24 x 48, with post_act 0 and 1 and
    with and without post_bias: the two stand-alone launches bit for bit, and within the float64 bar of the chain.

    The two launches run as the detector runs them, the 3x3 layer's pair-format map staying in HBM (post_separate). ops.conv2d twice
    takes that map through the host as hi + lo, and splitting hi + lo again does not always give the same two halves: where lo is
    exactly half an ulp of hi, fp16(hi + lo) is a tie and may round to the other neighbour. The value is the same, the operands of
    the three MFMAs are not, and a few outputs per map move by an ulp of fp32 (measured on MI355X: 4 of 9792 at 16 -> 32, 17 x 33).
    So the host-chained pair is held to the re-ordered-sum bar, and every pixel where it differs must hold such a tie."""
    from geotrax_amd import ops

    x, w1, b1, w2, b2 = _post_data(cin, cout, h, w)
    mid = ops.conv2d_fused(x, w1, b1, stride=2, force_kc=16, ctx=gtx_ctx)
    tie_px = _fp16_ties(mid).any(axis=-1)
    mid64 = fc.held(fc.conv64(pairs(x), w1, b1, stride=2))
    for act in (0, 1):
        for pb in (None, b2):
            fused = ops.conv2d_fused(x, w1, b1, stride=2, post_w=w2, post_bias=pb, post_act=act, ctx=gtx_ctx)
            two = ops.conv2d_fused(x, w1, b1, stride=2, post_w=w2, post_bias=pb, post_act=act, post_separate=True, ctx=gtx_ctx)
            host = ops.conv2d(mid, w2, pb, act=bool(act), split=True, ctx=gtx_ctx)
            y = fc.conv64(mid64, w2, pb, act=act)
            scale = np.abs(y).max()
            e_f64, e_host = rel(fused, y, scale), rel(fused, host, scale)
            differs = (fused != host).any(axis=-1)
            print(f"post {cin}->{cout}->{cout} {h}x{w} act={act} bias={pb is not None}: float64 {e_f64:.2e} (bar {F64_BAR:.0e}), two launches "
                  f"bit-equal {np.array_equal(fused, two)}; through the host {e_host:.2e} (bar {FORMS_BAR:.0e}), {int(differs.sum())} pixels differ, "
                  f"{int(tie_px.sum())} hold a tie")
            np.testing.assert_array_equal(fused, two)
            assert e_f64 < F64_BAR and e_host < FORMS_BAR
            assert not (differs & ~tie_px).any()
            assert not np.array_equal(fused, mid)


def test_post_stage_refusals(gtx_ctx, monkeypatch):
    """The launchers refuse a residual, a Cout that is not the cout tile, a stride-1 launch and the fp16 kernels."""
    from geotrax_amd import ops

    x, w1, b1, w2, b2 = _post_data(32, 64, 17, 33)
    res = np.zeros((2, 9, 17, 64), np.float32)
    _refused(lambda: ops.conv2d_fused(x, w1, b1, stride=2, residual=res, post_w=w2, post_bias=b2, ctx=gtx_ctx), "post stage")
    w1w, b1w = fc.conv_weights(1, 128, 3, 32)           # Cout = 128: two cout tiles of 64
    w2w, b2w = fc.conv_weights(2, 128, 1, 128)
    _refused(lambda: ops.conv2d_fused(x, w1w, b1w, stride=2, post_w=w2w, post_bias=b2w, ctx=gtx_ctx), "post stage")
    w1s, _ = fc.conv_weights(3, 64, 3, 32)
    for k32, why in (("0", "post stage"), ("1", "a plain 3x3 layer")):           # a stride-1 launch, either form
        monkeypatch.setenv("GTX_K32", k32)
        _refused(lambda: ops.conv2d_fused(x, w1s, b1, stride=1, post_w=w2, post_bias=b2, ctx=gtx_ctx), why)
    xh = x.astype(np.float16)                           # off the split path: the fp16 and the exact-fp32 kernels
    _refused(lambda: ops.conv2d_fused(xh, w1, b1, stride=2, split=False, post_w=w2, post_bias=b2, ctx=gtx_ctx), "need the split-f16x3 path")
    _refused(lambda: ops.conv2d_fused(x, w1, b1, stride=2, split=False, post_w=w2, post_bias=b2, ctx=gtx_ctx), "need the split-f16x3 path")


@pytest.mark.parametrize("h,w", [(36, 68), (96, 192)])
@pytest.mark.parametrize("cin,cout", [(16, 32), (32, 64)])
def test_front_and_post_stage(gtx_ctx, cin, cout, h, w):
    """The launch the default path issues: stem + 3x3 stride 2 + 1x1 in one. Against the three separate launches at the re-ordered-sum
    bar and against the float64 chain (both intermediates held as pairs)."""
    from geotrax_amd import ops

    img, w27, b0, w1, b1 = _front_data(cin, cout, h, w)
    w2, b2 = fc.conv_weights(600 + cout, cout, 1, cout)
    fused = ops.conv2d_fused(None, w1, b1, stride=2, front_img=img, front_w27=w27, front_bias=b0, post_w=w2, post_bias=b2, post_act=1, ctx=gtx_ctx)
    s = ops.stem(img, w27, b0, dtype=F32S, ctx=gtx_ctx)
    three = ops.conv2d(ops.conv2d(s, w1, b1, stride=2, act=True, split=True, ctx=gtx_ctx), w2, b2, act=True, split=True, ctx=gtx_ctx)
    y = fc.conv64(fc.held(_front_chain64(cin, cout, h, w)), w2, b2)
    scale = np.abs(y).max()
    e_f64, e_forms, e_three = rel(fused, y, scale), rel(fused, three, scale), rel(three, y, scale)
    print(f"front+post {cin}->{cout}->{cout} {h}x{w}: float64 {e_f64:.2e} (bar {F64_BAR:.0e}) three launches {e_forms:.2e} (bar {FORMS_BAR:.0e}); "
          f"the three launches against float64 {e_three:.2e}")
    assert not np.array_equal(fused, three)
    assert e_f64 < F64_BAR and e_forms < FORMS_BAR


# ---------------------------------------------------------------------------------------------------- the second source

def _two_source_data(h, w, c_split, rest, cout):
    """in2: channels [16, 16 + c_split) of a wider half-resolution buffer; in: channels [8, 8 + Cin) of a wider buffer whose first
    c_split channels of the slice -- the part of the Concat no launch writes -- hold values that must not be read."""
    rng = np.random.default_rng(h + c_split + rest)
    cin = c_split + rest
    x2 = rng.standard_normal((2, h // 2, w // 2, c_split + 24)).astype(np.float32)
    x = rng.standard_normal((2, h, w, cin + 16)).astype(np.float32)
    x[..., 8:8 + c_split] = 1000.0
    wt, b = fc.conv_weights(700 + cin, cout, 1, cin)
    explicit = x.copy()
    explicit[..., 8:8 + c_split] = fc.upsample2x(x2[..., 16:16 + c_split])
    return x, x2, wt, b, explicit


@pytest.mark.parametrize("kc", [32, 16])
@pytest.mark.parametrize("c_split,rest,cout", [(64, 32, 64), (32, 96, 32), (128, 64, 64)])
@pytest.mark.parametrize("h,w", [(10, 18), (16, 32)])
def test_second_source(gtx_ctx, h, w, c_split, rest, cout, kc):
    """The 1x1 split kernel with both K chunk sizes conv_pick_config has for 1x1 layers: the same kernel on the explicitly built
    concat(upsample2x(in2 slice), in slice), bit for bit (same k order), and within the float64 bar."""
    from geotrax_amd import ops

    x, x2, wt, b, explicit = _two_source_data(h, w, c_split, rest, cout)
    cin = c_split + rest
    got = ops.conv2d_fused(x, wt, b, in_coff=8, cin=cin, x2=x2, in2_coff=16, c_split=c_split, force_kc=kc, ctx=gtx_ctx)
    same = ops.conv2d_fused(explicit, wt, b, in_coff=8, cin=cin, force_kc=kc, ctx=gtx_ctx)
    if kc == 32:                                        # the library's own pick for these widths
        np.testing.assert_array_equal(same, ops.conv2d(explicit, wt, b, in_coff=8, cin=cin, split=True, ctx=gtx_ctx))
    y = fc.conv64(pairs(explicit[..., 8:8 + cin]), wt, b)
    e_f64 = rel(got, y, np.abs(y).max())
    print(f"second source {h}x{w} c_split={c_split} rest={rest} cout={cout} kc={kc}: float64 {e_f64:.2e} (bar {F64_BAR:.0e}), "
          f"explicit concat bit-equal {np.array_equal(got, same)}")
    np.testing.assert_array_equal(got, same)
    assert e_f64 < F64_BAR


def test_second_source_refusals(gtx_ctx, monkeypatch):
    """conv_launch refuses what the 1x1 kernel cannot do, and every other form refuses a second source instead of ignoring it."""
    from geotrax_amd import ops

    x, x2, wt, b, _ = _two_source_data(10, 18, 64, 32, 64)
    kw = dict(in_coff=8, cin=96, x2=x2, in2_coff=16, ctx=gtx_ctx)
    bad = "bad second source"
    _refused(lambda: ops.conv2d_fused(x, wt, b, c_split=48, **kw), bad)                       # not a multiple of the 32-channel chunk
    _refused(lambda: ops.conv2d_fused(x, wt, b, c_split=16, force_kc=32, **kw), bad)
    x2w = np.zeros((2, 5, 9, 128), np.float32)
    _refused(lambda: ops.conv2d_fused(x, wt, b, in_coff=8, cin=96, x2=x2w, in2_coff=0, c_split=96, ctx=gtx_ctx), bad)     # c_split = Cin
    _refused(lambda: ops.conv2d_fused(x, wt, b, in_coff=8, cin=96, x2=x2w, in2_coff=0, c_split=128, ctx=gtx_ctx), bad)    # c_split > Cin
    xo = np.zeros((2, 9, 18, 112), np.float32)
    _refused(lambda: ops.conv2d_fused(xo, wt, b, in_coff=8, cin=96, x2=np.zeros((2, 4, 9, 88), np.float32), in2_coff=16, c_split=64, ctx=gtx_ctx), bad)   # odd H
    xw = np.zeros((2, 10, 17, 112), np.float32)
    _refused(lambda: ops.conv2d_fused(xw, wt, b, in_coff=8, cin=96, x2=np.zeros((2, 5, 8, 88), np.float32), in2_coff=16, c_split=64, ctx=gtx_ctx), bad)   # odd W
    # the 3x3 kernels: the 32x32x16 ones (stride 1 and 2) and the 16x16x32 ones
    w3, b3 = fc.conv_weights(1, 64, 3, 96)
    needs_1x1 = "needs the split-f16x3 1x1 kernel"
    for stride in (1, 2):
        for k32 in ("0", "1"):
            monkeypatch.setenv("GTX_K32", k32)
            monkeypatch.setenv("GTX_K32S2", k32)
            _refused(lambda: ops.conv2d_fused(x, w3, b3, stride=stride, c_split=64, **kw), needs_1x1)
    xh = x.astype(np.float16)                           # the fp16 and exact-fp32 kernels
    _refused(lambda: ops.conv2d_fused(xh, wt, b, split=False, in_coff=8, cin=96, x2=x2.astype(np.float16), in2_coff=16, c_split=64, ctx=gtx_ctx), needs_1x1)
    _refused(lambda: ops.conv2d_fused(x, wt, b, split=False, c_split=64, **kw), needs_1x1)


# ---------------------------------------------------------------------------------------------------- out_plain and sat_flag

# split form -> (ksize, stride, the switches that select it, cin, cout)
SPLIT_FORMS = {"1x1": (1, 1, {}, 64, 64), "3x3s1": (3, 1, {"GTX_K32": "0"}, 32, 64), "3x3s2": (3, 2, {"GTX_K32S2": "0"}, 32, 64),
               "k32": (3, 1, {"GTX_K32": "1"}, 32, 64), "k32s2": (3, 2, {"GTX_K32S2": "1"}, 32, 64)}


@pytest.mark.parametrize("form", list(SPLIT_FORMS))
def test_out_plain_and_sat_flag(gtx_ctx, monkeypatch, form):
    """On every split form of the default library, 19 x 37 maps (partial tiles), batch 2: the plain-fp32 output re-split equals the
    same launch's pair-format output bit for bit and meets the float64 bar; the saturation flag stays 0 on ordinary data and with a
    residual that is within range, and becomes 1, every output finite, when an input channel holds 1e6."""
    from geotrax_amd import ops

    k, stride, env, cin, cout = SPLIT_FORMS[form]
    for name, v in env.items():
        monkeypatch.setenv(name, v)
    rng = np.random.default_rng(len(form) + k + stride)
    x = rng.standard_normal((2, 19, 37, cin)).astype(np.float32)
    wt, b = fc.conv_weights(800 + k + stride, cout, k, cin)
    if form in ("k32", "k32s2"):                        # the switch did select the other kernel
        other = "GTX_K32" if form == "k32" else "GTX_K32S2"
        monkeypatch.setenv(other, "0")
        base = ops.conv2d(x, wt, b, stride=stride, split=True, ctx=gtx_ctx)
        monkeypatch.setenv(other, "1")
        assert not np.array_equal(base, ops.conv2d(x, wt, b, stride=stride, split=True, ctx=gtx_ctx))
    pair_out, sat0 = ops.conv2d_fused(x, wt, b, stride=stride, want_sat=True, ctx=gtx_ctx)
    plain, sat1 = ops.conv2d_fused(x, wt, b, stride=stride, out_plain=True, want_sat=True, ctx=gtx_ctx)
    np.testing.assert_array_equal(pair_out, ops.conv2d(x, wt, b, stride=stride, split=True, ctx=gtx_ctx))
    y = fc.conv64(pairs(x), wt, b, stride=stride)
    e_f64 = rel(plain, y, np.abs(y).max())
    print(f"out_plain {form}: float64 {e_f64:.2e} (bar {F64_BAR:.0e}), sat {sat0} / {sat1}")
    np.testing.assert_array_equal(pairs(plain), pair_out.astype(np.float64))
    assert not np.array_equal(plain, pair_out)          # fp32 values, not their 22-bit split
    assert e_f64 < F64_BAR and sat0 == 0 and sat1 == 0
    res = np.full(pair_out.shape, 3.0e4, np.float32)    # within fp16's range, and so is the sum
    with_res, sat2 = ops.conv2d_fused(x, wt, b, stride=stride, residual=res, want_sat=True, ctx=gtx_ctx)
    y_res = y + pairs(res)
    assert sat2 == 0 and rel(with_res, y_res, np.abs(y_res).max()) < F64_BAR
    hot = x.copy()
    hot[..., 3] = 1e6                                   # clamped to 65504 on its way into the pair format; 8 x that leaves fp16's range
    wh = wt.copy()
    wh[0, k // 2, k // 2, 3] = 8.0
    clamped, sat3 = ops.conv2d_fused(hot, wh, b, stride=stride, want_sat=True, ctx=gtx_ctx)
    assert sat3 == 1 and np.isfinite(clamped).all() and np.abs(clamped).max() == 65504.0
    unclamped, sat4 = ops.conv2d_fused(hot, wh, b, stride=stride, out_plain=True, want_sat=True, ctx=gtx_ctx)
    assert sat4 == 0 and np.isfinite(unclamped).all() and unclamped.max() > 65504.0       # nothing enters the pair format


@pytest.mark.parametrize("dtype", [np.float16, np.float32])
def test_out_plain_and_sat_flag_refused_off_the_split_path(gtx_ctx, dtype):
    """The fp16 and exact-fp32 kernels have neither: conv_launch refuses instead of ignoring them."""
    from geotrax_amd import ops

    x = np.zeros((1, 8, 16, 32), dtype)
    wt, b = fc.conv_weights(1, 64, 1, 32)
    _refused(lambda: ops.conv2d_fused(x, wt, b, split=False, out_plain=True, ctx=gtx_ctx), "need the split-f16x3 path")
    _refused(lambda: ops.conv2d_fused(x, wt, b, split=False, want_sat=True, ctx=gtx_ctx), "need the split-f16x3 path")
    assert ops.conv2d_fused(x, wt, b, split=False, ctx=gtx_ctx).shape == (1, 8, 16, 64)       # without them the launch runs
