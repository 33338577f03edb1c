"""RT-DETR's token-side kernels (csrc/rtdetr_kernels.hip) one launcher at a time through gtx_op_rt_*, each against a float64
reference written here, on the smallest shapes that reach every path: non-square levels, partial tiles and stages, border
samples, exact ties, the second class-mask word. The whole-detector tests (test_rtdetr_gpu.py) run square maps, small sampling
offsets and forgive tie order, so none of this is visible to them.

Bars.
  Values: error = max-abs over the float64 reference's max-abs; e_kernel < 8 * e_fp32ref + 1e-7 (test_ops_gpu.py's rule), where
  e_fp32ref is the error of the same recipe in plain float32 on the CPU, computed in the test and printed beside e_kernel. Where the
  output is stored in a map format (fp16, or hi + lo fp16 pairs) the float32 recipe's result is stored in that format too: the
  store's rounding (2^-11, 2^-22) is the format's, not the kernel's. Map-format inputs: the float64 reference starts from the values
  the format holds.
  Integers (top-k indices; the score stage's count, class and order): exact.
  Anchor logits: 4 float32 ulps counted at max(|logit|, 1). Counted at the logit itself the bar cannot be met by any float32
  evaluation: near v = 0.5 the logit goes to 0 while the rounding of v alone moves it by 2^-24 / (v (1 - v)). The test prints, beside
  the kernel's figure, how far the float32 oracle (RtDetrRef._anchors, torch on the CPU) is from float64 counted both ways: past 4
  ulps at the logit itself, inside 4 at max(|logit|, 1). Below |logit| = 1 the bar is the absolute 4 x 2^-23, which is what
  sigmoid(delta + anchor) sees. Reference boxes and scores: 4 ulps of 1; frame boxes: 4 ulps of the frame's larger side.

Every value test prints its e_kernel and e_fp32ref (pytest -s). The attention kernels use the fast exponential; their peaked cases
are held to the common bar: an error in a rescaling factor exp(m_old - m_new) multiplies numerator and denominator alike and
cancels, and a probability's own relative error, |s - m| 2^-24, is below the float32 rounding of the score it comes from.
"""
import functools
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ULP1 = float(np.spacing(np.float32(1.0)))          # 2^-23


def _seed(*parts):
    return zlib.crc32(repr(parts).encode())


def _pairs(a):
    """What the pair format keeps of an fp32 array: hi + lo, as float64 (tests/test_conv_k32s2_gpu.py)."""
    hi = a.astype(np.float16).astype(np.float32)
    return hi.astype(np.float64) + (a - hi).astype(np.float16).astype(np.float64)


def _exact_pairs(rng, shape):
    """Values every format carries bit for bit (fp16 values): what a buffer holds before a launch."""
    return rng.standard_normal(shape).astype(np.float16).astype(np.float32)


def _held(a, fmt):
    """float64 view of what a host array becomes in the device format; fmt: 'f32', 'f32s', 'f16'."""
    return _pairs(a) if fmt == "f32s" else a.astype(np.float64)


def _stored(a32, fmt):
    """A float32 result stored in an output format, as float64."""
    if fmt == "f16":
        return a32.astype(np.float16).astype(np.float64)
    return _pairs(a32) if fmt == "f32s" else a32.astype(np.float64)


def _host(a64, fmt):
    """Host array of a map in `fmt` from float64 data: (array, split flag)."""
    return (a64.astype(np.float16) if fmt == "f16" else a64.astype(np.float32)), fmt == "f32s"


def _errors(got, ref64, ref32):
    scale = float(np.abs(ref64).max())
    return float(np.abs(got.astype(np.float64) - ref64).max() / scale), float(np.abs(ref32.astype(np.float64) - ref64).max() / scale)


def _value_bar(label, got, ref64, ref32):
    e_k, e_r = _errors(got, ref64, ref32)
    print(f"{label}: e_kernel {e_k:.3e} e_fp32ref {e_r:.3e} ratio {e_k / max(e_r, 1e-30):.2f}")
    assert e_k < 8 * e_r + 1e-7, (label, e_k, e_r)
    return e_k, e_r


# ============================================================================ linear
def _linear_refs(x, w, b, x2, x2_cols, res, act):
    import torch

    def run(dt):
        xt, wt = torch.from_numpy(x).to(dt), torch.from_numpy(w).to(dt)
        y = xt @ wt.T
        if x2 is not None:
            y[:, :x2_cols] = ((xt + torch.from_numpy(x2).to(dt)) @ wt.T)[:, :x2_cols]
        if b is not None:
            y = y + torch.from_numpy(b).to(dt)
        if act == 2:
            y = torch.relu(y)
        elif act == 3:
            y = torch.nn.functional.gelu(y)
        if res is not None:
            y = y + torch.from_numpy(res).to(dt)
        return y.numpy()

    return run(torch.float64), run(torch.float32)


# (M, K, Nout, x2_cols or None, residual, act)
LINEAR_CASES = [
    (1, 16, 16, None, False, 0),          # one row, one K step, three of the four waves without a column block
    (12, 16, 256, None, False, 0),        # the `refer` rows into query_pos_head
    (300, 256, 768, 512, False, 0),       # in_proj: q and k take query + pos, v the query alone
    (37, 1024, 256, None, True, 0),       # two staging spans, residual
    (37, 656, 64, None, False, 0),        # last span 144, last K step 16
    (50, 256, 1024, None, False, 2),      # ReLU
    (50, 256, 1024, None, False, 3),      # GELU
    (600, 256, 80, None, False, 0),       # Nout = 80: a workgroup's second wave is the last with columns
    (50, 256, 128, None, True, 2),        # ReLU, then the residual
    (37, 64, 96, None, True, 3),          # GELU, then the residual; M not a multiple of 16
    (21, 48, 192, 64, False, 0),          # x2_cols strictly inside Nout, one workgroup column with and two without
]


@pytest.mark.parametrize("case", LINEAR_CASES, ids=lambda c: "M{}K{}N{}x{}r{}a{}".format(*c))
def test_linear_matches_float64(gtx_ctx, case):
    from geotrax_amd import ops

    m, k, nout, x2_cols, use_res, act = case
    rng = np.random.default_rng(_seed("linear", case))
    x = rng.standard_normal((m, k)).astype(np.float32)
    w = (rng.standard_normal((nout, k)) / np.sqrt(k)).astype(np.float32)
    b = rng.standard_normal(nout).astype(np.float32)
    x2 = rng.standard_normal((m, k)).astype(np.float32) if x2_cols else None
    res = rng.standard_normal((m, nout)).astype(np.float32) if use_res else None
    got = ops.rt_linear(x, w, b, x2=x2, x2_cols=x2_cols or 0, res=res, act=act, ctx=gtx_ctx)
    ref64, ref32 = _linear_refs(x, w, b, x2, x2_cols, res, act)
    _value_bar(f"linear {case}", got, ref64, ref32)
    if x2_cols:                                       # the columns past x2_cols never saw x2: the launch without it, bit for bit
        plain = ops.rt_linear(x, w, b, res=res, act=act, ctx=gtx_ctx)
        assert got[:, x2_cols:].tobytes() == plain[:, x2_cols:].tobytes()
        assert not np.array_equal(got[:, :x2_cols], plain[:, :x2_cols])


def test_linear_strides_and_column_offset(gtx_ctx):
    """ldx > K, ldr > Nout, ldy > Nout with the block at a column offset, no bias: everything outside the block comes back bit for bit."""
    from geotrax_amd import ops

    m, k, nout, ldx, ldr, ldy, ycol = 21, 48, 32, 52, 40, 80, 24
    rng = np.random.default_rng(5)
    x = rng.standard_normal((m, ldx)).astype(np.float32)
    x[:, k:] = 1e6                                     # read past K and the result is visibly wrong
    x2 = rng.standard_normal((m, ldx + 4)).astype(np.float32)
    x2[:, k:] = -1e6
    w = (rng.standard_normal((nout, k)) / np.sqrt(k)).astype(np.float32)
    res = rng.standard_normal((m, ldr)).astype(np.float32)
    y0 = rng.standard_normal((m, ldy)).astype(np.float32)
    got = ops.rt_linear(x, w, None, k=k, x2=x2, x2_cols=nout, res=res, y=y0, ycol=ycol, ctx=gtx_ctx)
    keep = np.ones(ldy, bool)
    keep[ycol:ycol + nout] = False
    assert got[:, keep].tobytes() == y0[:, keep].tobytes()
    ref64, ref32 = _linear_refs(x[:, :k], w, None, x2[:, :k], nout, res[:, :nout], 0)
    _value_bar("linear strides", got[:, ycol:ycol + nout], ref64, ref32)


# ============================================================================ LayerNorm
def _ln_refs(x64, g, b, out_fmt):
    mean = x64.mean(-1, keepdims=True)
    var = ((x64 - mean) ** 2).mean(-1, keepdims=True)
    ref64 = (x64 - mean) / np.sqrt(var + 1e-5) * g.astype(np.float64) + b.astype(np.float64)
    x32 = x64.astype(np.float32)                      # map-format values are float32 numbers
    c = np.float32(x32.shape[-1])
    m32 = x32.sum(-1, keepdims=True, dtype=np.float32) / c
    d = x32 - m32
    v32 = (d * d).sum(-1, keepdims=True, dtype=np.float32) / c
    ref32 = d * (np.float32(1) / np.sqrt(v32 + np.float32(1e-5))) * g + b
    return ref64, _stored(ref32.astype(np.float32), out_fmt)


def _ln_params(rng, c):
    return (1 + 0.3 * rng.standard_normal(c)).astype(np.float32), rng.standard_normal(c).astype(np.float32)


@pytest.mark.parametrize("rows", [1, 5, 301])
@pytest.mark.parametrize("c", [8, 64, 256, 512, 520, 1024])
def test_layernorm_token_rows(gtx_ctx, c, rows):
    """One lane, a partial first round, exactly 64 groups, 65 groups, both rounds full; the last workgroup partial."""
    from geotrax_amd import ops

    rng = np.random.default_rng(1000 * c + rows)
    x = (rng.standard_normal((rows, c)) * np.exp(rng.uniform(-1, 1, (rows, 1)))).astype(np.float32)
    g, b = _ln_params(rng, c)
    got, sat = ops.rt_layernorm(x, g, b, ctx=gtx_ctx)
    assert not sat
    _value_bar(f"layernorm C={c} rows={rows}", got, *_ln_refs(x.astype(np.float64), g, b, "f32"))


@pytest.mark.parametrize("rows", [5, 301])
@pytest.mark.parametrize("fmts", [("f32", "f32s"), ("f32s", "f32s"), ("f32", "f16"), ("f16", "f16")], ids="-".join)
def test_layernorm_map_formats_in_a_channel_slice(gtx_ctx, fmts, rows):
    """C = 256 read at coff 8 of 272 channels, written at coff 64 of 384: the rest of the output buffer is untouched."""
    from geotrax_amd import ops

    fin, fout = fmts
    c, ics, ico, ocs, oco = 256, 272, 8, 384, 64
    rng = np.random.default_rng(77 + rows)
    xin, in_split = _host(rng.standard_normal((rows, ics)) * 3, fin)
    g, b = _ln_params(rng, c)
    out0, out_split = _host(_exact_pairs(rng, (rows, ocs)).astype(np.float64), fout)
    got, sat = ops.rt_layernorm(xin, g, b, c=c, in_coff=ico, in_split=in_split, out=out0, out_coff=oco, out_split=out_split, ctx=gtx_ctx)
    assert not sat and got.dtype == out0.dtype
    keep = np.ones(ocs, bool)
    keep[oco:oco + c] = False
    assert got[:, keep].tobytes() == out0[:, keep].tobytes()
    x64 = _held(xin, fin)[:, ico:ico + c]
    _value_bar(f"layernorm {fin}->{fout} rows={rows}", got[:, oco:oco + c], *_ln_refs(x64, g, b, fout))


def test_layernorm_large_common_offset(gtx_ctx):
    """x = 1e3 + N(0, 1): E[x^2] - mean^2 in float32 would lose the variance (1e6 against 1); the two-pass form does not."""
    from geotrax_amd import ops

    rng = np.random.default_rng(3)
    x = (1e3 + rng.standard_normal((301, 256))).astype(np.float32)
    g, b = _ln_params(rng, 256)
    got, _ = ops.rt_layernorm(x, g, b, ctx=gtx_ctx)
    _value_bar("layernorm offset 1e3", got, *_ln_refs(x.astype(np.float64), g, b, "f32"))


@pytest.mark.parametrize("c", [8, 256, 1024])
def test_layernorm_constant_row_gives_beta(gtx_ctx, c):
    """Every partial sum of a row of 3.25s is exact: mean = 3.25, the deviations are 0 and the output is beta, exactly."""
    from geotrax_amd import ops

    rng = np.random.default_rng(c)
    g, b = _ln_params(rng, c)
    got, _ = ops.rt_layernorm(np.full((3, c), 3.25, np.float32), g, b, ctx=gtx_ctx)
    assert got.tobytes() == np.broadcast_to(b, (3, c)).astype(np.float32).tobytes()


def test_layernorm_saturation_flag(gtx_ctx):
    from geotrax_amd import ops

    rng = np.random.default_rng(9)
    x = rng.standard_normal((5, 256)).astype(np.float32)
    g, b = _ln_params(rng, 256)
    _, sat = ops.rt_layernorm(x, g, b, out_dtype=np.float32, out_split=True, ctx=gtx_ctx)
    assert not sat
    got, sat = ops.rt_layernorm(x, g * np.float32(1e5), b, out_dtype=np.float32, out_split=True, ctx=gtx_ctx)
    assert sat and np.abs(got).max() == 65504.0


# ============================================================================ multi-head attention
MHA_T_D32 = [1, 3, 16, 63, 64, 65, 225, 300, 1000]
MHA_SHAPES = [(32, t) for t in MHA_T_D32] + [(d, t) for d in (8, 16) for t in (3, 65, 300)]
MHA_HEADS_N = [(1, 1), (8, 2), (8, 1), (1, 2)]      # dealt round the shape list: every pair meets small, middle and large T
# form 1 (the generic kernel whatever D is) differs from form 0 only at D = 32: at 8 and 16 both launch rt_mha_kernel<D>
MHA_CASES = [(0, d, t) for d, t in MHA_SHAPES] + [(1, 32, t) for t in MHA_T_D32]


def _heads_n(d, t):
    return MHA_HEADS_N[MHA_SHAPES.index((d, t)) % 4]


@functools.lru_cache(maxsize=None)
def _mha_case(d, t, variant):
    import torch

    heads, n = _heads_n(d, t)
    c = heads * d
    rng = np.random.default_rng(_seed("mha", d, t, variant))
    q, k, v = (rng.standard_normal((n, t, heads, d)).astype(np.float32) for _ in range(3))
    if variant == "peaked":                           # softmax close to one-hot
        q *= np.float32(8)
    elif variant == "offset":                         # a constant q.k component adds 50 to every score: max-subtraction
        q[..., d - 1] = k[..., d - 1] = np.float32(np.sqrt(50 * np.sqrt(d)))
    qkv = rng.standard_normal((n, t, 3 * c + 4)).astype(np.float32)
    qkv[..., :c], qkv[..., c:2 * c], qkv[..., 2 * c:3 * c] = q.reshape(n, t, c), k.reshape(n, t, c), v.reshape(n, t, c)
    qkv[..., 3 * c:] = 1e6

    def run(dt):
        qt, kt, vt = (torch.from_numpy(a).to(dt).permute(0, 2, 1, 3) for a in (q, k, v))
        p = torch.softmax((qt * (1.0 / np.sqrt(d))) @ kt.transpose(-1, -2), -1)
        return (p @ vt).permute(0, 2, 1, 3).reshape(n, t, c).numpy()

    out0 = rng.standard_normal((n, t, c + 4)).astype(np.float32)
    for a in (qkv, out0):
        a.setflags(write=False)
    return qkv, out0, run(torch.float64), run(torch.float32), heads, c


def _mha_run(ctx, d, t, variant, form):
    from geotrax_amd import ops

    qkv, out0, ref64, ref32, heads, c = _mha_case(d, t, variant)
    got = ops.rt_mha(qkv, c, heads, out=out0, form=form, ctx=ctx)
    assert got[..., c:].tobytes() == out0[..., c:].tobytes()          # the padding columns of the output rows
    return got[..., :c], ref64, ref32


@pytest.mark.parametrize("variant", ["normal", "peaked", "offset"])
@pytest.mark.parametrize("form,d,t", MHA_CASES)
def test_mha_matches_float64(gtx_ctx, form, d, t, variant):
    got, ref64, ref32 = _mha_run(gtx_ctx, d, t, variant, form)
    _value_bar(f"mha form={form} D={d} T={t} heads,n={_heads_n(d, t)} {variant}", got, ref64, ref32)


@pytest.mark.parametrize("variant", ["normal", "peaked", "offset"])
@pytest.mark.parametrize("t", MHA_T_D32)
def test_mha_forms_agree_at_d32(gtx_ctx, t, variant):
    mfma, ref64, ref32 = _mha_run(gtx_ctx, 32, t, variant, 0)
    generic, _, _ = _mha_run(gtx_ctx, 32, t, variant, 1)
    scale = np.abs(ref64).max()
    e_forms, e_r = float(np.abs(mfma - generic).max() / scale), _errors(mfma, ref64, ref32)[1]
    print(f"mha forms T={t} {variant}: e_forms {e_forms:.3e} e_fp32ref {e_r:.3e}")
    assert e_forms < 8 * e_r + 1e-7
    if t == 300:
        assert not np.array_equal(mfma, generic)      # the other kernel did run


# ============================================================================ query selection
TOPK_LEVELS = {"A": [(5, 7), (3, 4), (2, 2)], "B": [(40, 40), (20, 20), (10, 10)], "C": [(33, 31)]}
TOPK_SHAPES = [("A", 1), ("A", 17), ("A", 51), ("B", 300), ("B", 1024), ("C", 300)]
TOPK_CASES = [(lv, nq, var) for lv, nq in TOPK_SHAPES for var in ("normal", "quantised", "equal", "lastch", "crafted") if var != "crafted" or lv != "A"]
N_TIES = 40


def _topk_keys(rng, variant, lv, nq, n, S):
    """Per-anchor keys [n][S] (float64, exact in fp16) for the variants that are built from the key; None for the others."""
    if variant == "quantised":                        # multiples of 1/8 over [-2, 2]: hundreds of exact ties, negative keys
        return np.clip(np.round(rng.standard_normal((n, S)) * 8) / 8, -2, 2) + 0.0
    if variant == "equal":
        return np.full((n, S), 0.375)
    if variant == "crafted":                          # exactly nq - 5 keys above a value that N_TIES anchors carry
        key = np.empty((n, S))
        parts = {"B": ([(0, 1024), (1024, 1600), (1600, 2000), (2000, 2100)], [(3, 17, 15, 5), (0, 20, 15, 5)]), "C": ([(0, 1023)], [(N_TIES,), (N_TIES,)])}[lv]
        for i, v in enumerate((0.5, -0.25)):          # the tied value is positive in one image and negative in the other
            ties = np.concatenate([rng.choice(np.arange(a, b), cnt, replace=False) for (a, b), cnt in zip(parts[0], parts[1][i])])
            rest = np.setdiff1d(np.arange(S), ties)
            above = rng.choice(rest, nq - 5, replace=False)
            below = np.setdiff1d(rest, above)
            key[i, ties] = v
            key[i, above] = v + rng.permutation(nq - 5)[: len(above)] / 64 + 1 / 64
            key[i, below] = v - rng.integers(1, 200, len(below)) / 64
            assert (key[i] > v).sum() == nq - 5 and (key[i] == v).sum() == N_TIES
        return key
    return None


@pytest.mark.parametrize("dtype", [np.float32, np.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("nc", [1, 4, 80])
@pytest.mark.parametrize("lv,nq,variant", TOPK_CASES)
def test_topk_order_and_ties(gtx_ctx, lv, nq, variant, nc, dtype):
    """Descending key, ties by ascending anchor index, exactly: np.argsort(-key, kind='stable') on the per-anchor maxima. Classes at
    coff 3 of nc + 5 channels; the other channels hold 1e4, so a kernel that reads them selects other anchors."""
    from geotrax_amd import ops

    levels = TOPK_LEVELS[lv]
    n, S, cs, coff = 2, sum(h * w for h, w in levels), nc + 5, 3
    rng = np.random.default_rng(_seed("topk", lv, nq, variant, nc))
    key = _topk_keys(rng, variant, lv, nq, n, S)
    if key is None:
        cls = rng.standard_normal((n, S, nc))
        if variant == "lastch":                       # the maximum sits in the last class channel of every anchor
            cls[..., nc - 1] = cls.max(-1) + np.abs(rng.standard_normal((n, S))) + 0.01
    else:                                             # the key in one channel, the others at or below it (on the same grid)
        cls = key[..., None] - rng.integers(0, 9, (n, S, nc)) / 8
        np.put_along_axis(cls, rng.integers(0, nc, (n, S, 1)), key[..., None], -1)
    cls = cls.astype(dtype) + dtype(0)                # a value that rounds to -0.0 becomes +0.0
    assert not np.isnan(cls).any() and not (np.signbit(cls) & (cls == 0)).any()       # the kernel's order for NaN and -0.0 is its own
    maps, o = [], 0
    for h, w in levels:
        m = np.full((n, h, w, cs), 1e4, dtype)
        m[..., coff:coff + nc] = cls[:, o:o + h * w].reshape(n, h, w, nc)
        maps.append(m)
        o += h * w
    got = ops.rt_topk(maps, nc, nq, coff=coff, ctx=gtx_ctx)
    kmax = cls.max(-1).astype(np.float64)
    if key is not None:
        assert np.array_equal(kmax, key)
    want = np.stack([np.argsort(-kmax[i], kind="stable")[:nq] for i in range(n)])
    if variant == "equal":
        assert np.array_equal(want[0], np.arange(nq))
    if variant == "quantised" and lv == "B":
        assert len(np.unique(kmax[0])) <= 33 and (kmax < 0).any()
    assert variant == "equal" or nq < 17 or not np.array_equal(want[0], want[1])      # the two images differ
    np.testing.assert_array_equal(got, want)


# ============================================================================ gather + reference boxes
GATHER_LEVELS = {"issue": [(6, 10), (3, 5), (2, 3)],
                 # anchors are invalid where a centre leaves (0.01, 0.99): a side of more than 50 cells. 64: the centres (x + .5) / 64
                 # are float32 numbers, so the float64 logit starts from the same v
                 "wide": [(2, 64), (3, 5), (2, 3)]}


def _anchor_ref(levels):
    v = []
    for l, (h, w) in enumerate(levels):
        y, x = np.mgrid[0:h, 0:w]
        s = np.full((h, w), 0.05 * 2.0 ** l)
        v.append(np.stack([(x + 0.5) / w, (y + 0.5) / h, s, s], -1).reshape(-1, 4))
    v = np.concatenate(v)
    return np.log(v / (1 - v)), ((v > 1e-2) & (v < 1 - 1e-2)).all(-1)


def _sigmoid64(x):
    return 1.0 / (1.0 + np.exp(-x))


@pytest.mark.parametrize("fmt", ["f32", "f32s", "f16"])
@pytest.mark.parametrize("c", [64, 256])
@pytest.mark.parametrize("lv", ["issue", "wide"])
def test_gather_anchors_and_first_boxes(gtx_ctx, lv, c, fmt):
    from geotrax_amd import ops
    from oracle.rtdetr_ref import RtDetrRef

    levels = GATHER_LEVELS[lv]
    n, S, cs, coff = 2, sum(h * w for h, w in levels), c + 16, 8
    rng = np.random.default_rng(c + len(lv))
    maps, rows = [], []
    for h, w in levels:
        m, split = _host(rng.standard_normal((n, h, w, cs)) * 2, fmt)
        maps.append(m)
        rows.append(_held(m, fmt)[..., coff:coff + c].reshape(n, h * w, c))
    rows = np.concatenate(rows, 1)                     # [n][S][c]: what the maps hold
    idx = np.stack([rng.permutation(S) for _ in range(n)]).astype(np.int32)        # every anchor once per image
    delta = rng.standard_normal((n * S, 8)).astype(np.float32)
    embed, anchors, refer = ops.rt_gather_refer(maps, c, idx, delta, coff=coff, split=split, ctx=gtx_ctx)
    assert np.array_equal(embed.astype(np.float64).reshape(n, S, c), np.stack([rows[i, idx[i]] for i in range(n)]))
    logit, valid = _anchor_ref(levels)
    oracle_logit, oracle_valid = RtDetrRef._anchors(None, levels)
    assert np.array_equal(valid, oracle_valid[0, :, 0].numpy())
    assert valid.any() and (lv == "issue" or (~valid).any())                        # both kinds occur
    flat = idx.ravel()
    want, ok = logit[flat], valid[flat]
    assert np.all(anchors[~ok] == np.inf) and np.isfinite(anchors[ok]).all()
    ulps = np.abs(anchors[ok].astype(np.float64) - want[ok]) / np.spacing(np.maximum(np.abs(want[ok]), 1).astype(np.float32))
    o_err = np.abs(oracle_logit[0].numpy().astype(np.float64) - logit)[valid]      # the float32 oracle against the same float64
    o_at1 = (o_err / np.spacing(np.maximum(np.abs(logit[valid]), 1).astype(np.float32))).max()
    o_own = (o_err / np.spacing(np.abs(logit[valid]).astype(np.float32))).max()
    print(f"anchors {lv}: worst {ulps.max():.2f} ulps at max(|logit|, 1); the float32 oracle {o_at1:.2f}, and {o_own:.2f} at the logit itself")
    assert ulps.max() <= 4
    # refer = sigmoid(delta + logit) from the float64 logits, not from what the kernel returned; an invalid anchor's box is 1 exactly
    ref = _sigmoid64(delta[:, :4].astype(np.float64) + np.where(ok[:, None], want, np.inf))
    e = np.abs(refer[:, :4] - ref).max() / ULP1
    print(f"refer mode 0 {lv}: worst {e:.2f} ulps of 1")
    assert e <= 4 and np.all(refer[:, :4][~ok] == 1.0)
    assert not refer[:, 4:].any()


def test_refer_update_at_the_clamps(gtx_ctx):
    """mode 1 on refer in {0, 1e-7, 1e-5, 0.5, 1 - 1e-5, 1} x delta in {-20, -1, 0, 1, 20}, every pair in every column."""
    import torch
    from geotrax_amd import ops
    from oracle.rtdetr_ref import inverse_sigmoid

    xs = np.array([0, 1e-7, 1e-5, 0.5, 1 - 1e-5, 1], np.float32)
    ds = np.array([-20, -1, 0, 1, 20], np.float32)
    pairs = np.array([(x, d) for x in xs for d in ds], np.float32)                  # 30 pairs
    refer, delta = np.zeros((30, 16), np.float32), np.full((30, 6), 1e3, np.float32)
    for j in range(4):
        refer[:, j], delta[:, j] = np.roll(pairs, 7 * j, 0).T
    got = ops.rt_refer_update(refer, delta, ctx=gtx_ctx)
    want = torch.sigmoid(torch.from_numpy(delta[:, :4]).double() + inverse_sigmoid(torch.from_numpy(refer[:, :4]).double(), eps=1e-5)).numpy()
    e = np.abs(got[:, :4] - want).max() / ULP1
    print(f"refer mode 1: worst {e:.2f} ulps of 1")
    assert e <= 4
    assert not got[:, 4:].any()


# ============================================================================ deformable attention sampling
DEFORM_LEVELS = [(7, 11), (4, 6), (2, 3)]
N_CRAFTED = 5


def _deform_inputs(rng, n, nq, nh, npts):
    """refer [n, nq, 16], offsets [n, nq, nh, L, P, 2], attention logits [n, nq, nh, L * P]. With nq > N_CRAFTED the first queries of
    every image are crafted (all in float32-exact numbers): samples on pixel centres at every level, at ix = iy = -0.5, at ix = W - 0.5
    and iy = H - 0.5, and the two mixed corners."""
    L = len(DEFORM_LEVELS)
    refer = np.zeros((n, nq, 16), np.float32)
    edge = np.array([0.0, 1.0, 0.02, 0.98, 0.5])
    xy = np.where(rng.random((n, nq, 2)) < 0.5, rng.choice(edge, (n, nq, 2)), rng.random((n, nq, 2)))
    refer[..., :2], refer[..., 2:4] = xy, rng.uniform(0.05, 1.0, (n, nq, 2))
    off = (3.0 * rng.standard_normal((n, nq, nh, L, npts, 2))).astype(np.float32)
    awl = rng.standard_normal((n, nq, nh, L * npts)).astype(np.float32)
    awl[:, 1::2] += np.float32(30)                    # a common offset on every other query: max-subtraction
    if nq > N_CRAFTED:
        refer[:, :N_CRAFTED, 2:4] = 1.0
        off[:, :N_CRAFTED] = 0
        refer[:, 0, :2] = 0.5                         # centres: level 0 (7, 11) at loc (.5, .5) -> pixel (5, 3); level 1 (4, 6): x in
        for p in range(npts):                         # {.25, .75}, y in {1, 3, 5, 7} / 8; level 2 (2, 3): x = .5, y in {.25, .75}
            for hh in range(nh):
                lx1, ly1, ly2 = (0.25, 0.75)[(p + hh) % 2], (1 + 2 * ((p + hh) % 4)) / 8, (0.25, 0.75)[p % 2]
                off[:, 0, hh, 1, p] = [(lx1 - 0.5) * 2 * npts, (ly1 - 0.5) * 2 * npts]
                off[:, 0, hh, 2, p] = [0.0, (ly2 - 0.5) * 2 * npts]
        for q, c in zip(range(1, 5), [(0, 0), (1, 1), (0, 1), (1, 0)]):
            refer[:, q, :2] = c
    return refer, off, awl


def _deform_coords(refer, off, npts):
    """Pixel coordinates [n, nq, nh, L, P] (x, y) in float64 and the sampling locations in [0, 1]."""
    r = refer.astype(np.float64)
    loc = r[:, :, None, None, None, :2] + off.astype(np.float64) / npts * r[:, :, None, None, None, 2:4] * 0.5
    wh = np.array([(w, h) for h, w in DEFORM_LEVELS], np.float64)[None, None, None, :, None, :]
    return loc, loc * wh - 0.5, wh


@pytest.mark.parametrize("fmt", ["f32", "f32s", "f16"])
@pytest.mark.parametrize("nq", [1, 37])
@pytest.mark.parametrize("hd,nh,npts", [(256, 8, 4), (64, 4, 2), (32, 1, 1)])
def test_deform_matches_float64(gtx_ctx, hd, nh, npts, nq, fmt):
    import torch
    from geotrax_amd import ops
    from oracle.rtdetr_ref import ms_deform_attn_core

    n, L, coff, cs = 2, len(DEFORM_LEVELS), 32, hd + 40
    rng = np.random.default_rng(hd + nq)
    maps, vals = [], []
    for h, w in DEFORM_LEVELS:
        full = rng.standard_normal((n, h, w, cs))
        full[..., :coff], full[..., coff + hd:] = 1e3, -1e3                        # the channels around the slice
        m, split = _host(full, fmt)
        maps.append(m)
        vals.append(_held(m, fmt)[..., coff:coff + hd].reshape(n, h * w, nh, hd // nh))
    refer, off, awl = _deform_inputs(rng, n, nq, nh, npts)
    loc, pix, wh = _deform_coords(refer, off, npts)
    if nq > N_CRAFTED:                                # the input is what it claims to be
        px, py, W, H = pix[..., 0], pix[..., 1], wh[..., 0], wh[..., 1]
        outside = (px <= -1) | (px >= W) | (py <= -1) | (py >= H)
        assert outside.mean() >= 0.2, outside.mean()
        for band in ((px > -1) & (px < 0), (px > W - 1) & (px < W), (py > -1) & (py < 0), (py > H - 1) & (py < H)):
            assert (band & ~outside).any()
        assert np.all(pix[:, 0] == np.floor(pix[:, 0])) and np.all(pix[:, 0] >= 0) and np.all(pix[:, 0] < wh[0, 0])      # on pixel centres
        assert np.all(pix[:, 1] == -0.5) and np.all(pix[:, 2] == wh[0, 0] - 0.5)
    offaw = np.concatenate([off.reshape(n, nq, -1), awl.reshape(n, nq, -1)], -1)
    got = ops.rt_deform(maps, hd, nh, npts, offaw, refer, coff=coff, split=split, ctx=gtx_ctx)

    def run(dt):
        value = torch.from_numpy(np.concatenate(vals, 1)).to(dt)
        r = torch.from_numpy(refer).to(dt)
        lo = r[:, :, None, None, None, :2] + torch.from_numpy(off).to(dt) / npts * r[:, :, None, None, None, 2:4] * 0.5
        wt = torch.softmax(torch.from_numpy(awl).to(dt), -1).view(n, nq, nh, L, npts)
        return ms_deform_attn_core(value, DEFORM_LEVELS, lo, wt).numpy()

    ref64, ref32 = run(torch.float64), run(torch.float32)
    assert np.abs(ref64).max() > 0.1
    _value_bar(f"deform hd={hd} nh={nh} P={npts} nq={nq} {fmt}", got, ref64, ref32)


# ============================================================================ scores, filter, order, frame boxes
FRAME_WH = (3840, 2160)
POST_VARIANTS = {                                     # classes, conf grid index (None: nothing clears 0.999), max_det (None: nq), raw
    "all": (None, 0, None, True), "filter": ("two", 0, None, True), "c64": ([64], -40, None, True), "c63": ([63], -40, None, True),
    "none_kept": (None, None, None, True), "max_det": (None, -20, 7, True), "raw_null": (None, 0, None, False)}
POST_CASES = [(1, 1, v) for v in ("all", "none_kept", "raw_null")] + [(300, 4, v) for v in ("all", "filter", "none_kept", "max_det", "raw_null")] + \
             [(nq, 80, v) for nq in (100, 512) for v in POST_VARIANTS]


def _post_logits(rng, n, nq, nc, ldl):
    """Grid logits k / 16, |k| <= 96: a best class per query, the others below it (or equal to it at the grid's floor); 25 queries of
    every image share the best score exactly; every tenth query has its best score in two classes."""
    best = rng.integers(-96, 97, (n, nq)) if nq > 1 else np.array([[48], [-48]])[:n]      # one query: kept in image 0, not in image 1
    if nq >= 100:
        for i in range(n):
            best[i, rng.choice(nq, 25, replace=False)] = 40
    k = np.maximum(best[..., None] - rng.integers(1, 60, (n, nq, nc)), -96)
    cls = rng.integers(0, nc, (n, nq))
    if nc == 80:                                      # the classes the filters ask for are not rare
        cls = np.where(rng.random((n, nq)) < 0.5, rng.choice([3, 63, 64, 70], (n, nq)), cls)
    np.put_along_axis(k, cls[..., None], best[..., None], -1)
    if nc > 1:
        twin = (cls + 1 + rng.integers(0, nc - 1, (n, nq))) % nc
        rows = np.arange(nq) % 10 == 0
        for i in range(n):
            k[i, rows, twin[i, rows]] = best[i, rows]
    logits = np.full((n, nq, ldl), 6.5, np.float32)   # the padding columns would win every argmax
    logits[..., :nc] = k / 16
    return logits


@pytest.mark.parametrize("nq,nc,variant", POST_CASES)
def test_post_matches_float64(gtx_ctx, nq, nc, variant):
    from geotrax_amd import ops

    classes, conf_k, max_det, want_raw = POST_VARIANTS[variant]
    if classes == "two":
        classes = [3, 70] if nc == 80 else [1, 3]
    n, ldl = 2, nc + 3
    max_det = max_det or nq
    rng = np.random.default_rng(nq * 100 + nc)
    logits = _post_logits(rng, n, nq, nc, ldl)
    refer = np.zeros((n, nq, 16), np.float32)
    refer[..., :4] = rng.uniform(0.01, 0.99, (n, nq, 4))
    conf = 0.999 if conf_k is None else np.float32((_sigmoid64(conf_k / 16) + _sigmoid64((conf_k + 1) / 16)) / 2)    # midway between two grid scores
    mask = [2**64 - 1, 2**64 - 1] if classes is None else [sum(1 << c for c in classes if c < 64), sum(1 << (c - 64) for c in classes if c >= 64)]
    rows0 = rng.standard_normal((n, max_det, 6)).astype(np.float32)
    rows, out_n, raw = ops.rt_post(logits, nc, refer, conf, FRAME_WH, max_det, class_mask=mask, out_rows=rows0, want_raw=want_raw, ctx=gtx_ctx)
    assert (raw is None) == (not want_raw)
    score = _sigmoid64(logits[..., :nc].astype(np.float64))
    best, cls = score.max(-1), score.argmax(-1)       # argmax: the first maximum
    r = refer.astype(np.float64)
    box = np.stack([(r[..., 0] - r[..., 2] / 2) * FRAME_WH[0], (r[..., 1] - r[..., 3] / 2) * FRAME_WH[1],
                    (r[..., 0] + r[..., 2] / 2) * FRAME_WH[0], (r[..., 1] + r[..., 3] / 2) * FRAME_WH[1]], -1)
    kept_total = 0
    for i in range(n):
        keep = best[i] > float(conf)
        if classes is not None:
            keep &= np.isin(cls[i], classes)
        q = np.flatnonzero(keep)
        q = q[np.argsort(-best[i, q], kind="stable")]                              # ties keep query order
        if variant == "all" and nq >= 100:
            assert (np.diff(best[i, q]) == 0).sum() >= 20                          # at least 20 exact ties among the kept rows
        if variant == "max_det":
            assert len(q) > max_det
        if variant in ("c63", "c64", "filter"):
            assert 0 < len(q) < (best[i] > float(conf)).sum()                      # the filter cuts, and not everything
        q = q[:max_det]
        kept_total += len(q)
        assert out_n[i] == len(q), (i, out_n[i], len(q))
        got = rows[i, :len(q)]
        np.testing.assert_array_equal(got[:, 5], cls[i, q])                        # class and order, exactly
        assert np.abs(got[:, 4] - best[i, q]).max(initial=0) <= 4 * ULP1
        assert np.abs(got[:, :4] - box[i, q]).max(initial=0) <= 4 * float(np.spacing(np.float32(max(FRAME_WH))))
        assert rows[i, len(q):].tobytes() == rows0[i, len(q):].tobytes()           # rows past the count come back as they went in
    if variant == "none_kept":
        assert kept_total == 0 and rows.tobytes() == rows0.tobytes()
    else:
        assert kept_total > 0
    if want_raw:
        assert np.abs(raw[..., 4:] - score).max() <= 4 * ULP1
        assert raw[..., :4].tobytes() == refer[..., :4].tobytes()
