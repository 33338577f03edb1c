"""The convolution kernels class by class, as the trunk calls them (ops.conv2d_fused, ops.conv_config): every (dtype, ksize, stride,
form, cout tile, K chunk) that conv_pick_config can give a layer -- tests/conv_cases.py's CASES -- with input, residual and output as
channel slices of wider buffers, on 9 x 17 output maps (two tiles each way, the second one pixel wide) of a batch of two.

  test_case_table_covers_every_dispatch_class   host only: the table against a sweep of conv_pick_config
  test_exact_data_is_exact                      host only: the exact data sets are exact in every row's formats
  test_exact_products                           bit for bit against float64: integers; on the split rows also each of the two cross
                                                products alone; with and without a residual slice (res_cstride = 3 cout, res_coff = cout)
  test_tap_and_channel_map                      one-hot weights: which tap of which input channel every output channel reads
  test_in_place_bottleneck                      input, residual and output as abutting chunks of ONE device buffer (stride-1 rows)
  test_tile_rows                                ty_first / ty_count on a 24-row map (every form but K32S2, which has its own test)
  test_values_per_element                       wide-range data, SiLU / ReLU / identity: the project's bars and a per-element bound

Every measured figure is printed with its row id (pytest -s). Worst |got - ref| / B of test_values_per_element per class over the three
activations, MI355X:

  f16   1x1     Staged  bn64 kc64 0.959   bn32 kc64 0.961   bn64 kc32 0.971   bn32 kc32 0.969   bn64 kc16 0.978   bn32 kc16 0.979
  f16   3x3 s1  Staged  bn64 kc16 0.911   bn32 kc16 0.914   bn64 kc32 0.615   bn32 kc32 0.600
  f16   3x3 s2  Staged  bn64 kc16 0.929   bn32 kc16 0.895   bn64 kc32 0.621   bn32 kc32 0.664
  f32   1x1     Staged  bn64 kc32 0.116   bn32 kc32 0.109   bn64 kc16 0.143   bn32 kc16 0.124
  f32   3x3 s1  Staged  bn64 kc16 0.028   bn32 kc16 0.033
  f32   3x3 s2  Staged  bn64 kc16 0.037   bn32 kc16 0.037
  split 1x1     Split   bn64 kc32 0.067   bn32 kc32 0.068   bn64 kc16 0.086   bn32 kc16 0.082
  split 3x3 s1  Split   bn32 kc16 0.023   bn64 kc16 0.017   K32   bn64 kc32 0.018
  split 3x3 s2  Split   bn32 kc16 0.033   bn64 kc16 0.029   K32S2 bn64 kc32 0.027

(fp16: nearly all of B is the output's own rounding, half an ulp = 2^-11 of a value just above a power of two, and some element
comes close to it; the sums' share of B is as idle there as in the other formats.)
"""
import numpy as np
import pytest

import conv_cases as cc
from conv_cases import CASES, row_id
from front_cases import F64_BAR, TOL_F16, TOL_F32, pairs, rel, tol_ratio

gpu = pytest.mark.gpu
ROWS = [pytest.param(i, id=row_id(r)) for i, r in enumerate(CASES)]
ROWS_S1 = [p for p, r in zip(ROWS, CASES) if r.stride == 1]
ROWS_TY = [p for p, r in zip(ROWS, CASES) if r.form != "K32S2"]


def _switches(monkeypatch, r):
    """The environment the row's class is reached in; the launch then runs the class the table names."""
    from geotrax_amd import ops

    for name in cc.SWITCHES + ("GTX_CONV_CPR3",):
        monkeypatch.delenv(name, raising=False)
    if r.switch:
        monkeypatch.setenv(*r.switch)
    assert ops.conv_config(cc.DTYPE_CODE[r.dtype], r.ks, r.stride, r.cin, r.cout)[:3] == (r.form, r.bn, r.kc)


def _launch(ctx, r, x, wt, b, act=0, res=None, coff=cc.PAD_C, n_rows=None, **kw):
    """One launch of row r as the trunk makes it: x [n, h, w, cin] sits at channel 16 of a buffer 32 channels wider (7.0 elsewhere),
    the output slice at channel `coff` of a sentinel-filled buffer 2 coff wider than cout, the residual (if any) at channel cout of
    a buffer of 3 cout channels. Returns the output slice as float64, after checking that the channels on both sides of it came back
    as the buffer's format holds the sentinel."""
    from geotrax_amd import ops

    xb = cc.embed(r, x, cc.PAD_C, r.cin + 2 * cc.PAD_C, cc.GARBAGE)
    ho, wo = cc.out_hw(r, x.shape[1:3])
    ob = np.full((x.shape[0], ho, wo, r.cout + 2 * coff), cc.SENTINEL, cc.np_dtype(r))
    if res is not None:
        kw.update(residual=cc.embed(r, res, r.cout, 3 * r.cout, cc.GARBAGE), res_coff=r.cout)
    got = ops.conv2d_fused(xb, wt, b, stride=r.stride, act=act, in_coff=cc.PAD_C, cin=r.cin, out=ob, out_coff=coff, split=r.dtype == "split",
                           ctx=ctx, **kw)
    assert got.shape == ob.shape and got.dtype == ob.dtype
    np.testing.assert_array_equal(cc.held(r, got[..., :coff]), cc.held(r, ob[..., :coff]))
    np.testing.assert_array_equal(cc.held(r, got[..., coff + r.cout:]), cc.held(r, ob[..., coff + r.cout:]))
    return got[..., coff:coff + r.cout].astype(np.float64)


# ---------------------------------------------------------------------------------------------------- host only

def test_case_table_covers_every_dispatch_class(monkeypatch):
    """Host only. conv_pick_config over the three dtypes, 1x1, 3x3 and 3x3 stride 2, cin in 16..512 and cout in 16..256 in steps of 16,
    with GTX_K32 and GTX_K32S2 each on and off: every row's expectation is the library's answer in the row's environment, and the set
    of classes the sweep meets is the set the table has. A dispatch change that creates, removes or moves a class fails here until
    CASES follows."""
    from geotrax_amd import ops

    monkeypatch.delenv("GTX_CONV_CPR3", raising=False)
    for r in CASES:
        _switches(monkeypatch, r)
        form, bn, kc, name = ops.conv_config(cc.DTYPE_CODE[r.dtype], r.ks, r.stride, r.cin, r.cout)
        assert (form, bn, kc) == (r.form, r.bn, r.kc), row_id(r)
        assert name.startswith({"Staged": "conv_igemm_kernel<", "Split": "conv_igemm_split_kernel<", "K32": "conv_k32_split_kernel",
                                "K32S2": "conv_k32s2_split_kernel"}[form]), name
    met = set()
    for k32 in ("0", "1"):
        for k32s2 in ("0", "1"):
            monkeypatch.setenv("GTX_K32", k32)
            monkeypatch.setenv("GTX_K32S2", k32s2)
            for dtype, code in cc.DTYPE_CODE.items():
                for ks, stride in ((1, 1), (3, 1), (3, 2)):
                    for cin in range(16, 513, 16):
                        for cout in range(16, 257, 16):
                            met.add((dtype, ks, stride) + ops.conv_config(code, ks, stride, cin, cout)[:3])
    table = {cc.klass(r) for r in CASES}
    assert met == table, f"classes without a row: {sorted(met - table)}; rows without a class: {sorted(table - met)}"
    assert len({row_id(r) for r in CASES}) == len(CASES)


def test_conv_config_refuses_what_no_kernel_takes():
    """Host only: the hook answers a shape outside the kernels' reach with an error code, not with a class."""
    from geotrax_amd import _lib, ops

    for bad in ((cc.F32S, 5, 1, 32, 32), (cc.F16, 3, 3, 32, 32), (cc.F32, 1, 2, 32, 32), (cc.F32S, 3, 1, 24, 32), (cc.F16, 1, 1, 32, 24),
                (3, 1, 1, 32, 32), (cc.F32, 1, 1, 0, 32)):
        with pytest.raises(_lib.GtxError):
            ops.conv_config(*bad)
    assert ops.conv_config(cc.F32S, 3, 2, 32, 64, force_kc=16)[:3] == ("Split", 64, 16)          # a pinned K chunk keeps the 32x32x16 kernel


def test_exact_data_is_exact():
    """Host only: every exact data set of every row and geometry is exact in the row's formats (conv_cases.assert_exact runs inside
    exact_case), before any of it is given to a kernel."""
    for i, r in enumerate(CASES):
        for kind in cc.KINDS[r.dtype]:
            for geo in cc.geometries(r.stride):
                x, wt, b, res, ref, ref_res = cc.exact_case(i, kind, geo)
                assert ref.shape == (cc.N,) + cc.out_hw(r, cc.geometries(r.stride)[geo]) + (r.cout,) == res.shape
                if kind == 2 and r.dtype == "split":
                    lo = x - x.astype(np.float16).astype(np.float64)
                    assert np.count_nonzero(lo) > x.size // 2                    # the lo halves do carry bits


# ---------------------------------------------------------------------------------------------------- on the GPU

@gpu
@pytest.mark.parametrize("i", ROWS)
def test_exact_products(gtx_ctx, monkeypatch, i):
    """Identity activation, bit for bit against float64, on every geometry, with and without a residual slice. Kind 1: small integers.
    Kinds 2 and 3 (split rows): one of the scheme's two cross products carries real bits and no lo x lo term exists, so a form that
    loses, doubles or misplaces a cross product on any fragment is off by whole units of 2^-12. fp16 rows take the single tile with
    the output slice 4 channels into its buffer: the kernel's 8-byte store path (the 9 x 17 maps take the 16-byte one)."""
    r = CASES[i]
    _switches(monkeypatch, r)
    for kind in cc.KINDS[r.dtype]:
        for geo in cc.geometries(r.stride):
            x, wt, b, res, ref, ref_res = cc.exact_case(i, kind, geo)
            coff = cc.NARROW_C if (r.dtype == "f16" and geo == "tile") else cc.PAD_C
            np.testing.assert_array_equal(_launch(gtx_ctx, r, x, wt, b, coff=coff), ref, err_msg=f"{row_id(r)} kind {kind} {geo}")
            np.testing.assert_array_equal(_launch(gtx_ctx, r, x, wt, b, res=res, coff=coff), ref_res, err_msg=f"{row_id(r)} kind {kind} {geo} residual")


@gpu
@pytest.mark.parametrize("i", ROWS)
def test_tap_and_channel_map(gtx_ctx, monkeypatch, i):
    """One-hot weights: output channel o must be exactly the input's tap and channel conv_cases.tap_select names (0 beyond the border),
    on an input whose value tells (y % 3, x % 3), the channel and the coarse position. The reference is built by indexing."""
    r = CASES[i]
    _switches(monkeypatch, r)
    for geo, hw in cc.geometries(r.stride).items():
        x = cc.tap_input(r, hw)
        for rnd in range(cc.tap_rounds(r)):
            sel = cc.tap_select(r, rnd)
            got = _launch(gtx_ctx, r, x, cc.tap_weights(r, sel), None)
            want = cc.tap_reference(r, x, sel)
            bad = [f"cout {o}: tap {tap} (ky {tap // r.ks}, kx {tap % r.ks}) of cin {c}, {np.count_nonzero(got[..., o] != want[..., o])} pixels"
                   for o, (tap, c) in enumerate(sel) if not np.array_equal(got[..., o], want[..., o])]
            assert not bad, f"{row_id(r)} {geo} round {rnd}: " + "; ".join(bad[:8])
    seen = [s for rnd in range(cc.tap_rounds(r)) for s in cc.tap_select(r, rnd)]
    assert {t for t, _ in seen} == set(range(r.ks * r.ks)) and {c % r.kc for _, c in seen} == set(range(r.kc))
    assert len({c // r.kc for _, c in seen}) == r.cin // r.kc


@gpu
@pytest.mark.parametrize("i", ROWS_S1)
def test_in_place_bottleneck(gtx_ctx, monkeypatch, i):
    """The bottleneck's pattern: ONE device buffer of cin + 2 cout channels; a 3x3 layer reads chunk 0 (cin wide), adds chunk 1 as the
    residual and writes chunk 2, a 1x1 layer reads chunks 0-1 and writes chunk 2. The slices abut: the cache lines at both edges
    of the output are shared with what the launch reads. Bit for bit the same launch through three separate buffers, float64 on
    exact data, and chunks 0 and 1 unchanged. The second data set is wide-range with SiLU (against the separate buffers only)."""
    from geotrax_amd import ops

    r = CASES[i]
    _switches(monkeypatch, r)
    with_res = r.ks == 3
    cs = r.cin + (2 if with_res else 1) * r.cout
    oc = cs - r.cout
    kind = 2 if r.dtype == "split" else 1
    x, wt, b, res, ref, ref_res = cc.exact_case(i, kind, "9x17")
    xv, wv, bv, _, _ = cc.value_case(i)
    rng = np.random.default_rng(i)
    for name, (xa, wa, ba, ra, act) in {"exact": (x, wt, b, res, 0), "values": (xv, wv, bv, rng.standard_normal(res.shape), 1)}.items():
        buf = cc.embed(r, xa, 0, cs, cc.SENTINEL)
        if with_res:
            buf[..., r.cin:oc] = ra
        kw = dict(stride=1, act=act, in_coff=0, cin=r.cin, out_coff=oc, split=r.dtype == "split", ctx=gtx_ctx)
        got = ops.conv2d_fused(buf, wa, ba, in_place=True, res_coff=r.cin if with_res else None, **kw)
        apart = ops.conv2d_fused(buf.copy(), wa, ba, out=buf.copy(), residual=buf.copy() if with_res else None,
                                 res_coff=r.cin if with_res else None, **kw)
        np.testing.assert_array_equal(got, apart, err_msg=f"{row_id(r)} {name}")
        np.testing.assert_array_equal(cc.held(r, got[..., :oc]), cc.held(r, buf[..., :oc]), err_msg=f"{row_id(r)} {name}: chunks 0 and 1")
        if name == "exact":
            np.testing.assert_array_equal(got[..., oc:].astype(np.float64), ref_res if with_res else ref, err_msg=row_id(r))
        else:
            assert np.isfinite(got.astype(np.float64)).all() and not np.array_equal(got[..., oc:], buf[..., oc:])


@gpu
@pytest.mark.parametrize("i", ROWS_TY)
def test_tile_rows(gtx_ctx, monkeypatch, i):
    """A 24-row output (three tile rows) with ty_first = 1, ty_count = 1: rows 8..15 equal the full launch bit for bit, every other
    row keeps the sentinel. No launcher of these forms refuses tile rows."""
    r = CASES[i]
    _switches(monkeypatch, r)
    xv, wv, bv, _, _ = cc.value_case(i)
    h, w = (24, 17) if r.stride == 1 else (47, 33)
    rng = np.random.default_rng(100 + i)
    x = rng.standard_normal((cc.N, h, w, r.cin)).astype(cc.np_dtype(r))
    full = _launch(gtx_ctx, r, x, wv, bv, act=1)
    part = _launch(gtx_ctx, r, x, wv, bv, act=1, ty_first=1, ty_count=1)
    assert full.shape == (cc.N, 24, 17, r.cout)
    np.testing.assert_array_equal(part[:, 8:16], full[:, 8:16], err_msg=row_id(r))
    sent = cc.held(r, np.full(1, cc.SENTINEL, cc.np_dtype(r)))[0]
    assert (part[:, :8] == sent).all() and (part[:, 16:] == sent).all(), row_id(r)
    assert not (full == sent).any()


@gpu
@pytest.mark.parametrize("i", ROWS)
def test_values_per_element(gtx_ctx, monkeypatch, i):
    """Wide-range random data under SiLU, ReLU and identity against float64 on the operands as the format stores them: the project's
    bars (F64_BAR of the layer's maximum on the split path, TOL_F32 / TOL_F16 elsewhere) and, per element, conv_cases.value_bound --
    derived from the arithmetic, so an error that the layer's maximum would hide on a small output does not pass."""
    r = CASES[i]
    _switches(monkeypatch, r)
    x, wt, b, pre, mag = cc.value_case(i)
    worst = 0.0
    for act in (1, 2, 0):
        ref = cc.activate(pre, act)
        got = _launch(gtx_ctx, r, x, wt, b, act=act)
        ratio = float((np.abs(got - ref) / cc.value_bound(r, ref, mag, act)).max())
        worst = max(worst, ratio)
        if r.dtype == "split":
            e = rel(got, ref, np.abs(ref).max())
            print(f"{row_id(r)} act {act}: err / B {ratio:.3f}, float64 {e:.2e} of max (bar {F64_BAR:.0e})")
            assert e < F64_BAR
            np.testing.assert_array_equal(pairs(got), got)                      # legal pair format
        else:
            tol = TOL_F16 if r.dtype == "f16" else TOL_F32
            print(f"{row_id(r)} act {act}: err / B {ratio:.3f}, {tol_ratio(got, ref, tol):.3f} of rtol/atol {tol[0]:.0e}")
            np.testing.assert_allclose(got, ref, rtol=tol[0], atol=tol[1])
        assert ratio <= 1.0, f"{row_id(r)} act {act}: |got - ref| is {ratio:.3f} of the derived bound"
    print(f"{row_id(r)}: worst err / B {worst:.3f}")
