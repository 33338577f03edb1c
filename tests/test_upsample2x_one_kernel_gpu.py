"""One nearest-2x kernel behind two hooks. gtx_op_upsample2x (the YOLO trunks' Upsample) and gtx_op_rt_upsample2x (RT-DETR's CCFM) run
the same launch, upsample2x_kernel: a raw copy of 16-byte groups into a channel slice. Both must give the same bytes, the numpy
`repeat` of the input, and leave the other channels of the destination as they were.

Shapes: n = 2, h = 3, w = 5, c = 8 read at channel 8 of 16 and written at channel 8 of 24: odd sizes, two images, and an offset and two
strides that all differ from the channel count, so a stride / offset mix-up moves data. Formats: fp16, fp32 and the pair format. The
values are nonzero fp16 numbers, which every format holds exactly (a pair is then hi = the value, lo = 0), so the comparison is on
bytes in all three. Exact: there is no tolerance."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, H, W, C = 2, 3, 5, 8
IN_CS, IN_COFF, OUT_CS, OUT_COFF = 16, 8, 24, 8


def _fp16_values(rng, shape, dtype):
    v = rng.standard_normal(shape).astype(np.float16)
    v[v == 0] = np.float16(0.5)
    return v.astype(dtype)


@pytest.mark.parametrize("fmt", ["f16", "f32", "split"])
def test_both_upsample_hooks_run_one_copy(gtx_ctx, fmt):
    from geotrax_amd import ops
    from geotrax_amd._lib import check, ptr

    dtype = np.float16 if fmt == "f16" else np.float32
    code = {"f16": ops.GTX_F16, "f32": ops.GTX_F32, "split": ops.GTX_F32S}[fmt]
    rng = np.random.default_rng(20)
    x = _fp16_values(rng, (N, H, W, IN_CS), dtype)
    out0 = _fp16_values(rng, (N, 2 * H, 2 * W, OUT_CS), dtype)

    trunk = out0.copy()
    check(gtx_ctx.lib.gtx_op_upsample2x(gtx_ctx.handle, code, N, H, W, C, ptr(x), IN_CS, IN_COFF, ptr(trunk), OUT_CS, OUT_COFF))
    rt = ops.rt_upsample2x(x, C, out0, in_coff=IN_COFF, out_coff=OUT_COFF, split=fmt == "split", ctx=gtx_ctx)

    want = out0.copy()
    want[..., OUT_COFF:OUT_COFF + C] = x[..., IN_COFF:IN_COFF + C].repeat(2, axis=1).repeat(2, axis=2)
    assert not np.array_equal(want, out0)
    assert trunk.dtype == rt.dtype == dtype and trunk.tobytes() == rt.tobytes(), "the two hooks differ"
    assert trunk.tobytes() == want.tobytes(), "not the input's repeat, or the channels beside the slice changed"
    keep = np.ones(OUT_CS, bool)
    keep[OUT_COFF:OUT_COFF + C] = False
    assert np.array_equal(rt[..., keep], out0[..., keep]) and np.array_equal(trunk[..., keep], out0[..., keep])
    print(f"upsample2x hooks {fmt}: byte-identical, equal to repeat, {int(keep.sum())} of {OUT_CS} channels untouched")
