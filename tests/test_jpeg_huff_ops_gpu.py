"""The GPU entropy coder's kernels at the hook (gtx_op_jpeg_huff, csrc/jpeg_huff.hip) on hand-built records: the picture equals the
host emitter's (jpeg.record_to_bytes = gtx_jpeg_emit) byte for byte and the per-block bit counts equal the numpy twin's. Integer
arithmetic on both sides: any difference is a bug. The records are built in tests/test_jpeg_huff.py, which checks them on the
host alone."""
import ctypes as C

import numpy as np
import pytest
from test_jpeg_huff import (STUFF_CHUNK, gray, hand_built, padding_records, stuffing_properties, stuffing_record, tile_records)

pytestmark = pytest.mark.gpu


def check(ctx, rec, where):
    from geotrax_amd import jpeg

    want = jpeg.record_to_bytes(rec)
    got, bits = jpeg.huff_dev(ctx, rec, want_bits=True)
    np.testing.assert_array_equal(bits, jpeg.block_bits(rec), err_msg=where)
    assert len(got) == len(want), where
    assert got == want, where


@pytest.mark.parametrize("name", sorted(hand_built()))
def test_smallest_streams_categories_and_dc_prediction(gtx_ctx, name):
    """One block of length 0, of length 64 with position 63 set, with position 63 alone; zero runs around the ZRL's 16; runs that
    end in zeros; every AC and DC category at both signs under the luma and the chroma tables; DC prediction over 3 x 2 MCUs of
    every sampling with distinct DC values and empty blocks."""
    check(gtx_ctx, hand_built()[name], name)


def test_stuffing_across_every_chunk_boundary_and_from_the_padding(gtx_ctx):
    from geotrax_amd import jpeg

    rec = stuffing_record()
    want = jpeg.record_to_bytes(rec)
    many, straddle, last = stuffing_properties(want, int(jpeg.block_bits(rec).sum()))
    assert many, "fewer than 32 stuffed pairs in the expected bytes"
    assert straddle, f"no stuffed pair across every {STUFF_CHUNK}-byte chunk boundary of the stuff pass"
    assert last, "the scan's last byte is not an FF made by the padding"
    check(gtx_ctx, rec, "stuffing")


def test_every_count_of_padding_bits(gtx_ctx):
    recs = padding_records()                                           # asserts that all of 0..7 were found
    for pad, rec in recs.items():
        check(gtx_ctx, rec, f"{pad} padding bits")


@pytest.mark.parametrize("name", ["mixed", "all64", "all0"])
def test_three_scan_tiles_and_a_half(gtx_ctx, name):
    check(gtx_ctx, tile_records()[name], name)


def test_values_without_a_code_are_refused_like_the_emitter_refuses_them(gtx_ctx):
    from geotrax_amd import _lib, jpeg

    lib = gtx_ctx.lib
    for what, runs in (("an AC of 1024", [[0, 1024]]), ("a DC difference of 2048", [[1024], [-1024]])):
        rec = gray(runs)
        n = C.c_size_t()
        tmp = np.empty(4096, np.uint8)
        emit = lib.gtx_jpeg_emit(_lib.ptr(rec), rec.nbytes, _lib.ptr(tmp), tmp.nbytes, C.byref(n))
        out = np.full(4096, 0xA5, np.uint8)
        got = lib.gtx_op_jpeg_huff(gtx_ctx.handle, _lib.ptr(rec), rec.nbytes, _lib.ptr(out), out.nbytes, C.byref(n), None)
        assert got == emit == -1, what
        assert (out == 0xA5).all(), what
        with pytest.raises(jpeg.JpegError):
            jpeg.huff_dev(gtx_ctx, rec)
    check(gtx_ctx, gray([[0, 1023], [-1024], [1023]]), "the largest values that have a code")   # and the context still works


def test_short_output_buffer_reports_the_size(gtx_ctx):
    from geotrax_amd import _lib, jpeg

    rec = hand_built()["prediction_4:2:0"]
    want = jpeg.record_to_bytes(rec)
    n = C.c_size_t()
    small = np.full(len(want) - 1, 0xA5, np.uint8)
    assert gtx_ctx.lib.gtx_op_jpeg_huff(gtx_ctx.handle, _lib.ptr(rec), rec.nbytes, _lib.ptr(small), small.nbytes, C.byref(n), None) == 1
    assert n.value == len(want) and (small == 0xA5).all()
    assert gtx_ctx.lib.gtx_op_jpeg_huff(None, _lib.ptr(rec), rec.nbytes, _lib.ptr(small), small.nbytes, C.byref(n), None) == -1
