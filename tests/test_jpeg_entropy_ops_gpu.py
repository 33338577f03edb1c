"""The kernels of csrc/jpeg_entropy.hip one frame at a time through gtx_op_jpeg_entropy, against the numpy twin (status, record,
rounds used) and the host parser (the record's bytes). The kernels are total functions of their input; the damaged frames
compare outcomes."""
import numpy as np
import pytest

import jpeg_entropy_cases as cases

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", cases.picture_names())
def test_record_status_and_rounds_equal_the_twins_and_the_parsers(gtx_ctx, name):
    from geotrax_amd import jpeg

    want = cases.parsed(name)
    for sub_bits in cases.SUB_BITS:
        t_status, t_rec, t_used = cases.twin(name, sub_bits)
        status, rec, used = jpeg.entropy_dev(gtx_ctx, cases.picture_bytes(name), sub_bits, cases.MANY_ROUNDS)
        assert (status, used) == (t_status, t_used) == (0, t_used), (name, sub_bits, status, used, t_used)
        assert rec.tobytes() == t_rec.tobytes() == want.tobytes(), (name, sub_bits)


def test_production_rounds_and_one_round_too_few(gtx_ctx):
    from geotrax_amd import jpeg

    data = cases.picture_bytes("b_long")
    t_status, t_rec, t_used = jpeg.entropy_decode_twin(data)
    status, rec, used = jpeg.entropy_dev(gtx_ctx, data)             # sub_bits 0, rounds 0: the production choices
    assert (status, used) == (0, t_used) and used <= jpeg.ENTROPY_ROUNDS and rec.tobytes() == cases.parsed("b_long").tobytes()
    status, rec, _ = jpeg.entropy_dev(gtx_ctx, data, 0, used - 1)
    assert status == jpeg.entropy_decode_twin(data, 0, 0, used - 1)[0] and status & jpeg.ENTROPY_NOT_CONVERGED and rec is None


def test_damaged_frames_give_the_twins_outcome(gtx_ctx):
    from geotrax_amd import jpeg

    n = 0
    for label, got in cases.damaged_outcomes().items():
        if got[0] != "plan":
            continue
        _, plan, t_status, t_rec, t_used = got
        status, rec, used = jpeg.entropy_plan_dev(gtx_ctx, plan)
        assert (status, used) == (t_status, t_used), (label, status, used, t_status, t_used)
        if status == 0:
            assert rec.tobytes() == t_rec.tobytes(), label
        n += 1
    assert n > 200


def test_hook_refuses_before_any_launch(gtx_ctx):
    import ctypes as C

    from geotrax_amd import _lib, jpeg

    lib = gtx_ctx.lib
    plan = jpeg.entropy_plan(cases.fixture_bytes("r17x9_420"))
    rec = np.zeros(4096, np.uint32).view(np.uint8)
    n, st, used = C.c_size_t(), C.c_int(), C.c_int()
    p = _lib.ptr
    args = (p(rec), rec.nbytes, C.byref(n), C.byref(st), C.byref(used))
    assert lib.gtx_op_jpeg_entropy(gtx_ctx.handle, p(plan), jpeg.PLAN_STREAM_OFFSET - 4, 0, 0, *args) == -1 and b"JPEG plan" in lib.gtx_last_error()
    assert lib.gtx_op_jpeg_entropy(gtx_ctx.handle, p(plan), plan.nbytes, 300, 0, *args) == -1 and b"sub_bits" in lib.gtx_last_error()
    assert lib.gtx_op_jpeg_entropy(gtx_ctx.handle, None, plan.nbytes, 0, 0, *args) == -1 and b"plan is NULL" in lib.gtx_last_error()
    assert lib.gtx_op_jpeg_entropy(gtx_ctx.handle, p(plan), plan.nbytes, 0, 0, None, 16, C.byref(n), C.byref(st), C.byref(used)) == -1
    assert lib.gtx_op_jpeg_entropy(gtx_ctx.handle, p(plan), plan.nbytes, 0, 0, p(rec), rec.nbytes, None, C.byref(st), C.byref(used)) == -1
    small = np.zeros(64, np.uint32).view(np.uint8)                 # the capacity protocol: the size, nothing copied
    assert lib.gtx_op_jpeg_entropy(gtx_ctx.handle, p(plan), plan.nbytes, 0, 0, p(small), small.nbytes, C.byref(n), C.byref(st), C.byref(used)) == 1
    assert n.value == cases.parsed("r17x9_420").nbytes and not small.any()
