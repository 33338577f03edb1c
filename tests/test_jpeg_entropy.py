"""The GPU entropy route of the JPEG frame source, without a GPU: jpeg::plan() (the host half), and the numpy twin of the kernels
of csrc/jpeg_entropy.hip against the host parser. What the twin shows is what the kernel design rests on: the fixed point of the
self-synchronising decode is the sequential decode, byte for byte, and a frame that has not reached it says so."""
import ctypes as C
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import jpeg_entropy_cases as cases

ROOT = Path(__file__).resolve().parent.parent


@pytest.mark.parametrize("name", cases.picture_names())
def test_twin_record_equals_the_parsers_byte_for_byte(name):
    want = cases.parsed(name)
    for sub_bits in cases.SUB_BITS:
        status, rec, used = cases.twin(name, sub_bits)
        assert status == 0 and 1 <= used <= cases.MANY_ROUNDS, (name, sub_bits, status, used)
        assert rec.tobytes() == want.tobytes(), (name, sub_bits)


def test_hand_built_pictures_are_what_they_are_meant_to_be():
    from geotrax_amd import jpeg

    hb = cases.hand_built()
    f, _, _, stream = jpeg.plan_fields(jpeg.entropy_plan(hb["a_empty"][1]))
    assert f["stream_bits"] // f["n_blocks"] <= 6                 # six bits a block at most: 170 blocks in 1024 bits
    f, _, _, stream = jpeg.plan_fields(jpeg.entropy_plan(hb["b_long"][1]))
    assert f["stream_bits"] / f["n_blocks"] > 1024 and f["stream_bytes"] > 100_000        # a block outlasts a subsequence
    assert -(-f["stream_bits"] // 1024) > 3 * jpeg.entropy_lanes(1024)                    # four workgroups or more
    f, _, _, stream = jpeg.plan_fields(jpeg.entropy_plan(hb["c_ff"][1]))
    assert (stream == 0xFF).mean() > 0.2 and len(hb["c_ff"][1]) > f["stream_bytes"] * 1.2  # dense in FF: the file is stuffed
    assert jpeg.plan_fields(jpeg.entropy_plan(hb["e_8x8"][1]))[0]["stream_bits"] < 256
    assert jpeg.plan_fields(jpeg.entropy_plan(hb["f_gray"][1]))[0]["ncomp"] == 1
    f = jpeg.plan_fields(jpeg.entropy_plan(hb["f_422"][1]))[0]
    assert (f["hs"], f["vs"]) == (2, 1)


def test_restart_intervals_go_to_the_host_and_progressive_is_refused_as_by_parse():
    from geotrax_amd import jpeg

    for name in cases.HOST_ROUTE:
        assert jpeg.entropy_plan(cases.fixture_bytes(name)) is None
        with pytest.raises(ValueError):
            jpeg.entropy_decode_twin(cases.fixture_bytes(name))
    for name in cases.REFUSED:
        with pytest.raises(jpeg.JpegError) as a:
            jpeg.entropy_plan(cases.fixture_bytes(name), 3)
        with pytest.raises(jpeg.JpegError) as b:
            jpeg.parse(cases.fixture_bytes(name), 3)
        assert str(a.value) == str(b.value) and a.value.code == -3 and "JPEG frame 3" in str(a.value)


def test_rounds_on_the_long_block_picture():
    """Picture (b) never ends a block with an EOB, so a wrong entry state never corrects itself: every workgroup waits for the one
    before it. The rounds it needs are within the production count, and one round fewer says `not converged`."""
    from geotrax_amd import jpeg

    data = cases.picture_bytes("b_long")
    status, rec, used = jpeg.entropy_decode_twin(data)             # production sizes
    assert status == 0 and rec.tobytes() == cases.parsed("b_long").tobytes()
    assert 1 < used <= jpeg.ENTROPY_ROUNDS
    status, rec, again = jpeg.entropy_decode_twin(data, rounds=used)
    assert status == 0 and again == used
    status, rec, _ = jpeg.entropy_decode_twin(data, rounds=used - 1)
    assert status & jpeg.ENTROPY_NOT_CONVERGED and rec is None
    status, rec, used256 = cases.twin("b_long", 256)
    assert status == 0 and used256 > jpeg.ENTROPY_ROUNDS          # (what the small subsequence costs on such data)
    status, rec, _ = jpeg.entropy_decode_twin(data, 256, 0, used256 - 1)
    assert status & jpeg.ENTROPY_NOT_CONVERGED and rec is None


def test_damaged_frames_are_ok_with_the_parsers_record_or_not_ok():
    from geotrax_amd import jpeg

    seen = {"refused": 0, "host": 0, "ok": 0, "status": 0}
    outcomes = cases.damaged_outcomes()
    for label, data in cases.damaged():
        got = outcomes[label]
        if got[0] == "refused":
            with pytest.raises(jpeg.JpegError) as e:
                jpeg.parse(data)
            assert str(e.value) == got[1], label                   # the header's refusal, word for word
            seen["refused"] += 1
        elif got[0] == "host":
            seen["host"] += 1
        elif got[2] == 0:
            assert got[3].tobytes() == jpeg.parse(data)[0].tobytes(), label
            seen["ok"] += 1
        else:
            assert got[3] is None
            seen["status"] += 1
    assert seen["ok"] > 20 and seen["status"] > 60, seen            # both sides of the claim were exercised
    # the converse is not promised (a frame the parser takes may fall back), but on these pictures it holds for every truncation:
    # the twin says invalid exactly where the parser refuses the data
    for label, data in cases.damaged()[:64]:
        got = outcomes[label]
        if got[0] == "plan" and got[2] != 0:
            with pytest.raises(jpeg.JpegError):
                jpeg.parse(data)


def test_plan_protocol_and_refusals():
    from geotrax_amd import _lib, jpeg

    lib = _lib.load()
    data = np.frombuffer(cases.fixture_bytes("r17x9_420"), np.uint8)
    plan = jpeg.entropy_plan(data.tobytes())
    f, quant, tables, stream = jpeg.plan_fields(plan)
    rf, rquant, _, _ = jpeg.record_fields(cases.parsed("r17x9_420"))
    assert (f["w"], f["h"], f["n_blocks"], f["restart"]) == (17, 9, rf["n_blocks"], 0) and f["stream_bits"] == 8 * len(stream)
    np.testing.assert_array_equal(quant, rquant)
    assert plan.nbytes == jpeg.PLAN_STREAM_OFFSET + (len(stream) + 3) // 4 * 4 <= lib.gtx_jpeg_plan_bound(9, 17)
    assert lib.gtx_jpeg_plan_bound(0, 5) == 0 and lib.gtx_jpeg_plan_bound(5, 16385) == 0
    needed, h, w = C.c_size_t(), C.c_int(), C.c_int()
    p = _lib.ptr

    def call(out, cap, src=data, n=None, frame=0):
        return lib.gtx_jpeg_plan(p(src), len(src) if n is None else n, frame, C.byref(h), C.byref(w), None, None, None, out, cap, C.byref(needed))

    assert call(None, 0) == 1 and needed.value == plan.nbytes and (h.value, w.value) == (9, 17)
    small = np.full(plan.nbytes, 0xAB, np.uint8)
    assert call(p(small), 1) == 1 and needed.value == plan.nbytes and (small == 0xAB).all()
    assert call(p(small), plan.nbytes - 4) == 1 and (small == 0xAB).all()         # a plan that does not fit leaves the buffer untouched
    assert call(p(small), plan.nbytes) == 0 and small.tobytes() == plan.tobytes()
    assert call(p(small), -1 % 2**64) == 0                          # a capacity that is "negative": just large
    assert call(None, 8) == -1 and b"out is NULL" in lib.gtx_last_error()
    assert lib.gtx_jpeg_plan(None, 4, 0, None, None, None, None, None, None, 0, C.byref(needed)) == -1 and b"NULL" in lib.gtx_last_error()
    assert lib.gtx_jpeg_plan(p(data), len(data), 0, None, None, None, None, None, None, 0, None) == -1 and b"NULL" in lib.gtx_last_error()
    odd = np.zeros(plan.nbytes + 8, np.uint8)
    assert lib.gtx_jpeg_plan(p(data), len(data), 0, None, None, None, None, None, C.c_void_p(odd.ctypes.data + 1), plan.nbytes, C.byref(needed)) == -1
    assert b"4-byte aligned" in lib.gtx_last_error()
    # refusals carry the marker and the frame number, as parse()'s do
    prog = np.frombuffer(cases.fixture_bytes("p70x45_progressive"), np.uint8)
    assert call(None, 0, prog, frame=41) == -3 and b"JPEG frame 41: SOF2 (progressive)" in lib.gtx_last_error()
    assert call(None, 0, data, n=20, frame=7) == -1 and b"JPEG frame 7:" in lib.gtx_last_error()
    rst = np.frombuffer(cases.fixture_bytes("p70x45_420_rst3"), np.uint8)
    assert call(None, 0, rst) == 2 and needed.value == 0 and (h.value, w.value) == (45, 70)


def test_feeder_entropy_switch_refuses_null_without_a_gpu():
    from geotrax_amd import _lib

    lib = _lib.load()
    assert lib.gtx_feeder_set_jpeg_entropy(None, 1) == -1 and b"feeder is NULL" in lib.gtx_last_error()
    out = (C.c_int64 * 3)()
    assert lib.gtx_feeder_jpeg_stats(None, out) == -1 and b"NULL" in lib.gtx_last_error()


def test_entropy_hook_refuses_bad_arguments_before_any_launch():
    """Host only: no context is given, so anything that gets as far as asking for one passed every check."""
    from geotrax_amd import _lib, jpeg

    lib = _lib.load()
    plan = jpeg.entropy_plan(cases.fixture_bytes("r17x9_420"))
    rec = np.zeros(4096, np.uint32).view(np.uint8)
    n, st, used = C.c_size_t(), C.c_int(), C.c_int()
    p = _lib.ptr

    def call(pl=plan, nbytes=None, sub=0, rounds=0, out=rec, cap=None, n_=n, st_=st, used_=used):
        return lib.gtx_op_jpeg_entropy(None, p(pl) if pl is not None else None, plan.nbytes if nbytes is None else nbytes, sub, rounds,
                                       p(out) if out is not None else None, (out.nbytes if out is not None else 0) if cap is None else cap,
                                       C.byref(n_) if n_ is not None else None, C.byref(st_) if st_ is not None else None,
                                       C.byref(used_) if used_ is not None else None)

    assert call() == -1 and b"ctx is NULL" in lib.gtx_last_error()                     # everything else was fine
    for sub in (256, 512, 1024, 2048):
        assert call(sub=sub, rounds=64) == -1 and b"ctx is NULL" in lib.gtx_last_error()
    assert call(nbytes=jpeg.PLAN_STREAM_OFFSET - 4) == -1 and b"JPEG plan: shorter than its header" in lib.gtx_last_error()
    assert call(nbytes=plan.nbytes - 4) == -1 and b"JPEG plan" in lib.gtx_last_error()
    for sub in (-1, 1, 128, 1000, 4096):
        assert call(sub=sub) == -1 and b"sub_bits" in lib.gtx_last_error()
    for rounds in (-1, 65):
        assert call(rounds=rounds) == -1 and b"rounds" in lib.gtx_last_error()
    assert call(pl=None) == -1 and b"plan is NULL" in lib.gtx_last_error()
    assert call(out=None, cap=8) == -1 and b"record is NULL" in lib.gtx_last_error()
    assert call(n_=None) == -1 and call(st_=None) == -1 and call(used_=None) == -1
    bad = plan.copy()
    bad[64:68].view(np.uint32)[0] = 3                              # a restart interval
    assert call(pl=bad) == -1 and b"restart" in lib.gtx_last_error()
    bad = plan.copy()
    bad[36:40].view(np.uint32)[0] += 1                             # n_blocks
    assert call(pl=bad) == -1 and b"block count" in lib.gtx_last_error()


def test_plan_is_memory_clean_under_the_sanitizers(tmp_path):
    """`make jpegplancheck` as a test: jpeg::plan() alone (csrc/diag/jpeg_plan_check.cpp, no GPU, no Python in the process) under
    AddressSanitizer and UBSan over the fixtures, every truncation of one and 2000 seeded corruptions."""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the stand-alone plan check"
    src = ROOT / "geo-trax_amd" / "csrc"
    exe = tmp_path / "jpeg_plan_check"
    flags = ["-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer"]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    sources = [str(src / "jpeg_parse.cpp"), str(src / "diag" / "jpeg_plan_check.cpp")]
    r = subprocess.run([gxx, *flags, *san, *sources, "-o", str(exe)], capture_output=True, text=True)
    no_runtime = any(t in r.stderr for t in ("cannot find -lasan", "cannot find -lubsan", "cannot find libasan", "cannot find libubsan",
                                            "libasan_preinit.o: No such file", "libclang_rt.asan", "libclang_rt.ubsan"))
    if r.returncode != 0 and no_runtime:                           # only a missing sanitizer runtime lets the plain program stand in
        r = subprocess.run([gxx, *flags, *sources, "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe), str(cases.GOLDEN)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "16 fixtures (13 plans, 2 for the host route)" in r.stdout and "2000 corruptions" in r.stdout, r.stdout
