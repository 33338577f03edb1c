"""Restart-interval JPEG on the host: the interval plan (gtx_jpeg_plan_intervals), the numpy twin of csrc/jpeg_restart.hip with
every index asserted, and the host emitter with restart markers (gtx_jpeg_emit_restart). No GPU. Records are compared for
equality; there is no tolerance anywhere."""
import io

import numpy as np
import pytest
from jpeg_entropy_cases import fixture_bytes
from jpeg_restart_cases import RESTART_FIXTURES, damaged, frames, marker_positions, records, restarts_of

from geotrax_amd import jpeg


def _status(e):
    return e.code


@pytest.mark.parametrize("name", RESTART_FIXTURES)
def test_the_twin_on_a_committed_fixture_is_the_parsers_record(name):
    b = fixture_bytes(name)
    plan = jpeg.restart_plan(b)
    status, rec = jpeg.restart_decode_twin(plan)
    assert status == 0 and rec.tobytes() == jpeg.parse(b)[0].tobytes()
    assert jpeg.entropy_plan(b) is None                           # the older route still hands the frame back


@pytest.mark.parametrize("name", RESTART_FIXTURES)
def test_each_lane_alone_reproduces_its_blocks(name):
    b = fixture_bytes(name)
    plan = jpeg.restart_plan(b)
    f, _, _, start, _ = jpeg.restart_plan_fields(plan)
    ref_f, _, off, coefs = jpeg.record_fields(jpeg.parse(b)[0])
    bpm = f["hs"] * f["vs"] + 2
    seen = 0
    for i in reversed(range(f["n_intervals"])):                   # any order: a lane needs nothing from the others
        bad, b0, dense, lens = jpeg.restart_lane_twin(plan, i)
        assert not bad and b0 == i * f["restart"] * bpm
        for j in range(len(lens)):
            want = coefs[off[b0 + j]:off[b0 + j + 1]]
            assert lens[j] == len(want) and (dense[j, :lens[j]] == want).all() and not dense[j, lens[j]:].any()
        seen += len(lens)
    assert seen == ref_f["n_blocks"] and int(start[-1]) == f["stream_bytes"]


@pytest.mark.parametrize("label", sorted(frames()))
def test_emit_with_restarts_round_trips_through_the_parser_and_the_twin(label):
    rec, blob = frames()[label]
    assert jpeg.parse(blob)[0].tobytes() == rec.tobytes()
    plan = jpeg.restart_plan(blob)
    status, got = jpeg.restart_decode_twin(plan)
    assert status == 0 and got.tobytes() == rec.tobytes()


def test_the_smallest_interval_on_70x45_wraps_past_rst7_and_the_last_interval_is_short():
    rec, blob = frames()["420_70x45_r1"]
    f = jpeg.restart_plan_fields(jpeg.restart_plan(blob))[0]
    assert f["n_intervals"] == 15 and [blob[p + 1] & 7 for p in marker_positions(blob)] == [0, 1, 2, 3, 4, 5, 6, 7, 0, 1, 2, 3, 4, 5]
    f3 = jpeg.restart_plan_fields(jpeg.restart_plan(frames()["420_70x45_r3"][1]))[0]
    assert f3["n_intervals"] == 5
    f4 = jpeg.restart_plan_fields(jpeg.restart_plan(frames()["420_70x45_r4"][1]))[0]   # 15 MCUs in intervals of 4: the last holds 3
    assert f4["n_intervals"] == 4
    f_all = jpeg.restart_plan_fields(jpeg.restart_plan(frames()["420_70x45_r20"][1]))[0]   # more than the frame: one interval, no marker
    assert f_all["n_intervals"] == 1 and f_all["restart"] == 20


@pytest.mark.parametrize("name", sorted(n for n in records() if not n.startswith("hand_") and n not in ("empty_interval", "no_eob")))
def test_pillow_decodes_the_restart_file_to_the_same_pixels(name):
    from PIL import Image

    rec = records()[name]
    want = np.asarray(Image.open(io.BytesIO(jpeg.emit(rec, 0))))
    for r in restarts_of(rec):
        np.testing.assert_array_equal(np.asarray(Image.open(io.BytesIO(jpeg.emit(rec, r)))), want)


def test_emit_without_restarts_is_the_emitter_as_it_was_and_large_intervals_are_refused():
    for rec in records().values():
        assert jpeg.emit(rec, 0) == jpeg.emit(rec) == jpeg.record_to_bytes(rec)
    rec = records()["420_17x9"]
    assert b"\xff\xdd\x00\x04\xff\xff" in jpeg.emit(rec, 65535)
    with pytest.raises(jpeg.JpegError) as e:
        jpeg.emit(rec, 65536)
    assert _status(e.value) == -1


def test_hand_built_records_an_empty_interval_and_a_block_without_eob():
    rec, blob = frames()["empty_interval_r1"]
    plan = jpeg.restart_plan(blob)
    _, _, _, start, _ = jpeg.restart_plan_fields(plan)
    # six empty blocks after a reset, Annex K.3: luma DC category 0 (00) + EOB (1010) four times, chroma 00 + 00 twice: 32 bits
    assert int(start[3]) - int(start[2]) == 4
    bad, _, dense, lens = jpeg.restart_lane_twin(plan, 2)
    assert not bad and not dense.any() and not lens.any()
    rec, blob = frames()["no_eob_r1"]
    bad, _, dense, lens = jpeg.restart_lane_twin(jpeg.restart_plan(blob), 1)
    assert not bad and lens.tolist() == [64, 0, 64] and dense[0, 63] == -1


@pytest.mark.parametrize("label", sorted(damaged()))
def test_damaged_data_gets_the_parsers_verdict(label):
    blob = damaged()[label]
    with pytest.raises(jpeg.JpegError) as want:
        jpeg.parse(blob)
    try:
        plan = jpeg.restart_plan(blob)
    except jpeg.JpegError as e:                                   # the plan walk: parse()'s status and message
        assert _status(e) == _status(want.value) and str(e) == str(want.value)
        assert label.startswith(("out_of_sequence", "missing"))
        return
    status, rec = jpeg.restart_decode_twin(plan)                  # the markers stand where the walk needs them: the bits do not add up
    assert status != 0 and rec is None
    assert label in ("truncated_last", "stray_byte")


def test_the_messages_of_the_marker_rules():
    for label, text in (("out_of_sequence", "restart markers out of sequence: FFD6 where RST4 belongs"),
                        ("out_of_sequence_after_wrap", "FFD2 where RST1 belongs")):
        with pytest.raises(jpeg.JpegError, match=text):
            jpeg.restart_plan(damaged()[label])


def test_a_frame_without_dri_and_a_progressive_frame():
    lib = jpeg._lib.load()
    assert jpeg.restart_plan(fixture_bytes("p70x45_420")) is None
    raw = fixture_bytes("p70x45_420")
    buf = np.frombuffer(raw, np.uint8)
    import ctypes as C
    needed = C.c_size_t(7)
    rc = lib.gtx_jpeg_plan_intervals(jpeg._lib.ptr(buf), len(raw), 0, None, None, None, None, None, None, 0, C.byref(needed))
    assert rc == jpeg.NO_RESTART == 3 and needed.value == 0
    with pytest.raises(jpeg.JpegError) as want:
        jpeg.parse(fixture_bytes("p70x45_progressive"))
    with pytest.raises(jpeg.JpegError) as got:
        jpeg.restart_plan(fixture_bytes("p70x45_progressive"))
    assert str(got.value) == str(want.value) and _status(got.value) == _status(want.value) == -3


def _check(plan):
    """gtx_op_jpeg_restart refuses a bad plan before it needs a context: the refusal is check_plan_intervals'."""
    import ctypes as C
    lib = jpeg._lib.load()
    p = np.concatenate([plan, np.zeros(0, np.uint8)]).copy()
    p = np.frombuffer(p.tobytes() + b"\0" * 3, np.uint8)[:len(plan)]
    n, status = C.c_size_t(), C.c_int()
    rc = lib.gtx_op_jpeg_restart(None, jpeg._lib.ptr(p), p.nbytes, None, 0, C.byref(n), C.byref(status))
    return rc, lib.gtx_last_error().decode()


def test_check_plan_intervals_refuses_what_the_kernel_could_not_bound():
    plan = jpeg.restart_plan(fixture_bytes("p70x45_420_rst3"))
    rc, msg = _check(plan)
    assert rc == -1 and "ctx" in msg                              # a good plan gets as far as the missing context
    bad = plan.copy()
    bad[jpeg.PLAN_STREAM_OFFSET + 8:jpeg.PLAN_STREAM_OFFSET + 12].view(np.uint32)[0] = 5       # start[2] < start[1]
    rc, msg = _check(bad)
    assert rc == -1 and "monotone" in msg
    bad = plan.copy()
    bad[:112].view(np.uint32)[24] = 4                             # n_intervals: 5 for 15 MCUs in intervals of 3
    rc, msg = _check(bad)
    assert rc == -1 and "interval count" in msg
    bad = plan.copy()
    bad[:112].view(np.uint32)[16] = 4                             # restart 4: ceil(15 / 4) = 4 intervals, the plan holds 5
    assert _check(bad)[0] == -1 and "interval count" in _check(bad)[1]
    rc, msg = _check(plan[:len(plan) - 4])
    assert rc == -1 and "length" in msg
    assert _check(plan[:64])[0] == -1
    ordinary = jpeg.entropy_plan(fixture_bytes("p70x45_420"))
    assert _check(ordinary)[0] == -1 and "magic" in _check(ordinary)[1]
    import ctypes as C
    lib = jpeg._lib.load()
    n, status, used = C.c_size_t(), C.c_int(), C.c_int()
    rc = lib.gtx_op_jpeg_entropy(None, jpeg._lib.ptr(plan), plan.nbytes, 0, 0, None, 0, C.byref(n), C.byref(status), C.byref(used))
    assert rc == -1 and "magic" in lib.gtx_last_error().decode()   # check_plan goes on refusing the new format


def test_plan_intervals_bound_holds_every_plan():
    lib = jpeg._lib.load()
    assert lib.gtx_jpeg_plan_intervals_bound(0, 5) == 0 and lib.gtx_jpeg_plan_intervals_bound(16385, 5) == 0
    for label, (_, blob) in frames().items():
        plan = jpeg.restart_plan(blob)
        f = jpeg.restart_plan_fields(plan)[0]
        assert plan.nbytes <= lib.gtx_jpeg_plan_intervals_bound(f["h"], f["w"]), label


def test_recode_with_restarts_on_the_640x360_fixture_is_lossless():
    b = fixture_bytes("w640x360_420")
    want = jpeg.parse(b)[0]
    row = jpeg.mcus_per_row(b)
    assert row == 40
    for r in (row, 8):
        out = jpeg.recode_with_restarts(b, r)
        assert jpeg.parse(out)[0].tobytes() == want.tobytes()
        plan = jpeg.restart_plan(out)
        assert jpeg.restart_plan_fields(plan)[0]["n_intervals"] == -(-40 * 23 // r)
    status, rec = jpeg.restart_decode_twin(jpeg.restart_plan(jpeg.recode_with_restarts(b, row)))
    assert status == 0 and rec.tobytes() == want.tobytes()
    assert jpeg.recode_with_restarts(b, 0) == jpeg.record_to_bytes(want)


def test_mjpeg_writer_writes_restart_frames_through_the_host_emitter(tmp_path):
    from geotrax_amd.video_writer import MjpegWriter

    rec = records()["420_70x45"]
    w = MjpegWriter(tmp_path / "a.mjpeg", 25, (70, 45), restart_interval=5)
    w.write_record(rec)
    w.write_record(rec)
    w.release()
    assert (tmp_path / "a.mjpeg").read_bytes() == 2 * jpeg.emit(rec, 5)
    with pytest.raises(ValueError, match="host emitter"):
        MjpegWriter(tmp_path / "b.mjpeg", 25, (70, 45), entropy="gpu", restart_interval=5)
    with pytest.raises(ValueError, match="65535"):
        MjpegWriter(tmp_path / "c.mjpeg", 25, (70, 45), restart_interval=65536)


def test_the_stages_take_a_restart_interval_and_refuse_it_with_the_gpu_coder(tmp_path):
    from geotrax_amd import stabilized_video, visualize
    from geotrax_amd.video_writer import check_restart_interval

    assert check_restart_interval("host", 8) == 8 and check_restart_interval("gpu", 0) == 0
    for main in (stabilized_video.main, visualize.main):
        with pytest.raises(ValueError, match="host emitter"):
            main([str(tmp_path / "none.mjpeg"), "--entropy", "gpu", "--restart-interval", "8"])
        with pytest.raises(ValueError, match="65535"):
            main([str(tmp_path / "none.mjpeg"), "--restart-interval", "65536"])
    with pytest.raises(ValueError, match="host emitter"):
        stabilized_video.write_stabilized(tmp_path / "none.mjpeg", entropy="gpu", restart_interval=8)


def test_the_recode_command_line_on_a_clip_and_a_folder(tmp_path):
    from geotrax_amd import jpeg_restart
    from geotrax_amd.frames import open_source

    b = fixture_bytes("w640x360_420")
    small = [frames()[k][1] for k in ("420_70x45_r20", "420_70x45_r1")]   # the second has markers already: they are replaced
    clip = tmp_path / "in.mjpeg"
    clip.write_bytes(b + b)
    assert jpeg_restart.main([str(clip), str(tmp_path / "rows.mjpeg"), "--rows", "1"]) == 0
    assert (tmp_path / "rows.mjpeg").read_bytes() == 2 * jpeg.recode_with_restarts(b, 40)
    assert jpeg_restart.main([str(clip), str(tmp_path / "mcus.avi"), "--mcus", "8"]) == 0
    src = open_source(tmp_path / "mcus.avi")
    paths, findex, off, ln = src.jpeg_layout()
    src.release()
    data = (tmp_path / "mcus.avi").read_bytes()
    assert len(off) == 2 and all(data[int(o):int(o) + int(n)] == jpeg.recode_with_restarts(b, 8) for o, n in zip(off, ln))
    folder = tmp_path / "dir"
    folder.mkdir()
    for i, s in enumerate(small):
        (folder / f"f{i}.jpg").write_bytes(s)
    assert jpeg_restart.main([str(folder), str(tmp_path / "out"), "--rows", "2", "--threads", "2"]) == 0
    for i, s in enumerate(small):
        got = (tmp_path / "out" / f"f{i}.jpg").read_bytes()
        assert got == jpeg.recode_with_restarts(s, 10) and jpeg.parse(got)[0].tobytes() == jpeg.parse(s)[0].tobytes()
    assert jpeg_restart.main([str(clip), str(tmp_path / "bad.mjpeg"), "--mcus", "70000"]) == 1
    assert jpeg_restart.main([str(tmp_path / "absent.mjpeg"), str(tmp_path / "x.mjpeg"), "--rows", "1"]) == 1
    with pytest.raises(SystemExit):
        jpeg_restart.main([str(clip), str(tmp_path / "x.mjpeg")])
