"""The JPEG frame source on the host: csrc/jpeg_parse.cpp (gtx_jpeg_parse) + the numpy twin of the kernels (geotrax_amd/jpeg.py)
against Pillow's stored decode of every fixture (tests/golden/jpeg, written by tests/golden/make_jpeg.py), byte for byte; what is
refused, with the marker named; truncations and corruptions; the three readers' indexes; the parser under the sanitizers as a
stand-alone program. No GPU, no Pillow."""
import shutil
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden" / "jpeg"
ACCEPTED = ["b8x8_444", "m16x16_420", "r17x9_420", "r33x16_422", "p70x45_444", "p70x45_422", "p70x45_420", "g9x6_gray", "p70x45_420_opt",
            "p70x45_420_rst3", "p70x45_420_rstrow", "p70x45_420_q100", "p70x45_420_q5", "w640x360_420", "t3x5_420"]


def fixture(name: str) -> bytes:
    return (GOLDEN / f"{name}.jpg").read_bytes()


def expected(name: str) -> np.ndarray:
    return np.load(GOLDEN / f"{name}.npy")


def segments(data: bytes):
    """(marker, start of the FF, end of the segment) of the header segments up to and including SOS."""
    at, out = 2, []
    while True:
        m, n = data[at + 1], struct.unpack(">H", data[at + 2:at + 4])[0]
        out.append((m, at, at + 2 + n))
        if m == 0xDA:
            return out
        at += 2 + n


def with_thumbnail(data: bytes, thumb: bytes) -> bytes:
    """`data` with an APP1 segment right after SOI that embeds a whole JPEG picture (its own SOI, SOS, EOI)."""
    body = b"Exif\0\0" + thumb
    return data[:2] + b"\xff\xe1" + struct.pack(">H", len(body) + 2) + body + data[2:]


def write_mjpeg(path, frames) -> None:
    Path(path).write_bytes(b"".join(frames))


def write_avi(path, frames, hw, fourcc=b"MJPG", split=None) -> None:
    """A minimal AVI: hdrl with one video stream (`fourcc`) and one audio stream, movi with 00dc chunks and a 01wb chunk in
    between; frames from index `split` on go into a second RIFF 'AVIX' list."""
    def chunk(cid, body):
        return cid + struct.pack("<I", len(body)) + body + (b"\0" if len(body) & 1 else b"")

    def lst(kind, body, cid=b"LIST"):
        return cid + struct.pack("<I", len(body) + 4) + kind + body

    h, w = hw
    strh_v = b"vids" + fourcc + struct.pack("<IHHIIIIIIIIhhhh", 0, 0, 0, 0, 1001, 30000, 0, len(frames), 0, 0, 0, 0, 0, w, h)
    strf_v = struct.pack("<IiiHH4sIiiII", 40, w, h, 1, 24, fourcc, w * h * 3, 0, 0, 0, 0)
    strh_a = b"auds" + b"\0\0\0\0" + struct.pack("<IHHIIIIIIIIhhhh", 0, 0, 0, 0, 1, 8000, 0, 1, 0, 0, 1, 0, 0, 0, 0)
    strf_a = struct.pack("<HHIIHH", 1, 1, 8000, 8000, 1, 8)
    hdrl = lst(b"hdrl", chunk(b"avih", bytes(56)) + lst(b"strl", chunk(b"strh", strh_v) + chunk(b"strf", strf_v))
               + lst(b"strl", chunk(b"strh", strh_a) + chunk(b"strf", strf_a)))
    split = len(frames) if split is None else split

    def movi(fr, audio):
        body = b""
        for k, f in enumerate(fr):
            body += chunk(b"00dc", f)
            if audio and k == 0:
                body += chunk(b"01wb", bytes(801))            # odd length: padded
        return lst(b"movi", body)

    out = lst(b"AVI ", hdrl + movi(frames[:split], True) + chunk(b"idx1", bytes(32)), cid=b"RIFF")
    if split < len(frames):
        out += lst(b"AVIX", movi(frames[split:], False), cid=b"RIFF")
    Path(path).write_bytes(out)


# ---------------------------------------------------------------------------------------------- decode


@pytest.mark.parametrize("name", ACCEPTED)
def test_parser_and_twin_equal_pillow_byte_for_byte(name):
    from geotrax_amd import jpeg

    want = expected(name)
    rec, info = jpeg.parse(fixture(name))
    assert (info["h"], info["w"]) == want.shape[:2]
    got = jpeg.record_to_bgr(rec)
    diff = np.abs(got.astype(int) - want.astype(int)).reshape(-1, 3).max(0)
    print(f"{name}: record {rec.nbytes} bytes for a {len(fixture(name))}-byte file, largest difference per channel {diff}")
    np.testing.assert_array_equal(got, want)                   # libjpeg's decode is documented integer arithmetic: no tolerance


def test_a_frame_without_dht_decodes_with_the_annex_k_tables():
    """Motion-JPEG frames may leave DHT out. Pillow writes exactly the Annex K.3 tables when it does not optimise, so the
    fixture minus its DHT segments must decode to the same picture."""
    from geotrax_amd import jpeg

    data = fixture("p70x45_420")
    cut = [(a, b) for m, a, b in segments(data) if m == 0xC4]
    assert cut
    bare = data
    for a, b in reversed(cut):
        bare = bare[:a] + bare[b:]
    assert b"\xff\xc4" not in bare[:segments(bare)[-1][2]]
    np.testing.assert_array_equal(jpeg.decode_host(bare), expected("p70x45_420"))
    # ... and an optimised frame's codes are not Annex K's: with its DHT gone it must not decode to its picture
    opt = fixture("p70x45_420_opt")
    for a, b in reversed([(a, b) for m, a, b in segments(opt) if m == 0xC4]):
        opt = opt[:a] + opt[b:]
    try:
        assert not np.array_equal(jpeg.decode_host(opt), expected("p70x45_420_opt"))
    except jpeg.JpegError:
        pass


def test_avi1_app0_thumbnails_and_comments_are_stepped_over():
    from geotrax_amd import jpeg

    data = fixture("p70x45_420")
    avi1 = b"\xff\xe0" + struct.pack(">H", 16) + b"AVI1" + bytes(10)          # what ffmpeg's mjpeg encoder writes instead of JFIF
    com = b"\xff\xfe" + struct.pack(">H", 9) + b"Lavc60."
    dressed = with_thumbnail(data[:2] + avi1 + com + data[2:], fixture("b8x8_444"))
    np.testing.assert_array_equal(jpeg.decode_host(dressed), expected("p70x45_420"))


def _edit_sof(data: bytes, **kw) -> bytes:
    m, a, b = next(s for s in segments(data) if s[0] == 0xC0)
    d = bytearray(data)
    if "precision" in kw:
        d[a + 4] = kw["precision"]
    if "ncomp" in kw:
        d[a + 9] = kw["ncomp"]
    if "luma" in kw:
        d[a + 11] = kw["luma"]
    return bytes(d)


def _rgb_ids(data: bytes) -> bytes:
    """The frame without its JFIF APP0 and with component ids 'R', 'G', 'B' in SOF0 and SOS: what libjpeg reads as RGB data."""
    d = bytearray(data)
    sof, sos = (next(s for s in segments(data) if s[0] == m) for m in (0xC0, 0xDA))
    for c, ch in enumerate(b"RGB"):
        d[sof[1] + 10 + 3 * c] = ch
        d[sos[1] + 5 + 2 * c] = ch
    app0 = next(s for s in segments(data) if s[0] == 0xE0)
    return bytes(d[:app0[1]] + d[app0[2]:])


def test_what_is_refused_names_its_marker_and_frame():
    from geotrax_amd import jpeg

    data = fixture("p70x45_420")
    dqt = next(s for s in segments(data) if s[0] == 0xDB)
    dqt16 = bytearray(data)
    dqt16[dqt[1] + 4] |= 0x10
    sos = next(s for s in segments(data) if s[0] == 0xDA)
    one_comp_scan = data[:sos[1]] + b"\xff\xda" + struct.pack(">H", 8) + bytes([1]) + data[sos[1] + 5:sos[1] + 7] + bytes([0, 63, 0]) + data[sos[2]:]
    adobe_rgb = data[:2] + b"\xff\xee" + struct.pack(">H", 14) + b"Adobe" + bytes([0, 100, 0, 0, 0, 0, 0]) + data[2:]
    cases = [
        (fixture("p70x45_progressive"), "SOF2"),
        (_edit_sof(data, precision=12), "SOF0 with 12-bit"),
        (_edit_sof(data, ncomp=4), "SOF0 with four components"),
        (bytes(dqt16), "DQT with 16-bit"),
        (_edit_sof(data, luma=0x12), "sampling 1x2"),                           # 4:4:0
        (_edit_sof(data, luma=0x41), "sampling 4x1"),                           # 4:1:1
        (bytes(one_comp_scan), "SOS with 1 of 3 components"),
        (adobe_rgb, "APP14 Adobe transform 0"),
        (data.replace(b"\xff\xc0", b"\xff\xc9", 1), "SOF9 (arithmetic"),
        (data.replace(b"\xff\xc0", b"\xff\xc1", 1), "SOF1"),
        (_rgb_ids(data), "component ids 'R', 'G', 'B'"),
    ]
    for bad, what in cases:
        with pytest.raises(jpeg.JpegError) as e:
            jpeg.parse(bad, frame=7)
        assert e.value.code == -3 and what in str(e.value) and "frame 7" in str(e.value), (what, str(e.value))


def test_record_protocol_and_the_host_check_before_any_launch():
    import ctypes as C

    from geotrax_amd import _lib, jpeg

    lib = _lib.load()
    data = np.frombuffer(fixture("r17x9_420"), np.uint8)
    rec, info = jpeg.parse(data.tobytes())
    assert rec.nbytes <= lib.gtx_jpeg_record_bound(9, 17) and lib.gtx_jpeg_record_bound(0, 5) == 0
    needed, h = C.c_size_t(), C.c_int()
    small = np.full(rec.nbytes, 0xAB, np.uint8)
    rc = lib.gtx_jpeg_parse(_lib.ptr(data), len(data), 0, C.byref(h), None, None, None, None, _lib.ptr(small), rec.nbytes - 2, C.byref(needed))
    assert rc == 1 and needed.value == rec.nbytes and h.value == 9 and small[-2:].tolist() == [0xAB, 0xAB]
    # gtx_jpeg_decode_dev checks the record on the host, before it asks for a context: damaged offsets never reach a kernel
    f, quant, offsets, coefs = jpeg.record_fields(rec)
    for edit, what in [(lambda r: r[jpeg.OFFSETS_OFFSET + 4:jpeg.OFFSETS_OFFSET + 8].view(np.uint32).__setitem__(0, 2 ** 31), "monotone"),
                       (lambda r: r[jpeg.OFFSETS_OFFSET + 4 * f["n_blocks"]:][:4].view(np.uint32).__setitem__(0, f["n_coef"] - 1), "closing offset"),
                       (lambda r: r[:80].view(np.uint32).__setitem__(9, f["n_blocks"] + 64), "block count")]:
        bad = rec.copy()
        edit(bad)
        assert lib.gtx_jpeg_decode_dev(None, _lib.ptr(bad), bad.nbytes, 9, 17, None) == -1 and what.encode() in lib.gtx_last_error(), what
    assert lib.gtx_jpeg_decode_dev(None, _lib.ptr(rec), rec.nbytes, 9, 18, None) == -1 and b"frame size" in lib.gtx_last_error()
    assert lib.gtx_jpeg_decode_dev(None, _lib.ptr(rec), rec.nbytes, 9, 17, None) == -1 and b"ctx is NULL" in lib.gtx_last_error()   # the record was fine


def test_every_truncation_fails_cleanly_or_decodes_whole():
    from geotrax_amd import jpeg

    data, want = fixture("r17x9_420"), expected("r17x9_420")
    decoded = 0
    for n in range(len(data)):
        try:
            got = jpeg.decode_host(data[:n])
        except jpeg.JpegError as e:
            assert e.code in (-1, -3) and "frame 0" in str(e)
            assert n < len(data) - 2, f"cut to {n} of {len(data)} bytes: only the EOI is missing, the picture is complete"
            continue
        np.testing.assert_array_equal(got, want)               # never a partial picture
        assert n >= len(data) - 2
        decoded += 1
    assert decoded == 2


def test_seeded_corruptions_fail_or_decode_to_the_right_size():
    from geotrax_amd import jpeg

    data = bytearray(fixture("p70x45_420_rst3"))
    rng = np.random.default_rng(2000)
    ok = failed = 0
    for k in range(2000):
        at = int(rng.integers(len(data)))
        was = data[at]
        data[at] = was ^ int(rng.integers(1, 256))
        try:
            rec, info = jpeg.parse(bytes(data))
            f, quant, offsets, coefs = jpeg.record_fields(rec)
            assert (f["h"], f["w"]) == (info["h"], info["w"]) and len(coefs) == f["n_coef"] == int(offsets[-1])
            assert np.all(np.diff(offsets.astype(np.int64)) >= 0) and np.all(np.diff(offsets.astype(np.int64)) <= 64)
            if ok % 10 == 0:
                assert jpeg.record_to_bgr(rec).shape == (info["h"], info["w"], 3)
            ok += 1
        except jpeg.JpegError as e:
            assert str(e)
            failed += 1
        data[at] = was
    assert ok > 100 and failed > 100, (ok, failed)             # both outcomes are exercised


def test_restart_markers_out_of_sequence_fail_the_frame():
    from geotrax_amd import jpeg

    data = fixture("p70x45_420_rstrow")
    scan = segments(data)[-1][2]
    k = data.index(b"\xff\xd1", scan)
    with pytest.raises(jpeg.JpegError, match="out of sequence"):
        jpeg.parse(data[:k] + b"\xff\xd3" + data[k + 2:])


def test_parser_runs_clean_under_the_sanitizers_as_a_program_of_its_own(tmp_path):
    """csrc/diag/jpeg_parse_check.cpp + csrc/jpeg_parse.cpp built with -fsanitize=address,undefined and run directly (nothing is
    loaded into this interpreter): fixtures, every truncation, 2 000 corruptions, with inputs and records in exact-size blocks."""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the stand-alone parser check"
    src = ROOT / "geo-trax_amd" / "csrc"
    exe = tmp_path / "jpeg_parse_check"
    flags = ["-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer"]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    sources = [str(src / "jpeg_parse.cpp"), str(src / "diag" / "jpeg_parse_check.cpp")]
    r = subprocess.run([gxx, *flags, *san, *sources, "-o", str(exe)], capture_output=True, text=True)
    sanitized = r.returncode == 0
    # only a missing sanitizer runtime (the linker cannot find libasan / libubsan) lets the plain program stand in; it still
    # checks every result, and the output says which build ran. Any other compiler error fails the test.
    no_runtime = any(t in r.stderr for t in ("cannot find -lasan", "cannot find -lubsan", "cannot find libasan", "cannot find libubsan",
                                            "libasan_preinit.o: No such file", "libclang_rt.asan", "libclang_rt.ubsan"))
    if not sanitized and no_runtime:
        r = subprocess.run([gxx, *flags, *sources, "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    print("jpeg_parse_check built " + ("with -fsanitize=address,undefined" if sanitized else "WITHOUT the sanitizers (their runtime is not installed)"))
    r = subprocess.run([str(exe), str(GOLDEN)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "2000 corruptions" in r.stdout, r.stdout + r.stderr


# ---------------------------------------------------------------------------------------------- readers

CLIP = ["p70x45_420", "p70x45_420_opt", "p70x45_420_rst3"]


def _clip_frames():
    fr = [fixture(n) for n in CLIP] * 2
    fr[1] = with_thumbnail(fr[1], fixture("b8x8_444"))          # an embedded picture with its own SOI / EOI inside APP1
    return fr, [expected(n) for n in CLIP] * 2


def _check_reader(r, want, n):
    assert r.frame_count == n and r.frame_hw == (45, 70) and r.raw_layout() is None
    paths, idx, off, ln = r.jpeg_layout()
    assert len(idx) == len(off) == len(ln) == n
    for k in range(n):
        ok, f = r.read()
        assert ok
        np.testing.assert_array_equal(f, want[k])
    assert r.read() == (False, None)
    r.seek(n - 2)
    np.testing.assert_array_equal(r.read()[1], want[n - 2])
    r.release()
    return paths, idx, off, ln


def test_mjpeg_reader_indexes_by_walking_segments(tmp_path, caplog):
    from geotrax_amd.frames import MjpegReader, open_source

    frames, want = _clip_frames()
    path = tmp_path / "clip.mjpeg"
    write_mjpeg(path, frames)
    r = open_source(path)
    assert isinstance(r, MjpegReader)
    paths, idx, off, ln = _check_reader(r, want, 6)
    assert paths == [str(path)] and ln.tolist() == [len(f) for f in frames] and off.tolist() == np.cumsum([0] + [len(f) for f in frames[:-1]]).tolist()
    # a file that ends inside a frame plays the complete frames before it, with a warning
    cut = tmp_path / "cut.mjpg"
    write_mjpeg(cut, frames + [frames[0][:700]])
    with caplog.at_level("WARNING"):
        r = open_source(cut)
    assert r.frame_count == 6 and "complete frames" in caplog.text
    r.release()
    prog = tmp_path / "prog.mjpeg"
    write_mjpeg(prog, [fixture("p70x45_progressive")])
    with pytest.raises(Exception, match="SOF2"):
        open_source(prog)
    none = tmp_path / "none.mjpeg"
    none.write_bytes(frames[0][:500])
    with pytest.raises(ValueError):
        open_source(none)


def test_avi_mjpeg_reader_walks_movi_lists_and_skips_audio(tmp_path, caplog):
    from geotrax_amd.frames import AviMjpegReader, open_source

    frames, want = _clip_frames()
    path = tmp_path / "clip.avi"
    write_avi(path, frames, (45, 70), split=4)                   # four frames in RIFF 'AVI ', two in RIFF 'AVIX'
    r = open_source(path)
    assert isinstance(r, AviMjpegReader) and abs(r.fps - 30000 / 1001) < 1e-9
    paths, idx, off, ln = _check_reader(r, want, 6)
    raw = path.read_bytes()
    assert [raw[o:o + n] for o, n in zip(off.tolist(), ln.tolist())] == frames
    cut = tmp_path / "cut.avi"
    cut.write_bytes(raw[:int(off[5]) + 100])
    with caplog.at_level("WARNING"):
        r = open_source(cut)
    assert r.frame_count == 5 and "complete frames" in caplog.text
    r.release()


def test_an_avi_with_another_codec_keeps_todays_behaviour(tmp_path):
    from geotrax_amd.frames import Cv2Reader, avi_is_mjpeg, open_source

    path = tmp_path / "clip.avi"
    write_avi(path, [bytes(64)] * 2, (45, 70), fourcc=b"H264")
    assert not avi_is_mjpeg(path)
    try:
        import cv2  # noqa: F401
    except ImportError:
        with pytest.raises(RuntimeError, match="video decoder"):
            open_source(path)
    else:
        assert isinstance(open_source(path), Cv2Reader)


def test_a_folder_of_jpegs_exposes_a_layout_and_other_folders_do_not(tmp_path):
    from geotrax_amd.frames import DirReader, open_source

    frames, want = _clip_frames()
    d = tmp_path / "frames"
    d.mkdir()
    for k, f in enumerate(frames):
        (d / f"f{k:03d}.jpg").write_bytes(f)
    r = open_source(d)
    assert isinstance(r, DirReader) and r.frame_count == 6 and r.raw_layout() is None
    paths, idx, off, ln = r.jpeg_layout()
    assert [Path(p).name for p in paths] == [f"f{k:03d}.jpg" for k in range(6)] and idx.tolist() == list(range(6)) and not off.any()
    assert ln.tolist() == [len(f) for f in frames]
    # a progressive picture among them, or a frame of another kind: the folder keeps its Pillow route
    (d / "f006.jpg").write_bytes(fixture("p70x45_progressive"))
    assert open_source(d).jpeg_layout() is None
    (d / "f006.jpg").write_bytes(_rgb_ids(frames[0]))           # libjpeg reads this one as RGB: one rule set, the C parser's
    assert open_source(d).jpeg_layout() is None
    sos = next(s for s in segments(frames[0]) if s[0] == 0xDA)
    swapped = bytearray(frames[0])
    swapped[sos[1] + 5], swapped[sos[1] + 7] = swapped[sos[1] + 7], swapped[sos[1] + 5]      # scan lists the components in another order
    (d / "f006.jpg").write_bytes(bytes(swapped))
    assert open_source(d).jpeg_layout() is None
    (d / "f006.jpg").unlink()
    np.save(d / "f006.npy", want[0])
    assert open_source(d).jpeg_layout() is None


def test_batch_lists_the_new_suffixes():
    from geotrax_amd.batch import VIDEO_FORMATS

    assert {".mjpeg", ".mjpg", ".avi"} <= VIDEO_FORMATS
