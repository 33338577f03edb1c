"""The JPEG frame sink on the host (no GPU): the numpy twin of the encoder against Pillow / libjpeg-turbo coefficient for
coefficient, the emitter (csrc/jpeg_emit.cpp) round-tripping every fixture and reproducing Pillow's entropy-coded bytes, the
MJPG .avi / .mjpeg containers read back by the existing readers, the refusals, and the emitter under the sanitizers as a program
of its own."""
import ctypes as C
import io
import shutil
import subprocess

import numpy as np
import pytest
from PIL import Image
from test_jpeg import ACCEPTED, GOLDEN, ROOT, expected, fixture

SIZES = [(1, 1), (8, 8), (16, 16), (17, 23), (33, 15), (640, 360)]           # width x height
QUALITIES = [5, 50, 90, 100]
SUBSAMPLINGS = ["4:2:0", "4:4:4"]


def inputs(w: int, h: int) -> dict:
    """The test frames of one size, BGR: seeded noise, flat 128 / 0 / 255, a horizontal ramp, the synthetic scene."""
    from geotrax_amd.synth import make_scene

    rng = np.random.default_rng(1000 * w + h)
    ramp = (np.arange(w) * 255 // max(w - 1, 1)).astype(np.uint8)
    scene = make_scene(seed=0, h=max(h, 64), w=max(w, 64)).render(0)[:h, :w]
    return dict(noise=rng.integers(0, 256, (h, w, 3), dtype=np.uint8), flat128=np.full((h, w, 3), 128, np.uint8), flat0=np.zeros((h, w, 3), np.uint8),
                flat255=np.full((h, w, 3), 255, np.uint8), ramp=np.ascontiguousarray(np.broadcast_to(ramp[None, :, None], (h, w, 3))),
                scene=np.ascontiguousarray(scene))


def pillow_jpeg(bgr: np.ndarray, quality: int, subsampling: str) -> bytes:
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(bgr[..., ::-1])).save(buf, "JPEG", quality=quality, subsampling=subsampling, optimize=False)
    return buf.getvalue()


def scan_bytes(data: bytes) -> bytes:
    """The entropy-coded bytes between the SOS header and EOI."""
    at = 2
    while data[at + 1] != 0xDA:
        at += 2 + ((data[at + 2] << 8) | data[at + 3])
    at += 2 + ((data[at + 2] << 8) | data[at + 3])
    assert data[-2:] == b"\xff\xd9"
    return data[at:-2]


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_twin_equals_pillow_coefficient_for_coefficient(size):
    """bgr_to_record against the record the parser reads out of Pillow's file for the same pixels: quantisation tables, block
    offsets and coefficients are equal (libjpeg-turbo's slow-integer paths equal libjpeg's C definition, which the twin restates);
    and the emitter's entropy-coded bytes for the twin's record are Pillow's."""
    from geotrax_amd import jpeg

    w, h = size
    for name, bgr in inputs(w, h).items():
        for q in QUALITIES:
            for s in SUBSAMPLINGS:
                ref = pillow_jpeg(bgr, q, s)
                want, _ = jpeg.parse(ref)
                got = jpeg.bgr_to_record(bgr, q, s)
                fw, qw, ow, cw = jpeg.record_fields(want)
                fg, qg, og, cg = jpeg.record_fields(got)
                where = f"{w}x{h} {name} q{q} {s}"
                assert fg == fw, where
                np.testing.assert_array_equal(qg, qw, err_msg=where)
                np.testing.assert_array_equal(og, ow, err_msg=where)
                np.testing.assert_array_equal(cg, cw, err_msg=where)
                assert got.tobytes() == want.tobytes(), where
                if name in ("noise", "scene", "flat128") and (q in (5, 90) or w < 100):
                    assert scan_bytes(jpeg.record_to_bytes(got)) == scan_bytes(ref), where


def test_flat_and_noise_records_have_the_lengths_the_capacity_checks_rely_on():
    """Flat 128 -> every block empty; noise at quality 100 in 4:4:4 -> (nearly) every block 64 long: the two ends of the record's size."""
    from geotrax_amd import jpeg

    f, _, off, _ = jpeg.record_fields(jpeg.bgr_to_record(np.full((23, 17, 3), 128, np.uint8), 90))
    assert f["n_coef"] == 0 and not off.any()
    rng = np.random.default_rng(5)
    f, _, off, _ = jpeg.record_fields(jpeg.bgr_to_record(rng.integers(0, 256, (64, 64, 3), dtype=np.uint8), 100, "4:4:4"))
    assert np.diff(off.astype(np.int64)).max() == 64 and f["n_coef"] > 60 * f["n_blocks"]


@pytest.mark.parametrize("name", ACCEPTED)
def test_emitter_round_trips_every_fixture(name):
    """parse -> emit -> parse gives the same record byte for byte, and Pillow decodes the emitted file to the fixture's pixels."""
    from geotrax_amd import jpeg

    rec, info = jpeg.parse(fixture(name))
    out = jpeg.record_to_bytes(rec)
    again, info2 = jpeg.parse(out)
    assert info2 == info and again.tobytes() == rec.tobytes()
    im = Image.open(io.BytesIO(out))
    got = np.asarray(im.convert("RGB"))[..., ::-1]
    np.testing.assert_array_equal(got, expected(name))


def _write(path, recs, **kw):
    from geotrax_amd.video_writer import MjpegWriter

    w = MjpegWriter(path, 30.0, (47, 33), encode_threads=2, **kw)
    assert w.isOpened()
    for r in recs:
        w.write_record(r)
    w.release()
    assert w.frames == len(recs) and not w.isOpened()


def test_containers_read_back_by_the_existing_readers(tmp_path):
    """5 frames to .avi, to .mjpeg and to an .avi cut into RIFF AVIX lists every few KB: the readers return the count, the size, the
    frame rate (the raw stream carries none: MjpegReader's 0.0) and every frame's bytes. The emit step alone, no GPU."""
    from geotrax_amd import jpeg
    from geotrax_amd.frames import AviMjpegReader, MjpegReader, avi_is_mjpeg, open_source

    rng = np.random.default_rng(0)
    frames = [rng.integers(0, 256, (33, 47, 3), dtype=np.uint8) for _ in range(5)]
    recs = [jpeg.bgr_to_record(f, 90) for f in frames]
    want = [jpeg.record_to_bytes(r) for r in recs]
    for name, kw, n_avix in (("a.avi", {}, 0), ("b.mjpeg", {}, 0), ("c.avi", dict(riff_limit=6000), 2), ("d.avi", dict(riff_limit=1), 4)):
        path = tmp_path / name
        _write(path, recs, **kw)
        rd = (AviMjpegReader if name.endswith(".avi") else MjpegReader)(path)
        assert rd.frame_count == 5 and rd.frame_hw == (33, 47) and rd.truncated is None
        assert rd.fps == (30.0 if name.endswith(".avi") else 0.0)
        assert [rd._bytes(i) for i in range(5)] == want
        ok, f0 = rd.read()
        np.testing.assert_array_equal(f0, jpeg.record_to_bgr(recs[0]))
        rd.release()
        data = path.read_bytes()
        assert data.count(b"AVIX") == n_avix
        if name.endswith(".avi"):
            assert avi_is_mjpeg(path) and type(open_source(path)) is AviMjpegReader
            riff = int.from_bytes(data[4:8], "little")                 # the first RIFF list ends where the next begins, or the file
            assert data[8 + riff:8 + riff + 4] in (b"", b"RIFF")
            if kw:
                assert riff + 8 <= max(kw["riff_limit"], 3000)


def test_refusals():
    from geotrax_amd import _lib, jpeg
    from geotrax_amd.video_writer import MjpegWriter

    lib = _lib.load()
    a = np.zeros((8, 8, 3), np.uint8)
    for q in (0, 101, -1):
        with pytest.raises(ValueError, match="quality"):
            jpeg.bgr_to_record(a, q)
    with pytest.raises(ValueError, match="subsampling"):
        jpeg.bgr_to_record(a, 90, "4:2:2")
    with pytest.raises(ValueError):
        jpeg.bgr_to_record(np.zeros((0, 8, 3), np.uint8))
    with pytest.raises(ValueError):
        jpeg.bgr_to_record(np.zeros((1, 16385, 3), np.uint8))
    # the C ABI: every refusal comes before a context is looked at (none is given)
    h, n = C.c_void_p(), C.c_size_t()
    rec = np.zeros(1024, np.uint32).view(np.uint8)
    p = _lib.ptr

    def create(hh=8, ww=8, q=90, s=2):
        return lib.gtx_jpeg_enc_create(None, hh, ww, q, s, C.byref(h))

    def op(hh=8, ww=8, q=90, s=2):
        return lib.gtx_op_jpeg_encode(None, p(a), hh, ww, q, s, p(rec), rec.nbytes, C.byref(n))

    for call in (create, op):
        assert call() == -1 and b"ctx is NULL" in lib.gtx_last_error()               # the sizes were fine
        assert call(hh=16384, ww=16384, q=1) == -1 and b"ctx is NULL" in lib.gtx_last_error()
        assert call(q=100, s=0) == -1 and b"ctx is NULL" in lib.gtx_last_error()
        for bad in (dict(q=0), dict(q=101)):
            assert call(**bad) == -1 and b"quality" in lib.gtx_last_error()
        for bad in (dict(s=1), dict(s=3), dict(s=-1)):
            assert call(**bad) == -1 and b"subsampling" in lib.gtx_last_error()
        for bad in (dict(hh=0), dict(ww=0), dict(hh=16385), dict(ww=16385), dict(hh=-4)):
            assert call(**bad) == -1 and b"outside 1..16384" in lib.gtx_last_error()
    assert not h.value
    assert lib.gtx_jpeg_enc_submit_dev(None, None) == -1 and b"enc is NULL" in lib.gtx_last_error()
    assert lib.gtx_jpeg_enc_collect(None, p(rec), rec.nbytes, C.byref(n)) == -1 and b"enc is NULL" in lib.gtx_last_error()
    # the emitter: a short buffer yields the size and leaves everything past the capacity alone
    good = jpeg.bgr_to_record(np.random.default_rng(2).integers(0, 256, (23, 17, 3), dtype=np.uint8), 90)
    full = jpeg.record_to_bytes(good)
    assert lib.gtx_jpeg_emit(p(good), good.nbytes, None, 0, C.byref(n)) == 1 and n.value == len(full)
    out = np.full(len(full) + 16, 0xA5, np.uint8)
    assert lib.gtx_jpeg_emit(p(good), good.nbytes, p(out), len(full) - 1, C.byref(n)) == 1 and n.value == len(full)
    assert out[:len(full) - 1].tobytes() == full[:-1] and (out[len(full) - 1:] == 0xA5).all()
    assert lib.gtx_jpeg_emit(p(good), good.nbytes, p(out), len(full), C.byref(n)) == 0 and out[:len(full)].tobytes() == full and (out[len(full):] == 0xA5).all()
    assert lib.gtx_jpeg_emit(None, 0, p(out), out.nbytes, C.byref(n)) == -1 and b"record is NULL" in lib.gtx_last_error()
    assert lib.gtx_jpeg_emit(p(good), good.nbytes - 2, p(out), out.nbytes, C.byref(n)) == -1 and b"JPEG record" in lib.gtx_last_error()
    bad = good.copy()
    bad[jpeg.OFFSETS_OFFSET + 4] = 200                                                  # the first block 200 coefficients long
    with pytest.raises(jpeg.JpegError, match="offsets"):
        jpeg.record_to_bytes(bad)
    bad = good.copy()
    f, _, off, _ = jpeg.record_fields(bad)
    coef = bad[jpeg.OFFSETS_OFFSET + 4 * (f["n_blocks"] + 1):].view(np.int16)
    coef[1] = 1024                                                                      # an AC value of 11 bits
    with pytest.raises(jpeg.JpegError, match="AC coefficient"):
        jpeg.record_to_bytes(bad)
    # the writer
    for kw in (dict(quality=0), dict(quality=101), dict(subsampling="4:1:1"), dict(encode_threads=0)):
        with pytest.raises(ValueError):
            MjpegWriter("/nonexistent/x.avi", 30.0, (8, 8), **kw)
    for size in ((0, 8), (8, 16385)):
        with pytest.raises(ValueError):
            MjpegWriter("/nonexistent/x.avi", 30.0, size)
    with pytest.raises(ValueError, match="suffix"):
        MjpegWriter("/nonexistent/x.mp4", 30.0, (8, 8))


def test_emitter_runs_clean_under_the_sanitizers_as_a_program_of_its_own(tmp_path):
    """`make jpegemitcheck`: csrc/diag/jpeg_emit_check.cpp + the emitter + the parser built with -fsanitize=address,undefined and run
    directly (nothing is loaded into this interpreter): every fixture's record emitted and parsed again, 4 000 corruptions and the
    truncations of one record, with records and outputs in exact-size blocks. Built into the test's own directory."""
    assert shutil.which("g++") and shutil.which("make"), "g++ and make are needed to build the stand-alone emitter check"
    r = subprocess.run(["make", "-C", str(ROOT / "geo-trax_amd"), "jpegemitcheck", f"BUILD={tmp_path}", f"JPEG_FIXTURES={GOLDEN}"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "fixtures round-tripped, 4000 corruptions" in r.stdout, r.stdout + r.stderr
    assert "-fsanitize=address,undefined" in r.stdout
