"""Pictures, records and damaged frames shared by the restart-interval tests (tests/test_jpeg_restart.py on the CPU,
tests/test_jpeg_restart_gpu.py on the GPU). Everything is computed once and never changed."""
from __future__ import annotations

import functools
import io

import numpy as np
from jpeg_entropy_cases import fixture_bytes, hand_built

from geotrax_amd import jpeg

RESTART_FIXTURES = ("p70x45_420_rst3", "p70x45_420_rstrow")
SIZES = ((17, 9), (70, 45))                                       # (w, h)
KINDS = ("gray", "444", "422", "420")


def _image(w: int, h: int) -> np.ndarray:
    y, x = np.mgrid[0:h, 0:w]
    rng = np.random.default_rng(w * 1000 + h)
    base = np.stack([x * 255 // max(w - 1, 1), y * 255 // max(h - 1, 1), (x + y) * 3 % 256], -1)
    return np.clip(base + rng.integers(-40, 41, (h, w, 3)), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def records():
    """name -> record: a grayscale, a 4:4:4, a 4:2:2 and a 4:2:0 picture of 17 x 9 and of 70 x 45 (Pillow's files, parsed), and the
    hand-built records of jpeg_entropy_cases plus two of this route's own."""
    from PIL import Image

    out = {}
    for w, h in SIZES:
        rgb = _image(w, h)
        for kind in KINDS:
            buf = io.BytesIO()
            if kind == "gray":
                Image.fromarray(rgb[..., 1]).save(buf, "JPEG", quality=85)
            else:
                Image.fromarray(rgb).save(buf, "JPEG", quality=85, subsampling={"444": 0, "422": 1, "420": 2}[kind])
            out[f"{kind}_{w}x{h}"] = jpeg.parse(buf.getvalue())[0]
    for k, (_, blob) in hand_built().items():                       # as the parser reads them back (it drops zeros that end a run)
        out[f"hand_{k}"] = jpeg.parse(blob)[0]
    # an interval of all-empty blocks between two that are not: 4:2:0, 3 x 2 MCUs; at r = 1 MCU 2's interval is six bits of codes
    runs = [[5, 1, 0, -2]] * 12 + [[]] * 6 + [[-3, 0, 0, 7]] * 18
    out["empty_interval"] = jpeg.blocks_to_record(48, 32, 3, 2, 2, runs)
    # blocks with no EOB: 64 coefficients, the last one non-zero
    full = [9] + [1 if z % 5 == 0 else 0 for z in range(1, 63)] + [-1]
    out["no_eob"] = jpeg.blocks_to_record(16, 16, 3, 1, 1, [full, [], full] * 4)
    return out


def restarts_of(rec: np.ndarray):
    """The restart intervals of the issue for a record: 1, 3, one MCU row, the whole frame, more than the frame; and 4, which
    leaves the 15 MCUs of 70 x 45 4:2:0 a short last interval."""
    f = jpeg.record_fields(rec)[0]
    n_mcus = f["mcus_x"] * f["mcus_y"]
    return sorted({1, 3, 4, f["mcus_x"], n_mcus, n_mcus + 5})


@functools.lru_cache(maxsize=None)
def frames():
    """label -> (record, the file emit() writes for it with restarts): every record at every interval, and the two committed
    fixtures as they are (Pillow's tables and markers)."""
    out = {}
    for name, rec in records().items():
        for r in restarts_of(rec):
            out[f"{name}_r{r}"] = (rec, jpeg.emit(rec, r))
    for name in RESTART_FIXTURES:
        b = fixture_bytes(name)
        out[name] = (jpeg.parse(b)[0], b)
    return out


def marker_positions(blob: bytes):
    """Offsets of the RSTn markers (the FF) in the entropy-coded segment of a file emit() wrote."""
    at = blob.index(b"\xff\xda")
    at += 2 + int.from_bytes(blob[at + 2:at + 4], "big")
    return [i for i in range(at, len(blob) - 1) if blob[i] == 0xFF and 0xD0 <= blob[i + 1] <= 0xD7]


@functools.lru_cache(maxsize=None)
def damaged():
    """label -> bytes: the 70 x 45 4:2:0 picture at one MCU per interval (15 intervals, so RST0..RST7 and the wrap) with a marker
    out of sequence, a marker missing, the last interval truncated and one stray byte in front of a marker."""
    good = frames()["420_70x45_r1"][1]
    pos = marker_positions(good)
    assert len(pos) == 14
    out = {}
    b = bytearray(good)
    b[pos[4] + 1] = 0xD0 + 6
    out["out_of_sequence"] = bytes(b)
    b = bytearray(good)
    b[pos[9] + 1] = 0xD0 + 2                                      # past the wrap: RST1 belongs here
    out["out_of_sequence_after_wrap"] = bytes(b)
    out["missing"] = good[:pos[3]] + good[pos[3] + 2:]
    out["missing_last"] = good[:pos[-1]] + good[pos[-1] + 2:]
    out["truncated_last"] = good[:pos[-1] + 3]
    out["stray_byte"] = good[:pos[6]] + b"\x55" + good[pos[6]:]
    return out

