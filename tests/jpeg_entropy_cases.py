"""Pictures and expected outcomes shared by tests/test_jpeg_entropy.py (the numpy twin against the host parser, no GPU) and
tests/test_jpeg_entropy_ops_gpu.py (the kernels against the twin). Every outcome is computed once per process."""
from __future__ import annotations

import functools
from pathlib import Path

import numpy as np

from geotrax_amd import jpeg

GOLDEN = Path(__file__).resolve().parent / "golden" / "jpeg"
HOST_ROUTE = ("p70x45_420_rst3", "p70x45_420_rstrow")
REFUSED = ("p70x45_progressive",)
SUB_BITS = (256, 0)                      # the smallest subsequence and the production choice
MANY_ROUNDS = 64                         # for the runs that must converge whatever the picture (picture (b) at 256 bits needs 18)


def fixture_names():
    return sorted(p.stem for p in GOLDEN.glob("*.jpg") if p.stem not in HOST_ROUTE + REFUSED)


def fixture_bytes(name: str) -> bytes:
    return (GOLDEN / f"{name}.jpg").read_bytes()


def _full(dc, ac):
    return [dc] + [ac(z) for z in range(1, 64)]


def _hand_built():
    rng = np.random.default_rng(7)
    out = {}
    # (a) every block empty: six bits a block, about 170 blocks in a subsequence of 1024 bits
    out["a_empty"] = jpeg.blocks_to_record(256, 256, 3, 2, 2, [[]] * 1536)
    # (b) every block 64 long, AC +-1023, alternating DC, 128 x 128 in 4:4:4: a block (1660 bits) is longer than a subsequence, no
    # block ends in an EOB, and the scan (about 160 KB) spans several workgroups that carry into each other
    nb = 16 * 16 * 3
    out["b_long"] = jpeg.blocks_to_record(128, 128, 3, 1, 1, [_full(1000 if (b // 3) % 2 else -1000, lambda z: 1023 if z % 2 else -1023) for b in range(nb)])
    # (c) the same with +1023 throughout: the coded bytes are dense in FF, stuffing sits on subsequence borders
    out["c_ff"] = jpeg.blocks_to_record(128, 128, 3, 1, 1, [_full(1000 if (b // 3) % 2 else -1000, lambda z: 1023) for b in range(nb)])
    # (d) three ZRLs, then a coefficient at zigzag 63 (no EOB behind it), mixed with empty blocks and short ones
    runs = []
    for b in range(8 * 8 * 6):
        runs.append([[5] + [0] * 62 + [7], [], [-3, 2] + [0] * 61 + [-1], [0, 0, 0, 9]][b % 4])
    out["d_zrl"] = jpeg.blocks_to_record(128, 128, 3, 2, 2, runs)
    # (e) the 8 x 8 picture: a scan shorter than one subsequence
    out["e_8x8"] = jpeg.blocks_to_record(8, 8, 3, 1, 1, [[40, -3, 2], [], [-7]])

    def random_runs(n):
        runs, dc = [], 0
        for _ in range(n):
            dc = int(np.clip(dc + rng.integers(-200, 201), -1000, 1000))
            ln = int(rng.integers(0, 65))
            r = [dc] + [int(v) if rng.random() < 0.4 else 0 for v in rng.integers(-300, 301, 63)]
            runs.append(r[:ln])
        return runs

    # (f) grayscale, and 4:2:2
    out["f_gray"] = jpeg.blocks_to_record(75, 41, 1, 1, 1, random_runs(10 * 6))
    out["f_422"] = jpeg.blocks_to_record(70, 45, 3, 2, 1, random_runs(5 * 6 * 4))
    return out


@functools.lru_cache(maxsize=None)
def hand_built():
    """name -> (record as built, the baseline JPEG the host emitter writes for it)"""
    return {k: (rec, jpeg.record_to_bytes(rec)) for k, rec in _hand_built().items()}


def picture_names():
    return fixture_names() + sorted(hand_built())


def picture_bytes(name: str) -> bytes:
    return hand_built()[name][1] if name in hand_built() else fixture_bytes(name)


@functools.lru_cache(maxsize=None)
def parsed(name: str) -> np.ndarray:
    return jpeg.parse(picture_bytes(name))[0]


@functools.lru_cache(maxsize=None)
def twin(name: str, sub_bits: int, rounds: int = MANY_ROUNDS):
    return jpeg.entropy_decode_twin(picture_bytes(name), sub_bits, 0, rounds)


def damaged():
    """(label, bytes): 64 evenly spaced truncations of w640x360_420.jpg, 200 seeded single-byte corruptions of p70x45_420.jpg"""
    out = []
    d = fixture_bytes("w640x360_420")
    for i in range(64):
        out.append((f"trunc{i}", d[:len(d) * (i + 1) // 65]))
    d = fixture_bytes("p70x45_420")
    rng = np.random.default_rng(11)
    for i in range(200):
        at, v = int(rng.integers(len(d))), int(rng.integers(1, 256))
        out.append((f"flip{i}", d[:at] + bytes([d[at] ^ v]) + d[at + 1:]))
    return out


@functools.lru_cache(maxsize=None)
def damaged_outcomes():
    """label -> ("refused", message) | ("host",) | ("plan", plan, status, record or None, rounds_used) from the twin, production sizes"""
    out = {}
    for label, data in damaged():
        try:
            plan = jpeg.entropy_plan(data)
        except jpeg.JpegError as e:
            out[label] = ("refused", str(e))
            continue
        out[label] = ("host",) if plan is None else ("plan", plan, *jpeg.entropy_decode_plan_twin(plan))
    return out
