"""The drawing entry points' refusals, on the host alone: every bad size or record comes back as GTX_ERR_INVALID with the record's
index in the message before any launch (no context is even given: a call that passed its checks answers "ctx is NULL"), the twin's
`validate` refuses the same lists, and the ABI number is unchanged."""
import ctypes as C

import numpy as np

from geotrax_amd import _lib, draw
from geotrax_amd.draw import FILL, GLYPH, RING, SEGMENT

GOOD = [(FILL, 0, 0, 1, 1, 0, 0, 0), (SEGMENT, -32768, 32767, 5, 5, 1, 0, 0), (RING, 3, 3, 0, 0, 1, 0, 0), (GLYPH, 0, 0, 4, 3, 2, 5, 0)]
ATLAS = np.arange(2 + 2 * 5 + 4, dtype=np.uint8)                   # the GLYPH of GOOD ends exactly at the atlas's end


def _op(lib, frame, prims, atlas=ATLAS, n=None, h=None, w=None):
    p = draw.as_prims(prims)
    a = None if atlas is None else _lib.ptr(atlas)
    return lib.gtx_op_draw(None, _lib.ptr(frame), frame.shape[0] if h is None else h, frame.shape[1] if w is None else w,
                           _lib.ptr(p) if len(p) else None, len(p) if n is None else n, a, 0 if atlas is None else atlas.size)


def test_abi_version_is_unchanged():
    lib = _lib.load()
    assert lib.gtx_abi_version() == 14 == _lib.ABI_VERSION
    for name in ("gtx_drawer_create", "gtx_drawer_destroy", "gtx_drawer_draw_dev", "gtx_drawer_last_ms", "gtx_op_draw", "gtx_dev_copy"):
        assert hasattr(lib, name)


def test_draw_hook_refuses_bad_records_before_any_launch():
    lib = _lib.load()
    f = np.zeros((6, 7, 3), np.uint8)
    assert _op(lib, f, GOOD) == -1 and b"ctx is NULL" in lib.gtx_last_error()          # the list was fine
    draw.validate(GOOD, ATLAS.size)
    bad = {
        "kind": (4, 0, 0, 1, 1, 0, 0, 0),
        "kind<0": (-1, 0, 0, 1, 1, 0, 0, 0),
        "segment t": (SEGMENT, 0, 0, 5, 5, 0, 0, 0),
        "ring t": (RING, 0, 0, 5, 0, -3, 0, 0),
        "ring r": (RING, 0, 0, -1, 0, 1, 0, 0),
        "x0": (FILL, -32769, 0, 0, 0, 0, 0, 0),
        "y0": (SEGMENT, 0, 32768, 0, 0, 1, 0, 0),
        "x1": (FILL, 0, 0, 40000, 0, 0, 0, 0),
        "y1": (SEGMENT, 0, 0, 0, -2**31, 1, 0, 0),
        "glyph end": (GLYPH, 0, 0, 4, 3, 3, 5, 0),                   # one byte past the atlas
        "glyph w": (GLYPH, 0, 0, 0, 3, 0, 5, 0),
        "glyph h": (GLYPH, 0, 0, 4, 0, 0, 5, 0),
        "glyph pitch": (GLYPH, 0, 0, 4, 3, 0, 0, 0),
        "glyph offset": (GLYPH, 0, 0, 4, 3, -1, 5, 0),
        "glyph huge": (GLYPH, 0, 0, 32767, 32767, 2**31 - 1, 2**31 - 1, 0),
    }
    for where, rec in bad.items():
        for at in (0, 3, 4):
            prims = list(GOOD)
            prims.insert(at, rec)
            assert _op(lib, f, prims) == -1, where
            msg = lib.gtx_last_error()
            assert f"primitive {at}:".encode() in msg and b"ctx" not in msg, (where, msg)
            try:
                draw.validate(prims, ATLAS.size)
            except ValueError as e:
                assert f"primitive {at}:" in str(e)
            else:
                raise AssertionError(f"the twin accepts {where}")
    # a glyph without an atlas
    assert _op(lib, f, [GOOD[3]], atlas=None) == -1 and b"primitive 0:" in lib.gtx_last_error()
    # the frame
    for h, w in ((0, 7), (6, 0), (-1, 7), (16385, 7), (6, 16385)):
        assert _op(lib, f, GOOD[:1], h=h, w=w) == -1 and b"frame" in lib.gtx_last_error()
    # the list's length
    assert _op(lib, f, GOOD[:1], n=-1) == -1 and b"n = -1" in lib.gtx_last_error()
    assert _op(lib, f, GOOD[:1], n=draw.MAX_PRIMS + 1) == -1 and b"holds" in lib.gtx_last_error()
    assert lib.gtx_op_draw(None, _lib.ptr(f), 6, 7, None, 2, None, 0) == -1 and b"prims is NULL" in lib.gtx_last_error()
    assert lib.gtx_op_draw(None, None, 6, 7, None, 0, None, 0) == -1 and b"bgr is NULL" in lib.gtx_last_error()
    assert lib.gtx_op_draw(None, _lib.ptr(f), 6, 7, None, 0, None, 5) == -1 and b"atlas is NULL" in lib.gtx_last_error()
    assert lib.gtx_op_draw(None, _lib.ptr(f), 6, 7, None, 0, None, 0) == -1 and b"ctx is NULL" in lib.gtx_last_error()   # n = 0 is a valid list
    assert not f.any()


def test_drawer_create_refuses_bad_sizes_before_the_context_is_used():
    lib = _lib.load()
    h = C.c_void_p(1)
    for args, word in (((0, 8, 4, None, 0), b"frame"), ((8, 16385, 4, None, 0), b"frame"), ((8, 8, 0, None, 0), b"max_prims"),
                       ((8, 8, draw.MAX_PRIMS + 1, None, 0), b"max_prims"), ((8, 8, 4, None, 16), b"atlas is NULL")):
        h.value = 1
        assert lib.gtx_drawer_create(None, *args, C.byref(h)) == -1 and word in lib.gtx_last_error() and not h.value
    assert lib.gtx_drawer_create(None, 8, 8, draw.MAX_PRIMS, None, 0, C.byref(h)) == -1 and b"ctx is NULL" in lib.gtx_last_error()
    assert lib.gtx_drawer_create(None, 8, 8, 4, None, 0, None) == -1 and b"out is NULL" in lib.gtx_last_error()
    ms = C.c_float()
    assert lib.gtx_drawer_draw_dev(None, None, None, 0) == -1 and b"drawer is NULL" in lib.gtx_last_error()
    assert lib.gtx_drawer_last_ms(None, C.byref(ms)) == -1
    lib.gtx_drawer_destroy(None)
    one = C.c_void_p(8)
    assert lib.gtx_dev_copy(None, one, one, 4) == -1 and b"ctx is NULL" in lib.gtx_last_error()
