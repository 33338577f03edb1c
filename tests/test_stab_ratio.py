"""Host side of ORB stabilization at any downsample_ratio: the working-size rule, the route an engine takes to the stabilizers'
gray image, the answers extract.pipelined() / stabilizer_class keep, and the ABI (new entry points only). No GPU."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent

# (frame (h, w), ratio) -> (gh, gw); the last two are the sizes ratios 0.5 and 1.0 have always had
WORKING_SIZES = [
    ((2160, 3840), 0.25, (540, 960)),
    ((2160, 3840), 0.75, (1620, 2880)),
    ((2160, 3840), 0.3, (648, 1152)),
    ((37, 50), 0.6, (22, 30)),
    ((37, 51), 0.5, (18, 25)),
    ((37, 51), 1.0, (37, 51)),
]


@pytest.mark.parametrize("hw,ratio,want", WORKING_SIZES)
def test_working_size_known_answers(hw, ratio, want):
    from geotrax_amd.stabilizer import working_size

    assert working_size(hw, ratio) == want


def test_working_size_is_the_librarys_rule():
    """The pure-Python rule and the library's (host only, no context) agree, halves included: rint in double from the float32 ratio,
    to even -- 130 * 0.25 = 32.5 -> 32, 1030 * 0.25 = 257.5 -> 258."""
    from geotrax_amd import _lib
    from geotrax_amd.stabilizer import working_size

    lib = _lib.load()
    assert working_size((130, 1030), 0.25) == (32, 258)
    rng = np.random.default_rng(0)
    cases = [(hw, r) for hw, r, _ in WORKING_SIZES] + [((130, 1030), 0.25), ((9, 9), 0.2), ((64, 260), 0.75)]
    cases += [((int(h), int(w)), float(r)) for h, w, r in zip(rng.integers(1, 5000, 200), rng.integers(1, 5000, 200), rng.uniform(0.01, 1.0, 200))]
    for hw, r in cases:
        gh, gw = C.c_int(), C.c_int()
        assert lib.gtx_op_gray_working_size(hw[0], hw[1], r, C.byref(gh), C.byref(gw)) == 0, lib.gtx_last_error()
        assert (gh.value, gw.value) == working_size(hw, r), (hw, r)
    for bad in (0.0, -0.5, 1.5, float("nan")):
        assert lib.gtx_op_gray_working_size(64, 64, bad, C.byref(gh), C.byref(gw)) == -1 and b"(0, 1]" in lib.gtx_last_error()
        if bad == bad:
            with pytest.raises(ValueError, match=r"\(0, 1\]"):
                working_size((64, 64), bad)


def test_gray_route():
    from geotrax_amd.engine import gray_route

    assert gray_route(dict(detector_name="orb", downsample_ratio=0.5)) == "detector"
    assert gray_route(dict(max_features=500)) == "detector"                     # the defaults: orb at 0.5
    for r in (1.0, 0.75, 0.25):
        assert gray_route(dict(detector_name="orb", downsample_ratio=r)) == "frame"
        assert gray_route(dict(downsample_ratio=r)) == "frame"
    assert gray_route(dict(detector_name="rsift", downsample_ratio=1.0)) == "host"
    assert gray_route(dict(detector_name="sift", downsample_ratio=0.25)) == "host"      # Stabilizer refuses it at the first frame, as before
    assert gray_route(dict(detector_name="rsift", downsample_ratio=0.5)) == "detector"  # the resident SiftStabilizer chain
    assert gray_route(None) is None                                             # no stabilizer: ExtractEngine.stab_dev_gray is False, nothing to route


def _config(**stab):
    return {"main": {"engine": {}, "extraction": {"stabilize": True}},
            "stabilo": dict(dict(detector_name="rsift", downsample_ratio=0.5, filter_type="ratio", transformation_type="projective", clahe=False), **stab)}


def test_pipelined_and_stabilizer_class_keep_their_answers():
    """The answers tests/test_sift_stab.py asks for, asked again beside the new route: ORB is pipelined at every ratio, sift / rsift
    away from 0.5 is not, and the classes are chosen as before."""
    from geotrax_amd import extract as ex
    from geotrax_amd.engine import stabilizer_class
    from geotrax_amd.sift_stabilizer import SiftStabilizer
    from geotrax_amd.stabilizer import Stabilizer

    assert ex.pipelined(_config()) is True
    assert ex.pipelined(_config(detector_name="sift")) is True
    assert ex.pipelined(_config(detector_name="orb")) is True
    for r in (1.0, 0.75, 0.25):
        assert ex.pipelined(_config(detector_name="orb", downsample_ratio=r)) is True
    assert ex.pipelined(_config(downsample_ratio=1.0)) is False
    assert ex.pipelined(_config(transformation_type="affine")) is False
    assert ex.pipelined(_config(filter_type="none")) is False
    assert ex.pipelined(_config(clahe=True)) is False
    cfg = _config(detector_name="orb", downsample_ratio=0.75)
    cfg["main"]["engine"]["pipelined"] = False
    assert ex.pipelined(cfg) is False
    assert stabilizer_class(_config()["stabilo"]) is SiftStabilizer
    for over in (dict(downsample_ratio=1.0), dict(downsample_ratio=0.25), dict(detector_name="orb"), dict(detector_name="orb", downsample_ratio=0.75)):
        assert stabilizer_class(_config(**over)["stabilo"]) is Stabilizer, over
    assert stabilizer_class(None) is Stabilizer
    assert ex.sharded_engine_kwargs() == dict(stab_cls=Stabilizer)


def test_sift_blocks_are_still_refused_where_they_were():
    from geotrax_amd.stabilizer import Stabilizer

    st = Stabilizer((64, 64), detector_name="rsift", sift_enable_precise_upscale=True, downsample_ratio=0.75, ctx=object())
    with pytest.raises(NotImplementedError, match="1.0 or 0.5"):
        st.set_ref_frame(np.zeros((64, 64, 3), np.uint8))
    with pytest.raises(NotImplementedError):
        st.set_ref_gray_dev(0, 48, 48)


def test_abi_is_additive():
    from geotrax_amd import _lib

    lib = _lib.load()
    assert lib.gtx_abi_version() == 14 == _lib.ABI_VERSION
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "gtx.h").read_text(), flags=re.S)
    for name in ("gtx_op_gray_resize_dev", "gtx_op_gray_resize", "gtx_op_gray_resize_ms", "gtx_op_gray_working_size"):
        assert name in _lib._SIGNATURES and hasattr(lib, name)
        assert re.search(rf"\b{name}\s*\(", header), name
    assert "#define GTX_ABI_VERSION 14" in header
    # one number for the detector's gray ring (csrc/net_runtime.hpp takes it from the header) and the engine's working-gray ring
    from geotrax_amd.engine import ExtractEngine

    assert f"#define GTX_GRAY_RING {_lib.GRAY_RING}\n" in header and ExtractEngine._GRAY_RING == _lib.GRAY_RING
    assert "kGrayRing = GTX_GRAY_RING;" in (ROOT / "geo-trax_amd" / "csrc" / "net_runtime.hpp").read_text()
    # gtx_stab_config keeps its layout: the fields of the bindings' struct, in order
    assert [f[0] for f in _lib.StabConfig._fields_] == [
        "downsample_ratio", "max_features", "ref_multiplier", "filter_ratio", "ransac_threshold", "ransac_max_iter", "ransac_confidence",
        "mask_use", "mask_margin_ratio", "fast_threshold", "n_levels", "scale_factor", "seed", "frame_h", "frame_w", "clahe", "affine",
        "filter_type"]


def test_gray_resize_hooks_refuse_bad_sizes_before_any_launch():
    from geotrax_amd import _lib

    lib = _lib.load()
    f = np.zeros((37, 50, 3), np.uint8)
    g = np.zeros((22, 30), np.uint8)
    p = _lib.ptr

    def refused(what, rc):
        assert rc == -1 and what in lib.gtx_last_error(), lib.gtx_last_error()

    refused(b"ctx is NULL", lib.gtx_op_gray_resize(None, p(f), 37, 50, 0.6, p(g), 22, 30))      # all sizes right: only the context is missing
    refused(b"ctx is NULL", lib.gtx_op_gray_resize_dev(None, p(f), 37, 50, 0.6, p(g), 22, 30))
    refused(b"working size", lib.gtx_op_gray_resize(None, p(f), 37, 50, 0.6, p(g), 22, 31))
    refused(b"working size", lib.gtx_op_gray_resize_dev(None, p(f), 37, 50, 0.6, p(g), 23, 30))
    refused(b"working size", lib.gtx_op_gray_resize(None, p(f), 37, 50, 0.5, p(g), 19, 25))     # 0.5 keeps h / 2, w / 2
    refused(b"(0, 1]", lib.gtx_op_gray_resize(None, p(f), 37, 50, 0.0, p(g), 22, 30))
    refused(b"(0, 1]", lib.gtx_op_gray_resize_dev(None, p(f), 37, 50, 1.25, p(g), 22, 30))
    refused(b"empty", lib.gtx_op_gray_resize(None, p(f), 2, 2, 0.1, p(g), 0, 0))
    refused(b"65535", lib.gtx_op_gray_resize(None, p(f), 70000, 50, 0.6, p(g), 22, 30))
    refused(b"NULL", lib.gtx_op_gray_resize(None, None, 37, 50, 0.6, p(g), 22, 30))
    refused(b"NULL", lib.gtx_op_gray_resize_dev(None, p(f), 37, 50, 0.6, None, 22, 30))
