"""Host side of the resident sift / rsift stabilizer: what gtx_op_sift_select refuses before the GPU is touched, which `stabilo:`
blocks extract.pipelined() sends to the engine, and the ABI number (new entry points only)."""
import ctypes as C

import numpy as np


def _records(n, seed=0):
    from geotrax_amd import ops

    rng = np.random.default_rng(seed)
    rec = np.zeros(n, ops.SIFT_ORIENTED)
    rec["x"], rec["y"] = rng.uniform(0, 300, n), rng.uniform(0, 200, n)
    rec["size"], rec["angle"], rec["response"] = 3.0, rng.uniform(0, 359, n), rng.uniform(0.02, 0.2, n)
    rec["o"] = rec["key_o"] = 1
    rec["layer"] = rec["key_layer"] = 2
    rec["key_r"], rec["key_c"] = np.arange(n) // 50 + 5, np.arange(n) % 50 + 5      # one key per record
    rec["bin"] = 7
    return rec


def test_select_hook_refuses_bad_arguments_before_any_launch():
    from geotrax_amd import _lib

    lib = _lib.load()
    p = _lib.ptr
    rec = _records(8)
    rects = np.array([[0, 0, 4, 4]], np.int32)
    n = C.c_int(-7)

    def call(r=rec, k=None, max_features=4, rc=rects, n_rects=1, count=n):
        k = len(r) if k is None else k
        return lib.gtx_op_sift_select(None, p(r) if r is not None else None, k, max_features, p(rc) if rc is not None else None, n_rects,
                                      C.byref(count) if count is not None else None, None, None, None, None)

    def refused(what, **kw):
        assert call(**kw) == -1
        assert what in lib.gtx_last_error(), lib.gtx_last_error()

    refused(b"ctx is NULL")                                            # everything was fine: only the context is missing
    refused(b"ctx is NULL", k=0, r=None, rc=None, n_rects=0)           # no records, no rectangles
    refused(b"ctx is NULL", max_features=65536, n_rects=0, rc=None)
    refused(b"records", k=-1)
    refused(b"records", k=(1 << 20) + 1)
    refused(b"max_features", max_features=0)
    refused(b"max_features", max_features=65537)
    refused(b"rectangles", n_rects=1025)
    refused(b"rectangles", n_rects=-1)
    refused(b"NULL", r=None, k=8)
    refused(b"NULL", rc=None, n_rects=1)
    refused(b"NULL", count=None)
    for bad in (np.nan, np.inf, -np.inf, -0.5):
        r = rec.copy()
        r["response"][3] = bad
        refused(b"response", r=r)
    for field, bad, what in (("o", 16, b"octave"), ("key_o", -1, b"octave"), ("key_layer", 8, b"layer"), ("key_r", 1 << 20, b"row or column"),
                             ("key_c", -1, b"row or column"), ("bin", 256, b"bin")):
        r = rec.copy()
        r[field][5] = bad
        refused(what, r=r)
    r = rec.copy()
    r["key_r"][6], r["key_c"][6] = r["key_r"][2], r["key_c"][2]
    refused(b"one key", r=r)
    assert n.value == -7                                               # nothing was written


def _config(**stab):
    return {"main": {"engine": {}, "extraction": {"stabilize": True}},
            "stabilo": dict(dict(detector_name="rsift", downsample_ratio=0.5, filter_type="ratio", transformation_type="projective", clahe=False), **stab)}


def test_pipelined_takes_sift_at_ratio_one_half_only():
    from geotrax_amd import extract as ex

    assert ex.pipelined(_config()) is True
    assert ex.pipelined(_config(detector_name="sift")) is True
    assert ex.pipelined(_config(detector_name="orb")) is True
    assert ex.pipelined(_config(downsample_ratio=1.0)) is False
    assert ex.pipelined(_config(transformation_type="affine")) is False        # Stabilizer still raises for it on the blocking route
    assert ex.pipelined(_config(filter_type="none")) is False
    assert ex.pipelined(_config(clahe=True)) is False
    cfg = _config()
    cfg["main"]["engine"]["pipelined"] = False
    assert ex.pipelined(cfg) is False                                           # the switch still holds
    cfg = _config(downsample_ratio=1.0)
    cfg["main"]["extraction"]["stabilize"] = False
    assert ex.pipelined(cfg) is True                                            # no stabilizer at all: nothing to route


def test_the_engine_builds_siftstabilizer_for_resident_blocks_only():
    """What SiftStabilizer does not run keeps Stabilizer (which serves sift at other ratios on host frames and refuses the rest, as
    before), and the frame-sharded run keeps Stabilizer for every block: sift at ratio 0.5 is refused there as before."""
    from geotrax_amd import extract as ex
    from geotrax_amd.engine import stabilizer_class
    from geotrax_amd.sift_stabilizer import SiftStabilizer
    from geotrax_amd.stabilizer import Stabilizer

    assert stabilizer_class(_config()["stabilo"]) is SiftStabilizer
    assert stabilizer_class(_config(detector_name="sift", matcher_name="flann")["stabilo"]) is SiftStabilizer
    for over in (dict(downsample_ratio=1.0), dict(downsample_ratio=0.25), dict(transformation_type="affine"), dict(filter_type="none"),
                 dict(clahe=True), dict(matcher_name="annoy"), dict(detector_name="orb"), dict(detector_name="brisk")):
        assert stabilizer_class(_config(**over)["stabilo"]) is Stabilizer, over
    assert stabilizer_class(dict(max_features=500)) is Stabilizer and stabilizer_class(None) is Stabilizer
    assert ex.sharded_engine_kwargs() == dict(stab_cls=Stabilizer)
    import inspect

    assert "**sharded_engine_kwargs()" in inspect.getsource(ex.track_with_model_sharded)
    # and Stabilizer, the class the sharded engine then builds, still refuses the gray image in HBM for these detectors (no device
    # is touched: the sift path creates no handle)
    st = Stabilizer((64, 64), detector_name="rsift", sift_enable_precise_upscale=True, ctx=object())
    try:
        st.set_ref_gray_dev(0, 32, 32)
        raise AssertionError("Stabilizer.set_ref_gray_dev took a sift block")
    except NotImplementedError:
        pass


def test_abi_number_stays_and_the_new_symbols_are_bound():
    from geotrax_amd import _lib

    lib = _lib.load()
    assert lib.gtx_abi_version() == 14 == _lib.ABI_VERSION
    for name in ("create", "destroy", "set_ref_gray_dev", "submit_gray_dev", "collect", "stabilize_gray_dev", "last_ms", "keypoints", "pairs", "counters"):
        assert f"gtx_sift_stab_{name}" in _lib._SIGNATURES and hasattr(lib, f"gtx_sift_stab_{name}")
    assert "gtx_op_sift_select" in _lib._SIGNATURES
    assert C.sizeof(_lib.SiftStabConfig) == 14 * 4
