"""The GMC objects' surface for a frame-sharded run (geotrax_amd/gmc.py), without a device: every method can be primed by a
shard rank, and the stream-ordered ORB estimator's entry points (gtx_fgmc_*) are declared, bound and exported. CPU only."""
import inspect
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
FGMC = {"gtx_fgmc_create", "gtx_fgmc_destroy", "gtx_fgmc_reset", "gtx_fgmc_restart", "gtx_fgmc_submit_gray_dev", "gtx_fgmc_submit_gray",
        "gtx_fgmc_submit_frame_dev", "gtx_fgmc_collect", "gtx_fgmc_pairs", "gtx_fgmc_matches"}


def test_fgmc_entry_points_are_declared_bound_and_exported():
    from geotrax_amd import _lib

    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "gtx.h").read_text(), flags=re.S)
    declared = set(re.findall(r"\b(gtx_[a-z0-9_]+)\s*\(", text))
    assert FGMC | {"gtx_gray_half_dev"} <= declared
    assert FGMC | {"gtx_gray_half_dev"} <= set(_lib._SIGNATURES)
    lib = _lib.load()
    for name in sorted(FGMC):
        assert hasattr(lib, name), name
    # the submit call mirrors gtx_gmc_submit_frame_dev (frame, h, w, restart)
    assert _lib._SIGNATURES["gtx_fgmc_submit_frame_dev"] == _lib._SIGNATURES["gtx_gmc_submit_frame_dev"]
    assert _lib._SIGNATURES["gtx_fgmc_collect"] == _lib._SIGNATURES["gtx_gmc_collect"]


def test_every_gmc_method_takes_a_priming_frame():
    """FeatureGMC.submit_frame_dev is implemented (it raised NotImplementedError), and EccGMC ignores a priming frame: objects
    built with __new__, no device."""
    from geotrax_amd.gmc import GMC, EccGMC, FeatureGMC

    want = ["self", "frame_dptr", "h", "w", "restart"]
    for cls in (GMC, FeatureGMC, EccGMC):
        assert list(inspect.signature(cls.submit_frame_dev).parameters)[:5] == want, cls
    assert "NotImplementedError" not in inspect.getsource(FeatureGMC.submit_frame_dev)
    e = EccGMC.__new__(EccGMC)                       # no handle: a priming frame must not reach the library at all
    e.handle = None
    assert e.submit_frame_dev(0x1000, 64, 64, restart=True) == 0
    f = FeatureGMC.__new__(FeatureGMC)               # a frame of the wrong size is refused before anything is queued (orb and sift)
    f.handle, f.method, f.frame_hw = None, "orb", (64, 64)
    try:
        f.submit_frame_dev(0x1000, 32, 32, restart=True)
    except ValueError as err:
        assert "64x64" in str(err)
    else:
        raise AssertionError("wrong frame size accepted")
    assert FeatureGMC.reset_sequence is not FeatureGMC.reset_params     # restart with frames in flight is its own operation now
