"""Live tracing (gtx_detector_trace + the trace report bench.py --full reads) against the profile loop: the same passes must give
the same kernel families, launch counts and FLOP / byte totals through both, for both detector families. At batch 2, so a
per-image and a per-pass accounting cannot agree by accident."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FRAME_HW = (432, 768)


def _frame(seed):
    rng = np.random.default_rng(seed)
    h, w = FRAME_HW
    yy, xx = np.mgrid[0:h, 0:w]
    base = 110 + 50 * np.sin(xx / 37.0) * np.cos(yy / 23.0)
    f = np.stack([base + 20 * rng.standard_normal((h, w)) for _ in range(3)], -1)
    return np.clip(f, 0, 255).astype(np.uint8)


def _weights(arch):
    from geotrax_amd.weights import synthetic_rtdetr, synthetic_yolov8

    return synthetic_yolov8(seed=1, nc=4, scale="s", cls_bias=-3.0) if arch == "yolov8s" else synthetic_rtdetr(seed=3, nc=4)


@pytest.mark.parametrize("arch,imgsz", [("yolov8s", 640), ("rtdetr", 480)])
def test_trace_report_matches_profile(gtx_ctx, arch, imgsz):
    from geotrax_amd.detector import Detector

    nb, k = 2, 3
    det = Detector(_weights(arch), FRAME_HW, imgsz=imgsz, conf=0.25, max_det=100, max_batch=nb, fp32_split=True, ctx=gtx_ctx)
    frames = np.ascontiguousarray(np.stack([_frame(s) for s in range(nb)]))
    dptr = gtx_ctx.dev_alloc(frames.nbytes)
    try:
        gtx_ctx.dev_upload(dptr, frames)
        det.trace(1)
        for _ in range(k):
            det.detect_dev(dptr, nb)
        traced = det.trace_report()
        assert det.trace_report() == []          # the report clears the totals
        det.trace(0)
        det.detect_dev(dptr, nb)                 # tracing off: nothing is folded
        assert det.trace_report() == []
        profiled = det.profile(nb, k)
    finally:
        gtx_ctx.dev_free(dptr)
        det.close()
    assert len(traced) > 1
    assert [f["kernel"] for f in traced] == [f["kernel"] for f in profiled]
    for t, p in zip(traced, profiled):
        assert t["launches"] == p["launches"] and t["launches"] % k == 0, (t, p)
        np.testing.assert_allclose(t["flops"], p["flops"], rtol=1e-12, err_msg=t["kernel"])
        np.testing.assert_allclose(t["bytes"], p["bytes"], rtol=1e-12, err_msg=t["kernel"])
    assert sum(f["flops"] for f in traced) > 0
