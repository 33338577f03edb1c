"""YOLOv9s and YOLOv9c against YOLOv8s at the headline workload (DESIGN.md section 7j quotes it):
python tools/yolov9_time.py (one GPU) > profiles/yolov9_time.txt.

Seeded weights of the three models, each calibrated towards ~132 boxes per frame on the first 4K synthetic frame (bench.py's target),
the same box and run (only figures of one run compare):
1. frames/s through ExtractEngine (detect + ByteTrack + stabilize; 3840 x 2160 -> 1920 x 1920, B = 2, 2 detector streams,
   4 stabilizer streams: bench.py's defaults), frames resident in HBM; 3 runs each, interleaved, after a warm-up; the median.
2. per launch (GTX_PROFILE_PER_OP, mean of 10 passes at batch 2): every pool_down launch with the bytes it moves (input read once,
   both outputs written once) and its rate against the HBM figure of a float4 copy (6.29 TB/s measured; 8.0 TB/s on paper), next to
   the stride-2 convolution(s) it feeds.
3. the pooling kernel alone through gtx_op_pool_down (mean of 50 launches; includes nothing but the launch) on the same shapes."""
import os
import sys
import time

import numpy as np

os.environ["GTX_PROFILE_PER_OP"] = "1"
sys.path.insert(0, "geo-trax_amd")
sys.path.insert(0, "tools")
from geotrax_amd import _lib, ops  # noqa: E402
from geotrax_amd.detector import Detector  # noqa: E402
from geotrax_amd.engine import ExtractEngine  # noqa: E402
from geotrax_amd.synth import make_scene  # noqa: E402
from geotrax_amd.tracker import Tracker  # noqa: E402
from geotrax_amd.weights import synthetic_yolov8, synthetic_yolov9  # noqa: E402
from yolov10_time import B, DW_KW, H, KW, V8_KW, W, calibrated  # noqa: E402

HBM_MEASURED, HBM_PAPER = 6.29e12, 8.0e12


def main():
    ctx = _lib.default_context(0)
    scene = make_scene(seed=0, h=H, w=W)
    frames = [scene.render(t, 150) for t in range(32)]
    nbytes = H * W * 3
    dptrs = []
    for i in range(0, len(frames), B):
        q = ctx.dev_alloc(B * nbytes)
        ctx.dev_upload(q, np.ascontiguousarray(np.stack(frames[i:i + B])))
        dptrs.append(q)
    v9 = {k: v for k, v in DW_KW.items() if k != "scale"}
    models = {}
    # seed 5 / 2: the calm seeds of tests/test_yolov9_gpu.py (an amplifying stack saturates and falls back to exact fp32: another workload)
    for label, base in (("yolov8s", synthetic_yolov8(**V8_KW)), ("yolov9s", synthetic_yolov9(**{**v9, "seed": 5}, scale="s", gain=1.6)),
                        ("yolov9c", synthetic_yolov9(**{**v9, "seed": 2}, scale="c", gain=1.6))):
        w, n = calibrated(base, ctx, frames[0])
        models[label] = w
        print(f"{label}: calibrated to {n} boxes on frame 0", flush=True)

    print(f"\n1. frames/s through ExtractEngine, {W}x{H} -> 1920x1920, B = {B}, 2 detector / 4 stabilizer streams, ByteTrack, "
          f"{len(frames)} frames in HBM; 3 runs each, interleaved")
    fps = {k: [] for k in models}
    for rep in range(3):
        for label, w in models.items():
            eng = ExtractEngine(w, (H, W), KW, Tracker("bytetrack"), {}, batch=B, det_streams=2, stab_streams=4)
            list(eng.run(dptrs[:4]))                              # warm-up
            eng.reset()
            t0 = time.perf_counter()
            res = list(eng.run(dptrs))
            dt = time.perf_counter() - t0
            fps[label].append(len(res) / dt)
            nd = np.mean([len(r.xyxy) for r in res])
            eng.close()
            print(f"   run {rep}  {label:11s} {len(res) / dt:8.1f} frames/s  ({nd:.0f} boxes per frame)", flush=True)
    for label, v in fps.items():
        print(f"   {label:11s} median {np.median(v):8.1f} frames/s")

    print(f"\n2. per launch at batch {B} (mean of 10 passes): the pooling launches and the stride-2 convolutions behind them")
    for label in ("yolov9s", "yolov9c"):
        det = Detector(models[label], (H, W), ctx=ctx, max_batch=B, **KW)
        det.detect_dev(dptrs[0], B)
        assert not det.fell_back(), "the seeded weights saturated: the figures would be the exact-fp32 path's"
        rows = det.profile(B, 10)
        fwd = sum(r["total_ms"] for r in rows) / 10
        pool = conv = 0.0
        print(f"   {label}: forward {fwd:.3f} ms, {len(rows)} launches, sparse box {det.sparse_box()}, pad skip {det.pad_skip()}")
        for r in rows:
            name = r["kernel"].split(" ", 1)[-1]
            layer = name.split(".")[1] if name.startswith("model.") else ""
            if name.endswith(".pool"):
                us, mb = r["total_ms"] / 10 * 1e3, r["bytes"] / 10 / 1e6
                rate = mb * 1e6 / (us * 1e-6)
                pool += us
                print(f"      {name:22s} {us:8.1f} us  {mb:8.1f} MB  {rate / 1e9:7.0f} GB/s = {100 * rate / HBM_MEASURED:4.1f} % of 6.29 TB/s ({100 * rate / HBM_PAPER:4.1f} % of 8.0)")
            elif layer in ("3", "5", "7", "16", "19") and (name.endswith(".cv1.conv") or name.endswith(".cv2.conv")):
                us = r["total_ms"] / 10 * 1e3
                conv += us
                print(f"      {name:22s} {us:8.1f} us  {r['flops'] / 10 / (us * 1e-6) / 1e12:6.1f} TFLOP/s")
        print(f"      pooling launches together {pool:.1f} us, the convolutions behind them {conv:.1f} us")
        det.close()

    print("\n3. gtx_op_pool_down alone, pair format, batch 2, mean of 50 launches")
    rng = np.random.default_rng(0)
    for label, cases in (("AConv (s)", ((480, 64, 0), (240, 128, 0), (120, 192, 0))), ("ADown (c)", ((480, 128, 128), (240, 256, 256), (120, 256, 256)))):
        for hw, ca, cb in cases:
            x = rng.normal(0, 1, (B, hw, hw, ca + cb)).astype(np.float32)
            _, _, ms = ops.pool_down(x, ca, cb, split=True, iters=50, ctx=ctx)
            byts = 4.0 * B * (hw * hw * (ca + cb) + hw * hw * ca + (hw // 2) ** 2 * cb)
            rate = byts / (ms * 1e-3)
            print(f"   {label:10s} {hw:4d} x {hw:<4d} {ca + cb:4d} ch  {ms * 1e3:8.1f} us  {byts / 1e6:7.1f} MB  {rate / 1e9:7.0f} GB/s = {100 * rate / HBM_MEASURED:4.1f} % of 6.29 TB/s")
    for q in dptrs:
        ctx.dev_free(q)


if __name__ == "__main__":
    main()
