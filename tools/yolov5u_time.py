"""YOLOv5su beside YOLOv8s at the headline workload (DESIGN.md section 7o quotes it):
python tools/yolov5u_time.py (one GPU) -> profiles/yolov5u_time.txt.

Seeded weights of the two families (YOLOv5su at gain 1.3, where its seeded activations stay inside fp16's range, so that the default
path is timed and not its exact-fp32 fallback), each calibrated towards ~132 boxes per frame on the first 4K synthetic frame (bench.py's
target), the same box and run (boxes of the pool differ by up to 8 %: only figures of one run compare):
1. frames/s through ExtractEngine (detect + ByteTrack + stabilize; 3840 x 2160 -> 1920 x 1920, B = 2, 2 detector streams,
   4 stabilizer streams: bench.py's defaults), frames resident in HBM; 3 runs each, interleaved, after a warm-up; the median.
2. the forward time of gtx_detector_profile (mean of 10 passes at batch 2) and the pass tail -- everything behind the forward:
   score gate, sparse box branch, NMS, the copies of the rows -- as the `postprocess` figure of 20 blocking passes (HIP events around
   the tail), the median; for YOLOv5su the 6x6 stem launch (stem6_split_kernel) with its share of the forward, beside YOLOv8s' first launch
   (the 3x3 stem fused into model.1 + model.2.cv1).
3. the 6x6 stem launch alone on one 1920 x 1920 image (ops.stem6, 50 launches between two events), all three forms, c0 = 32 and 80,
   and the split form's largest error against float64 over tests/test_yolov5u_gpu.py's cases."""
import sys
import time

import numpy as np

sys.path.insert(0, "geo-trax_amd")
from geotrax_amd import _lib  # noqa: E402
from geotrax_amd.detector import Detector  # noqa: E402
from geotrax_amd.engine import ExtractEngine  # noqa: E402
from geotrax_amd.synth import make_scene  # noqa: E402
from geotrax_amd.tracker import Tracker  # noqa: E402
from geotrax_amd import ops  # noqa: E402
from geotrax_amd.weights import synthetic_yolov5u, synthetic_yolov8  # noqa: E402

H, W, B, TARGET = 2160, 3840, 2, 132
KW = dict(imgsz=1920, conf=0.25, iou=0.7, max_det=1000, classes=[0, 1, 2, 3], agnostic_nms=True, half=False, rect=False)
# bench.py's SYNTH_KW for YOLOv8s (vehicle-sized boxes, clustered candidates); the same box knobs for the other two
V8_KW = dict(seed=0, nc=4, scale="s", level_bias=(0.0, -1e4, -1e4), box_weight_scale=0.002, smooth_cls=True, box_decay=(0.2, 0.3, 0.2, 0.3))
DW_KW = dict(seed=0, nc=4, scale="s", level_bias=(0.0, -1e4, -1e4), box_weight_scale=0.002, box_decay=(0.2, 0.3, 0.2, 0.3))


def shifted(base, logits, target):
    """base with the class biases of the head that ran shifted so that about `target` anchors clear conf (calibrate_cls_bias for either pair)"""
    lg = np.sort(logits.max(1).astype(np.float64))[::-1]
    k = min(max(int(target), 1), len(lg) - 1)
    delta = np.log(0.25 / 0.75) - 0.5 * (lg[k - 1] + lg[k])
    pair = "one2one_cv3." if any(".one2one_cv3." in n for n in base) else ".cv3."
    return {n: (v + np.float32(delta)).astype(np.float32) if pair in n and n.endswith(".2.bias") else v for n, v in base.items()}


def calibrated(base, ctx, frame):
    det = Detector(base, (H, W), ctx=ctx, max_batch=B, **KW)
    det.detect(frame)
    logits = det.raw_output(logits=True)[:, 4:]
    det.close()
    cand, w, n = 4 * TARGET, base, 0
    for _ in range(4):
        w = shifted(base, logits, cand)
        det = Detector(w, (H, W), ctx=ctx, max_batch=B, **KW)
        n = len(det.detect(frame))
        det.close()
        if 0.85 * TARGET <= n <= 1.15 * TARGET:
            break
        cand = max(int(cand * TARGET / max(n, 1)), 8)
    return w, n


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
    models = {}
    for label, base in (("yolov8s", synthetic_yolov8(**V8_KW)), ("yolov5su", synthetic_yolov5u(**{**DW_KW, "gain": 1.3}))):
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
    print("   (the families' boxes per frame differ, see the runs: the rates compare only as far as those do)")

    print(f"\n2. forward (gtx_detector_profile, mean of 10 passes at batch {B}) and pass tail (`postprocess` of 20 blocking passes at batch {B}, median)")
    for label, w in models.items():
        det = Detector(w, (H, W), ctx=ctx, max_batch=B, **KW)
        det.detect_dev(dptrs[0], B)
        tail = []
        for i in range(20):
            tail.append(det.detect_dev(dptrs[i % len(dptrs)], B)[0].speed["postprocess"])
        rows = det.profile(B, 10)
        fwd_ms = sum(r["total_ms"] for r in rows) / 10
        dw = sum(r["total_ms"] for r in rows if "dwconv" in r["kernel"]) / 10
        print(f"   {label:11s} forward {fwd_ms:7.3f} ms ({len(rows)} kernel families, depthwise {dw * 1e3:6.1f} us)   tail {np.median(tail) * 1e3:7.1f} us "
              f"(min {min(tail) * 1e3:.1f})   end2end {det.end2end}, sparse box {det.sparse_box()}, pad skip {det.pad_skip()}", flush=True)
        assert not det.fell_back()
        for r in rows:
            if "stem" in r["kernel"] or "front" in r["kernel"]:
                print(f"      {r['kernel']:32s} {r['launches'] // 10:4d} launches {r['total_ms'] / 10 * 1e3:9.1f} us  {r['bytes'] / 10 / 1e6:8.1f} MB  "
                      f"{r['flops'] / 10 / 1e9:8.1f} GFLOP  {100 * r['total_ms'] / 10 / fwd_ms:5.1f} % of the forward")
        det.close()

    print("\n3. the 6x6 stem launch alone, one 1920 x 1920 RGB0 image -> 960 x 960 x c0 (ops.stem6, 50 launches between two events)")
    img = np.random.default_rng(0).integers(0, 256, (1, 1920, 1920, 4), dtype=np.uint8)
    for c0 in (32, 80):
        rng = np.random.default_rng(c0)
        w108, bias = (rng.standard_normal((108, c0)) / np.sqrt(108)).astype(np.float32), (rng.standard_normal(c0) * 0.1).astype(np.float32)
        for form, dtype, es in (("split-f16x3", 2, 4), ("fp16 MFMA", 0, 2), ("exact fp32", 1, 4)):
            _, ms = ops.stem6(img, w108, bias, dtype=dtype, iters=50, ctx=ctx)
            mb = (1920 * 1920 * 4 + 960 * 960 * c0 * es) / 1e6
            print(f"   c0 = {c0:2d}  {form:12s} {ms * 1e3:8.1f} us   {mb:6.1f} MB -> {mb / ms / 1e3:6.2f} TB/s   {2 * 108 * c0 * 960 * 960 / ms / 1e9:7.2f} TFLOP/s", flush=True)
    for q in dptrs:
        ctx.dev_free(q)


if __name__ == "__main__":
    main()
