"""YOLOv8-RTDETR against rtdetr-l and YOLOv8s at the headline workload (DESIGN.md section 7c quotes it):
python tools/rtdetr_time.py (one GPU) -> profiles/yolov8_rtdetr_time.txt.

Seeded YOLOv8s-RTDETR and rtdetr-l weights, their last score head calibrated by calibrate_rtdetr_scores to ~132 queries over
conf on the first 4K synthetic frame (bench.py's box target), and bench.py's seeded YOLOv8s calibrated the same way with
calibrate_cls_bias; the same box and run, interleaved:
1. frames/s through ExtractEngine (detect + ByteTrack + stabilize; 3840 x 2160 -> 1920 x 1920, B = 2, 2 detector streams,
   4 stabilizer streams: bench.py's defaults), frames resident in HBM, 3 runs each.
2. executed GFLOP per frame (what the launches of one pass compute, from the op table) next to that rate.
3. the per-family table of each model (its totals give the forward time and GFLOP above); for the hybrid also the whole
   per-launch table of one pass at batch 2 (Detector.profile with GTX_PROFILE_PER_OP=1, mean of 10 passes), split into the
   trunk, the decoder's dense side and its query side.
python tools/rtdetr_time.py --passes N: N forward passes of the hybrid alone at batch 2 (uncalibrated weights: the same launches),
for `rocprofv3 --kernel-trace --stats -- python tools/rtdetr_time.py --passes 50`."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, "geo-trax_amd")
from geotrax_amd import _lib  # noqa: E402
from geotrax_amd.detector import Detector  # noqa: E402
from geotrax_amd.engine import ExtractEngine  # noqa: E402
from geotrax_amd.synth import make_scene  # noqa: E402
from geotrax_amd.tracker import Tracker  # noqa: E402
from geotrax_amd.weights import (calibrate_cls_bias, calibrate_rtdetr_scores, synthetic_rtdetr, synthetic_yolov8,  # noqa: E402
                                 synthetic_yolov8_rtdetr)

H, W, B, TARGET = 2160, 3840, 2, 132
KW = dict(imgsz=1920, conf=0.25, iou=0.7, max_det=1000, classes=[0, 1, 2, 3], agnostic_nms=True, half=False, rect=False)
V8_KW = dict(seed=0, nc=4, scale="s", level_bias=(0.0, -1e4, -1e4), box_weight_scale=0.002, smooth_cls=True, box_decay=(0.2, 0.3, 0.2, 0.3))


def calibrated(base, rtdetr, ctx, frame):
    det = Detector(base, (H, W), ctx=ctx, max_batch=B, **KW)
    det.detect(frame)
    logits = det.raw_output(logits=True)[:, 4:]
    det.close()
    if rtdetr:                                     # no NMS: the queries over conf are the boxes
        w = calibrate_rtdetr_scores(base, logits, 0.25, TARGET)
    else:
        cand, w = 4 * TARGET, base
        for _ in range(4):
            w = calibrate_cls_bias(base, logits, 0.25, cand)
            det = Detector(w, (H, W), ctx=ctx, max_batch=B, **KW)
            n = len(det.detect(frame))
            det.close()
            if 0.85 * TARGET <= n <= 1.15 * TARGET:
                break
            cand = max(int(cand * TARGET / max(n, 1)), 8)
    det = Detector(w, (H, W), ctx=ctx, max_batch=B, **KW)
    n = len(det.detect(frame))
    det.close()
    return w, n


def passes(n):
    ctx = _lib.default_context(0)
    frame = make_scene(seed=0, h=H, w=W).render(0, 150)
    q = ctx.dev_alloc(B * H * W * 3)
    ctx.dev_upload(q, np.ascontiguousarray(np.stack([frame] * B)))
    det = Detector(synthetic_yolov8_rtdetr(seed=0, nc=4, scale="s"), (H, W), ctx=ctx, max_batch=B, **KW)
    for _ in range(n):
        det.detect_dev(q, B)
    det.close()
    ctx.dev_free(q)
    print(f"{n} passes of yolov8s-rtdetr at batch {B}")


def main():
    if "--passes" in sys.argv:
        return passes(int(sys.argv[sys.argv.index("--passes") + 1]))
    ctx = _lib.default_context(0)
    scene = make_scene(seed=0, h=H, w=W)
    frames = [scene.render(t, 150) for t in range(64)]
    nbytes = H * W * 3
    dptrs = []
    for i in range(0, len(frames), B):
        q = ctx.dev_alloc(B * nbytes)
        ctx.dev_upload(q, np.ascontiguousarray(np.stack(frames[i:i + B])))
        dptrs.append(q)
    models = {}
    for label, base, rt in (("yolov8s", synthetic_yolov8(**V8_KW), False),
                            ("yolov8s-rtdetr", synthetic_yolov8_rtdetr(seed=0, nc=4, scale="s"), True),
                            ("rtdetr-l", synthetic_rtdetr(seed=0, nc=4), True)):
        w, n = calibrated(base, rt, ctx, frames[0])
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
            print(f"   run {rep}  {label:15s} {len(res) / dt:8.1f} frames/s  ({nd:.0f} boxes per frame)", flush=True)
    for label, v in fps.items():
        print(f"   {label:15s} median {np.median(v):8.1f} frames/s")

    for label, w in models.items():
        det = Detector(w, (H, W), ctx=ctx, max_batch=B, **KW)
        det.detect_dev(dptrs[0], B)
        fam = det.profile(B, 10)                                      # the totals come from the per-family table
        executed = sum(r["flops"] for r in fam) / 10 / B / 1e9
        fwd_ms = sum(r["total_ms"] for r in fam) / 10
        n_launch = sum(r["launches"] for r in fam) // 10
        print(f"\n2. {label}: {executed:.1f} GFLOP executed per frame; forward {fwd_ms:.3f} ms per pass of {B} = "
              f"{fwd_ms / B:.3f} ms per frame ({n_launch} launches a pass); engine median {np.median(fps[label]):.1f} frames/s")
        tables = [("per-family", fam)]
        if label == "yolov8s-rtdetr":                                 # the hybrid: every launch, and the pass in three parts
            os.environ["GTX_PROFILE_PER_OP"] = "1"
            ops = det.profile(B, 10)
            del os.environ["GTX_PROFILE_PER_OP"]
            assert len(ops) == n_launch, (len(ops), n_launch)            # one row per launch, none cut off
            dense = (".input_proj.", ".value_proj.", ".valid_mask.", ".enc_output.", ".enc_score_head.")
            parts = {"trunk (model.0-21)": [], "decoder, dense side (input_proj .. enc_score_head, mask)": [],
                     "decoder, query side (top-k, gather, box / score heads, 6 layers)": []}
            for r in ops:
                name = r["kernel"].split(" ", 1)[1]
                k = 0 if not name.startswith("model.22.") else 1 if any(d in name for d in dense) else 2
                parts[list(parts)[k]].append(r)
            print(f"   {label}: one pass at batch {B} in three parts (per-launch table, mean of 10 passes)")
            for key, rows in parts.items():
                ms = sum(r["total_ms"] for r in rows) / 10
                gf = sum(r["flops"] for r in rows) / 10 / B / 1e9
                print(f"   {key:64s} {len(rows):4d} launches {ms:7.3f} ms per pass  {gf:7.1f} GFLOP per frame")
            tables.append((f"per-launch (all {len(ops)} launches)", ops))
        for kind, rows in tables:
            print(f"3. {label}: {kind} table of one pass at batch {B} (mean of 10 passes)")
            for r in rows:
                ms = r["total_ms"] / 10
                fl = r["flops"] / 10
                rate = fl / (ms * 1e-3) / 1e12 if ms > 0 else 0.0
                print(f"   {r['kernel']:64s} {ms * 1e3:8.1f} us  {fl / 1e9:7.2f} GFLOP  {rate:6.1f} TFLOP/s")
        det.close()
    for q in dptrs:
        ctx.dev_free(q)


if __name__ == "__main__":
    main()
