"""YOLO26s beside YOLO11s and YOLOv10s at the headline workload (DESIGN.md section 7m quotes it):
python tools/yolo26_time.py (one GPU) -> profiles/yolo26_time.txt. The recipe of tools/yolo11_time.py / tools/yolov10_time.py.

Seeded weights of the three families (the same trunk but for YOLOv10's SCDown / CIB rows and YOLO26's SPPF and model.22), each calibrated towards ~132 boxes per frame on the first 4K synthetic frame (bench.py's
target), the same box and run (boxes of the pool differ by up to 8 %: only figures of one run compare):
1. frames/s through ExtractEngine (detect + ByteTrack + stabilize; 3840 x 2160 -> 1920 x 1920, B = 2, 2 detector streams,
   4 stabilizer streams: bench.py's defaults), frames resident in HBM; 3 runs each, interleaved, after a warm-up; the median.
2. the forward time of gtx_detector_profile (mean of 10 passes at batch 2) and the pass tail -- everything behind the forward:
   YOLO11s: score gate, sparse box branch (16 DFL bins), NMS, the copies of the rows; YOLOv10s / YOLO26s: score gate, v10_select,
   sparse box branch (16 bins / reg_max = 1), v10_rows, the copies -- as the `postprocess` figure of 20 blocking passes, the median.
3. the two reg_max = 1 box forms beside their 16-bin siblings, as launches of their own: the dense decode through the operator
   hooks (gtx_op_head_boxes / gtx_op_head_boxes_r1; wall time of the call less that of an empty call, 300 candidates on three
   levels), and the sparse launch as the difference of the tails of a default and a GTX_SPARSE_BOX=0 detector.
4. `python tools/yolo26_time.py trace` under a kernel trace: the four box kernels' own launch times (see main)."""
import sys
import time

import numpy as np

sys.path.insert(0, "geo-trax_amd")
from geotrax_amd import _lib  # noqa: E402
from geotrax_amd.detector import Detector  # noqa: E402
from geotrax_amd.engine import ExtractEngine  # noqa: E402
from geotrax_amd.synth import make_scene  # noqa: E402
from geotrax_amd.tracker import Tracker  # noqa: E402
from geotrax_amd.weights import synthetic_yolo11, synthetic_yolo26, synthetic_yolov10  # noqa: E402

H, W, B, TARGET = 2160, 3840, 2, 132
KW = dict(imgsz=1920, conf=0.25, iou=0.7, max_det=1000, classes=[0, 1, 2, 3], agnostic_nms=True, half=False, rect=False)
# bench.py's box knobs (vehicle-sized boxes on the stride-8 level); synthetic_yolo26 has no level_bias / box_decay: its boxes are 4 x 2
# strides, and yolo26_base() silences its two coarse heads afterwards, so that all three families' candidates lie on the stride-8 level
DW_KW = dict(seed=0, nc=4, scale="s", level_bias=(0.0, -1e4, -1e4), box_weight_scale=0.002, box_decay=(0.2, 0.3, 0.2, 0.3))


def yolo26_base():
    w = synthetic_yolo26(seed=0, nc=4, scale="s", box_weight_scale=0.002)
    for n in list(w):
        if n.startswith("model.23.") and "cv3." in n and n.endswith(".2.bias") and n.split(".")[3] in "12":
            w[n] = (w[n] - np.float32(1e4)).astype(np.float32)
    return w


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


def main(trace_only=False):
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
    for label, base in (("yolo11s", synthetic_yolo11(**DW_KW)), ("yolov10s", synthetic_yolov10(**DW_KW)),
                        ("yolo26s", yolo26_base())):
        if trace_only and label == "yolo11s":
            continue
        w, n = calibrated(base, ctx, frames[0])
        models[label] = w
        print(f"{label}: calibrated to {n} boxes on frame 0", flush=True)

    if trace_only:
        # 4. under a kernel trace (rocprofv3 --kernel-trace --stats -- python tools/yolo26_time.py trace): 60 blocking passes at batch B of
        # YOLOv10s and YOLO26s with the sparse box form and 60 with GTX_SPARSE_BOX=0; the trace's per-kernel averages of
        # head_sparse_box_kernel<false / true>, head_boxes_kernel and head_boxes_r1_kernel are the box forms' launch times
        import os

        for label, w in models.items():
            for sparse in ("1", "0"):
                os.environ["GTX_SPARSE_BOX"] = sparse
                det = Detector(w, (H, W), ctx=ctx, max_batch=B, **KW)
                nd = [len(det.detect_dev(dptrs[i % len(dptrs)], B)[0]) for i in range(60)]
                print(f"   {label:11s} GTX_SPARSE_BOX={sparse}: 60 passes, {np.mean(nd):.0f} boxes per frame", flush=True)
                det.close()
        return
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
        if label == "yolo26s":
            for r in rows:
                if "psa" in r["kernel"] or "pool" in r["kernel"]:
                    print(f"      {r['kernel']:32s} {r['launches'] // 10:4d} launches {r['total_ms'] / 10 * 1e3:9.1f} us  {r['bytes'] / 10 / 1e6:8.1f} MB")
        det.close()

    print("\n3. the box forms as launches of their own")
    import os

    from geotrax_amd import ops

    for label in ("yolov10s", "yolo26s"):
        tails = {}
        for sparse in ("1", "0"):
            os.environ["GTX_SPARSE_BOX"] = sparse
            det = Detector(models[label], (H, W), ctx=ctx, max_batch=B, **KW)
            det.detect_dev(dptrs[0], B)
            tails[sparse] = float(np.median([det.detect_dev(dptrs[i % len(dptrs)], B)[0].speed["postprocess"] for i in range(20)]))
            det.close()
        os.environ.pop("GTX_SPARSE_BOX")
        print(f"   {label:11s} tail with the sparse box form {tails['1'] * 1e3:7.1f} us, with the dense decode alone {tails['0'] * 1e3:7.1f} us (its 3x3 layers run in the forward)")
    rng = np.random.default_rng(0)
    sizes = ((240, 240), (120, 120), (60, 60))
    A = sum(h * w for h, w in sizes)
    anchors = np.sort(rng.choice(A, 300, replace=False)).astype(np.int32)[None]
    for label, r in (("16 bins", 64), ("reg_max 1", 4)):
        lv = [dict(feat=rng.normal(0, 1, (1, h, w, 64)).astype(np.float32), cb=64, cc=0, stride=st, wb=rng.normal(0, 0.1, (64, r)).astype(np.float32),
                   bb=np.zeros(r, np.float32)) for (h, w), st in zip(sizes, (8.0, 16.0, 32.0))]
        fn = ops.head_boxes if r == 64 else ops.head_boxes_r1
        t = {}
        for cnt in (300, 0):
            fn(lv, np.asarray([cnt], np.int32), anchors, ctx=ctx)
            ts = []
            for _ in range(10):
                t0 = time.perf_counter()
                fn(lv, np.asarray([cnt], np.int32), anchors, ctx=ctx)
                ts.append(time.perf_counter() - t0)
            t[cnt] = float(np.median(ts))
        print(f"   dense decode, {label:9s}: hook call with 300 candidates {t[300] * 1e3:8.3f} ms, with none {t[0] * 1e3:8.3f} ms (uploads of the maps included in both)")
    for q in dptrs:
        ctx.dev_free(q)


if __name__ == "__main__":
    main(trace_only=len(sys.argv) > 1 and sys.argv[1] == "trace")
