"""Timing of the separate ReID network (`with_reid: true, model: <cls>.safetensors`; DESIGN.md section 7a quotes it):
python tools/reid_time.py (one GPU) -> profiles/reid_time.txt.

1. ReIDEncoder time per call (submit + collect, the frame already in HBM) at 0 / 1 / 50 / 100 / 300 crops of vehicle-sized boxes
   (40-200 px) in a 3840 x 2160 frame, YOLOv8-cls n and s, split-f16x3 (the default); host coefficient set-up included.
2. Per-launch times of the backbone at 100 crops (gtx_embedder_profile), their FLOP rate and fraction of the split roof
   (833 TFLOP/s of useful work); what the call takes beyond the backbone is the crop kernel, the pool, the
   host set-up and the copies.
3. Frames/s through ExtractEngine (2 detector streams, B = 2, no stabilizer) with BoT-SORT + ReID (n scale) against BoT-SORT with
   `model: auto`, same seeded YOLOv8s weights and 4K synthetic frames, gmc_method none for both."""
import sys
import time

import numpy as np

sys.path.insert(0, "geo-trax_amd")
from geotrax_amd import _lib  # noqa: E402
from geotrax_amd.reid import ReIDEncoder  # noqa: E402
from geotrax_amd.synth import make_scene  # noqa: E402
from geotrax_amd.weights import synthetic_yolov8_cls  # noqa: E402

H, W = 2160, 3840
SPLIT_ROOF = 833e12


def boxes(n, seed=0):
    rng = np.random.default_rng(seed)
    wh = rng.uniform(40, 200, (n, 2))
    xy = rng.uniform(0, [W - 200, H - 200], (n, 2))
    return np.concatenate([xy, xy + wh], 1).astype(np.float32)


def main():
    ctx = _lib.default_context(0)
    frame = make_scene(seed=3, h=H, w=W).render(0)
    p = ctx.dev_alloc(frame.nbytes)
    ctx.dev_upload(p, frame)
    print(f"1. embedder time per call, {W}x{H} frame in HBM, boxes 40-200 px, split-f16x3")
    for scale in ("n", "s"):
        enc = ReIDEncoder(synthetic_yolov8_cls(seed=0, scale=scale), ctx=ctx, max_crops=300)
        for n in (0, 1, 50, 100, 300):
            b = boxes(n)
            for _ in range(3):
                enc.submit_dev(p, H, W, [b]); enc.collect()
            it = 20
            t0 = time.perf_counter()
            for _ in range(it):
                enc.submit_dev(p, H, W, [b]); enc.collect()
            ms = 1e3 * (time.perf_counter() - t0) / it
            print(f"   {scale}  {n:4d} crops: {ms:8.3f} ms per call" + (f"  ({1e3 * ms / n:7.1f} us per crop)" if n else ""))
        enc.submit_dev(p, H, W, [boxes(100)]); enc.collect()
        t0 = time.perf_counter()
        for _ in range(10):
            enc.submit_dev(p, H, W, [boxes(100)]); enc.collect()
        call_ms = 1e3 * (time.perf_counter() - t0) / 10
        rows = enc.profile(100, iters=10)
        tot_ms = sum(r[1] for r in rows)
        tot_fl = sum(r[2] for r in rows)
        print(f"2. {scale}: per-launch times of the backbone at 100 crops (mean of 10 passes, events around every launch)")
        for name, lms, fl in rows:
            rate = fl / (lms * 1e-3) if lms > 0 else 0.0
            print(f"   {name:72s} {lms * 1e3:8.1f} us  {fl / 1e9:7.2f} GFLOP  {rate / 1e12:6.1f} TFLOP/s  {rate / SPLIT_ROOF:5.3f} of roof")
        print(f"   backbone: {tot_ms:.3f} ms, {tot_fl / 1e9:.1f} GFLOP, {tot_fl / (tot_ms * 1e-3) / 1e12:.1f} TFLOP/s = "
              f"{tot_fl / (tot_ms * 1e-3) / SPLIT_ROOF:.3f} of the split roof; whole call {call_ms:.3f} ms (crop kernel, pool, "
              f"host set-up and copies: {call_ms - tot_ms:.3f} ms)")
        enc.close()
    ctx.dev_free(p)
    engine_fps()


def engine_fps():
    from geotrax_amd.detector import Detector
    from geotrax_amd.engine import ExtractEngine
    from geotrax_amd.tracker import Tracker
    from geotrax_amd.weights import calibrate_cls_bias, synthetic_yolov8

    ctx = _lib.default_context(0)
    scene = make_scene(seed=3, h=H, w=W)
    frames = [scene.render(t, 150) for t in range(0, 64 * 4, 4)]
    kw = dict(imgsz=1920, conf=0.25, iou=0.7, max_det=300, classes=[0, 1, 2, 3], agnostic_nms=True, half=False, rect=False)
    w = synthetic_yolov8(seed=0, nc=4, level_bias=(0.0, -1e4, -1e4), box_weight_scale=0.002)
    det = Detector(w, (H, W), ctx=ctx, **kw)
    det.detect(frames[0])
    w = calibrate_cls_bias(w, det.raw_output(logits=True)[:, 4:], 0.25, 130)
    det.close()
    cls = synthetic_yolov8_cls(seed=0, scale="n")
    print("3. frames/s through ExtractEngine (2 detector streams, B = 2, no stabilizer), YOLOv8s 1920, BoT-SORT, gmc none, 4K frames")
    for label in ("auto", "reid n"):
        trk = Tracker("botsort", with_reid=True, track_high_thresh=0.25, new_track_thresh=0.25)
        trk.reid_tensors = cls if label != "auto" else None
        eng = ExtractEngine(w, (H, W), kw, trk, None, batch=2, det_streams=2)
        dptrs = []
        nbytes = H * W * 3
        for i in range(0, len(frames), 2):
            q = ctx.dev_alloc(2 * nbytes)
            ctx.dev_upload(q, np.ascontiguousarray(np.stack(frames[i:i + 2])))
            dptrs.append(q)
        list(eng.run(dptrs[:5]))                            # warm-up (graph capture, first launches)
        eng.reset()
        t0 = time.perf_counter()
        res = list(eng.run(dptrs))
        dt = time.perf_counter() - t0
        nd = np.mean([len(r.xyxy) for r in res])
        print(f"   {label:7s}: {len(res) / dt:7.1f} frames/s ({len(res)} frames, {nd:.0f} boxes per frame)")
        eng.close()
        for q in dptrs:
            ctx.dev_free(q)


if __name__ == "__main__":
    main()
