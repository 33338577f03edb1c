"""Timing of the separate ReID network (`with_reid: true, model: <cls>.safetensors`; DESIGN.md section 7a quotes it):
python tools/reid_time.py (one GPU) -> profiles/reid_time.txt.

1. ReIDEncoder time per call (submit + collect, the frame already in HBM) at 0 / 1 / 50 / 100 / 300 crops of vehicle-sized boxes
   (40-200 px) in a 3840 x 2160 frame, YOLOv8-cls n and s, split-f16x3 (the default); host coefficient set-up included.
2. Per-launch times of the backbone at 100 crops (gtx_embedder_profile), their FLOP rate and fraction of the split roof
   (833 TFLOP/s of useful work); what the call takes beyond the backbone is the crop kernel, the pool, the
   host set-up and the copies.
3. Frames/s through ExtractEngine (2 detector streams, B = 2, no stabilizer) with BoT-SORT + ReID (n scale) against BoT-SORT with
   `model: auto`, same seeded YOLOv8s weights and 4K synthetic frames, gmc_method none for both.

python tools/reid_time.py --family yolo11 -> profiles/reid_time_yolo11.txt: the same three sections for YOLO11-cls n and s next to
YOLOv8-cls n and s (section 1 as the median of three rounds that visit the four networks in turn; section 3 with both n-scale
networks), and
4. the attention launch alone on the crops' 7 x 7 maps at 100 and 300 crops, 2 heads (n) and 4 heads (s), pair format: the
   small-map kernel against psa_attn_kernel forced onto the same inputs (gtx_op_psa_attention's `form`), five rounds that
   alternate the two, 200 launches each; medians (min - max)."""
import argparse
import contextlib
import sys
import time

import numpy as np

sys.path.insert(0, "geo-trax_amd")
from geotrax_amd import _lib  # noqa: E402
from geotrax_amd.reid import ReIDEncoder  # noqa: E402
from geotrax_amd.synth import make_scene  # noqa: E402
from geotrax_amd.weights import synthetic_yolo11_cls, synthetic_yolov8_cls  # noqa: E402

H, W = 2160, 3840
SPLIT_ROOF = 833e12


def boxes(n, seed=0):
    rng = np.random.default_rng(seed)
    wh = rng.uniform(40, 200, (n, 2))
    xy = rng.uniform(0, [W - 200, H - 200], (n, 2))
    return np.concatenate([xy, xy + wh], 1).astype(np.float32)


def time_call(enc, p, b, it=20):
    for _ in range(3):
        enc.submit_dev(p, H, W, [b]); enc.collect()
    t0 = time.perf_counter()
    for _ in range(it):
        enc.submit_dev(p, H, W, [b]); enc.collect()
    return 1e3 * (time.perf_counter() - t0) / it


def profile_rows(enc, p, scale):
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


def main_yolo11():
    from geotrax_amd import ops

    ctx = _lib.default_context(0)
    frame = make_scene(seed=3, h=H, w=W).render(0)
    p = ctx.dev_alloc(frame.nbytes)
    ctx.dev_upload(p, frame)
    nets = {"yolov8n-cls": synthetic_yolov8_cls(seed=0, scale="n"), "yolo11n-cls": synthetic_yolo11_cls(seed=1, scale="n"),
            "yolov8s-cls": synthetic_yolov8_cls(seed=0, scale="s"), "yolo11s-cls": synthetic_yolo11_cls(seed=2, scale="s", gain=1.5)}
    encs = {k: ReIDEncoder(t, ctx=ctx, max_crops=300) for k, t in nets.items()}
    counts = (0, 1, 50, 100, 300)
    ms = {k: {n: [] for n in counts} for k in encs}
    for _ in range(3):                                       # three rounds, the four networks in turn
        for n in counts:
            for k, enc in encs.items():
                ms[k][n].append(time_call(enc, p, boxes(n)))
    print(f"1. embedder time per call, {W}x{H} frame in HBM, boxes 40-200 px, split-f16x3, imgsz 224: median of 3 interleaved rounds (min - max)")
    for k in encs:
        for n in counts:
            v = sorted(ms[k][n])
            print(f"   {k:12s} {n:4d} crops: {v[1]:8.3f} ms per call ({v[0]:.3f} - {v[2]:.3f})" + (f"  ({1e3 * v[1] / n:7.1f} us per crop)" if n else ""))
    for k in ("yolo11n-cls", "yolo11s-cls"):
        assert not encs[k].fell_back()
        profile_rows(encs[k], p, k)
    for e in encs.values():
        e.close()
    ctx.dev_free(p)
    print("4. the attention launch alone, 7 x 7 maps, pair format, us per launch (200 launches), median (min - max) of five rounds alternating the kernels")
    rng = np.random.default_rng(0)
    for heads in (2, 4):
        pe_w, pe_b = rng.standard_normal((heads * 64, 1, 3, 3)).astype(np.float32), rng.standard_normal(heads * 64).astype(np.float32)
        for n in (100, 300, 600):
            qkv = rng.standard_normal((n, 7, 7, heads * 128)).astype(np.float32)
            t = {1: [], 2: []}
            for _ in range(5):
                for form in (2, 1):
                    t[form].append(1e3 * ops.psa_attention(qkv, pe_w, pe_b, heads, split=True, form=form, iters=200, ctx=ctx)[2])
            t = {k: sorted(v) for k, v in t.items()}
            cell = lambda v: f"{v[2]:6.1f} ({v[0]:.1f} - {v[4]:.1f})"
            print(f"   {heads} heads {n:4d} crops: psa_attn_small_kernel {cell(t[2])}   "
                  f"psa_attn_kernel {cell(t[1])}   ratio {t[1][2] / t[2][2]:.2f}")
    engine_fps({"reid v8n": nets["yolov8n-cls"], "reid 11n": nets["yolo11n-cls"]})


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


def engine_fps(models=None):
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
    models = models or {"reid n": synthetic_yolov8_cls(seed=0, scale="n")}
    print("3. frames/s through ExtractEngine (2 detector streams, B = 2, no stabilizer), YOLOv8s 1920, BoT-SORT, gmc none, 4K frames")
    for label in ("auto",) + tuple(models):
        trk = Tracker("botsort", with_reid=True, track_high_thresh=0.25, new_track_thresh=0.25)
        trk.reid_tensors = models.get(label)
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
        print(f"   {label:8s}: {len(res) / dt:7.1f} frames/s ({len(res)} frames, {nd:.0f} boxes per frame)")
        eng.close()
        for q in dptrs:
            ctx.dev_free(q)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--family", choices=["yolov8", "yolo11"], default="yolov8")
    ap.add_argument("--out", default=None, help="the report file (yolo11: profiles/reid_time_yolo11.txt; yolov8: stdout)")
    a = ap.parse_args()
    if a.family == "yolov8" and not a.out:
        main()
    else:
        path = a.out or "profiles/reid_time_yolo11.txt"
        with open(path, "w") as f, contextlib.redirect_stdout(f):
            main_yolo11() if a.family == "yolo11" else main()
        print(open(path).read())
