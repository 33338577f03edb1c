"""Figures of the visualize stage at 4K; raw output: profiles/visualize_time.txt.

    python tools/visualize_time.py [--frames 150] [--distinct 6] [--out FILE]

The 150-frame synthetic 4K clip (3840 x 2160, `distinct` rendered frames in a cycle, written as .y4m) with the scene's own
vehicles as tracks (~130 boxes per frame, the 15-column layout, ground-truth transforms, a georeferenced csv), default flags:
  * per frame, GPU time of the drawing launch (events around it, gtx_drawer_last_ms; the list's upload ahead of it on the stream is
    outside the events and is reported by its size) in modes 0, 1 and 3, and the list's length
  * beside it, in the same process: the JPEG encoder's chain (gtx_jpeg_enc_last_ms) and the frame warp (500 launches back to back
    between two host clock readings, a window of some 20 ms; the library has no event pair around the warp)
  * frames/s of each mode's whole run (feeder -> warp -> draw -> encoder -> .avi), two passes after a warm-up pass
  * frames/s of `python -m geotrax_amd.stabilized_video` on the same clip in the same session: the stage without the drawing
"""
import argparse
import ctypes as C
import logging
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "geo-trax_amd"))


def write_inputs(folder: Path, scene, n_frames: int, distinct: int, step: int = 5):
    """results/clip.txt, clip_vid_transf.txt, clip.csv for a clip whose frame i shows the scene at t = step * (i % distinct)."""
    res = folder / "results"
    res.mkdir()
    rows, tr, geo = [], [], []
    for i in range(n_frames):
        t = step * (i % distinct)
        raw = scene.boxes(t, 150)
        G = scene.camera(t, 150)
        tr.append([i, *np.linalg.inv(G).ravel()])
        for vid, ((x, y, w, h), (sx, sy, sw, sh), v) in enumerate(zip(raw, scene.veh_xywh, scene.veh_vel)):
            if not (0 <= x < scene.w and 0 <= y < scene.h):
                continue
            rows.append([i, vid + 1, x, y, w, h, sx + v[0] * t, sy + v[1] * t, sw, sh, vid % 4, 0.8, max(sw, sh), min(sw, sh), 0])
            geo.append(f"{vid + 1},{i},{3.6 * 29.97 * 0.03 * float(np.hypot(*v)):.3f},{vid % 3 + 1}")
    with open(res / "clip.txt", "w") as f:
        for r in rows:
            f.write(",".join(str(int(v)) if k in (0, 1, 10, 14) else f"{float(v):.6g}" for k, v in enumerate(r)) + "\n")
    np.savetxt(res / "clip_vid_transf.txt", np.array(tr), fmt="%.16g", delimiter=",")
    (res / "clip.csv").write_text("Vehicle_ID,Frame_Number,Vehicle_Speed,Lane_Number\n" + "\n".join(geo) + "\n")
    return len(rows) / n_frames


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=150)
    ap.add_argument("--distinct", type=int, default=6)
    ap.add_argument("--h", type=int, default=2160)
    ap.add_argument("--w", type=int, default=3840)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    from geotrax_amd import _lib, stabilized_video
    from geotrax_amd import visualize as V
    from geotrax_amd.frames import bgr_to_i420, write_y4m
    from geotrax_amd.synth import make_scene

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    log = logging.getLogger("visualize_time")
    log.addHandler(logging.NullHandler())
    log.propagate = False
    h, w = a.h, a.w
    ctx = _lib.default_context()
    lib = ctx.lib
    scene = make_scene(seed=0, h=h, w=w)
    frames = [np.ascontiguousarray(scene.render(5 * t, 150)) for t in range(a.distinct)]
    with tempfile.TemporaryDirectory() as d:
        d = Path(d)
        clip = d / "clip.y4m"
        planes = [bgr_to_i420(f) for f in frames]
        write_y4m(clip, [frames[0]] + [planes[i % a.distinct] for i in range(1, a.frames)])
        per_frame = write_inputs(d, scene, a.frames, a.distinct)
        say(f"clip {w} x {h}, {a.frames} frames ({a.distinct} distinct), {per_frame:.0f} boxes per frame, default flags (labels, tails of 30, line width 2), quality 90")

        names = {k: str(k) for k in range(4)}
        base = dict(V.VIZ_DEFAULTS, source=clip, cut_frame_left=0, cut_frame_right=None)
        viz_config = {"tail_length": base["tail_length"], "line_width": base["line_width"]}
        for mode in (0, 1, 3):
            for k in range(4):                              # pass 0 warms up, pass 1 reads every launch's events (it waits per frame), passes 2 and 3 run free
                stats = {} if k == 1 else None
                t0 = time.perf_counter()
                _, n = V.visualize_mode(argparse.Namespace(**base), mode, names, viz_config, {}, log, ctx=ctx, stats=stats)
                dt = time.perf_counter() - t0
                if k == 1:
                    ms, pr = np.array(stats["draw_ms"]), np.array(stats["prims"])
                    tail = ms[len(ms) // 2:]                # the tails have reached their length
                    say(f"mode {mode}: drawing launch per frame (gtx_drawer_last_ms, {len(ms)} frames): mean {ms.mean():.4f} ms, median {np.median(ms):.4f}, "
                        f"min {ms.min():.4f}, max {ms.max():.4f}; second half of the clip: median {np.median(tail):.4f} ms; primitives per frame: "
                        f"mean {pr.mean():.0f}, max {pr.max()} ({40 * pr.max() / 1024:.0f} KiB of list and boxes uploaded ahead of the launch, not in the figure)")
                elif k >= 2:
                    say(f"mode {mode}: whole run, pass {k - 1}: {n} frames in {dt:.3f} s = {n / dt:.1f} frames/s")
        for k in range(3):
            t0 = time.perf_counter()
            _, n = stabilized_video.write_stabilized(clip, d / "stab.avi", ctx=ctx, logger=log)
            dt = time.perf_counter() - t0
            if k:
                say(f"stabilized_video (warp -> encoder, no drawing), pass {k}: {n} frames in {dt:.3f} s = {n / dt:.1f} frames/s")

    # the neighbours of the drawing launch on the stream, each alone
    nbytes = h * w * 3
    src, dst = ctx.dev_alloc(nbytes), ctx.dev_alloc(nbytes)
    ctx.dev_upload(src, frames[1])
    Hm = np.ascontiguousarray(np.linalg.inv(scene.camera(5, 150)), dtype=np.float64).reshape(9)
    for k in range(3):
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(500):
            _lib.check(lib.gtx_warp_frame_dev(ctx.handle, C.c_void_p(src), h, w, _lib.ptr(Hm), C.c_void_p(dst)))
        ctx.synchronize()
        if k:
            say(f"frame warp alone, pass {k}: {1e3 * (time.perf_counter() - t0) / 500:.4f} ms per frame (500 launches back to back, host-timed)")
    enc = C.c_void_p()
    _lib.check(lib.gtx_jpeg_enc_create(ctx.handle, h, w, 90, 2, C.byref(enc)))
    rec = np.zeros(lib.gtx_jpeg_record_bound(h, w) // 4 + 1, np.uint32).view(np.uint8)
    n, ms, t_enc = C.c_size_t(), C.c_float(), []
    for k in range(24):
        _lib.check(lib.gtx_jpeg_enc_submit_dev(enc, C.c_void_p(dst)))
        _lib.check(lib.gtx_jpeg_enc_collect(enc, _lib.ptr(rec), rec.nbytes, C.byref(n)))
        _lib.check(lib.gtx_jpeg_enc_last_ms(enc, C.byref(ms)))
        if k >= 4:
            t_enc.append(ms.value)
    lib.gtx_jpeg_enc_destroy(enc)
    say(f"JPEG encoder's chain alone (gtx_jpeg_enc_last_ms, {len(t_enc)} frames): mean {np.mean(t_enc):.4f} ms, median {np.median(t_enc):.4f}")
    ctx.dev_free(src)
    ctx.dev_free(dst)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
