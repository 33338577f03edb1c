"""Figures of the JPEG frame source at 4K ("JPEG frame source"); raw output: profiles/jpeg_time.txt.

    python tools/jpeg_time.py [--frames 150] [--distinct 6] [--out DIR]

  * host entropy decode (gtx_jpeg_parse): ms per 4K frame on one thread, Pillow quality 90, 4:2:0, the synthetic scene
  * bytes per frame: the .jpg, the packed record, I420
  * the two kernels' GPU time per frame (events around each launch, gtx_jpeg_kernel_ms) next to gtx_yuv420_to_bgr_dev's on the
    same frame in the same loop
  * the feeder alone (read -> decode / convert -> BGR batches in HBM, a consumer that only waits): frames/s of a .mjpeg clip at
    4, 8 and 12 decode threads and of the same frames as .y4m (page cache), in one process, three passes each
  * the product's loop (geotrax_amd.extract.track_with_model: reader -> engine -> tables) on the 150-frame clip as .y4m and as
    .mjpeg at 4, 8 and 12 decode threads, in one process: `bench.py --workload cli` writes the weights, the config and the .y4m,
    this script adds the .mjpeg of the same frames (--no-loop skips it)

    python tools/jpeg_time.py --entropy [--no-loop | --only-loop] [--entropy-out profiles/jpeg_entropy_time.txt]

  the GPU entropy route (engine.jpeg_entropy: gpu) next to the host route, raw output: profiles/jpeg_entropy_time.txt
  * bytes uploaded per frame (the plan) and the host's plan() time per frame on one thread, next to parse()'s
  * the entropy chain's GPU time per frame (events around the chain, gtx_jpeg_entropy_ms) at 512 / 1024 / 2048 bits a lane, the
    rounds used, and the twin's rounds on the same frame without a GPU (--no-gpu stops after these)
  * the feeder alone and the product loop on .mjpeg with the host and the gpu route at 2 / 4 / 8 reader threads, interleaved, three
    passes each, next to the .y4m figure, with the fall-back counts of gtx_feeder_jpeg_stats

Needs Pillow (the encoder) and a GPU for the feeder part (--no-gpu skips it)."""
import argparse
import io
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "geo-trax_amd"))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=150)
    ap.add_argument("--distinct", type=int, default=6)
    ap.add_argument("--h", type=int, default=2160)
    ap.add_argument("--w", type=int, default=3840)
    ap.add_argument("--no-gpu", action="store_true")
    ap.add_argument("--no-loop", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--entropy", action="store_true", help="the GPU entropy route's figures instead of the host route's")
    ap.add_argument("--only-loop", action="store_true", help="--entropy, --restart: the product loop alone")
    ap.add_argument("--twin", action="store_true", help="--entropy: also the numpy twin's rounds on the first 4K frame (minutes of host time)")
    ap.add_argument("--restart", action="store_true", help="the restart-interval route's figures (engine.jpeg_restart: gpu) next to the host route's")
    ap.add_argument("--restart-out", default=str(ROOT / "profiles" / "jpeg_restart_time.txt"))
    ap.add_argument("--entropy-out", default=str(ROOT / "profiles" / "jpeg_entropy_time.txt"))
    a = ap.parse_args()
    if a.entropy:
        return entropy_route(a)
    if a.restart:
        return restart_route(a)
    from PIL import Image

    from geotrax_amd import _lib, jpeg
    from geotrax_amd.frames import bgr_to_i420, open_source, write_y4m
    from geotrax_amd.synth import make_scene

    h, w = a.h, a.w
    sc = make_scene(seed=0, h=h, w=w)
    frames = [sc.render(5 * t, 150) for t in range(a.distinct)]
    blobs = []
    for f in frames:
        buf = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(f[..., ::-1]), "RGB").save(buf, "JPEG", quality=90, subsampling=2)
        blobs.append(buf.getvalue())
    i420 = h * w + 2 * ((h + 1) // 2) * ((w + 1) // 2)
    recs = [jpeg.parse(b)[0] for b in blobs]
    print(f"frame {w} x {h}, Pillow quality 90, 4:2:0, {a.distinct} distinct frames of the synthetic scene")
    print(f"bytes per frame: jpg {np.mean([len(b) for b in blobs]):.0f}, record {np.mean([r.nbytes for r in recs]):.0f}, "
          f"record bound {_lib.load().gtx_jpeg_record_bound(h, w)}, I420 {i420}, BGR {h * w * 3}")
    t = []
    for _ in range(3):
        for b in blobs:
            t0 = time.perf_counter()
            jpeg.parse(b)                                          # two passes: the size query and the fill
            t.append((time.perf_counter() - t0) / 2)
    print(f"host entropy decode: {1e3 * np.median(t):.2f} ms per frame on one thread (median of {len(t)}, min {1e3 * min(t):.2f})")
    if a.no_gpu:
        return
    import ctypes as C

    from geotrax_amd.feeder import FrameFeeder

    ctx = _lib.default_context(0)
    yuv = np.frombuffer(bgr_to_i420(frames[0]), np.uint8)
    d_yuv, d_bgr = ctx.dev_alloc(yuv.nbytes), ctx.dev_alloc(h * w * 3)
    ctx.dev_upload(d_yuv, yuv)
    for rep in range(3):
        ms = (C.c_float * 3)()
        _lib.check(ctx.lib.gtx_jpeg_kernel_ms(ctx.handle, _lib.ptr(recs[0]), recs[0].nbytes, h, w, C.c_void_p(d_bgr), C.c_void_p(d_yuv), 50, ms))
        print(f"GPU time per frame, pass {rep} (mean of 50, events): jpeg_idct_kernel {ms[0]:.4f} ms, jpeg_colour_kernel {ms[1]:.4f} ms, "
              f"both {ms[0] + ms[1]:.4f} ms; yuv420_to_bgr_kernel {ms[2]:.4f} ms")
    ctx.dev_free(d_yuv)
    ctx.dev_free(d_bgr)
    out = Path(a.out) if a.out else Path(tempfile.mkdtemp())
    out.mkdir(parents=True, exist_ok=True)
    n = a.frames
    clip = out / "clip.mjpeg"
    clip.write_bytes(b"".join(blobs[k % a.distinct] for k in range(n)))
    y4m = out / "clip.y4m"
    planes = [bgr_to_i420(f) for f in frames]
    write_y4m(y4m, [planes[k % a.distinct] if k else frames[0] for k in range(n)])

    def drain(fd):
        t0 = time.perf_counter()
        k = 0
        for b in fd.batches(in_flight=2):
            b.wait_on(None)                                        # the calling thread waits for the batch to be resident
            k += b.n
        dt = time.perf_counter() - t0
        fd.close()
        return k, dt

    r = open_source(y4m)
    path, kind, off = r.raw_layout()
    r.release()
    for rep in range(3):
        fd = FrameFeeder((h, w), kind=kind, batch=2, ring=6, ctx=None, device=ctx.device)
        fd.open_file(path, off, n_threads=3)
        k, dt = drain(fd)
        print(f"feeder alone, .y4m (page cache), 3 reader threads, pass {rep}: {k} frames in {dt:.3f} s = {k / dt:.0f} frames/s")
    r = open_source(clip)
    layout = r.jpeg_layout()
    r.release()
    for threads in (4, 8, 12):
        for rep in range(3):
            fd = FrameFeeder((h, w), kind="jpeg", batch=2, ring=6, device=ctx.device)
            fd.open_jpeg(layout, n_threads=threads)
            k, dt = drain(fd)
            print(f"feeder alone, .mjpeg, {threads} decode threads, pass {rep}: {k} frames in {dt:.3f} s = {k / dt:.0f} frames/s")
    print(f"files: .mjpeg {clip.stat().st_size} bytes, .y4m {y4m.stat().st_size} bytes")
    clip.unlink()
    y4m.unlink()
    if not a.no_loop:
        product_loop(out / "loop", n)


def entropy_route(a) -> None:
    """The GPU entropy route's figures; every line goes to stdout and is appended to --entropy-out as it is produced."""
    import ctypes as C
    import io

    from PIL import Image

    from geotrax_amd import _lib, jpeg
    from geotrax_amd.frames import bgr_to_i420, open_source, write_y4m
    from geotrax_amd.synth import make_scene

    log = open(a.entropy_out, "a")

    def say(line):
        print(line, flush=True)
        log.write(line + "\n")
        log.flush()

    h, w, n = a.h, a.w, a.frames
    out = Path(a.out) if a.out else Path(tempfile.mkdtemp())
    out.mkdir(parents=True, exist_ok=True)
    if a.only_loop:
        return product_loop(out / "loop", n, routes=("host", "gpu"), thread_counts=(2, 4, 8), say=say)
    sc = make_scene(seed=0, h=h, w=w)
    frames = [sc.render(5 * t, 150) for t in range(a.distinct)]
    blobs = []
    for f in frames:
        buf = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(f[..., ::-1]), "RGB").save(buf, "JPEG", quality=90, subsampling=2)
        blobs.append(buf.getvalue())
    plans = [jpeg.entropy_plan(b) for b in blobs]
    say(f"frame {w} x {h}, Pillow quality 90, 4:2:0, {a.distinct} distinct frames of the synthetic scene; production: {jpeg.ENTROPY_SUB_BITS} bits a lane, "
        f"{jpeg.ENTROPY_ROUNDS} rounds enqueued")
    say(f"bytes uploaded per frame: plan {np.mean([p.nbytes for p in plans]):.0f} (jpg {np.mean([len(b) for b in blobs]):.0f}; "
        f"record {np.mean([jpeg.parse(b)[0].nbytes for b in blobs]):.0f} on the host route)")
    t_plan, t_parse = [], []
    for _ in range(3):
        for b in blobs:
            t0 = time.perf_counter()
            jpeg.entropy_plan(b)                                   # two passes: the size query and the fill
            t1 = time.perf_counter()
            jpeg.parse(b)
            t_plan.append((t1 - t0) / 2), t_parse.append((time.perf_counter() - t1) / 2)
    say(f"host work per frame on one thread (median of {len(t_plan)}): plan() {1e3 * np.median(t_plan):.3f} ms, parse() {1e3 * np.median(t_parse):.2f} ms")
    if a.twin:
        t0 = time.perf_counter()
        for sub in (512, 1024, 2048):
            st, _, used = jpeg.entropy_decode_plan_twin(plans[0], sub, 0, jpeg.ENTROPY_MAX_ROUNDS)
            say(f"numpy twin, frame 0, {sub} bits a lane: status {st}, {used} round(s) used ({time.perf_counter() - t0:.0f} s of host time so far)")
    if a.no_gpu:
        return
    from geotrax_amd.feeder import FrameFeeder

    ctx = _lib.default_context(0)
    def chain(pl, sub, rounds, reps):
        ms, st, used = (C.c_float * 2)(), C.c_int(), C.c_int()
        _lib.check(ctx.lib.gtx_jpeg_entropy_ms(ctx.handle, _lib.ptr(pl), pl.nbytes, sub, rounds, reps, ms, C.byref(st), C.byref(used)))
        return ms[0], ms[1], st.value, used.value

    for sub in (512, 1024, 2048):
        lanes = -(-8 * max(jpeg.plan_fields(pl)[0]["stream_bytes"] for pl in plans) // sub)
        need = [chain(pl, sub, jpeg.ENTROPY_MAX_ROUNDS, 1) for pl in plans]          # what the frames need, whatever is enqueued in production
        say(f"{sub} bits a lane: {lanes} lanes, {-(-lanes // jpeg.entropy_lanes(sub))} workgroups; with {jpeg.ENTROPY_MAX_ROUNDS} rounds enqueued: "
            f"status {sorted({r[2] for r in need})}, rounds used {min(r[3] for r in need)}..{max(r[3] for r in need)}")
        for rounds, passes, reps in ((jpeg.ENTROPY_ROUNDS, 3, 5), (jpeg.ENTROPY_MAX_ROUNDS, 1, 2)):   # (a chain that does not converge takes 0.1 s and more)
            for rep in range(passes):
                got = [chain(pl, sub, rounds, reps) for pl in plans]
                say(f"GPU time per frame, {sub} bits a lane, {rounds} rounds enqueued, pass {rep} (events, mean of {reps} x {len(plans)} frames): "
                    f"entropy chain {np.mean([g[0] for g in got]):.4f} ms, the two pixel kernels {np.mean([g[1] for g in got]):.4f} ms; "
                    f"status {sorted({g[2] for g in got})} (0 ok, 1 invalid, 2 not converged, 3 both), rounds used {min(g[3] for g in got)}..{max(g[3] for g in got)}")
    clip = out / "clip.mjpeg"
    clip.write_bytes(b"".join(blobs[k % a.distinct] for k in range(n)))
    y4m = out / "clip.y4m"
    planes = [bgr_to_i420(f) for f in frames]
    write_y4m(y4m, [planes[k % a.distinct] if k else frames[0] for k in range(n)])

    def drain(fd):
        t0 = time.perf_counter()
        k = 0
        for b in fd.batches(in_flight=2):
            b.wait_on(None)
            k += b.n
        dt = time.perf_counter() - t0
        stats = fd.jpeg_stats() if fd.kind == 2 else None
        fd.close()
        return k, dt, stats

    r = open_source(y4m)
    path, kind, off = r.raw_layout()
    r.release()
    for rep in range(3):
        fd = FrameFeeder((h, w), kind=kind, batch=2, ring=6, ctx=None, device=ctx.device)
        fd.open_file(path, off, n_threads=3)
        k, dt, _ = drain(fd)
        say(f"feeder alone, .y4m (page cache), 3 reader threads, pass {rep}: {k} frames in {dt:.3f} s = {k / dt:.0f} frames/s")
    r = open_source(clip)
    layout = r.jpeg_layout()
    r.release()
    for rep in range(3):                                          # interleaved: every pass visits every case
        for threads in (2, 4, 8):
            for route in ("host", "gpu"):
                fd = FrameFeeder((h, w), kind="jpeg", batch=2, ring=6, device=ctx.device)
                fd.open_jpeg(layout, n_threads=threads, entropy=route)
                k, dt, stats = drain(fd)
                say(f"feeder alone, .mjpeg, {route} route, {threads} reader threads, pass {rep}: {k} frames in {dt:.3f} s = {k / dt:.0f} frames/s; "
                    f"frames by GPU / host on request / host after a GPU status: {stats[0]} / {stats[1]} / {stats[2]}")
    clip.unlink()
    y4m.unlink()
    if not a.no_loop:
        product_loop(out / "loop", n, routes=("host", "gpu"), thread_counts=(2, 4, 8), say=say)


def restart_route(a) -> None:
    """The restart-interval route's figures on the clip of the other legs, recoded at one MCU row per interval and at 8 MCUs per
    interval; every line goes to stdout and is appended to --restart-out as it is produced. The host route (parse() on the
    reader threads) is measured on the same files in the same passes. The product loop comes last (--no-loop leaves it out)."""
    import ctypes as C
    import io

    from PIL import Image

    from geotrax_amd import _lib, jpeg
    from geotrax_amd.frames import open_source
    from geotrax_amd.synth import make_scene

    log = open(a.restart_out, "a")

    def say(line):
        print(line, flush=True)
        log.write(line + "\n")
        log.flush()

    h, w, n = a.h, a.w, a.frames
    out = Path(a.out) if a.out else Path(tempfile.mkdtemp())
    out.mkdir(parents=True, exist_ok=True)
    if a.only_loop:                                               # (the product loop plays bench.py's 4K clip: 240 MCUs per MCU row)
        for r in (240, 8):
            product_loop(out / f"loop_{r}", n, routes=("host", "gpu"), thread_counts=(2, 4, 8), say=say, key="jpeg_restart", restart=r)
        return
    sc = make_scene(seed=0, h=h, w=w)
    frames = [sc.render(5 * t, 150) for t in range(a.distinct)]
    plain = []
    for f in frames:
        buf = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(f[..., ::-1]), "RGB").save(buf, "JPEG", quality=90, subsampling=2)
        plain.append(jpeg.recode_with_restarts(buf.getvalue(), 0))   # the Annex K.3 tables, no markers: what the sizes are compared with
    row = jpeg.mcus_per_row(plain[0])
    say(f"frame {w} x {h}, Pillow quality 90, 4:2:0, {a.distinct} distinct frames of the synthetic scene, recoded by the host emitter; {row} MCUs per MCU row")
    ctx = None if a.no_gpu else _lib.default_context(0)
    for name, r in (("one MCU row per interval", row), ("8 MCUs per interval", 8)):
        blobs = [jpeg.recode_with_restarts(b, r) for b in plain]
        plans = [jpeg.restart_plan(b) for b in blobs]
        n_int = jpeg.restart_plan_fields(plans[0])[0]["n_intervals"]
        size, size0 = np.mean([len(b) for b in blobs]), np.mean([len(b) for b in plain])
        say(f"{name} (Ri = {r}, {n_int} intervals = lanes per frame): file {size:.0f} bytes against {size0:.0f} without markers (+{100 * (size / size0 - 1):.3f} %); "
            f"plan {np.mean([p.nbytes for p in plans]):.0f} bytes uploaded per frame")
        t_plan, t_parse = [], []
        lib = _lib.load()
        room = np.zeros(lib.gtx_jpeg_plan_intervals_bound(h, w) // 4 + 1, np.uint32).view(np.uint8)   # one call into a slot-sized buffer, as the feeder makes it
        needed = C.c_size_t()
        for _ in range(3):
            for b in blobs:
                src = np.frombuffer(b, np.uint8)
                t0 = time.perf_counter()
                rc = lib.gtx_jpeg_plan_intervals(_lib.ptr(src), len(b), 0, None, None, None, None, None, _lib.ptr(room), room.nbytes, C.byref(needed))
                t1 = time.perf_counter()
                assert rc == 0, rc
                jpeg.parse(b)                                      # two calls, each with the full scan
                t_plan.append(t1 - t0), t_parse.append((time.perf_counter() - t1) / 2)
        say(f"{name}: host work per frame on one thread (median of {len(t_plan)}): plan_intervals() {1e3 * np.median(t_plan):.3f} ms, parse() {1e3 * np.median(t_parse):.2f} ms")
        if ctx is None:
            continue
        from geotrax_amd.feeder import FrameFeeder

        for copies in (1, 2, 8):
            for rep in range(3):
                got = []
                for pl in plans:
                    ms, st = (C.c_float * 2)(), C.c_int()
                    _lib.check(ctx.lib.gtx_jpeg_restart_ms(ctx.handle, _lib.ptr(pl), pl.nbytes, copies, 5, ms, C.byref(st)))
                    got.append((ms[0], ms[1], st.value))
                say(f"{name}: GPU time per frame, {copies} frame(s) a launch, pass {rep} (events, mean of 5 x {len(plans)} frames): entropy chain "
                    f"{np.mean([g[0] for g in got]):.4f} ms, the two pixel kernels {np.mean([g[1] for g in got]):.4f} ms; status {sorted({g[2] for g in got})}")
        clip = out / "clip_restart.mjpeg"
        clip.write_bytes(b"".join(blobs[k % a.distinct] for k in range(n)))
        rd = open_source(clip)
        layout = rd.jpeg_layout()
        rd.release()
        for rep in range(3):                                      # interleaved: every pass visits every case
            for threads in (2, 4, 8):
                for route in ("host", "gpu"):
                    fd = FrameFeeder((h, w), kind="jpeg", batch=2, ring=6, device=ctx.device)
                    fd.set_jpeg_restart(route)
                    fd.open_jpeg(layout, n_threads=threads, entropy="host")
                    t0 = time.perf_counter()
                    k = 0
                    for b in fd.batches(in_flight=2):
                        b.wait_on(None)
                        k += b.n
                    dt = time.perf_counter() - t0
                    stats = fd.jpeg_restart_stats()
                    fd.close()
                    say(f"{name}: feeder alone, jpeg_restart {route}, {threads} reader threads, pass {rep}: {k} frames in {dt:.3f} s = {k / dt:.0f} frames/s; "
                        f"frames by the interval route / handed back / host after a GPU status: {stats[0]} / {stats[1]} / {stats[2]}")
        clip.unlink()
    if ctx is not None and not a.no_loop:
        for r in (row, 8):
            product_loop(out / f"loop_{r}", n, routes=("host", "gpu"), thread_counts=(2, 4, 8), say=say, key="jpeg_restart", restart=r)


def product_loop(root: Path, n: int, routes=("host",), thread_counts=(4, 8, 12), say=print, key: str = "jpeg_entropy", restart: int = 0) -> None:
    """The product's loop on the same 150 frames as .y4m and as .mjpeg, one process, warm-up run + two timed runs each."""
    import argparse as ap_
    import io
    import logging
    import subprocess

    import yaml
    from PIL import Image

    from geotrax_amd import extract as ex
    from geotrax_amd.config_utils import load_config_all
    from geotrax_amd.synth import make_scene

    root.mkdir(parents=True, exist_ok=True)
    # weights calibrated to the golden clip's box count, the config and clip.y4m: written by the benchmark's own cli workload
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--workload", "cli", "--cli-dir", str(root), "--cli-formats", "y4m", "--cli-compare-sync", "0",
                        "--cli-frames", str(n)], capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit("bench.py --workload cli failed:\n" + r.stdout[-2000:] + r.stderr[-2000:])
    h, w, pool = 2160, 3840, 6                                   # bench.py's clip: 6 renders of scene 0 played ping-pong
    sc = make_scene(seed=0, h=h, w=w)
    blobs = []
    for t in range(pool):
        buf = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(sc.render(t, 150)[..., ::-1]), "RGB").save(buf, "JPEG", quality=90, subsampling=2)
        blobs.append(buf.getvalue())
    if restart:                                                  # the same coefficients with a restart marker every `restart` MCUs (host emitter)
        from geotrax_amd import jpeg

        blobs = [jpeg.recode_with_restarts(b, restart) for b in blobs]
    order = list(range(pool)) + list(range(pool - 2, 0, -1))
    (root / "clip.mjpeg").write_bytes(b"".join(blobs[order[i % len(order)]] for i in range(n)))
    cfg = yaml.safe_load((root / "cfg.yaml").read_text())
    logger = logging.getLogger("jpeg_time")
    logger.setLevel(logging.ERROR)

    def one_run(path, cfg_path):
        a = ap_.Namespace(source=str(path), cfg=cfg_path, output_folder=None, log_path=None, verbose=False, model=None, class_names=None, conf=None,
                          classes=None, cut_frame_left=None, cut_frame_right=None, interpolate=None)
        model = ex.load_detector(a, logger)
        config = load_config_all(a, logger, model_names=model.names)
        tracks, _ = ex.track_with_model(model, config, logger)
        lr = model.last_run
        assert len(tracks) and lr["frames"] == n, (len(tracks), lr)
        return lr["loop_fps"], len(tracks)

    cases = [("clip.y4m", None, "host")] + [("clip.mjpeg", t, route) for t in thread_counts for route in routes]
    paths = {}
    for name, threads, route in cases:
        c = dict(cfg)
        c["engine"] = dict(cfg.get("engine") or {})
        if threads:
            c["engine"]["decode_threads"] = threads
            c["engine"][key] = route
        paths[(name, threads, route)] = root / f"cfg_{threads or 'y4m'}_{route}.yaml"
        paths[(name, threads, route)].write_text(yaml.safe_dump(c))
    runs = {case: [] for case in cases}
    for _ in range(3):                                            # interleaved: every pass visits every case; the first pass warms up
        for case in cases:
            runs[case].append(one_run(root / case[0], paths[case]))
    for name, threads, route in cases:
        r = runs[(name, threads, route)]
        what = f"{name}{f' at {restart} MCUs per interval' if restart else ''}, {key} {route}, {threads} decode threads" if threads else f"{name} (page cache), 3 reader threads"
        say(f"product loop, {what}: {r[1][0]:.0f} and {r[2][0]:.0f} frames/s (warm-up run {r[0][0]:.0f}); {r[1][1]} track rows")


if __name__ == "__main__":
    main()
