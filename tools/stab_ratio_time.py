#!/usr/bin/env python
"""ORB stabilization away from downsample_ratio 0.5, measured: appends labelled lines to profiles/stab_ratio_time.txt.

1. The product loop, `python -m geotrax_amd.extract clip.y4m`, on a synthetic 150-frame 3840 x 2160 .y4m (six distinct renders played
   ping-pong, written once, read from the page cache afterwards), one process per run:
     * `--cfg stable` (ORB at ratio 1.0, CLAHE, 4000 / 8000 features) on every LABEL=TREE given, the trees taking turns --rounds
       times in one session (this commit beside a built tree of its parent: `this=. parent=../parent-tree`);
     * the default config at ratio 0.75, 0.25 and 0.5 on the first tree.
   Per run, from its own log: "Average stabilization time", the loop's wall-clock frames/s (the pipelined engine's line; the
   frame-at-a-time loop does not print one), the reference's convention frames / (detector + stabilizer time), and frames over the
   whole process's wall time, set-up included -- the one figure taken the same way on every route.
2. The gray kernels alone on one 4K frame in HBM (gtx_op_gray_resize_ms: events around --reps launches after 3 untimed ones):
   gray_resize_kernel at 0.75 and 0.25 beside gray_kernel at 1.0 and 0.5.

Every extract run has a time limit; a run that is killed at it, or ends with a signal, an abort or a fault, ends the tool: what was
measured until then is written, nothing more is started on the GPU. Nothing is asserted; without a GPU the tool fails."""
import argparse
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "geo-trax_amd"))


def write_clip(path: Path, frames: int, hw, pool: int = 6, seed: int = 0):
    from geotrax_amd.frames import bgr_to_i420, write_y4m
    from geotrax_amd.synth import make_scene

    scene = make_scene(seed=seed, h=hw[0], w=hw[1])
    renders = [scene.render(t, 150) for t in range(pool)]
    planes = [bgr_to_i420(f) for f in renders]
    order = list(range(pool)) + list(range(pool - 2, 0, -1))
    seq = [order[i % len(order)] for i in range(frames)]
    write_y4m(path, [planes[t] if k else renders[t] for k, t in enumerate(seq)])      # the first item tells write_y4m the size
    return renders[0]


class GpuTrouble(RuntimeError):
    """A GPU run hung or ended with a fault: the tool writes what it has and starts nothing more."""


def run_extract(label: str, tree: Path, clip: Path, tmp: Path, cfg_text: str, frames: int, limit_s: float = 180.0):
    pkg = tree.resolve() / "geo-trax_amd"
    cfg_path = tmp / f"cfg_{label}.yaml"
    cfg_path.write_text(cfg_text)
    env = dict(os.environ, PYTHONPATH=str(pkg))
    t0 = time.perf_counter()
    try:
        p = subprocess.run([sys.executable, "-m", "geotrax_amd.extract", str(clip), "--cfg", str(cfg_path), "--output-folder", str(tmp / f"out_{label}"), "-v"],
                           capture_output=True, text=True, cwd=tmp, env=env, timeout=limit_s)
    except subprocess.TimeoutExpired as e:                     # the child is killed: it counts as hung, nothing more is started on the GPU
        raise GpuTrouble(f"{label}: no result after {limit_s} s\n" + str((e.stdout or b"")[-2000:]))
    wall = time.perf_counter() - t0
    if p.returncode < 0 or p.returncode in (124, 134, 137, 139):   # a signal, an abort, a fault, a time limit: stop here
        raise GpuTrouble(f"{label}: the run ended with status {p.returncode}\n" + (p.stdout + p.stderr)[-3000:])
    text = p.stdout + p.stderr
    stab = re.search(r"Average stabilization time:\s*([0-9.]+)ms", text)
    loop = re.search(r"stages overlapped:\s*([0-9.]+)fps", text)
    conv = re.search(r"Average pipeline time:\s*([0-9.]+)fps", text)
    tr = tmp / f"out_{label}" / f"{clip.stem}_vid_transf.txt"
    rows = len(tr.read_text().splitlines()) if tr.is_file() else 0
    line = (f"{label}: frames={frames} rc={p.returncode} transform_rows={rows} stab_ms_per_frame={stab.group(1) if stab else 'n/a'} "
            f"loop_frames_per_s={loop.group(1) if loop else 'n/a (frame-at-a-time loop)'} detector_plus_stabilizer_frames_per_s={conv.group(1) if conv else 'n/a'} "
            f"process_wall_s={wall:.1f} frames_per_process_wall_s={frames / wall:.2f}")
    print(line, flush=True)
    if p.returncode != 0 or not rows:
        print(text[-3000:], flush=True)
    return line


def kernel_lines(frame: np.ndarray, reps: int):
    from geotrax_amd import _lib
    from geotrax_amd.stabilizer import working_size

    ctx = _lib.default_context()
    h, w = frame.shape[:2]
    src, dst = ctx.dev_alloc(frame.nbytes), ctx.dev_alloc(h * w)
    lines = []
    try:
        ctx.dev_upload(src, frame)
        for ratio in (0.75, 0.25, 1.0, 0.5):
            gh, gw = working_size((h, w), ratio)
            ms = C.c_float()
            _lib.check(ctx.lib.gtx_op_gray_resize_ms(ctx.handle, C.c_void_p(src), h, w, ratio, C.c_void_p(dst), gh, gw, reps, C.byref(ms)))
            kern = "gray_kernel" if ratio in (0.5, 1.0) else "gray_resize_kernel"
            # bytes the launch has to move at least: the frame's bytes once (bilinear at ratios below 1/2 skips source pixels, but
            # not whole 64-byte lines before about 1/8) and the gray image once
            moved = frame.nbytes + gh * gw
            lines.append(f"kernel {kern} ratio={ratio}: frame={w}x{h} gray={gw}x{gh} us_per_frame={1000 * ms.value:.1f} (mean of {reps} launches between two events) "
                         f"frame_plus_gray_bytes={moved} achieved_GB_per_s={moved / (ms.value * 1e-3) / 1e9:.0f}")
            print(lines[-1], flush=True)
    finally:
        ctx.dev_free(src)
        ctx.dev_free(dst)
    return lines


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("trees", nargs="+", metavar="LABEL=TREE", help="built repository trees; the first one also runs the ratio sweep")
    ap.add_argument("--frames", type=int, default=150)
    ap.add_argument("--hw", type=int, nargs=2, default=(2160, 3840))
    ap.add_argument("--rounds", type=int, default=2, help="times the trees take turns on the stable preset")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--limit", type=float, default=180.0, help="seconds one extract run may take before it is killed and the tool stops")
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "stab_ratio_time.txt")
    args = ap.parse_args(argv)
    trees = [(item.partition("=")[0], Path(item.partition("=")[2])) for item in args.trees]
    model = "extraction: {model: 'synthetic:1'}\n"
    lines = [f"# tools/stab_ratio_time.py {' '.join(args.trees)} --frames {args.frames} --hw {args.hw[0]} {args.hw[1]} --rounds {args.rounds}"]
    with tempfile.TemporaryDirectory() as tmp:
        tmp = Path(tmp)
        clip = tmp / "clip.y4m"
        t0 = time.perf_counter()
        frame0 = write_clip(clip, args.frames, args.hw)
        print(f"clip of {args.frames} frames written in {time.perf_counter() - t0:.1f} s", flush=True)
        rc = 0
        try:
            lines += kernel_lines(frame0, args.reps)
            for k in range(args.rounds):
                for label, tree in trees:
                    lines.append(run_extract(f"stable-{label}-run{k}", tree, clip, tmp, "_base: stable\n" + model, args.frames, args.limit))
            for ratio in (0.75, 0.25, 0.5):
                lines.append(run_extract(f"default-ratio{ratio}-{trees[0][0]}", trees[0][1], clip, tmp,
                                         f"_base: default\nstabilo: {{downsample_ratio: {ratio}}}\n" + model, args.frames, args.limit))
        except GpuTrouble as e:
            print(e, flush=True)
            lines.append(f"# stopped: {str(e).splitlines()[0]}")
            rc = 1
    args.out.parent.mkdir(parents=True, exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
