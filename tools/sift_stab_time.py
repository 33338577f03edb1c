#!/usr/bin/env python
"""Frames/s and stabilizer ms per frame of `python -m geotrax_amd.extract` with `stabilo: {detector_name: rsift}` on a synthetic
3840 x 2160 clip (150 frames), for one or more built repository trees in one go, appended as labelled lines to
profiles/sift_stab_time.txt.

The clip is rendered once (host processes, no GPU) into a memory-mapped .npy file that every run then reads, so the source costs a
page-cache read per frame and not a render. Each LABEL=TREE is measured on that clip, one after the other:

    python tools/sift_stab_time.py pipelined=. parent-blocking=../parent-worktree

On this commit the run is the pipelined engine with SiftStabilizer; on a tree of the parent commit it is the blocking loop with one
gtx_register_images call per frame. Reported per tree, from the run's own log: "Average stabilization time" (the pipelined route
logs the stream-ordered GPU time of a pass, last_ms; the blocking route the wall time of its blocking call, which is all it has),
the log's frames/s line (pipelined: wall clock over the loop, stages overlapped; blocking: the reference's convention,
frames / (detector + stabilizer time)), and frames / the whole process's wall time, set-up included, which is the one figure taken
the same way on both. Nothing is asserted."""
import argparse
import os
import re
import subprocess
import sys
import tempfile
import time
from concurrent.futures import ProcessPoolExecutor
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent


def _render(job):
    path, shape, seed, lo, hi = job
    sys.path.insert(0, str(ROOT / "geo-trax_amd"))
    from geotrax_amd.synth import make_scene

    clip = np.load(path, mmap_mode="r+")
    sc = make_scene(seed=seed, h=shape[1], w=shape[2])
    for t in range(lo, hi):
        clip[t] = sc.render(t, shape[0])
    clip.flush()
    return hi - lo


def render_clip(path: Path, frames: int, hw, seed: int = 4, workers: int = 8):
    shape = (frames, hw[0], hw[1], 3)
    np.lib.format.open_memmap(path, mode="w+", dtype=np.uint8, shape=shape).flush()
    step = -(-frames // workers)
    jobs = [(str(path), shape, seed, lo, min(lo + step, frames)) for lo in range(0, frames, step)]
    with ProcessPoolExecutor(max_workers=workers) as pool:
        assert sum(pool.map(_render, jobs)) == frames


def measure(label: str, tree: Path, clip: Path, tmp: Path, detector: str, frames: int, hw):
    import yaml

    pkg = tree.resolve() / "geo-trax_amd"
    cfg = yaml.safe_load((pkg / "geotrax_amd" / "cfg" / "default.yaml").read_text()) if (pkg / "geotrax_amd" / "cfg" / "default.yaml").is_file() else None
    if cfg is None:
        sys.path.insert(0, str(pkg))
        from geotrax_amd.config_utils import DEFAULT_CFG

        cfg = yaml.safe_load(Path(DEFAULT_CFG).read_text())
    cfg["stabilo"].update(detector_name=detector, downsample_ratio=0.5, filter_type="ratio", transformation_type="projective", clahe=False,
                          sift_enable_precise_upscale=True)
    cfg["extraction"]["model"] = "synthetic:1"
    cfg_path = tmp / f"cfg_{label}.yaml"
    cfg_path.write_text(yaml.safe_dump(cfg))
    env = dict(os.environ, PYTHONPATH=str(pkg))
    t0 = time.perf_counter()
    p = subprocess.run([sys.executable, "-m", "geotrax_amd.extract", str(clip), "--cfg", str(cfg_path), "--output-folder", str(tmp / f"out_{label}"), "-v"],
                       capture_output=True, text=True, cwd=tmp, env=env)
    wall = time.perf_counter() - t0
    text = p.stdout + p.stderr
    stab = re.search(r"Average stabilization time:\s*([0-9.]+)ms", text)
    loop = re.search(r"stages overlapped:\s*([0-9.]+)fps", text)
    conv = re.search(r"Average pipeline time:\s*([0-9.]+)fps", text)
    line = (f"{label}: detector={detector} frames={frames} frame={hw[1]}x{hw[0]} rc={p.returncode} stab_ms_per_frame={stab.group(1) if stab else 'n/a'} "
            f"loop_frames_per_s={loop.group(1) if loop else 'n/a'} detector_plus_stabilizer_frames_per_s={conv.group(1) if conv else 'n/a'} "
            f"process_wall_s={wall:.1f} frames_per_process_wall_s={frames / wall:.2f}")
    print(line, flush=True)
    if p.returncode != 0 or not stab:
        print(text[-3000:], flush=True)
    return line


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("trees", nargs="+", metavar="LABEL=TREE", help="built repository trees to measure, in this order")
    ap.add_argument("--frames", type=int, default=150)
    ap.add_argument("--hw", type=int, nargs=2, default=(2160, 3840))
    ap.add_argument("--detector", default="rsift")
    ap.add_argument("--workers", type=int, default=8, help="host processes that render the clip")
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "sift_stab_time.txt")
    args = ap.parse_args(argv)
    with tempfile.TemporaryDirectory() as tmp:
        tmp = Path(tmp)
        clip = tmp / "clip.npy"
        t0 = time.perf_counter()
        render_clip(clip, args.frames, args.hw, workers=args.workers)
        print(f"clip of {args.frames} frames rendered in {time.perf_counter() - t0:.1f} s", flush=True)
        lines = []
        for item in args.trees:
            label, _, tree = item.partition("=")
            lines.append(measure(label, Path(tree), clip, tmp, args.detector, args.frames, args.hw))
    args.out.parent.mkdir(parents=True, exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
