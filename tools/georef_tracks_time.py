"""What the georeference stage's per-track columns cost on the host and on the GPU; raw output:
profiles/georef_tracks_time.txt.

    python tools/georef_tracks_time.py [--rows 20000 240000 2400000] [--out FILE]

Synthetic track tables (tracks of about 150 rows in file order, 2 % of the rows missing, 3 % out of the frame's margin, 40 lane
quads), both backends of geotrax_amd.georeference.track_columns in one process, alternating, after a warm-up call of each:
  * wall time per backend (host clock around calls that end in a device synchronise), every repeat listed
  * medians over as many further repeats, the backends again alternating, of:
  * the host backend's parts: the chain (gtx_op_georef_points), dimensions, visibility, kinematics, lanes
  * the gpu backend's parts: weights + visibility + plan on the host, the hook, and inside it the event times of the uploads, the
    nine kernels and the downloads (gtx_georef_tracks_ms)
  * whether the two backends' columns are the same bits at that size
"""
import argparse
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "geo-trax_amd"))

ORTHO = (126.6412, 37.3951, 2.4e-7, -1.9e-7, 1.1e-9, -0.7e-9)
HOM = np.array([[1.91, 0.08, 5120.5], [-0.07, 1.88, 3310.25], [1.3e-6, -0.9e-6, 1.0]])
FRAME = (2160, 3840)
CRS = ("EPSG:4326", "EPSG:5186")
STAGES = ("chain", "visibility", "dimensions", "compaction", "gap fill", "speed", "correlate", "accel+scatter", "lanes")


def table(n_rows: int, seed: int = 0) -> dict:
    rng = np.random.default_rng(seed)
    n_tracks = max(n_rows // 150, 1)
    length = rng.integers(100, 201, n_tracks)
    start = rng.integers(0, max(n_rows // 60, 1), n_tracks)              # about 60 vehicles in a frame
    tid = np.repeat(np.arange(1, n_tracks + 1), length)
    k = np.arange(len(tid)) - np.repeat(np.cumsum(length) - length, length)
    frame = np.repeat(start, length) + k
    x = np.repeat(rng.uniform(200, 3600, n_tracks), length) + np.repeat(rng.uniform(-1.5, 1.5, n_tracks), length) * k + rng.normal(0, 0.3, len(tid))
    y = np.repeat(rng.uniform(200, 1900, n_tracks), length) + np.repeat(rng.uniform(-1, 1, n_tracks), length) * k + rng.normal(0, 0.3, len(tid))
    keep = rng.random(len(tid)) > 0.02
    tid, frame, x, y = tid[keep], frame[keep], x[keep], y[keep]
    o = np.lexsort((tid, frame))
    tid, frame, x, y = tid[o], frame[o], x[o], y[o]
    n = len(tid)
    bbox = np.column_stack((np.clip(x, 60, 3700), np.clip(y, 60, 2000), np.full(n, 40.0), np.full(n, 20.0)))
    bbox[rng.random(n) < 0.03, 0] = 22.0
    dims = np.column_stack((np.full(n, 42.0), np.full(n, 18.0)))
    return dict(tid=tid, frame=frame, x=x, y=y, bbox=bbox, dims=dims, interp=(rng.random(n) < 0.02).astype(int))


def lane_quads():
    import pandas as pd

    rows = []
    for i in range(8):
        for j in range(5):
            x0, y0 = 5000 + 1000 * i, 3200 + 900 * j
            rows.append((f"S{i}", j, x0, y0, x0 + 40, y0 + 860, x0 + 980, y0 + 900, x0 + 940, y0 + 30))
    return pd.DataFrame(rows, columns=["Section", "Lane", "tlx", "tly", "blx", "bly", "brx", "bry", "trx", "try"])


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[20_000, 240_000, 2_400_000])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from geotrax_amd import _lib, ops
    from geotrax_amd import georeference as G

    ctx = _lib.default_context(0)
    seg = lane_quads()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("georeference stage, per-track columns: host functions vs gtx_op_georef_tracks (gaussian, kernel_size 14, 29.97 fps, 40 quads)")
    for n_rows in a.rows:
        tb = table(n_rows)
        n = len(tb["tid"])
        args = (tb["tid"], tb["frame"], tb["bbox"], tb["x"], tb["y"], tb["dims"], tb["interp"], FRAME, 29.97, HOM, ORTHO, *CRS, seg, "gaussian", 14)
        run = {b: (lambda b=b: G.track_columns(*args, backend=b, ctx=ctx)) for b in ("host", "gpu")}
        out = {b: f() for b, f in run.items()}                              # warm-up of both, and the outputs to compare
        reps = 9 if n <= 50_000 else 7 if n <= 500_000 else 3
        wall = {"host": [], "gpu": []}
        for _ in range(reps):
            for b in ("host", "gpu"):
                t0 = time.perf_counter()
                run[b]()
                wall[b].append((time.perf_counter() - t0) * 1e3)
        say(f"\n{n} rows, {len(np.unique(tb['tid']))} tracks")
        for b in ("host", "gpu"):
            say(f"  {b:4s} backend wall ms: median {np.median(wall[b]):9.2f}   all " + " ".join(f"{v:.2f}" for v in wall[b]))
        say(f"  host / gpu (medians): {np.median(wall['host']) / np.median(wall['gpu']):.2f} x")
        same = {k: bool(np.array_equal(out["host"][k], out["gpu"][k], equal_nan=True)) for k in ("visibility", "speed", "accel")}
        dim = max(float(np.nanmax(np.abs(out["host"][k] - out["gpu"][k]))) for k in ("length_m", "width_m"))
        lanes = all((p == q) or (p != p and q != q) for p, q in zip(out["host"]["lane"], out["gpu"]["lane"]))
        say(f"  same bits: {same}; dimensions differ by at most {dim:.2e} m; lanes equal: {lanes}")
        # the two backends' parts, alternating like the wall times; medians of the same number of repeats
        quads = seg.iloc[:, 2:10].to_numpy(np.float64)
        host_parts, gpu_parts, kernel_ms = [], [], []
        for _ in range(reps):
            t = [time.perf_counter()]
            c = G.transform_points(tb["x"], tb["y"], HOM, ORTHO, *CRS, ctx=ctx); t.append(time.perf_counter())
            G.convert_dimensions(tb["tid"], tb["dims"], FRAME, HOM, ORTHO, *CRS); t.append(time.perf_counter())
            vis = G.calculate_visibility(tb["tid"], tb["bbox"], FRAME, 4); t.append(time.perf_counter())
            G.compute_kinematics(tb["tid"], tb["frame"], c["x_local"], c["y_local"], vis, 29.97, "gaussian", 14, is_interpolated=tb["interp"]); t.append(time.perf_counter())
            G.assign_road_section_lane(c["ortho_x"], c["ortho_y"], seg); t.append(time.perf_counter())
            host_parts.append(np.diff(t) * 1e3)
            t0 = time.perf_counter()
            w, boundary = G.kinematics_weights("gaussian", 14)
            plan = G.track_plan(tb["tid"], tb["frame"], G.calculate_visibility(tb["tid"], tb["bbox"], FRAME, 4), tb["interp"])
            t1 = time.perf_counter()
            got = ops.georef_tracks(G.georef_chain(HOM, ORTHO, *CRS), tb["x"], tb["y"], tb["bbox"], tb["dims"], tb["frame"], tb["interp"], plan, quads, w,
                                    frame_size=FRAME, visibility_margin=4, fps=29.97, boundary=boundary, ctx=ctx)
            t2 = time.perf_counter()
            gpu_parts.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3))
            kernel_ms.append(got["ms"])
        d, g, ms = np.median(host_parts, axis=0), np.median(gpu_parts, axis=0), np.median(kernel_ms, axis=0)
        say(f"  medians of {reps} runs from here on")
        say(f"  host parts ms: chain (GPU) {d[0]:.2f}, dimensions {d[1]:.2f}, visibility {d[2]:.2f}, kinematics {d[3]:.2f}, lanes {d[4]:.2f}")
        say(f"  gpu parts ms: weights + visibility + plan (host) {g[0]:.2f}, hook {g[1]:.2f} of which events: uploads {ms[9]:.3f}, "
            f"kernels {ms[11]:.3f}, downloads {ms[10]:.3f}; gap-filled points {int(plan['exp_off'][-1])}")
        say("  kernels ms: " + ", ".join(f"{name} {ms[i]:.3f}" for i, name in enumerate(STAGES)))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
