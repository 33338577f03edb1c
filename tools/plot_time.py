#!/usr/bin/env python3
"""Times the plot stage's trajectory map on one seeded workload: ~2 x 10^5 segments (4 000 tracks of 50 steps, the style of an
aggregated location: width 0.6 pt, alpha 0.45) on a 7 500 x 7 500 canvas, the k = 2 reduction of a synthetic 15 000 x 15 000 RGB
image. Reports, as medians of --repeats interleaved rounds (each round: create = upload + reduce, draw = bin + paint, encode),
the GPU's upload, reduce, bin, paint and encode milliseconds, the tile-list statistics, the paint launch's canvas traffic against
the HBM rate, and Matplotlib's Agg drawing the same lines on this machine's CPU at --agg-side pixels (one Agg run at 7 500 pixels
takes minutes; the segments are scaled with the page, so the count and the coverage share are the same).

    python tools/plot_time.py [--repeats 5] [--agg-side 2500] [--out profiles/plot_time.txt]
"""
import argparse
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT / "geo-trax_amd"), str(ROOT)]


def workload(side: int, tracks: int = 4000, steps: int = 50, seed: int = 0):
    rng = np.random.default_rng(seed)
    lines = []
    for _ in range(tracks):
        heading = rng.uniform(0, 2 * np.pi) + np.cumsum(rng.normal(0, 0.05, steps + 1))
        step = rng.uniform(2.0, 12.0) * side / 7500.0
        lines.append((rng.uniform(0, side) + np.cumsum(step * np.cos(heading)), rng.uniform(0, side) + np.cumsum(step * np.sin(heading))))
    return lines


def agg_ms(side: int, lines, lw_pt: float, alpha: float) -> float:
    from matplotlib.backends.backend_agg import FigureCanvasAgg
    from matplotlib.figure import Figure

    fig = Figure(figsize=(6.4, 6.4), dpi=side / 6.4)
    FigureCanvasAgg(fig)
    ax = fig.add_axes([0, 0, 1, 1])
    ax.set_xlim(-0.5, side - 0.5), ax.set_ylim(side - 0.5, -0.5), ax.axis("off")
    for x, y in lines:
        ax.plot(x, y, color="#76b041", lw=lw_pt, alpha=alpha)
    t0 = time.perf_counter()
    fig.canvas.draw()
    return (time.perf_counter() - t0) * 1e3


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--side", type=int, default=15000)
    ap.add_argument("--agg-side", type=int, default=2500)
    ap.add_argument("--out", type=Path, default=None)
    a = ap.parse_args()
    from geotrax_amd import _lib, plot, plot_draw as PD

    ctx = _lib.default_context(0)
    k = 2
    side = -(-a.side // k)
    rng = np.random.default_rng(1)
    tile = rng.integers(90, 160, (500, 500, 3), dtype=np.uint8)
    image = np.ascontiguousarray(np.tile(tile, (a.side // 500 + 1, a.side // 500 + 1, 1))[:a.side, :a.side])
    lines = workload(side)
    width = plot.width_px(0.6, side)
    prims = np.concatenate([PD.polyline(x, y, width, plot.to_bgr("#76b041"), 115, i) for i, (x, y) in enumerate(lines)])
    rows = {n: [] for n in ("upload_ms", "reduce_ms", "bin_ms", "paint_ms", "encode_ms")}
    st = {}
    for r in range(a.repeats + 1):                                   # round 0 warms up (code objects, allocator) and is dropped
        c = PD.PlotCanvas(ctx, image, k)
        try:
            c.draw(prims)
            t0 = time.perf_counter()
            data = c.encode_jpeg(90)
            enc = (time.perf_counter() - t0) * 1e3
            st = c.stats()
        finally:
            c.close()
        if r:
            for n in rows:
                rows[n].append(enc if n == "encode_ms" else st[n])
    med = {n: statistics.median(v) for n, v in rows.items()}
    agg_lines = workload(a.agg_side)
    agg = statistics.median(agg_ms(a.agg_side, agg_lines, 0.6, 0.45) for _ in range(3))
    touched = st["entries"] and side * side * 3 * 2                   # an upper bound: every tile read and written once
    out = [f"plot_time: {len(prims)} segments of {len(lines)} tracks, width {width:.2f} px, alpha 115/256, canvas {side} x {side} (k = {k} of {a.side} x {a.side} RGB), {a.repeats} rounds, medians",
           f"  upload {med['upload_ms']:.1f} ms ({image.nbytes / 1e6:.0f} MB from pageable host memory)   reduce {med['reduce_ms']:.2f} ms   bin {med['bin_ms']:.2f} ms (count + scan + fill + sort)"
           f"   paint {med['paint_ms']:.2f} ms   encode {med['encode_ms']:.1f} ms (forward DCT on the GPU, Huffman coding on the host, {len(data) / 1e6:.1f} MB)",
           f"  rounds: " + "  ".join(f"{n}=" + "/".join(f"{v:.2f}" for v in vs) for n, vs in rows.items()),
           f"  tile lists: {int(st['tiles'])} tiles, {int(st['entries'])} entries, mean {st['entries'] / st['tiles']:.2f} per tile, longest {int(st['max_per_tile'])}",
           f"  paint traffic: at most {touched / 1e6:.0f} MB of canvas read + written (tiles with empty lists touch nothing) + {int(st['entries']) * 44 / 1e6:.0f} MB of list records"
           f" -> {touched / 1e6 / max(med['paint_ms'], 1e-9):.0f} GB/s against ~5 000 GB/s of HBM: "
           + ("bandwidth-bound" if touched / 1e6 / max(med['paint_ms'], 1e-9) > 2500 else "not bandwidth-bound: the time is the per-entry coverage arithmetic (int64) and the longest lists"),
           f"  Matplotlib Agg, same style, {len(agg_lines)} tracks scaled to a {a.agg_side} x {a.agg_side} page, one CPU core: {agg:.0f} ms (median of 3 draws)"]
    text = "\n".join(out)
    print(text)
    if a.out:
        a.out.parent.mkdir(parents=True, exist_ok=True)
        a.out.write_text(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
