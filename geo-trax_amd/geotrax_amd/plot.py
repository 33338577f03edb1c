#!/usr/bin/env python3
"""plot -- the trajectory maps of the reference's plot stage, drawn over the orthophoto in HBM on MI355X.

Host-side restatement of the trajectory half of geotrax/plot.py (:115-214 the driver and the aggregation, :270-394 which files are
read and how, :396-488 what is drawn, :740-756 where it is saved), with the same function names, flags, file conventions and
style; the pixels come from geotrax_amd.plot_draw (csrc/plot_draw.hip): the background is reduced into a BGR canvas in HBM,
every vehicle's track is one polyline blended into it, and the canvas goes to the JPEG encoder where it lies.

    results file(s) for a clip / a .txt / a .csv / a folder      determine_files_to_process, get_filepaths   :270-317
    tracks txt (image coordinates), georeferenced csv              read_trajectory_data, filter_classes        :320-393
    per-location merge of a folder's files                         aggregate_data, handle_aggregation          :168-212
    one picture per coordinate table entry                         plot_trajectories                           :396-416
    strokes / discs per vehicle, --id on top                       plot_trajectories_in_given_coordinates      :419-471   [HIP: bin + paint]
    <parent>/plots/<stem>_<name>.jpg                               save_or_show_plot                           :740-756   [HIP: JPEG encoder]

Pictures: 'Unstabilized image coordinates' and 'Stabilized image coordinates' from the tracks txt on a white page of the frame
size (y down), 'Orthophoto image coordinates' from the csv on a white page of the orthophoto's size, '... on orthophoto' over
<ortho-folder>/<location>.png and, with --plot-segmentations, '... on segmentation overlay' over <segmentation-folder>/<location>.png.

Stated differences. (1) A saved picture is a raster at the canvas's scale (JPEG, quality 90, 4:2:0), not a PDF: the reference's
vector strokes over a 300 dpi raster become strokes rasterised at orthophoto scale. (2) Matplotlib widths are points on a figure
that shrinks the orthophoto to 6.4 inches; here a width of lw points is max(0.5, lw * W_canvas / (6.4 * 72)) canvas pixels, the
same share of the picture's width. (3) An orthophoto wider or taller than the encoder's 16384 pixels is reduced by the smallest
integer factor that fits (--reduce picks another). (4) --plot-points draws discs instead of strokes (the reference adds the
scatter on top of the lines); a marker of area s points^2 is a disc of radius sqrt(s / pi) points, scaled like a width.
(5) --plot-show has no window here. (6) Axes, tick labels and the legend are not drawn: see below.

Not built: 'Local planar coordinates' and 'Geographic coordinates' (axes plots in metres / degrees without a
raster), legends and axes, the speed / acceleration / class / dimension distributions and the per-vehicle kinematics
(plot.py:491-720). They are host Matplotlib and can follow as a plain port.

Usage:  python -m geotrax_amd.plot <clip | results file | folder> [options]      (the trajectory flags of `geotrax plot`)
"""
from __future__ import annotations

import argparse
import logging
import math
import sys
from pathlib import Path

import numpy as np

from . import plot_draw as PD

VIDEO_FORMATS = (".mp4", ".mov", ".avi", ".mkv", ".mjpeg", ".mjpg")
RESULTS_FORMATS = (".txt", ".csv")
PLOT_DEFAULTS = {                                          # cfg -> plotting of the reference's default.yaml (:210-222), the keys this stage reads
    "save": True, "show": False, "aggregate": False, "plot_points": False, "use_segmentations": False, "class_filter": [],
    "colors": ["#76b041", "#3274d9", "#ff61b4", "#ff9d00", "#9954bb", "#ffc000", "#e84343", "#17becf", "#ef843c", "#2ca02c", "#8c564b", "#e377c2",
               "#7f7f7f", "#bcbd22", "#1f60c4", "#a05195"],
    "skip_filenames_with": ["bus", "ids", "transf"],
}
FIGURE_WIDTH_PT = 6.4 * 72.0                               # Matplotlib's default figure width in points
TRACK_COLUMNS = ["Frame_ID", "Vehicle_ID", "X_unstabilized", "Y_unstabilized", "W_unstabilized", "H_unstabilized", "X_stabilized", "Y_stabilized",
                 "W_stabilized", "H_stabilized", "Vehicle_Class", "Confidence", "Vehicle_Length", "Vehicle_Width"]
COORDINATES_IMG = {"Unstabilized image coordinates": ("X_unstabilized", "Y_unstabilized"), "Stabilized image coordinates": ("X_stabilized", "Y_stabilized")}
COORDINATES_GEO = {"Orthophoto image coordinates": ("Ortho_X", "Ortho_Y")}


class PlotColors:
    """data_utils.PlotColors: the configured cycle, then seeded random colours (the reference's are unseeded)."""

    def __init__(self, colors=None):
        self.colors = list(colors or [])

    def get_color(self, index: int) -> str:
        if index < len(self.colors):
            return self.colors[index]
        return "#{:06x}".format(int(np.random.default_rng(index).integers(0, 0x1000000)))


def to_bgr(color) -> tuple:
    named = {"black": "#000000", "red": "#ff0000", "white": "#ffffff"}
    c = named.get(color, color).lstrip("#")
    return int(c[4:6], 16), int(c[2:4], 16), int(c[0:2], 16)


def width_px(lw_pt: float, canvas_w: int) -> float:
    return float(min(max(0.5, lw_pt * canvas_w / FIGURE_WIDTH_PT), PD.MAX_WIDTH))


# --------------------------------------------------------------------------- which files (plot.py:270-317)

def determine_files_to_process(input_path: Path, skip_filenames_with: list, logger: logging.Logger) -> list:
    if not input_path.exists():
        logger.critical(f"File or directory '{input_path}' not found.")
        sys.exit(1)
    files = [input_path]
    if input_path.is_dir():
        files = sorted(f for f in input_path.iterdir() if (f.suffix.lower() in VIDEO_FORMATS or f.suffix in RESULTS_FORMATS)
                       and not any(word in f.stem for word in skip_filenames_with))
        if not files:
            logger.critical(f"No valid video files ({VIDEO_FORMATS}) or result files ({RESULTS_FORMATS}) found in the input folder {input_path}")
            sys.exit(1)
    return files


def get_filepaths(file: Path, ortho_folder, args, out_cfg: dict, logger: logging.Logger) -> tuple:
    from .extract import get_output_dir
    from .georef_stage import determine_location_id

    filepath_img = filepath_geo = filepath_ortho = filepath_seg = None
    if file.suffix.lower() in VIDEO_FORMATS:
        out_dir = get_output_dir(file, out_cfg)
        img = out_dir / f"{file.stem}{out_cfg.get('tracks_postfix', '')}.txt"
        geo = out_dir / f"{file.stem}{out_cfg.get('georeferenced_postfix', '')}.csv"
        filepath_img, filepath_geo = (img if img.is_file() else None), (geo if geo.is_file() else None)
    elif file.suffix == ".txt" and file.exists():
        filepath_img = file
    elif file.suffix == ".csv" and file.exists():
        filepath_geo = file
    location_id = determine_location_id(file, logger)
    if filepath_geo and ortho_folder:
        filepath_ortho = Path(ortho_folder) / f"{location_id}.png"
        if args.segmentations:
            filepath_seg = (Path(args.segmentation_folder) if args.segmentation_folder else Path(ortho_folder) / "segmentations") / f"{location_id}.png"
    return filepath_img, filepath_geo, filepath_ortho, filepath_seg, location_id


# --------------------------------------------------------------------------- what is read (plot.py:320-393)

def filter_classes(df, class_filter):
    if class_filter:
        df = df[~df["Vehicle_Class"].isin([int(c) for c in class_filter])]
    return df


def read_trajectory_data(filepath_img, filepath_geo, args, logger: logging.Logger) -> tuple:
    import pandas as pd

    from .georef_stage import detect_delimiter

    df_img = df_geo = coordinates_img = coordinates_geo = None
    if filepath_img:
        try:
            df_img = pd.read_csv(filepath_img, sep=detect_delimiter(filepath_img), header=None)
            coordinates_img = {"Unstabilized image coordinates": COORDINATES_IMG["Unstabilized image coordinates"]}
            if df_img.shape[1] >= 14:
                df_img = df_img.iloc[:, :14]
                df_img.columns = TRACK_COLUMNS
                coordinates_img = dict(COORDINATES_IMG)
            elif df_img.shape[1] in (10, 11):
                df_img = df_img.iloc[:, :10]
                df_img.columns = TRACK_COLUMNS[:6] + TRACK_COLUMNS[10:]
            else:
                raise ValueError("Invalid number of columns")
            df_img["Vehicle_Class"] = df_img["Vehicle_Class"].astype(int)
            df_img = filter_classes(df_img, args.class_filter)
        except Exception as e:
            logger.error(f"Error reading the tracking results in image coordinates: {e}")
            df_img = coordinates_img = None
    if filepath_geo:
        try:
            df_geo = pd.read_csv(filepath_geo, low_memory=False)
            coordinates_geo = dict(COORDINATES_GEO)
            df_geo["Vehicle_Class"] = df_geo["Vehicle_Class"].astype(int)
            df_geo = filter_classes(df_geo, args.class_filter)
        except Exception as e:
            logger.error(f"Error reading the tracking results in geo coordinates: {e}")
            df_geo = coordinates_geo = None
    return df_img, df_geo, (coordinates_img, coordinates_geo)


# --------------------------------------------------------------------------- what is drawn (plot.py:419-471)

def build_primitives(df, x_key: str, y_key: str, canvas_w: int, k: int, args, colors: PlotColors) -> np.ndarray:
    """One polyline (or, with --plot-points, one disc per observation) per vehicle in the reference's order and style, in canvas
    pixels: data (x, y) lies at ((x + 0.5) / k - 0.5, (y + 0.5) / k - 0.5) of a canvas reduced by k."""
    lw = 0.6 if args.save else 1.0
    alpha_max, alpha_min, alpha_step = (0.45, 0.225, 0.075) if args.save else (0.35, 0.125, 0.075)
    df = df.copy()
    df["Vehicle_ID_orig"] = df["Vehicle_ID"]
    if "Drone_ID" in df.columns:
        df["Vehicle_ID"] = "D" + df["Drone_ID"].astype(str) + "_" + df["Vehicle_ID"].astype(str)
    parts, source_index, poly = [], {}, 0

    def add(xs, ys, lw_pt, marker_area, color, alpha):
        nonlocal poly
        xs = (np.asarray(xs, np.float64) + 0.5) / k - 0.5
        ys = (np.asarray(ys, np.float64) + 0.5) / k - 0.5
        ok = np.isfinite(xs) & np.isfinite(ys) & (np.abs(xs) <= 32000) & (np.abs(ys) <= 32000)
        xs, ys = xs[ok], ys[ok]
        if not len(xs):
            return
        a = max(1, min(256, int(round(alpha * 256))))
        if args.points:
            r = max(0.25, math.sqrt(marker_area / math.pi) * canvas_w / FIGURE_WIDTH_PT)
            d = np.zeros(len(xs), PD.PRIM_DTYPE)
            d["x0"], d["y0"], d["x1"], d["y1"], d["width"], d["bgr"], d["alpha"] = xs, ys, xs, ys, min(2 * r, PD.MAX_WIDTH), PD.pack_bgr(to_bgr(color)), a
            d["poly"] = poly + np.arange(len(xs))
            poly += len(xs)
            parts.append(d)
        else:
            parts.append(PD.polyline(xs, ys, width_px(lw_pt, canvas_w), to_bgr(color), a, poly))
            poly += 1

    for vehicle_id, g in df.groupby("Vehicle_ID", sort=True):
        if args.id and vehicle_id == args.id:
            continue
        if not isinstance(vehicle_id, str):
            add(g[x_key], g[y_key], 0.5, 0.5, "black", 1.0)
        else:
            label = vehicle_id.split("_")[0]
            i = source_index.setdefault(label, len(source_index))
            add(g[x_key], g[y_key], lw, 0.4, colors.get_color(i), max(alpha_max - alpha_step * i, alpha_min))
    if args.id and args.id > 0:
        v = df[df["Vehicle_ID_orig"] == args.id]
        add(v[x_key], v[y_key], 2 * lw, 4.0, "red", 1.0)
    return np.concatenate(parts) if parts else np.zeros(0, PD.PRIM_DTYPE)


def _read_image(path: Path) -> np.ndarray:
    from PIL import Image

    Image.MAX_IMAGE_PIXELS = None                          # orthophotos are 15 000 x 15 000 (default.yaml:154)
    with Image.open(path) as im:
        if im.mode not in ("L", "RGB", "RGBA"):
            im = im.convert("RGBA" if "A" in im.getbands() or "transparency" in im.info else "RGB")
        return np.ascontiguousarray(np.asarray(im), dtype=np.uint8)


def pick_factor(h: int, w: int) -> int:
    return max(1, -(-max(h, w) // PD.MAX_SIDE))


def render(image: np.ndarray, k: int, prims: np.ndarray, backend: str, ctx=None, quality: int = 90, stats: dict | None = None) -> tuple:
    """(canvas BGR [h][w][3], JPEG bytes) of the image reduced by k with the list painted: on the GPU (PlotCanvas) or by the twin."""
    if backend == "twin":
        import io

        from PIL import Image

        canvas = PD.rasterize(PD.reduce(image, k), prims)
        buf = io.BytesIO()
        Image.fromarray(canvas[:, :, ::-1]).save(buf, "JPEG", quality=quality, subsampling=2)
        return canvas, buf.getvalue()
    from . import _lib

    c = PD.PlotCanvas(ctx or _lib.default_context(), image, k)
    try:
        c.draw(prims)
        data = c.encode_jpeg(quality)
        if stats is not None:
            stats.update(c.stats())
        return c.read(), data
    finally:
        c.close()


def save_plot(name: str, filepath: Path, canvas: np.ndarray, data: bytes, args, logger: logging.Logger) -> Path:
    """save_or_show_plot (:740-756): <parent>/plots/<stem>_<name with '_' for ' '>.jpg, and the canvas as .npy under --dump."""
    img_dir = filepath.parent / "plots"
    img_dir.mkdir(parents=True, exist_ok=True)
    out = img_dir / f"{filepath.stem}_{name.replace('(', '').replace(')', '').replace(' ', '_')}.jpg"
    out.write_bytes(data)
    if getattr(args, "dump", False):
        np.save(out.with_suffix(".npy"), canvas)
    logger.info(f"Plot saved as {out}")
    return out


def plot_trajectories(dfs: tuple, coordinates: tuple, filepaths: tuple, args, colors: PlotColors, logger: logging.Logger, ctx=None, frame_hw=None) -> list:
    """plot_trajectories (:396-416): one picture per entry of the coordinate tables, plus the raster backgrounds."""
    written = []
    filepath_ortho, filepath_seg = filepaths[2], filepaths[3]
    for i, df in enumerate(dfs):
        if df is None or coordinates[i] is None:
            continue
        for coordinate, (x_key, y_key) in coordinates[i].items():
            backgrounds = [(coordinate, None)]
            if "Orthophoto" in coordinate and filepath_ortho:
                backgrounds.append((coordinate + " on orthophoto", filepath_ortho))
            if "Orthophoto" in coordinate and filepath_seg:
                if filepath_seg.exists():
                    backgrounds.append((coordinate + " on segmentation overlay", filepath_seg))
                else:
                    logger.warning(f"Segmentation overlay PNG not found: {filepath_seg}.")
            page_hw = None
            for name, background in backgrounds:
                if background is not None:
                    try:
                        image = _read_image(background)
                    except Exception as e:
                        logger.warning(f"Could not read orthophoto '{background}': {e}")
                        continue
                    page_hw = page_hw or image.shape[:2]
                else:
                    hw = frame_hw if i == 0 and frame_hw else None
                    if hw is None and filepath_ortho and Path(filepath_ortho).exists() and i == 1:
                        hw = _read_image(filepath_ortho).shape[:2]
                    if hw is None:                         # no frame, no orthophoto: the data's own extent
                        hw = (int(min(max(np.nanmax(df[y_key]) + 2, 1), PD.MAX_SIDE)), int(min(max(np.nanmax(df[x_key]) + 2, 1), PD.MAX_SIDE)))
                    image = np.full((int(hw[0]), int(hw[1])), 255, np.uint8)
                k = getattr(args, "reduce", None) or pick_factor(*image.shape[:2])
                prims = build_primitives(df, x_key, y_key, -(-image.shape[1] // k), k, args, colors)
                canvas, data = render(image, k, prims, args.backend, ctx, args.quality)
                if args.save:
                    written.append(save_plot(name, filepaths[i], canvas, data, args, logger))
    return written


# --------------------------------------------------------------------------- the driver (plot.py:115-214)

def generate_plots(args: argparse.Namespace, logger: logging.Logger, ctx=None) -> list:
    import pandas as pd

    from .config_utils import backfill_args_from_config, load_config
    from .georef_stage import get_ortho_folder

    config = load_config(getattr(args, "cfg", None), logger)
    plot_cfg = {**PLOT_DEFAULTS, **(config.get("plotting") or {})}
    folders, out_raw = config.get("input") or {}, config.get("output") or {}
    backfill_args_from_config(args, {"save": plot_cfg["save"], "show": plot_cfg["show"], "aggregate": plot_cfg["aggregate"], "points": plot_cfg["plot_points"],
                                     "segmentations": plot_cfg["use_segmentations"], "class_filter": plot_cfg["class_filter"],
                                     "ortho_folder": Path(folders["ortho_folder"]) if folders.get("ortho_folder") else None,
                                     "segmentation_folder": Path(folders["segmentation_folder"]) if folders.get("segmentation_folder") else None,
                                     "output_folder": out_raw.get("folder", "results")})
    out_cfg = {**out_raw, "folder": args.output_folder}
    if args.show:
        logger.error("--plot-show is not part of this build: there is no window. The pictures are written with --plot-save.")
        return []
    colors = PlotColors(plot_cfg["colors"])
    files = determine_files_to_process(Path(args.input), plot_cfg["skip_filenames_with"], logger)
    ortho_folder = args.ortho_folder
    if ortho_folder is None:
        try:
            ortho_folder = get_ortho_folder(Path(args.input), None, logging.getLogger("geotrax_amd.plot.quiet"))
        except SystemExit:
            ortho_folder = None                            # plot.py:138 critical=False: no orthophoto, no raster background
    elif not Path(ortho_folder).exists():
        logger.warning(f"Orthophoto folder '{ortho_folder}' not found.")
        ortho_folder = None
    written, at_location = [], {}
    for file in files:
        filepath_img, filepath_geo, filepath_ortho, filepath_seg, location_id = get_filepaths(file, ortho_folder, args, out_cfg, logger)
        if filepath_img is None and filepath_geo is None:
            logger.warning(f"No tracking results found for {file.stem}. Skipping...")
            continue
        df_img, df_geo, coordinates = read_trajectory_data(filepath_img, filepath_geo, args, logger)
        frame_hw = None
        if file.suffix.lower() in VIDEO_FORMATS and file.is_file():
            from .frames import open_source

            reader = open_source(file)
            frame_hw = reader.frame_hw
            reader.release()
        if not args.aggregate or (df_geo is not None and "Drone_ID" in df_geo.columns):
            written += plot_trajectories((df_img, df_geo), coordinates, (filepath_img, filepath_geo, filepath_ortho, filepath_seg), args, colors, logger, ctx, frame_hw)
            continue
        for df in (df_img, df_geo):                        # aggregate_data (:168-194)
            if df is not None:
                df["Vehicle_ID"] = file.stem + "_" + df["Vehicle_ID"].astype(str)
        d = at_location.setdefault(location_id, {"img": [], "geo": [], "img_base": filepath_img.parent if filepath_img else None,
                                                 "geo_base": filepath_geo.parent if filepath_geo else None, "img_file": "agg", "geo_file": "agg",
                                                 "coordinates": coordinates, "ortho": filepath_ortho, "seg": filepath_seg, "frame_hw": frame_hw})
        d["img"].append(df_img), d["geo"].append(df_geo)
        if filepath_img:
            d["img_file"] += "_" + filepath_img.stem
            d["img_base"] = d["img_base"] or filepath_img.parent
        if filepath_geo:
            d["geo_file"] += "_" + filepath_geo.stem
            d["geo_base"] = d["geo_base"] or filepath_geo.parent
        d["coordinates"] = tuple(a or b for a, b in zip(d["coordinates"], coordinates))
    if args.aggregate and at_location:                     # handle_aggregation (:197-212)
        if args.id and args.id > 0:
            logger.warning("The vehicle ID argument is not supported when aggregating data per location ID. Ignoring the vehicle ID argument.")
            args.id = 0
        for location_id, d in at_location.items():
            imgs, geos = [x for x in d["img"] if x is not None], [x for x in d["geo"] if x is not None]
            df_img = pd.concat(imgs, ignore_index=True) if imgs else None
            df_geo = pd.concat(geos, ignore_index=True) if geos else None
            fp_img = d["img_base"] / f"{d['img_file']}.txt" if df_img is not None else None
            fp_geo = d["geo_base"] / f"{d['geo_file']}.csv" if df_geo is not None else None
            written += plot_trajectories((df_img, df_geo), d["coordinates"], (fp_img, fp_geo, d["ortho"], d["seg"]), args, colors, logger, ctx, d["frame_hw"])
    return written


def add_plotting_args(group, dest_prefix: str = "") -> None:
    """The trajectory flags of `geotrax plot` (plot.py:788-810): every default is None and is backfilled from the config."""
    B = argparse.BooleanOptionalAction
    group.add_argument("--plot-save", "-ps", dest=f"{dest_prefix}save", action=B, default=None, help="Save the pictures (.jpg).")
    group.add_argument("--plot-show", "-psh", dest=f"{dest_prefix}show", action=B, default=None, help="(not built: there is no window)")
    group.add_argument("--plot-aggregate", "-pa", dest=f"{dest_prefix}aggregate", action=B, default=None, help="Folder input: one picture per location ID.")
    group.add_argument("--plot-points", "-pp", dest=f"{dest_prefix}points", action=B, default=None, help="Discs at the observations instead of strokes.")
    group.add_argument("--plot-segmentations", "-pseg", dest=f"{dest_prefix}segmentations", action=B, default=None, help="Also draw over the lane segmentation overlay PNG.")
    group.add_argument("--plot-class-filter", "-pcf", dest=f"{dest_prefix}class_filter", type=int, nargs="+", default=None, help="Vehicle class IDs to leave out.")


def main(argv=None) -> int:
    from .extract import add_common_args, setup_logger

    ap = argparse.ArgumentParser(prog="python -m geotrax_amd.plot", description="Trajectory maps over the orthophoto")
    ap.add_argument("input", type=Path, help="A video file, a .txt / .csv results file, or a folder of them.")
    add_common_args(ap.add_argument_group("Optional arguments"))
    bg = ap.add_argument_group("Plot background arguments")
    bg.add_argument("--ortho-folder", "-orf", type=Path, default=None, help="Folder with the orthophotos (<location>.png).")
    bg.add_argument("--segmentation-folder", "-osf", type=Path, default=None, help="Folder with the segmentation overlay PNGs.")
    pg = ap.add_argument_group("Plotting arguments")
    add_plotting_args(pg)
    pg.add_argument("--id", "-i", type=int, default=0, help="Vehicle ID drawn red, on top (single-file input only).")
    pg.add_argument("--quality", type=int, default=90, help="JPEG quality of the pictures, 1..100")
    pg.add_argument("--reduce", type=int, default=None, help="Integer factor the background is reduced by (default: the smallest that fits 16384 pixels).")
    pg.add_argument("--backend", choices=["gpu", "twin"], default="gpu", help="gpu: the HIP kernels; twin: their numpy restatement (slow; for checking).")
    pg.add_argument("--dump", action="store_true", help="Also write each canvas as .npy beside its picture.")
    args = ap.parse_args(argv)
    logger = setup_logger(__name__, getattr(args, "verbose", False), getattr(args, "log_path", None))
    written = generate_plots(args, logger)
    for p in written:
        print(p)
    return 0 if written or not args.save else 1


if __name__ == "__main__":
    sys.exit(main())
