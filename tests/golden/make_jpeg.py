"""Writes the JPEG fixtures of tests/golden/jpeg/: every variant the decoder accepts (and one it refuses), each `.jpg` next to
Pillow's (libjpeg-turbo's) decode of it as `.npy` in BGR, so that the tests need no Pillow. Run once, by hand:

    python tests/golden/make_jpeg.py

The picture is seeded: a colour gradient plus noise plus a few hard edges (so that chroma edges exist and the fancy upsampler's
neighbours differ)."""
from pathlib import Path

import numpy as np
from PIL import Image

OUT = Path(__file__).resolve().parent / "jpeg"

# name: (w, h, Pillow save options); subsampling 0 = 4:4:4, 1 = 4:2:2, 2 = 4:2:0
FIXTURES = {
    "b8x8_444": (8, 8, dict(quality=90, subsampling=0)),
    "m16x16_420": (16, 16, dict(quality=90, subsampling=2)),
    "r17x9_420": (17, 9, dict(quality=90, subsampling=2)),
    "r33x16_422": (33, 16, dict(quality=90, subsampling=1)),
    "p70x45_444": (70, 45, dict(quality=90, subsampling=0)),
    "p70x45_422": (70, 45, dict(quality=90, subsampling=1)),
    "p70x45_420": (70, 45, dict(quality=90, subsampling=2)),
    "g9x6_gray": (9, 6, dict(quality=90)),
    "p70x45_420_opt": (70, 45, dict(quality=90, subsampling=2, optimize=True)),
    "p70x45_420_rst3": (70, 45, dict(quality=90, subsampling=2, restart_marker_blocks=3)),
    "p70x45_420_rstrow": (70, 45, dict(quality=90, subsampling=2, restart_marker_rows=1)),
    "p70x45_420_q100": (70, 45, dict(quality=100, subsampling=2)),
    "p70x45_420_q5": (70, 45, dict(quality=5, subsampling=2)),
    "w640x360_420": (640, 360, dict(quality=75, subsampling=2)),
    "t3x5_420": (3, 5, dict(quality=90, subsampling=2)),          # a chroma plane 2 samples wide: libjpeg replicates instead of filtering
    "p70x45_progressive": (70, 45, dict(quality=90, subsampling=2, progressive=True)),
}


def picture(w: int, h: int, seed: int) -> np.ndarray:
    """RGB u8 [h][w][3]: gradients per channel, noise, two rectangles and a diagonal with hard, saturated edges."""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.stack([255 * xs / max(w - 1, 1), 255 * ys / max(h - 1, 1), 255 * (1 - (xs + ys) / max(w + h - 2, 1))], -1)
    img += rng.normal(0, 12, img.shape)
    img[h // 5:h // 2, w // 4:w // 2] = (250, 10, 20)
    img[h // 2:, (2 * w) // 3:] = (5, 240, 250)
    img[np.abs(xs - ys) < 1.5] = (255, 255, 0)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def main() -> None:
    OUT.mkdir(parents=True, exist_ok=True)
    for k, (name, (w, h, opts)) in enumerate(FIXTURES.items()):
        rgb = picture(w, h, seed=100 + k)
        im = Image.fromarray(rgb[..., 1], "L") if name.endswith("gray") else Image.fromarray(rgb, "RGB")
        path = OUT / f"{name}.jpg"
        im.save(path, "JPEG", **opts)
        if "progressive" in name:
            continue                                      # refused by the decoder: no expected picture
        dec = np.asarray(Image.open(path).convert("RGB"))[..., ::-1]
        np.save(OUT / f"{name}.npy", np.ascontiguousarray(dec))
        print(f"{name}: {path.stat().st_size} bytes")


if __name__ == "__main__":
    main()
