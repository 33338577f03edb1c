"""Inputs and float64 references for tests/test_front_ops_gpu.py: the stem (model.0), the 3x3 stride-2 layer behind it (model.1), the
1x1 layer fused behind that (model.2.cv1) and the neck's two-source 1x1 layers, one launch at a time.

Every reference works on the values the kernel's number format holds, so what is left for the bars is the kernel's own arithmetic:
a pixel is float32(v) / float32(255) (ultralytics' `im / 255`), taken as is by the exact-fp32 kernel, rounded to fp16 by the fp16
kernels, and as hi + lo (pairs()) by the split-f16x3 kernels; an intermediate that a fused launch keeps in LDS in the pair format
(the stem's output inside the front stage, model.1's output inside the post stage) is cast to fp32 and taken as hi + lo here too."""
import numpy as np

# The project's bars (tests/test_conv_k32s2_gpu.py): a split-f16x3 launch against float64 on the pair format's values, and a
# re-ordered sum between two kernel forms, both as fractions of the layer's largest value.
F64_BAR, FORMS_BAR = 2e-6, 1e-5
# The fp16 and exact-fp32 kernels against float64 (rtol, atol): tests/test_ops_gpu.py's _tol
TOL_F32, TOL_F16 = (2e-4, 2e-4), (4e-3, 4e-3)

STEM_SIZES = [(4, 64), (7, 67), (20, 200), (21, 193), (2, 2)]
FRONT_SIZES = [(32, 64), (36, 68), (38, 70), (96, 192)]


def pairs(a):
    """What the pair format keeps of an fp32 array: hi + lo, as float64 (tests/test_conv_k32s2_gpu.py's _pairs)."""
    a = np.asarray(a, np.float32)
    hi = a.astype(np.float16).astype(np.float32)
    return hi.astype(np.float64) + (a - hi).astype(np.float16).astype(np.float64)


def exact_pairs(rng, shape):
    """Values the pair format carries bit for bit (fp16 values: lo = 0): what a buffer holds before a launch."""
    return rng.standard_normal(shape).astype(np.float16).astype(np.float32)


def silu(v):
    return v / (1.0 + np.exp(-v))


def images(seed, h, w):
    """Two RGB0 frames: random bytes, and random bytes inside a ring of 255 around a ring of 0 (the values at both ends of the
    byte table, right where the patches hang over the border)."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (2, h, w, 4), dtype=np.uint8)
    img[..., 3] = 0
    b = img[1]
    if h > 2 and w > 2:
        b[1:-1, 1:-1][[0, -1], :, :3] = 0
        b[1:-1, 1:-1][:, [0, -1], :3] = 0
    b[[0, -1], :, :3] = 255
    b[:, [0, -1], :3] = 255
    return img


def px_values(img, form):
    """[n, h, w, 3] float64: the pixel values the kernel form works on. form: "f32", "f16" or "split"."""
    v = img[..., :3].astype(np.float32) / np.float32(255)
    if form == "f16":
        return v.astype(np.float16).astype(np.float64)
    return pairs(v) if form == "split" else v.astype(np.float64)


def stem_weights(seed, c0):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((27, c0)) / np.sqrt(27)).astype(np.float32), (rng.standard_normal(c0) * 0.1).astype(np.float32)


def conv_weights(seed, cout, k, cin, bias_scale=0.1):
    rng = np.random.default_rng(seed)
    return ((rng.standard_normal((cout, k, k, cin)) / np.sqrt(k * k * cin)).astype(np.float32),
            (rng.standard_normal(cout) * bias_scale).astype(np.float32))


def conv64(x, w_ohwi, bias=None, stride=1, act=1):
    """act(conv k x k / stride / pad k // 2 + bias) in float64 on NHWC data."""
    import torch

    y = torch.nn.functional.conv2d(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).permute(0, 3, 1, 2),
                                   torch.from_numpy(np.ascontiguousarray(w_ohwi, dtype=np.float64)).permute(0, 3, 1, 2),
                                   None if bias is None else torch.from_numpy(np.asarray(bias, np.float64)), stride=stride,
                                   padding=w_ohwi.shape[1] // 2)
    y = y.permute(0, 2, 3, 1).numpy()
    return silu(y) if act else y


def w27_ohwi(w27):
    """[27][c0] with row (ky * 3 + kx) * 3 + colour -> [c0][3][3][3]"""
    return np.ascontiguousarray(np.asarray(w27).reshape(3, 3, 3, -1).transpose(3, 0, 1, 2))


def stem64(img, w27, bias, form, packed=True):
    """SiLU(stem conv + bias) in float64. The packed fp16 kernel holds its weights in fp16; every other form works on fp32
    weights (the split kernel on their 22-bit hi + lo split, which its bar covers)."""
    w = np.asarray(w27, np.float32)
    if form == "f16" and packed:
        w = w.astype(np.float16).astype(np.float32)
    return conv64(px_values(img, form), w27_ohwi(w), bias, stride=2)


def held(y):
    """A float64 intermediate as the pair format holds it: cast to fp32, then hi + lo."""
    return pairs(y.astype(np.float32))


def tap_map_case(h, w):
    """An image whose 27 values under any 3 x 3 window all differ, and one-hot stem weights: channel c reads tap c % 9 of colour
    (c // 9) % 3 and nothing else. Returns img [2, h, w, 4], w27 [27, 32], and (tap, colour) per channel."""
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.zeros((2, h, w, 4), np.uint8)
    for ch in range(3):
        img[0, ..., ch] = ((yy % 3) * 3 + xx % 3) * 27 + ch * 9 + (yy // 3 + xx // 3) % 9          # at most 8 * 27 + 18 + 8 = 242
        img[1, ..., ch] = 255 - img[0, ..., ch]
    w27 = np.zeros((27, 32), np.float32)
    sel = [(c % 9, (c // 9) % 3) for c in range(32)]
    for c, (tap, col) in enumerate(sel):
        w27[tap * 3 + col, c] = 1.0
    return img, w27, sel


def tap_map64(img, sel, form):
    """SiLU of the selected neighbour (0 beyond the border), by indexing: no convolution involved."""
    px = px_values(img, form)
    n, h, w, _ = px.shape
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    padded = np.zeros((n, 2 * ho + 1, 2 * wo + 1, 3))
    padded[:, 1:h + 1, 1:w + 1] = px
    out = np.zeros((n, ho, wo, len(sel)))
    for c, (tap, col) in enumerate(sel):
        ky, kx = divmod(tap, 3)
        out[..., c] = padded[:, ky:ky + 2 * ho:2, kx:kx + 2 * wo:2, col]       # padded row 2 oy + ky = image row 2 oy - 1 + ky
    return silu(out)


def upsample2x(a):
    return a.repeat(2, axis=1).repeat(2, axis=2)


def rel(a, b, scale):
    return float(np.abs(np.asarray(a, np.float64) - b).max() / scale)


def tol_ratio(got, ref, tol):
    """Largest |got - ref| / (atol + rtol |ref|): below 1 is what assert_allclose accepts."""
    rtol, atol = tol
    return float((np.abs(got.astype(np.float64) - ref) / (atol + rtol * np.abs(ref))).max())
