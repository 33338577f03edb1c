"""GMC method ecc (csrc/ecc.hip) kernel by kernel and one iteration at a time against oracle/ecc_ref.py, on the maps, borders and exits
its rendered scenes (tests/test_ecc_gpu.py) never reach: rotations that make the sin terms of the Jacobian carry weight, source
positions that are negative, outside or on a fixed-point tie, masks of 37 and of 0 pixels, a singular Hessian, every way
ecc_update_kernel can end, partial thread blocks of the prepare and gradient kernels, thread blocks of the reductions that own no
pixel or two per thread, and an iteration cap on and off the boundary of collect()'s batches of six launches.
Hooks: gtx_op_ecc_prepare, gtx_op_ecc_iterate (geotrax_amd.ops.ecc_prepare / ecc_iterate). Every case first asserts, from the
oracle alone, that its input reaches the branch it is there for.

The two bounds on sums are computed, not chosen. The kernels and the oracle run the same float32 operations per pixel with
contraction off, and the product of two float32 values is exact in float64, so the per-pixel terms are the same numbers on both
sides and only the order of the float64 additions differs: N - 1 additions in any order stay within N 2^-53 sum|terms| of the exact
sum (N = h w), which math.fsum of the oracle's terms gives. Where the terms are integers (integer translations of uint8-valued
images: every partial sum is an integer below 2^53) the sums must be equal.
The map after the step is asked to one float32 ulp: its inputs are the GPU's own totals, every operation but asin, cos and sin (in
float64, from two maths libraries) is shared bit for bit, and a last-bit difference in those can move the float32 rounding to the
neighbouring value and no further.

Seeds: the 37 x 53 pair and the other iterate pairs are smooth(h, w, seed=4) and its roll by (1, 2); the textured template of the
stripes cases is the same; the 75 x 107 frame pair of the product object is smooth(75 + 8, 107 + 8, seed=21) cut at (4, 4) and at
(2, 0): a shift by (2, 4) full-resolution pixels. Seed 4 is the first of 0..299 with which every map of the table ends in the oracle
as its case needs (the rotated and half-pixel maps take a step, 37 and 672 pixels give status 2, the stripes fit ends after two
iterations); with seed 4 the frame pair's fits end after exactly 6 iterations, on the batch boundary, so the pair has its own: 21 is
the first of 0..119 whose fits end with status 0 after 8 (exact) and 9 (fixed) iterations, inside the second batch."""
import functools
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K_BLOCKS, K_THREADS, K_SUMS = 512, 256, 13              # csrc/ecc.hip: kBlocks, kThreads, kSums
HW = (37, 53)
SEED = 4
OBJECT_SEED = 21
EPS = 1e-6
FILL = np.uint64(0xFFFFFFFFFFFFFFFF)                    # the hook fills the partial buffer with 0xFF bytes before the stats launch

# name -> ((theta, tx, ty), pixels under the mask at 37 x 53: a property of the coordinates alone, the same in both warp forms)
MAPS = {
    "identity": ((0.0, 0.0, 0.0), 1961),
    "rot+0.5": ((0.5, 10.0, -12.0), 1611),
    "rot-0.3": ((-0.3, -7.3, -4.6), 1218),
    "half_pixel": ((0.0, 0.5, -0.5), 1924),
    "one_column": ((0.0, 52.0, 0.0), 37),
    "outside_right": ((0.0, 53.5, 0.0), 0),
    "outside_up_left": ((0.0, -55.0, -39.0), 0),
    "quarter_turn": ((math.pi / 2, 20.0, 5.0), 672),
    "tie_1_64": ((0.0, 1.0 / 64, -1.0 / 64), None),      # the fixed-point position's rounding tie (1/32-pixel steps)
    "tie_1_2": ((0.0, -0.5, 0.5), None),                 # the nearest-neighbour mask's rounding tie
}
INTEGER_TRANSLATIONS = ("identity", "one_column", "outside_up_left")
ROTATIONS = ("rot+0.5", "rot-0.3", "quarter_turn")
STEP_MAPS = ("identity", "rot+0.5", "rot-0.3", "half_pixel", "tie_1_64", "tie_1_2")
WARPS = ("exact", "fixed")


def map_of(theta, tx, ty):
    c, s = np.float32(math.cos(theta)), np.float32(math.sin(theta))
    return np.array([[c, -s, tx], [s, c, ty]], np.float32)


def smooth(h, w, seed=SEED, k=2, passes=2):
    """Low-passed noise rescaled to 0..255 and rounded (box filter of 2k + 1, `passes` times, periodic) -> uint8 [h, w]."""
    a = np.random.default_rng(seed).random((h, w))
    for _ in range(passes):
        c = np.cumsum(np.pad(a, ((k + 1, k), (0, 0)), mode="wrap"), 0)
        a = c[2 * k + 1:] - c[:-2 * k - 1]
        c = np.cumsum(np.pad(a, ((0, 0), (k + 1, k)), mode="wrap"), 1)
        a = c[:, 2 * k + 1:] - c[:, :-2 * k - 1]
    a = (a - a.min()) / (a.max() - a.min())
    return np.round(a * 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def pair(h, w):
    """(template, image) float32 [h, w] of uint8 values: a smooth texture and the same array rolled by (1, 2)."""
    t = smooth(h, w)
    a, b = t.astype(np.float32), np.roll(t, (1, 2), (0, 1)).astype(np.float32)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


@functools.lru_cache(maxsize=None)
def stripes(h, w):
    """Constant along y: gy == 0 at every pixel."""
    a = np.ascontiguousarray(np.broadcast_to(smooth(h, w)[h // 2][None, :], (h, w))).astype(np.float32)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def trace(name, warp, hw=HW, kind="pair"):
    """The oracle's iteration from the starting state on one of the inputs above; computed once, shared, never written to."""
    from oracle import ecc_ref

    t, i = pair(*hw) if kind == "pair" else (pair(*hw)[0], stripes(*hw)) if kind == "stripes" else (np.full(hw, 100, np.float32),) * 2
    return ecc_ref.iteration(t, i, map_of(*MAPS[name][0]) if isinstance(name, str) else map_of(*name), -1.0, -EPS, warp)


@functools.lru_cache(maxsize=None)
def gpu(ctx, name, warp, hw=HW, kind="pair"):
    """One gtx_op_ecc_iterate call from the starting state, shared by the tests that look at its stages."""
    from geotrax_amd import ops

    t, i = pair(*hw) if kind == "pair" else (pair(*hw)[0], stripes(*hw)) if kind == "stripes" else (np.full(hw, 100, np.float32),) * 2
    return ops.ecc_iterate(t, i, map_of(*MAPS[name][0]) if isinstance(name, str) else map_of(*name), exact=warp == "exact", eps=EPS, ctx=ctx)


def owning_blocks(n_px):
    """Blocks of the 512 x 256 grid-stride loop that own at least one pixel."""
    return np.unique((np.arange(n_px) // K_THREADS) % K_BLOCKS)


def reduce_partials(col):
    """reduce_partials of csrc/ecc.hip on one column of the partial buffer: the same float64 additions in the same order."""
    acc = (0.0 + col[:K_THREADS]) + col[K_THREADS:]
    o = K_THREADS // 2
    while o > 0:
        acc = acc[:o] + acc[o:2 * o]
        o //= 2
    return float(acc[0])


def totals(partial, n):
    return np.array([reduce_partials(partial[:, k]) for k in range(n)])


def order_bound(terms):
    return terms.size * 2.0 ** -53 * math.fsum(np.abs(terms).ravel())


def check_empty_blocks(r, n_px, done=False):
    own = owning_blocks(n_px)
    empty = np.setdiff1d(np.arange(K_BLOCKS), own)
    bits_s, bits_a = r["partial_stats"].view(np.uint64), r["partial_accum"].view(np.uint64)
    if done:
        assert (bits_s == FILL).all() and (bits_a == FILL).all()
        return
    assert (bits_s[:, 5:] == FILL).all()                                 # the stats kernel writes 5 of the 13 columns
    assert (bits_s[empty, :5] == 0).all() and (bits_a[empty] == 0).all()  # +0.0, not what was there
    assert np.isfinite(r["partial_stats"][:, :5]).all() and np.isfinite(r["partial_accum"]).all()


def check_stats(r, tr, n_px, integer):
    """-> the GPU's own totals of the 5 sums (its reduction order)."""
    check_empty_blocks(r, n_px)
    assert r["n"] == tr["n"] == math.fsum(r["partial_stats"][:, 0])
    s = totals(r["partial_stats"], 5)
    for k in range(5):
        terms = tr["stats_terms"][k]
        exact, bound = math.fsum(terms.ravel()), order_bound(terms)
        got = math.fsum(r["partial_stats"][:, k])
        print(f"stats sum {k}: gpu {s[k]!r} fsum(partials) {got!r} fsum(terms) {exact!r} bound {bound:.3e}")
        if integer:
            assert got == exact == s[k]
        else:
            assert abs(s[k] - exact) <= bound and abs(got - exact) <= bound
    # ecc_stats_finish_kernel on the GPU's own totals: the same float64 operations
    n = s[0]
    im = isd = tm = tsd = 0.0
    if n > 0:
        im, tm = s[1] / n, s[3] / n
        isd, tsd = math.sqrt(max(s[2] / n - im * im, 0.0)), math.sqrt(max(s[4] / n - tm * tm, 0.0))
    assert r["img_mean"] == np.float32(im) == tr["img_mean"] and r["tmp_mean"] == np.float32(tm) == tr["tmp_mean"]
    for got, want, ref in ((r["img_norm"], math.sqrt(n * isd * isd), tr["img_norm"]), (r["tmp_norm"], math.sqrt(n * tsd * tsd), tr["tmp_norm"])):
        assert abs(got - want) <= 1e-15 * abs(want)
        assert abs(got - ref) <= 1e-9 * abs(ref)                         # the oracle's own sums, taken in numpy's order: two roundings of a variance
    return s


def check_accum(r, tr):
    """-> the GPU's own totals of the 13 sums."""
    s = totals(r["partial_accum"], K_SUMS)
    for k in range(K_SUMS):
        terms = tr["terms"][k]
        exact, bound = math.fsum(terms.ravel()), order_bound(terms)
        print(f"accum sum {k}: gpu {s[k]!r} fsum(terms) {exact!r} bound {bound:.3e}")
        assert abs(s[k] - exact) <= bound
    return s


def ulp32_apart(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.maximum(np.abs(a), np.abs(b))).astype(np.float64)


def check_update(r, M, state_in):
    """update_from_sums on the GPU's own reduced totals and the GPU's norms against the GPU's EccState. -> the oracle's new state."""
    from oracle import ecc_ref

    st = dict(M=np.array(M, np.float32), rho=-1.0, last_rho=-EPS, iter=0, max_iters=5000, eps=EPS, status=0, done=0)
    st.update(state_in)
    want = ecc_ref.update_from_sums(totals(r["partial_accum"], K_SUMS) if not st["done"] else np.zeros(K_SUMS), dict(st, img_norm=r["img_norm"], tmp_norm=r["tmp_norm"]))
    print(f"update: gpu iter {r['iter']} status {r['status']} done {r['done']} rho {r['rho']!r} last_rho {r['last_rho']!r} map {r['map'].ravel()}; "
          f"oracle rho {want['rho']!r} det {want['det']!r} map {want['M'].ravel()}")
    assert (r["iter"], r["status"], r["done"]) == (want["iter"], want["status"], want["done"])
    for got, ref in ((r["rho"], want["rho"]), (r["last_rho"], want["last_rho"])):
        assert (math.isnan(got) and math.isnan(ref)) or abs(got - ref) <= 1e-15 * abs(ref)
    assert ulp32_apart(r["map"], want["M"]).max() <= 1.0
    return want


# --------------------------------------------------------------------------- prepare
PREPARE_SIZES = [(8, 8), (9, 11), (8, 128), (9, 127), (10, 130), (8, 126)]   # half images of 4, 5, 63, 64 and 65 columns, 4 and 5 rows: around one 64 x 4 block


@pytest.mark.parametrize("hw", PREPARE_SIZES, ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_prepare_matches_the_oracle_bit_for_bit(gtx_ctx, hw):
    """Random bytes, an all-255 frame (the clamp to 255 and every rounding constant at its limit) and a 0 / 255 checkerboard."""
    from geotrax_amd import ops
    from oracle.ecc_ref import prepare

    H, W = hw
    rng = np.random.default_rng(H * 1000 + W)
    yy, xx = np.mgrid[0:H, 0:W]
    frames = {"random": rng.integers(0, 256, (H, W, 3), dtype=np.uint8), "white": np.full((H, W, 3), 255, np.uint8),
              "checkerboard": np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[..., None], 3, -1)}
    for name, f in frames.items():
        want = prepare(f).astype(np.float32)
        assert want.shape == (H // 2, W // 2)
        if name == "white":
            assert (want == 255).all()
        got = ops.ecc_prepare(f, ctx=gtx_ctx)
        np.testing.assert_array_equal(got, want, err_msg=name)


def test_prepare_drops_the_odd_column_from_the_mean_but_not_from_the_blur(gtx_ctx):
    """Odd H and W, the last row and column 255 on a zero frame: the 2 x 2 mean never reads them, the blur of the row and column
    before them does. Expected: what the oracle gives."""
    from geotrax_amd import ops
    from oracle.ecc_ref import prepare

    f = np.zeros((9, 11, 3), np.uint8)
    f[-1] = 255
    f[:, -1] = 255
    want = prepare(f).astype(np.float32)
    assert want[:-1, :-1].max() == 0 and want[-1, 0] > 0 and want[0, -1] > 0 and want[-1, -1] > want[-1, 0]      # the blur saw them
    np.testing.assert_array_equal(ops.ecc_prepare(f, ctx=gtx_ctx), want)


# --------------------------------------------------------------------------- gradient
@pytest.mark.parametrize("hw", [(4, 4), (3, 65), (5, 63), HW], ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_gradients_match_the_oracle_bit_for_bit(gtx_ctx, hw):
    """Values of both signs across twelve decades, and a ramp: REFLECT_101 makes its border gradients 0 (a clamping border: 0.5 steps)."""
    from geotrax_amd import ops
    from oracle.ecc_ref import gradients

    h, w = hw
    rng = np.random.default_rng(h * 100 + w)
    wild = (rng.standard_normal((h, w)) * 10.0 ** rng.uniform(-6, 6, (h, w))).astype(np.float32)
    yy, xx = np.mgrid[0:h, 0:w]
    ramp = (3 * xx + 7 * yy).astype(np.float32)
    I = np.eye(2, 3, dtype=np.float32)
    for name, img in (("wild", wild), ("ramp", ramp)):
        gx, gy = gradients(img)
        r = ops.ecc_iterate(img, img, I, ctx=gtx_ctx)
        np.testing.assert_array_equal(r["gx"].view(np.uint32), gx.view(np.uint32), err_msg=name)
        np.testing.assert_array_equal(r["gy"].view(np.uint32), gy.view(np.uint32), err_msg=name)
        if name == "ramp":
            assert (gx[:, 0] == 0).all() and (gx[:, -1] == 0).all() and (gx[:, 1:-1] == 3).all()
            assert (gy[0] == 0).all() and (gy[-1] == 0).all() and (gy[1:-1] == 7).all()
        else:
            assert (wild < 0).any() and np.abs(wild).max() > 1e9 * np.abs(wild).min()


# --------------------------------------------------------------------------- stats and accum
@pytest.mark.parametrize("warp", WARPS)
@pytest.mark.parametrize("name", list(MAPS))
def test_stats_and_accum_sums_on_the_hand_chosen_maps(gtx_ctx, name, warp):
    """The mask count exactly; the four other stats sums and the 13 accum sums within the summation-order bound of the oracle's
    terms, equal where the terms are integers; blocks 8..511 own no pixel at 37 x 53 and must hold +0.0."""
    from oracle import ecc_ref

    tr = trace(name, warp)
    want_n = MAPS[name][1]
    if want_n is not None:
        assert tr["n"] == want_n
    lin, _ = ecc_ref.warp_coords(map_of(*MAPS[name][0]), *HW)
    if name == "tie_1_64":
        assert ((lin[2] == 1) | (lin[2] == 0)).all() and (lin[2] == 1).any() and (lin[3] == 0).all()   # 16 + 16 and -16 + 16 of 1024ths: up to 1 / 32, up to 0
    if name in ("tie_1_2", "half_pixel"):
        assert (lin[2] == 16).all() and (lin[3] == 16).all()
    if name in ("rot-0.3", "outside_up_left", "tie_1_2"):
        assert (lin[0] < 0).any() or (lin[1] < 0).any()                  # negative source positions: floor, >> and & on negative values
    r = gpu(gtx_ctx, name, warp)
    check_stats(r, tr, HW[0] * HW[1], integer=name in INTEGER_TRANSLATIONS)
    check_accum(r, tr)


@pytest.mark.parametrize("warp", WARPS)
@pytest.mark.parametrize("name", ROTATIONS)
def test_a_rotated_map_makes_the_sin_terms_of_the_jacobian_count(gtx_ctx, name, warp):
    """First, on the oracle: with the sign of X h1 in hat_x flipped, the first Hessian sum moves by far more (1e6 x) than the bound
    the GPU's sum is held to -- the map discriminates. Then the GPU's sum is inside that bound of the unflipped one."""
    from oracle import ecc_ref

    tr = trace(name, warp)
    t, i = pair(*HW)
    M = map_of(*MAPS[name][0])
    assert abs(M[1, 0]) > 0.29
    gx, gy = ecc_ref.gradients(i)
    if warp == "exact":
        ex = ecc_ref.warp_coords_exact(M, *HW)
        gxw, gyw = ecc_ref.warp_linear_exact(gx, ex), ecc_ref.warp_linear_exact(gy, ex)
    else:
        lin, _ = ecc_ref.warp_coords(M, *HW)
        gxw, gyw = ecc_ref.warp_linear(gx, lin), ecc_ref.warp_linear(gy, lin)
    X = np.broadcast_to(np.arange(HW[1], dtype=np.float32)[None, :], HW)
    Y = np.broadcast_to(np.arange(HW[0], dtype=np.float32)[:, None], HW)
    h0, h1 = M[0, 0], M[1, 0]
    hat_y = (X * h0) - (Y * h1)
    s0 = {}
    for sign in (-1, 1):
        hat_x = (-(X * h1) if sign < 0 else (X * h1)) - (Y * h0)
        j0 = ((gxw * hat_x) + (gyw * hat_y)).astype(np.float64)
        s0[sign] = math.fsum((j0 * j0).ravel())
    bound = order_bound(tr["terms"][0])
    assert s0[-1] == math.fsum(tr["terms"][0].ravel())                    # the unflipped restatement is the oracle's
    print(f"s[0] {s0[-1]!r}, with X h1 flipped {s0[1]!r}, bound {bound:.3e}")
    assert abs(s0[1] - s0[-1]) > 1e6 * bound
    s = totals(gpu(gtx_ctx, name, warp)["partial_accum"], K_SUMS)
    assert abs(s[0] - s0[-1]) <= bound


@pytest.mark.parametrize("warp", WARPS)
@pytest.mark.parametrize("hw,motion", [((300, 450), (0.02, 3.3, -2.7)), ((4, 4), (0.0, 0.5, -0.5)), ((4, 4), (0.0, 0.0, 0.0))],
                         ids=["300x450", "4x4_half_pixel", "4x4_identity"])
def test_two_pixels_per_thread_and_one_block_for_all(gtx_ctx, hw, motion, warp):
    """300 x 450 = 135000 pixels: more than the grid's 131072 threads, the first 3928 take a second pixel and every block owns some.
    4 x 4: block 0 owns everything, the 511 others must write +0.0."""
    n_px = hw[0] * hw[1]
    own = owning_blocks(n_px)
    assert (len(own) == K_BLOCKS and n_px > K_BLOCKS * K_THREADS) if n_px > 16 else list(own) == [0]
    tr, r = trace(motion, warp, hw), gpu(gtx_ctx, motion, warp, hw)
    assert 0 < tr["n"] <= n_px
    check_stats(r, tr, n_px, integer=motion == (0.0, 0.0, 0.0))
    check_accum(r, tr)
    check_update(r, map_of(*motion), {})


# --------------------------------------------------------------------------- update
@pytest.mark.parametrize("warp", WARPS)
@pytest.mark.parametrize("name", STEP_MAPS)
def test_update_takes_the_oracles_step(gtx_ctx, name, warp):
    M = map_of(*MAPS[name][0])
    want = check_update(gpu(gtx_ctx, name, warp), M, {})
    assert want["status"] == 0 and want["done"] == 0 and want["iter"] == 1 and want["det"] != 0.0 and want["dp"] is not None
    assert ulp32_apart(want["M"], M).max() > 100                         # a step was taken


@pytest.mark.parametrize("warp", WARPS)
def test_a_singular_hessian_gives_no_step_and_the_second_round_ends(gtx_ctx, warp):
    """Stripes along y against the textured template: gy == 0, the float32 Hessian has a zero row, d == 0 -> the inverse is zero, no
    step, and rho repeats: the second round ends the fit at the identity with status 0."""
    from geotrax_amd import ops
    from oracle import ecc_ref

    I = np.eye(2, 3, dtype=np.float32)
    t, s = pair(*HW)[0], stripes(*HW)
    assert (ecc_ref.gradients(s)[1] == 0).all()
    r1 = gpu(gtx_ctx, "identity", warp, HW, "stripes")
    check_accum(r1, trace("identity", warp, HW, "stripes"))
    w1 = check_update(r1, I, {})
    assert w1["det"] == 0.0 and w1["status"] == 0 and w1["done"] == 0 and w1["rho"] > 0
    np.testing.assert_array_equal(r1["map"], I)
    r2 = ops.ecc_iterate(t, s, r1["map"], exact=warp == "exact", rho=r1["rho"], last_rho=r1["last_rho"], eps=EPS, iter_in=r1["iter"], ctx=gtx_ctx)
    w2 = check_update(r2, I, dict(rho=r1["rho"], last_rho=r1["last_rho"], iter=1))
    assert (r2["iter"], r2["status"], r2["done"]) == (2, 0, 1) and r2["rho"] == r2["last_rho"] == r1["rho"] and w2["det"] == 0.0
    np.testing.assert_array_equal(r2["map"], I)
    H = np.eye(2, 3, dtype=np.float32)
    assert ecc_ref.find_transform_ecc(t.astype(np.uint8), s.astype(np.uint8), H, warp=warp)[1:] == (2, 0) and (H == I).all()


@pytest.mark.parametrize("warp", WARPS)
@pytest.mark.parametrize("name", ["one_column", "quarter_turn"])
def test_a_correlation_about_to_be_minimised_ends_with_status_2(gtx_ctx, name, warp):
    M = map_of(*MAPS[name][0])
    r = gpu(gtx_ctx, name, warp)
    want = check_update(r, M, {})
    assert want["status"] == 2
    assert (r["iter"], r["status"], r["done"]) == (1, 2, 1) and r["rho"] == -1.0 and r["last_rho"] == -1.0
    np.testing.assert_array_equal(r["map"], M)


@pytest.mark.parametrize("warp", WARPS)
@pytest.mark.parametrize("name", ["outside_right", "outside_up_left", "flat"])
def test_no_pixel_under_the_mask_or_no_variance_ends_with_status_1(gtx_ctx, name, warp):
    key, kind = ("identity", "flat") if name == "flat" else (name, "pair")
    M = map_of(*MAPS[key][0])
    tr, r = trace(key, warp, HW, kind), gpu(gtx_ctx, key, warp, HW, kind)
    assert tr["n"] == (1961 if name == "flat" else 0) and tr["img_norm"] * tr["tmp_norm"] == 0
    check_stats(r, tr, HW[0] * HW[1], integer=True)
    want = check_update(r, M, {})
    assert want["status"] == 1
    assert (r["iter"], r["status"], r["done"]) == (1, 1, 1) and math.isnan(r["rho"]) and r["last_rho"] == -1.0
    np.testing.assert_array_equal(r["map"], M)


@pytest.mark.parametrize("warp", WARPS)
def test_the_cap_the_criterion_and_a_finished_state(gtx_ctx, warp):
    from geotrax_amd import ops

    t, i = pair(*HW)
    M = map_of(*MAPS["rot-0.3"][0])
    first = gpu(gtx_ctx, "rot-0.3", warp)
    assert first["done"] == 0 and abs(first["rho"] - first["last_rho"]) > 1000 * EPS
    kw = dict(exact=warp == "exact", eps=EPS, ctx=gtx_ctx)
    # the last iteration the cap allows: done, although rho moved
    r = ops.ecc_iterate(t, i, M, iter_in=6, max_iters=7, **kw)
    check_update(r, M, dict(iter=6, max_iters=7))
    assert (r["iter"], r["status"], r["done"]) == (7, 0, 1) and r["rho"] == first["rho"]
    np.testing.assert_array_equal(r["map"], first["map"])
    r = ops.ecc_iterate(t, i, M, iter_in=5, max_iters=7, **kw)
    assert (r["iter"], r["status"], r["done"]) == (6, 0, 0)
    # rho repeats to within eps: done, with the step taken
    for rho_in, done in ((first["rho"] + 0.5 * EPS, 1), (first["rho"] - 2 * EPS, 0)):
        r = ops.ecc_iterate(t, i, M, rho=rho_in, last_rho=0.1, iter_in=3, **kw)
        check_update(r, M, dict(rho=rho_in, last_rho=0.1, iter=3))
        assert (r["iter"], r["status"], r["done"]) == (4, 0, done) and r["last_rho"] == rho_in and r["rho"] == first["rho"]
        np.testing.assert_array_equal(r["map"], first["map"])
    # a finished state: every kernel of the round returns at once
    for status in (0, 2):
        r = ops.ecc_iterate(t, i, M, rho=0.25, last_rho=0.125, iter_in=3, status_in=status, done_in=1, **kw)
        check_empty_blocks(r, HW[0] * HW[1], done=True)
        assert (r["iter"], r["status"], r["done"], r["rho"], r["last_rho"]) == (3, status, 1, 0.25, 0.125)
        assert (r["n"], r["img_norm"], r["tmp_norm"], r["img_mean"], r["tmp_mean"]) == (0, 0, 0, 0, 0)   # as the hook's fresh state had them
        np.testing.assert_array_equal(r["map"], M)
        np.testing.assert_array_equal(r["gx"], first["gx"])              # the gradient kernel does not look at the state
        check_update(r, M, dict(rho=0.25, last_rho=0.125, iter=3, status=status, done=1))


# --------------------------------------------------------------------------- through the product object
def frame_pair():
    """75 x 107 BGR frames (equal channels): a smooth texture and the same texture shifted by (2, 4) full-resolution pixels."""
    big = smooth(75 + 8, 107 + 8, OBJECT_SEED)
    cut = lambda y, x: np.ascontiguousarray(np.repeat(big[y:y + 75, x:x + 107, None], 3, -1))
    return cut(4, 4), cut(2, 0)


@functools.lru_cache(maxsize=None)
def object_reference(warp, cap):
    from oracle.ecc_ref import EccRef

    f0, f1 = frame_pair()
    o = EccRef(max_iters=cap, warp=warp)
    o.apply(f0)
    return o.apply(f1), dict(o.last)


@pytest.mark.parametrize("warp", WARPS)
def test_the_object_at_caps_on_and_off_a_batch_boundary(gtx_ctx, warp):
    """collect() launches iterations in batches of six and looks at `done` between batches: caps of 5, 6, 7 and 12 fall inside the
    first batch, on its end, one past it and on the end of the second; launches after `done` must change nothing."""
    from geotrax_amd.gmc import EccGMC

    f0, f1 = frame_pair()
    A60, last60 = object_reference(warp, 60)
    assert last60["status"] == 0 and last60["rho"] > 0.9 and 7 < last60["iters"] < 12   # cap 7 bites inside the second batch; cap 12 leaves launches after `done`
    print(f"{warp}: cap 60 -> {last60}")
    for cap in (60, 5, 6, 7, 12):
        Ao, lo = object_reference(warp, cap)
        assert lo["status"] == 0 and lo["iters"] == min(cap, last60["iters"])
        g = EccGMC((75, 107), ctx=gtx_ctx, max_iters=cap, warp=warp)
        g.apply(f0)
        A = g.apply(f1)
        print(f"{warp}: cap {cap} -> gpu {g.last}, oracle {lo}")
        assert g.valid and g.last["status"] == 0 and g.last["iters"] == lo["iters"]
        assert abs(g.last["rho"] - lo["rho"]) < 1e-9
        np.testing.assert_allclose(A, Ao, rtol=0, atol=2e-6)
        g.close()


@pytest.mark.parametrize("warp", WARPS)
def test_the_object_on_stripes_ends_after_two_iterations_at_the_identity(gtx_ctx, warp):
    from geotrax_amd.gmc import EccGMC
    from oracle.ecc_ref import EccRef, gradients, prepare

    f0, _ = frame_pair()
    f1 = np.ascontiguousarray(np.broadcast_to(f0[37][None], f0.shape))
    assert (gradients(prepare(f1).astype(np.float32))[1] == 0).all()
    o = EccRef(max_iters=60, warp=warp)
    o.apply(f0)
    Ao = o.apply(f1)
    assert (o.last["iters"], o.last["status"]) == (2, 0) and (Ao == np.eye(2, 3)).all()
    g = EccGMC((75, 107), ctx=gtx_ctx, max_iters=60, warp=warp)
    g.apply(f0)
    A = g.apply(f1)
    assert g.valid and (g.last["iters"], g.last["status"]) == (2, 0) and abs(g.last["rho"] - o.last["rho"]) < 1e-9
    np.testing.assert_array_equal(A, np.eye(2, 3))
    g.close()
