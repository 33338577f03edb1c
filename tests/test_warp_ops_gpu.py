"""The frame warp kernel (csrc/warp.hip, behind gtx_warp_frame / gtx_warp_frame_dev) on small frames over every class of
homography: each case first shows, from a restatement of the kernel's per-tile plan (tests/warp_cases.py) or from the oracle's
own coordinates, that it is the edge it claims to be -- which tiles stage their footprint in LDS, which gather directly, where
W <= 0, where the box is clamped, where coordinates tie or saturate -- and then holds the kernel's frame against
oracle/warp_ref.py byte for byte. The oracle is given the library's own inverse (gtx_op_invert3x3, checked on the CPU in
tests/test_geometry.py), so no comparison here has a tolerance. Frames are uint8 noise: any mis-addressed tap changes the byte."""
from types import SimpleNamespace

import numpy as np
import pytest
import warp_cases as wc

pytestmark = pytest.mark.gpu
CAP = wc.LDS_CAP


def _case(f, H):
    from oracle.warp_ref import warp_perspective as ref

    h, w = f.shape[:2]
    Minv = wc.hook_inverse(H)
    return SimpleNamespace(f=f, H=np.asarray(H, np.float64), h=h, w=w, Minv=Minv, p=wc.plan(h, w, Minv), c=wc.coords(h, w, Minv),
                           want=ref(f, H, M_inv=Minv))


def _equal(ctx, case, label):
    from geotrax_amd.warp import warp_perspective

    assert case.h * case.w * 3 <= 384 * 1024
    print(f"{label} {case.h}x{case.w}: {wc.counts(case.p)}")
    np.testing.assert_array_equal(warp_perspective(case.f, case.H, ctx=ctx), case.want, err_msg=label)


@pytest.mark.parametrize("hw", [(21, 261), (16, 256)])
def test_ties_round_half_to_even(gtx_ctx, hw):
    """M = translation (1/64, 3/64): every coordinate is k + 1/2 in 1/32-pixel units before rounding. k is even in x (the tie goes
    down) and odd in y (it goes up), so both directions of round-half-to-even are taken; floor(v + 1/2) would move every x."""
    h, w = hw
    assert (261 * 3) % 4 != 0 and (256 * 3) % 16 == 0
    for name, f in (("noise", wc.noise(1, h, w)), ("ramp", wc.ramp(h, w))):
        k = _case(f, wc.TIES)
        c = k.c
        kx, ky = np.floor(c.fX), np.floor(c.fY)
        assert np.all(c.fX - kx == 0.5) and np.all(c.fY - ky == 0.5)
        assert np.all(kx.astype(np.int64) & 1 == 0) and np.all(ky.astype(np.int64) & 1 == 1)
        assert np.all(c.X == kx) and np.all(c.Y == ky + 1) and np.all(c.X & 1 == 0) and np.all(c.Y & 1 == 0)
        assert k.p.staged.all()
        _equal(gtx_ctx, k, f"ties/{name}")


def test_footprints_at_and_just_over_the_lds_cap(gtx_ctx):
    """A seeded scan (warp_cases.cap_scan) for an anisotropic zoom-out whose image holds a staged tile within 512 bytes under the cap
    and a tile with W > 0 that is not staged for being within 512 bytes over it; the scan prefers a tile of exactly the cap."""
    H, exact = wc.cap_scan()
    k = _case(wc.noise(2, *wc.CAP_HW), H)
    p = k.p
    under = p.staged & (p.nbytes > CAP - 512) & (p.nbytes <= CAP)
    over = p.pos & ~p.staged & (p.nbytes > CAP) & (p.nbytes <= CAP + 512)
    assert under.any() and over.any()
    assert exact == bool((p.staged & (p.nbytes == CAP)).any())
    print(f"near-cap: staged footprints {sorted(set(p.nbytes[under]))} B, unstaged {sorted(set(p.nbytes[over]))} B, cap {CAP} B, exact-cap tile: {exact}")
    _equal(gtx_ctx, k, "near-cap")


def test_mixed_staged_and_direct_tiles(gtx_ctx):
    """M = 2.25 I + (0.3, 0.7): interior tiles overflow the cap, the tiles clipped by the source's edge fit; part of the output reads
    outside the source."""
    k = _case(wc.noise(3, 48, 640), wc.MIXED)
    assert k.p.n_staged > 0 and (k.p.pos & ~k.p.staged).any()
    assert ((k.c.x0 >= k.w) | (k.c.y0 >= k.h)).any() and not k.want[-1, -1].any()
    _equal(gtx_ctx, k, "mixed")


def test_rot90_tall_footprints(gtx_ctx):
    k = _case(wc.noise(4, 200, 200), wc.rot90(200))
    p = k.p
    assert p.staged.all() and np.all((p.by1 - p.by0) > (p.bx1 - p.bx0))
    np.testing.assert_array_equal(k.want, np.rot90(k.f, -1))       # the oracle alone: an exact quarter turn
    _equal(gtx_ctx, k, "rot90")


@pytest.mark.parametrize("name", ["rot180", "flip-x", "flip-y"])
def test_mirrored_footprints(gtx_ctx, name):
    h, w = 21, 261
    H, flip = wc.flips(h, w)[name]
    k = _case(wc.noise(5, h, w), H)
    p = k.p
    multi_x, multi_y = p.X[:, 1] != p.X[:, 0], p.Y[1] != p.Y[0]     # (a last tile one pixel wide has its two corners in one place)
    if name != "flip-y":
        assert np.all(p.X[:, 1] <= p.X[:, 0]) and multi_x.any() and np.all(p.X[:, 1][multi_x] < p.X[:, 0][multi_x])
    if name != "flip-x":
        assert np.all(p.Y[1] <= p.Y[0]) and multi_y.any() and np.all(p.Y[1][multi_y] < p.Y[0][multi_y])
    assert p.staged.all()
    np.testing.assert_array_equal(k.want, flip(k.f))
    _equal(gtx_ctx, k, name)


def test_zoom_in_shares_source_texels(gtx_ctx):
    k = _case(wc.noise(6, 21, 261), wc.ZOOM_IN)
    assert k.p.staged.all() and k.p.nbytes.max() <= CAP // 16
    shared = np.unique(k.c.x0[0], return_counts=True)[1]
    assert len(shared) <= k.w // 4 + 2 and shared.max() == 4
    _equal(gtx_ctx, k, "zoom-in x4")


@pytest.mark.parametrize("side", ["left", "right", "top", "bottom"])
def test_footprint_clipped_on_each_side(gtx_ctx, side):
    h, w = 21, 261
    k = _case(wc.noise(7, h, w), wc.clipped(h, w)[side])
    p, c = k.p, k.c
    clamped, tap = {"left": (p.staged & (p.lo_x - 1 < 0) & (p.bx0 == 0) & (p.bx1 > 0), (c.x0 == -1) & (c.ax > 0)),
                    "right": (p.staged & (p.hi_x + 3 > w) & (p.bx1 == w) & (p.bx0 < w), (c.x0 + 1 == w) & (c.ax > 0)),
                    "top": (p.staged & (p.lo_y - 1 < 0) & (p.by0 == 0) & (p.by1 > 0), (c.y0 == -1) & (c.ay > 0)),
                    "bottom": (p.staged & (p.hi_y + 3 > h) & (p.by1 == h) & (p.by0 < h), (c.y0 + 1 == h) & (c.ay > 0))}[side]
    assert clamped.any() and tap.any()
    assert k.want[tap].any()                                       # the half-inside taps do contribute
    _equal(gtx_ctx, k, f"clipped/{side}")


@pytest.mark.parametrize("axis", ["x", "y"])
@pytest.mark.parametrize("t", wc.OUTSIDE)
def test_wholly_outside_and_saturating(gtx_ctx, t, axis):
    """Translations far off the frame: 1e7 px stays inside the int range (-3.2e8 units), +-3e9 px saturates every coordinate at
    -2^31 / 2^31 - 1. The output is all zero and no tile stages anything."""
    h, w = 21, 261
    k = _case(wc.noise(8, h, w), wc.translation(t, 0.0) if axis == "x" else wc.translation(0.0, t))
    v = k.c.X if axis == "x" else k.c.Y
    if abs(t) > 2.0**31 / 32:
        assert np.all(v == (wc.INT_MIN if t > 0 else wc.INT_MAX))
    else:
        assert np.all(v < -32 * 1e6) and np.all(v > wc.INT_MIN)
    assert not k.want.any() and k.p.n_staged == 0 and np.all(k.p.row_bytes * (k.p.by1 - k.p.by0) == 0)
    _equal(gtx_ctx, k, f"outside/{axis}{t:g}")


@pytest.mark.parametrize("which", ["x=64", "general"])
def test_horizon_inside_the_image(gtx_ctx, which):
    """W changes sign inside the frame. M = [[1,0,0],[0,1,0],[-1/64,0,1]] puts W == 0 exactly on column 64, where the coordinate is
    defined as 0 and the oracle reads source (0, 0); the general matrix (M6, M7 != 0) has whole tiles before the horizon, across it and
    behind it. Tiles with a corner at W <= 0 must take the direct path."""
    h, w = 24, 400
    k = _case(wc.noise(9, h, w), wc.HORIZON if which == "x=64" else wc.HORIZON_GENERAL)
    p, c = k.p, k.c
    before, behind = (p.Wc > 0).all((0, 1)), (p.Wc < 0).all((0, 1))
    across = ~before & ~behind
    assert (c.W > 0).any() and (c.W < 0).any()
    assert across.any() and behind.any() and not p.staged[across | behind].any() and not p.pos[across | behind].any()
    if which == "x=64":
        assert np.all(c.W[:, 64] == 0.0) and np.all(c.X[:, 64] == 0) and np.all(c.Y[:, 64] == 0)
        assert np.all(k.want[:, 64] == k.f[0, 0]) and np.count_nonzero(c.W == 0.0) == h
    else:
        assert k.Minv[2, 0] != 0 and k.Minv[2, 1] != 0
        assert before.any() and p.pos[before].all() and p.staged[before].any()
    print(f"horizon/{which}: {int(before.sum())} tiles before the horizon, {int(across.sum())} across, {int(behind.sum())} behind")
    _equal(gtx_ctx, k, f"horizon/{which}")


def test_strong_perspective_with_w_positive(gtx_ctx):
    """h31, h32 ~ 1e-3 on 150 x 300: W > 0 everywhere, and staged tiles whose footprint is no parallelogram (the corner sums
    X00 + X11 and X01 + X10 differ by more than a pixel)."""
    k = _case(wc.noise(10, 150, 300), wc.PERSPECTIVE)
    p = k.p
    skew = np.maximum(np.abs(p.X[0, 0] + p.X[1, 1] - p.X[0, 1] - p.X[1, 0]), np.abs(p.Y[0, 0] + p.Y[1, 1] - p.Y[0, 1] - p.Y[1, 0]))
    assert np.all(k.c.W > 0) and p.pos.all() and (p.staged & (skew > 32)).any()
    _equal(gtx_ctx, k, "strong perspective")


def test_rot34_both_paths(gtx_ctx):
    k = _case(wc.noise(11, 150, 300), wc.ROT34)
    assert k.p.n_staged > 0 and (k.p.pos & ~k.p.staged).any()
    _equal(gtx_ctx, k, "rot34")


@pytest.mark.parametrize("hw,partial_x,partial_y,store_tail", [((1, 1), True, True, True), ((1, 5), True, True, True), ((9, 5), True, True, True),
                                                               ((8, 128), False, False, False), ((9, 129), True, True, True),
                                                               ((3, 131), True, True, True)])
def test_degenerate_sizes(gtx_ctx, hw, partial_x, partial_y, store_tail):
    """Partial last tiles in x and in y and a last group of fewer than four pixels (the `xq + 4 > w` byte stores); 8 x 128 is exactly
    one full tile."""
    h, w = hw
    assert (w % wc.TW != 0) == partial_x and (h % wc.TH != 0) == partial_y and (w % 4 != 0) == store_tail
    f = wc.noise(12 + h + w, h, w)
    for name, H in (("identity", np.eye(3)), ("ties", wc.TIES), ("camera", wc.camera(h + w, 0.3))):
        k = _case(f, H)
        assert k.p.staged.size == -(-w // wc.TW) * -(-h // wc.TH)
        if name == "identity":
            np.testing.assert_array_equal(k.want, f)
        _equal(gtx_ctx, k, f"degenerate/{name}")


@pytest.mark.parametrize("hw", [(21, 261), (16, 256)])
def test_unaligned_device_pointers(gtx_ctx, hw):
    """gtx_warp_frame_dev on frames that start 0 / 1 / 4 / 8 bytes (source) and 0 / 1 / 2 bytes (destination) into their allocations, as
    the frames of a ring of h*w*3-byte slots do: the staging loop gathers bytes where the source or its rows are not 16-byte aligned,
    the stores go byte-wise where the destination is not 4-byte aligned, and nothing is written outside the frame.
    (Rows of a multiple of 16 bytes from an aligned base -- 16 x 256 at offset 0 -- take the 16-byte loads throughout: with such rows
    every chunk ends inside the image, so the image-tail branch can only be reached with ragged rows; it is, on 21 x 261.)"""
    from geotrax_amd.warp import FrameWarper

    h, w = hw
    k = _case(wc.noise(13, h, w), wc.MIXED)
    assert k.p.n_staged > 0 and k.p.n_unstaged > 0
    s0 = wc.staging(k.p, 0)
    if hw == (16, 256):
        assert s0.aligned and s0.tail_chunks == 0 and not wc.staging(k.p, 4).aligned
    else:
        assert not s0.aligned and s0.tail_chunks >= 1
    print(f"unaligned {h}x{w}: {wc.counts(k.p)}; at offset 0 aligned = {s0.aligned}, {s0.tail_chunks} of {s0.chunks} chunks on the image tail")
    n = h * w * 3
    wp = FrameWarper(hw, ctx=gtx_ctx)
    src, dst = gtx_ctx.dev_alloc(n + 32), gtx_ctx.dev_alloc(n + 32)
    try:
        assert src % 16 == 0 and dst % 16 == 0
        sentinel = np.full(n + 32, 0xA5, np.uint8)
        for so in (0, 1, 4, 8):
            gtx_ctx.dev_upload(src, sentinel)
            gtx_ctx.dev_upload(src + so, k.f)
            for do in (0, 1, 2):
                gtx_ctx.dev_upload(dst, sentinel)
                wp.warp_dev(src + so, k.H, dst + do)
                out = np.empty(n + 32, np.uint8)
                gtx_ctx.dev_download(out, dst)
                np.testing.assert_array_equal(out[do:do + n].reshape(h, w, 3), k.want, err_msg=f"src + {so}, dst + {do}")
                assert np.all(out[:do] == 0xA5) and np.all(out[do + n:] == 0xA5), (so, do)
    finally:
        gtx_ctx.dev_free(src)
        gtx_ctx.dev_free(dst)
        wp.close()
