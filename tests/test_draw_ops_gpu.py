"""The drawing kernel (csrc/draw.hip, behind gtx_op_draw / gtx_drawer_*) against the numpy twin (geotrax_amd/draw.py) byte for byte
on uint8 noise frames of at most 96 x 200. Both sides are integer arithmetic apart from the SEGMENT distance, whose float64
operations are stated one by one and correctly rounded on both sides: there is no tolerance. Each case first shows from the twin
that it is the edge it claims to be (which tiles a box reaches, how many hits a tile collects, that order matters)."""
import itertools
import re
from pathlib import Path

import numpy as np
import pytest
from test_draw import noise, random_prims, toy_atlas

pytestmark = pytest.mark.gpu

_hpp = (Path(__file__).resolve().parent.parent / "geo-trax_amd" / "csrc" / "draw.hpp").read_text()
CHUNK = int(re.search(r"kDrawChunk\s*=\s*(\d+)", _hpp).group(1))
TW, TH = (int(v) for v in re.search(r"kDrawTileW\s*=\s*(\d+),\s*kDrawTileH\s*=\s*(\d+)", _hpp).groups())
CELLS, ATLAS = toy_atlas()


def tiles_hit(prims, h, w):
    """[n][tiles_y][tiles_x] bool: the kernel's cull, restated from the twin's boxes."""
    from geotrax_amd import draw

    b = draw.bounding_boxes(prims).astype(np.int64)
    tx0 = np.arange(0, w, TW)
    ty0 = np.arange(0, h, TH)
    tx1, ty1 = np.minimum(tx0 + TW, w) - 1, np.minimum(ty0 + TH, h) - 1
    hx = (b[:, 0, None] <= tx1) & (b[:, 2, None] >= tx0)
    hy = (b[:, 1, None] <= ty1) & (b[:, 3, None] >= ty0)
    return hy[:, :, None] & hx[:, None, :]


def equal(ctx, f, prims, label, atlas=ATLAS):
    from geotrax_amd import draw

    assert f.shape[0] <= 96 and f.shape[1] <= 200
    draw.validate(prims, 0 if atlas is None else atlas.size)
    want = draw.rasterize(f, prims, atlas)
    got = draw.draw_dev(ctx, f, prims, atlas)
    np.testing.assert_array_equal(got, want, err_msg=label)
    return want


@pytest.mark.parametrize("hw", [(70, 150), (TH, TW), (1, 1), (TH + 1, TW + 1), (96, 200)])
def test_random_lists_on_ragged_frames(gtx_ctx, hw):
    """70 x 150: neither side a multiple of the tile, 450-byte rows (not a multiple of 4, so rows start at every alignment); exactly
    one tile; one pixel; one pixel over the tile in both directions."""
    h, w = hw
    if hw == (70, 150):
        assert h % TH and w % TW and (w * 3) % 4
    f = noise(h * 1000 + w, h, w)
    prims = random_prims(h + w, 420, h, w, CELLS)
    hit = tiles_hit(prims, h, w)
    assert hit.any(axis=(1, 2)).sum() < len(prims) or hw != (70, 150)       # some primitives reach no tile at all
    want = equal(gtx_ctx, f, prims, f"random {h}x{w}")
    assert (want != f).any()


def test_primitives_across_a_four_tile_corner_off_frame_and_reaching_in(gtx_ctx):
    from geotrax_amd import draw
    from geotrax_amd.draw import FILL, GLYPH, RING, SEGMENT

    h, w = 3 * TH, 2 * TW + 9
    f = noise(7, h, w)
    off, cw, ch = CELLS[1]
    corner = [(FILL, TW - 2, TH - 2, TW + 1, TH + 1, 0, 0, 0x00FF00), (SEGMENT, TW - 5, TH - 3, TW + 4, TH + 2, 3, 0, 0xFF0000),
              (RING, TW, TH, 4, 0, 2, 0, 0x0000FF), (GLYPH, TW - 4, TH - 2, cw, ch, off, cw, 0xFFFFFF)]
    hit = tiles_hit(corner, h, w)
    assert (hit[:, :2, :2].sum(axis=(1, 2)) == 4).all()
    for k, p in enumerate(corner):
        want = equal(gtx_ctx, f, [p], f"corner {k}")
        changed = (want != f).any(axis=2)
        assert changed[:TH, :TW].any() and changed[:TH, TW:].any() and changed[TH:, :TW].any() and changed[TH:, TW:].any(), k
    equal(gtx_ctx, f, corner, "corner, all")
    gone = [(FILL, w + 5, 2, w + 30, 9, 0, 0, 0xFFFFFF), (SEGMENT, -40, -9, -7, -30, 4, 0, 0xFFFFFF), (RING, 10, h + 20, 6, 0, 3, 0, 0xFFFFFF),
            (GLYPH, -cw, 3, cw, ch, off, cw, 0xFFFFFF), (SEGMENT, -32768, -32768, -32768, 32767, 1, 0, 0xFFFFFF), (RING, 32767, 32767, 32767, 0, 5, 0, 0xFFFFFF)]
    assert not tiles_hit(gone[:5], h, w).any()
    assert np.array_equal(equal(gtx_ctx, f, gone, "off-frame"), f)
    reach = [(SEGMENT, -20, -11, 30, 17, 4, 0, 0x10F0A0), (FILL, -9, -9, 3, 2, 0, 0, 0x112233), (RING, -3, h // 2, 9, 0, 2, 0, 0x445566),
             (GLYPH, w - 4, -2, cw, ch, off, cw, 0x778899), (SEGMENT, -32768, -32768, 32767, 32767, 2, 0, 0xABCDEF)]
    want = equal(gtx_ctx, f, reach, "reaching in")
    for p in reach:
        assert (draw.rasterize(f, [p], ATLAS) != f).any(), p


@pytest.mark.parametrize("n", [CHUNK + 1, 3 * CHUNK])
def test_more_hits_on_one_tile_than_a_chunk_holds(gtx_ctx, n):
    """n overlapping primitives that all reach tile (0, 0) -- one more than a chunk, and three chunks' worth -- with a few that miss
    it spread between them: the tile's hits pass chunk boundaries, and painter's order must hold across them (the reversed list
    gives another picture)."""
    from geotrax_amd import draw
    from geotrax_amd.draw import FILL, RING, SEGMENT

    h, w = 2 * TH + 3, 2 * TW + 5
    rng = np.random.default_rng(n)
    prims = []
    for i in range(n):
        bgr = int(rng.integers(0, 1 << 24))
        x, y = int(rng.integers(0, TW)), int(rng.integers(0, TH))
        kind = i % 3
        if i % 37 == 36:
            prims.append((FILL, TW + 20, TH + 8, TW + 30, TH + 12, 0, 0, bgr ^ 0xFFFFFF))   # misses tile (0, 0)
        if kind == 0:
            prims.append((FILL, x, y, x + int(rng.integers(0, 30)), y + int(rng.integers(0, 9)), 0, 0, bgr))
        elif kind == 1:
            prims.append((SEGMENT, x, y, int(rng.integers(-5, w)), int(rng.integers(-5, h)), int(rng.integers(1, 5)), 0, bgr))
        else:
            prims.append((RING, x, y, int(rng.integers(0, 9)), 0, int(rng.integers(1, 4)), 0, bgr))
    hits = tiles_hit(prims, h, w)[:, 0, 0]
    per_chunk = [int(hits[c:c + CHUNK].sum()) for c in range(0, len(prims), CHUNK)]
    print(f"{len(prims)} primitives, {int(hits.sum())} reach tile (0, 0); per chunk {per_chunk}")
    assert hits.sum() == n > CHUNK and len(prims) > n and not hits.all() and all(per_chunk)
    assert len(per_chunk) == (2 if n == CHUNK + 1 else 4) and all(0 < c < CHUNK for c in per_chunk)     # every chunk's list is compacted
    f = noise(n, h, w)
    want = equal(gtx_ctx, f, prims, f"{n} on one tile", atlas=None)
    assert not np.array_equal(want[:TH, :TW], draw.rasterize(f, prims[::-1])[:TH, :TW])
    # the last primitive of the first chunk and the first of the second overlap: swapping the two changes the twin's picture
    a, b = CHUNK - 1, CHUNK
    pair = list(prims)
    pair[a] = (FILL, 3, 3, 12, 9, 0, 0, 0x0000FF)
    pair[b] = (FILL, 8, 5, 20, 12, 0, 0, 0x00FF00)
    swapped = list(pair)
    swapped[a], swapped[b] = pair[b], pair[a]
    if n == CHUNK + 1:                                               # nothing after the pair: the overlap shows the later one's colour
        assert tuple(draw.rasterize(f, pair)[6, 10]) == (0, 255, 0) and tuple(draw.rasterize(f, swapped)[6, 10]) == (255, 0, 0)
    equal(gtx_ctx, f, pair, "chunk boundary pair", atlas=None)
    equal(gtx_ctx, f, swapped, "chunk boundary pair, swapped", atlas=None)


def test_all_four_kinds_on_one_pixel_in_every_order(gtx_ctx):
    from geotrax_amd import draw
    from geotrax_amd.draw import FILL, GLYPH, RING, SEGMENT

    off, cw, ch = CELLS[0]
    f = noise(4, 12, 14)
    four = [(FILL, 4, 4, 8, 8, 0, 0, 0x2040F0), (SEGMENT, 0, 5, 13, 7, 2, 0, 0xF02040), (RING, 6, 6, 1, 0, 3, 0, 0x40F020), (GLYPH, 4, 3, cw, ch, off, cw, 0xFFFFFF)]
    x, y = 6, 6
    cov = [int(draw.coverage(p, [x], [y], ATLAS)[0, 0]) for p in four]
    assert all(c > 0 for c in cov), cov
    seen = set()
    for order in itertools.permutations(range(4)):
        want = equal(gtx_ctx, f, [four[k] for k in order], f"order {order}")
        seen.add(tuple(want[y, x]))
    assert len(seen) > 1


def test_single_primitive_edges(gtx_ctx):
    """A glyph clipped at the right and at the bottom edge, a ring with 2r < t (a disc), a zero-length segment, corners in any order,
    a segment as thick as the frame."""
    from geotrax_amd import draw
    from geotrax_amd.draw import FILL, GLYPH, RING, SEGMENT

    h, w = 23, 75
    f = noise(9, h, w)
    off, cw, ch = CELLS[2]
    for p, label in (((GLYPH, w - 1, 5, cw, ch, off, cw, 0xFFFFFF), "glyph right"), ((GLYPH, 30, h - 4, cw, ch, off, cw, 0x33CC66), "glyph bottom"),
                     ((GLYPH, w - 2, h - 5, cw, ch, off, cw, 0x3366CC), "glyph right and bottom")):
        want = equal(gtx_ctx, f, [p], label)
        bx0, by0, bx1, by1 = draw.bounding_boxes([p])[0]
        assert bx1 >= w or by1 >= h
        assert (want != f).any()
    disc = (RING, 40, 11, 1, 0, 5, 0, 0x0000FF)
    assert 2 * disc[3] < disc[5]
    want = equal(gtx_ctx, f, [disc], "disc")
    assert tuple(want[11, 40]) == (255, 0, 0) and tuple(want[11, 43]) == (255, 0, 0)
    dot = (SEGMENT, 64, 16, 64, 16, 3, 0, 0x00FF00)
    want = equal(gtx_ctx, f, [dot], "zero-length segment")
    assert tuple(want[16, 64]) == (0, 255, 0) and np.array_equal(want[16, 61], f[16, 61])
    equal(gtx_ctx, f, [(FILL, 70, 20, 60, 3, 0, 0, 0x123456)], "corners in any order")
    equal(gtx_ctx, f, [(SEGMENT, 3, 3, 70, 19, 60, 0, 0x654321)], "thick segment")
    equal(gtx_ctx, f, [(RING, 10, 10, 0, 0, 2**31 - 1, 0, 0x010203), (SEGMENT, 1, 1, 2, 2, 2**31 - 1, 0, 0x030201)], "largest thickness")


def test_a_label_from_the_glyph_atlas(gtx_ctx):
    """A box, its label fill and the label's glyph cells from the Pillow atlas, as a vehicle's annotation is made of them; the label
    starts left of the frame and ends right of it."""
    from geotrax_amd import draw
    from geotrax_amd.draw import FILL, SEGMENT

    at = draw.GlyphAtlas(line_width=2)
    h, w = 60, 150
    f = noise(17, h, w)
    label = "id:12 car 47 km/h L2"
    tw, th = at.text_size(label)
    assert tw > w
    prims = [(SEGMENT, 5, 30, 90, 30, 2, 0, 0xB4771F), (FILL, -8, 30, -8 + tw, 30 - th - 3, 0, 0, 0xB4771F)] + at.layout(label, -8, 28, (255, 255, 255))
    assert len(prims) == 2 + len(label.replace(" ", ""))
    want = equal(gtx_ctx, f, prims, "label", atlas=at.data)
    assert (want[10:28] == 255).all(axis=2).any() and (want[:8] == f[:8]).all()


def test_drawer_object_empty_lists_capacity_and_staging_ring(gtx_ctx):
    """n = 0 launches nothing (the frame is unchanged and the timer reads 0); n = max_prims is accepted and max_prims + 1 is refused
    with nothing drawn; nine draws in a row without a wait in between (more than the staging ring holds) each paint their own list."""
    from geotrax_amd import _lib, draw

    h, w = 40, 100
    cap = 64
    f = noise(13, h, w)
    dr = draw.Drawer(gtx_ctx, (h, w), cap, ATLAS)
    bufs = [gtx_ctx.dev_alloc(f.nbytes) for _ in range(9)]
    try:
        gtx_ctx.dev_upload(bufs[0], f)
        dr.draw(bufs[0], [])
        assert dr.last_ms() == 0.0
        got = np.empty_like(f)
        gtx_ctx.dev_download(got, bufs[0])
        assert np.array_equal(got, f)
        full = random_prims(3, cap, h, w, CELLS)
        dr.draw(bufs[0], full)
        assert 0.0 < dr.last_ms() < 1000.0
        gtx_ctx.dev_download(got, bufs[0])
        np.testing.assert_array_equal(got, draw.rasterize(f, full, ATLAS))
        with pytest.raises(_lib.GtxError, match=f"holds {cap}"):
            dr.draw(bufs[0], full + full[:1])
        with pytest.raises(_lib.GtxError, match="primitive 5:"):
            dr.draw(bufs[0], full[:5] + [(9, 0, 0, 0, 0, 0, 0, 0)])
        assert dr.last_ms() == 0.0
        gtx_ctx.dev_download(got, bufs[0])
        np.testing.assert_array_equal(got, draw.rasterize(f, full, ATLAS))      # the refused lists drew nothing
        # the ring: distinct lists back to back
        lists = [random_prims(100 + k, 10 + 6 * k, h, w, CELLS) for k in range(9)]
        for b in bufs:
            gtx_ctx.dev_upload(b, f)
        for b, lst in zip(bufs, lists):
            dr.draw(b, lst)
        for k, (b, lst) in enumerate(zip(bufs, lists)):
            gtx_ctx.dev_download(got, b)
            np.testing.assert_array_equal(got, draw.rasterize(f, lst, ATLAS), err_msg=f"draw {k}")
    finally:
        dr.close()
        for b in bufs:
            gtx_ctx.dev_free(b)
