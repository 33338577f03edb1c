"""The sparse Detect box launch (csrc/head_sparse.hip: head_sparse_box_kernel<false> and <true>) on its own, through
gtx_op_head_sparse_box, entry by entry against a float64 reference written here. The whole-detector tests reach this kernel at the
candidates that one or two checkpoints' score gates happen to pick; here the candidates are given, so every anchor, every count on
both sides of the 4-per-wave and 16-per-workgroup boundaries, the clamp at lvl_cap, 1 x 1 to 5 x 7 maps, four levels, every K-step
count from 9 to 72, a channel slice inside a wider buffer, a stacked first layer and the saturation flag are all driven directly.

Reference. float64, from the values the pair format holds (hi = fp16(x), lo = fp16(x - hi)): 3x3 zero-padded convolution + SiLU,
the same again (its padding is zeros of the first layer's OUTPUT), then the decode -- reg_max 16: the 64 x 64 1x1, a softmax
expectation over 16 bins per side, dist2bbox, xywh -> xyxy, times the stride; reg_max 1: the four-output 1x1 as signed distances
from the cell centre, times the stride. The same recipe in plain float32 on the CPU gives e_fp32ref.

Bar (test_ops_gpu.py's rule, as test_head_ops_gpu.py takes it): error = max-abs over the float64 reference's max-abs, per level so
that a small level is not hidden by a large one's scale; e_kernel < 8 * e_fp32ref + 1e-7, both printed (pytest -s). Box weights are
1 / sqrt(fan-in) with a bias of 0.3 sigma, and every case asserts on the CPU that the distances are 0.02 cells or more (on
average) away from what the bias alone would give: the boxes depend on the features. The kernel takes its candidates as given: no case depends on a decision.

Entries the lists do not name must keep the hook's 0xFF canary (NaN bits, checked as bits). Unnamed entries of cand_anchor hold
valid anchors and list tails hold entry 0, which no list names: a kernel that read past a count would break entry 0's canary
instead of following a wild index.
"""
import functools
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F16, F32, F64 = np.float16, np.float32, np.float64
MAPS = [(5, 7), (3, 4), (2, 2), (1, 1)]              # 35 + 12 + 4 + 1 anchors; the 2 x 2 and 1 x 1 maps are mostly second-layer padding
CINS = [96, 32, 128, 64]                             # 27, 9, 36 and 18 K steps: odd and even chunk counts, the shortest pipeline
LVL_CAP = 48                                         # three workgroups of 16 per level
CAP = 80
CANARY = np.uint32(0xFFFFFFFF)
FOREIGN = 1000.0                                     # what the map's channels outside [coff, coff + cin) hold


def _seed(*parts):
    return zlib.crc32(repr(parts).encode())


def _value_bar(label, got, ref64, ref32):
    scale = float(np.abs(ref64).max())
    e_k = float(np.abs(np.asarray(got, F64) - ref64).max() / scale)
    e_r = float(np.abs(np.asarray(ref32, F64) - ref64).max() / scale)
    print(f"{label}: e_kernel {e_k:.3e} e_fp32ref {e_r:.3e} ratio {e_k / max(e_r, 1e-30):.2f}")
    assert e_k < 8 * e_r + 1e-7, (label, e_k, e_r)


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _pairs(a):
    """The float64 values the pair format holds of a float32 array."""
    hi = a.astype(F16).astype(F32)
    return hi.astype(F64) + (a - hi).astype(F16).astype(F64)


# ---------------------------------------------------------------------------- levels and the reference
def _make_levels(rng, maps, cins, *, n=2, reg_max=16, c1out=64, coff=8, room=24):
    lv = []
    for l, ((h, w), cin) in enumerate(zip(maps, cins)):
        feat = np.full((n, h, w, cin + room), FOREIGN, F32)
        feat[..., coff:coff + cin] = rng.standard_normal((n, h, w, cin))
        lv.append(dict(feat=feat, coff=coff, cin=cin, stride=float(8 << l),
                       w1=(rng.standard_normal((c1out, 3, 3, cin)) / np.sqrt(9 * cin)).astype(F32), b1=(0.3 * rng.standard_normal(c1out)).astype(F32),
                       w2=(rng.standard_normal((64, 3, 3, 64)) / np.sqrt(9 * 64)).astype(F32), b2=(0.3 * rng.standard_normal(64)).astype(F32),
                       wb=(rng.standard_normal((64, 4 * reg_max)) / np.sqrt(64)).astype(F32), bb=(0.3 * rng.standard_normal(4 * reg_max)).astype(F32)))
    return lv


def _begins(levels):
    return np.cumsum([0] + [lv["feat"].shape[1] * lv["feat"].shape[2] for lv in levels])


def _conv3x3(x, w, b, prec):
    """Zero-padded 3x3 convolution of x [n, h, w, c] with w [o, 3, 3, c] + b, no activation, in `prec`."""
    n, h, wd, _ = x.shape
    xp = np.zeros((n, h + 2, wd + 2, x.shape[3]), prec)
    xp[:, 1:-1, 1:-1] = x
    wt = w.astype(prec)
    y = np.zeros((n, h, wd, w.shape[0]), prec) + b.astype(prec)
    for ky in range(3):
        for kx in range(3):
            y = y + xp[:, ky:ky + h, kx:kx + wd] @ wt[:, ky, kx].T
    return y


def _silu(z):
    with np.errstate(over="ignore"):                 # exp(-z) = inf for a very negative z: the quotient is -0, as it should be
        return z / (1 + np.exp(-z))


def _layers(L, prec):
    """The level's 64 box features at every pixel [n, h, w, 64] and the first layer's pre-activation [n, h, w, 64], in `prec`."""
    x = _pairs(L["feat"][..., L["coff"]:L["coff"] + L["cin"]]).astype(prec)          # hi + lo is exact in float32
    z1 = _conv3x3(x, L["w1"][:64], L["b1"][:64], prec)
    return _silu(_conv3x3(_silu(z1), L["w2"], L["b2"], prec)), z1


def _decode(L, f, la, reg_max, prec):
    """xyxy [k, 4] and the distances [k, 4] of the anchors la (level-local) with features f [k, 64]."""
    z = f @ L["wb"].astype(prec) + L["bb"].astype(prec)
    w = L["feat"].shape[2]
    ax, ay = (la % w).astype(prec) + prec(0.5), (la // w).astype(prec) + prec(0.5)
    s = prec(L["stride"])
    if reg_max == 1:
        return np.stack([(ax - z[:, 0]) * s, (ay - z[:, 1]) * s, (ax + z[:, 2]) * s, (ay + z[:, 3]) * s], -1), z
    z = z.reshape(-1, 4, 16)
    e = np.exp(z - z.max(-1, keepdims=True))
    d = (e * np.arange(16).astype(prec)).sum(-1) / e.sum(-1)
    x1, y1, x2, y2 = ax - d[:, 0], ay - d[:, 1], ax + d[:, 2], ay + d[:, 3]
    cx, cy, bw, bh = (x1 + x2) * prec(0.5) * s, (y1 + y2) * prec(0.5) * s, (x2 - x1) * s, (y2 - y1) * s
    return np.stack([cx - bw / prec(2), cy - bh / prec(2), cx + bw / prec(2), cy + bh / prec(2)], -1), d


def _reference(levels, reg_max, prec, vary=True):
    """Boxes of every anchor of every image [n, A, 4] in `prec`."""
    out = []
    for L in levels:
        f, _ = _layers(L, prec)
        n, h, w, _ = f.shape
        la = np.tile(np.arange(h * w), n)
        box, d = _decode(L, f.reshape(n * h * w, 64), la, reg_max, prec)
        _, d0 = _decode(L, np.zeros((n * h * w, 64), prec), la, reg_max, prec)
        assert not vary or np.abs(d - d0).mean() > 0.02, "the distances must depend on the features, not on the bias alone"
        out.append(box.reshape(n, h * w, 4))
    return np.concatenate(out, 1)


class Case:
    """Levels with their float64 and float32 boxes of every anchor, computed once."""

    def __init__(self, levels, reg_max, vary=True):
        self.levels, self.reg_max = levels, reg_max
        self.r64, self.r32 = _reference(levels, reg_max, F64, vary), _reference(levels, reg_max, F32, vary)
        self.begin = _begins(levels)
        self.n = levels[0]["feat"].shape[0]

    def level_of(self, a):
        return int(np.searchsorted(self.begin[1:], a, side="right"))


@functools.lru_cache(maxsize=None)
def _base(reg_max):
    return Case(_make_levels(np.random.default_rng(_seed("base", reg_max)), MAPS, CINS, reg_max=reg_max), reg_max)


def _file(case, rng, per_image, cap=CAP, lvl_cap=LVL_CAP, counts=None):
    """per_image[b][l]: the anchors (global) of image b's level-l list, in list order. Entry indices are drawn at random from
    [1, cap): list order, entry index and anchor are three different things. counts overrides lvl_count (the clamp case)."""
    n = case.n
    A = int(case.begin[-1])
    anchor = rng.integers(0, A, (n, cap)).astype(np.int32)
    lvl_count, lvl_list = np.zeros((n, 4), np.int32), np.zeros((n, 4, lvl_cap), np.int32)
    for b in range(n):
        total = sum(len(x) for x in per_image[b])
        assert total < cap and all(len(x) <= lvl_cap for x in per_image[b])
        free = (1 + rng.permutation(cap - 1))[:total].tolist()
        for l, lst in enumerate(per_image[b]):
            for k, a in enumerate(lst):
                assert case.level_of(a) == l
                e = free.pop()
                anchor[b, e] = a
                lvl_list[b, l, k] = e
            lvl_count[b, l] = len(lst)
    if counts is not None:
        lvl_count = np.asarray(counts, np.int32)
    count = np.array([sum(len(x) for x in per_image[b]) for b in range(n)], np.int32)
    return count, anchor, lvl_count, lvl_list


def _run(case, filed):
    from geotrax_amd import ops

    return ops.head_sparse_box(case.levels, *filed, reg_max=case.reg_max)


def _check(label, case, filed, box, per_image):
    """Each listed entry meets the bar, per level; two entries of one anchor hold bit-equal boxes; every other entry is canary."""
    _, anchor, _, lvl_list = filed
    named = np.zeros(box.shape[:2], bool)
    for l in range(len(case.levels)):
        got, r64, r32 = [], [], []
        for b in range(case.n):
            k = len(per_image[b][l])
            e = lvl_list[b, l, :k]
            assert (anchor[b, e] == np.asarray(per_image[b][l], np.int32)).all()
            named[b, e] = True
            assert not np.isnan(box[b, e]).any(), (label, b, l)
            got.append(box[b, e]); r64.append(case.r64[b, anchor[b, e]]); r32.append(case.r32[b, anchor[b, e]])
            seen = {}
            for i, a in zip(e.tolist(), anchor[b, e].tolist()):
                if a in seen:
                    np.testing.assert_array_equal(_bits(box[b, i]), _bits(box[b, seen[a]]), err_msg=f"{label}: anchor {a} twice")
                seen[a] = i
        if sum(len(g) for g in got):
            _value_bar(f"{label} level {l}", np.concatenate(got), np.concatenate(r64), np.concatenate(r32))
    assert (_bits(box)[~named] == CANARY).all(), (label, "an entry no list names was written")


def _level_anchors(case, l):
    return np.arange(case.begin[l], case.begin[l + 1])


# ---------------------------------------------------------------------------- the cases
@pytest.mark.parametrize("reg_max", [16, 1])
def test_every_anchor(reg_max):
    """Every anchor of every level once, in shuffled list order at shuffled entry indices: all four corners and edges of each map,
    the 2 x 2 map (every first-layer neighbourhood crosses the border) and the 1 x 1 map (eight of nine first-layer pixels are padding)."""
    case = _base(reg_max)
    rng = np.random.default_rng(_seed("every", reg_max))
    per_image = [[rng.permutation(_level_anchors(case, l)).tolist() for l in range(4)] for _ in range(case.n)]
    filed = _file(case, rng, per_image)
    box, sat = _run(case, filed)
    assert sat == 0
    _check(f"every anchor reg_max={reg_max}", case, filed, box, per_image)


@pytest.mark.parametrize("c0", [0, 1, 3, 4, 5, 15, 16, 17, 33])
@pytest.mark.parametrize("reg_max", [16, 1])
def test_counts(reg_max, c0):
    """Level 0's count on both sides of the wave (4) and workgroup (16) boundaries, with anchors repeated (the last entry repeats
    the first from c0 = 3 on; c0 = 33 draws 31 distinct anchors of the 35). The other image has no level-0 entry (6 when c0 = 0);
    the other levels hold 0 or 1."""
    case = _base(reg_max)
    rng = np.random.default_rng(_seed("counts", reg_max, c0))
    a0 = rng.permutation(_level_anchors(case, 0)).tolist()
    lst = a0[:c0]
    if c0 >= 3:
        lst[-1] = lst[0]
    if c0 >= 17:
        lst[-2] = lst[5]
    one = lambda l: [int(rng.choice(_level_anchors(case, l)))]
    per_image = [[lst, one(1), [], one(3)], [a0[3:9] if c0 == 0 else [], [], one(2), []]]
    filed = _file(case, rng, per_image)
    box, sat = _run(case, filed)
    assert sat == 0
    _check(f"counts reg_max={reg_max} c0={c0}", case, filed, box, per_image)


@pytest.mark.parametrize("reg_max", [16, 1])
@pytest.mark.parametrize("lvl_cap", [44, 47, 48])
def test_lvl_count_above_lvl_cap_is_clamped(reg_max, lvl_cap):
    """lvl_count = lvl_cap + 5 over a full list: exactly the list's lvl_cap entries are computed, nothing else is touched. The grid
    holds ceil(lvl_cap / 16) = 3 workgroups per level, so only a lvl_cap that is no multiple of 16 (the detector passes any) leaves
    list slots 44..47 or 47 within the grid's reach: without the clamp the last wave would go on into the NEXT level's list (inside
    the buffer: the full lists are on levels 0 and 1), whose slots hold entry 0, which no list names -- its canary would break. At
    48 the clamp decides nothing (the last wave ends at slot 47 either way): the full-list case."""
    case = _base(reg_max)
    rng = np.random.default_rng(_seed("clamp", reg_max, lvl_cap))
    full = lambda l: rng.choice(_level_anchors(case, l), lvl_cap).tolist()
    per_image = [[full(0), [], [], []], [[], full(1), [], []]]
    counts = [[lvl_cap + 5, 0, 0, 0], [0, lvl_cap + 5, 0, 0]]
    filed = _file(case, rng, per_image, lvl_cap=lvl_cap, counts=counts)
    filed[1][0, 0], filed[1][1, 0] = case.begin[0] + 3, case.begin[1] + 3    # entry 0 holds an anchor of the full level: reg_max 1 re-checks the level before it stores
    box, sat = _run(case, filed)
    assert sat == 0
    _check(f"clamp reg_max={reg_max} lvl_cap={lvl_cap}", case, filed, box, per_image)


@pytest.mark.parametrize("coff", [0, 40])
@pytest.mark.parametrize("cin", [32, 64, 96, 256])
def test_widths(cin, coff):
    """One 3 x 4 level: 9, 18, 27 and 72 K steps (the prefetch guard on the first trip; an odd chunk count; the widest shipped
    width), the slice at the buffer's start and 40 channels in. The channels around the slice hold 1000."""
    rng = np.random.default_rng(_seed("widths", cin, coff))
    case = Case(_make_levels(rng, [(3, 4)], [cin], coff=coff, room=48), 16)
    per_image = [[rng.permutation(12).tolist()] + [[]] * 3 for _ in range(2)]
    filed = _file(case, rng, per_image, cap=24, lvl_cap=16)
    box, sat = _run(case, filed)
    assert sat == 0
    _check(f"widths cin={cin} coff={coff}", case, filed, box, per_image)


def test_stacked_first_layer_shares_the_class_tiles_scale():
    """c1out = 192: the box tile is the first 64 rows of a stacked image whose power-of-two scale is set by a class row 60 times
    larger. The bar holds, and the boxes are not the c1out = 64 run's bits: the stack's scale was in force."""
    rng = np.random.default_rng(_seed("stacked"))
    lv = _make_levels(rng, MAPS[:2], [64, 32], c1out=192)
    for L in lv:
        L["w1"][64 + int(rng.integers(0, 128))] *= 60.0
    case = Case(lv, 16)
    alone = Case([dict(L, w1=L["w1"][:64].copy(), b1=L["b1"][:64].copy()) for L in lv], 16)
    np.testing.assert_array_equal(case.r64, alone.r64)                   # the reference reads the box tile only
    per_image = [[rng.permutation(_level_anchors(case, l)).tolist() for l in range(2)] + [[], []] for _ in range(2)]
    filed = _file(case, rng, per_image)
    box, sat = _run(case, filed)
    assert sat == 0
    _check("stacked c1out=192", case, filed, box, per_image)
    box1, _ = _run(alone, filed)
    _check("stacked c1out=64", alone, filed, box1, per_image)
    differ = int((_bits(box) != _bits(box1)).sum())
    print(f"stacked: {differ} of {box.size} box words differ between the c1out = 192 and c1out = 64 runs")
    assert differ > 0


@pytest.mark.parametrize("reg_max", [16, 1])
def test_exact_case(reg_max):
    """Small integers throughout: a constant integer input vector per pixel and integer weights whose every tap sums to exactly zero
    over the channels (so padding changes nothing, while the partial sums are non-zero integers, exact in fp16 and fp32), a centre
    tap that sums to S and a bias of -S: SiLU sees exactly 0 at every first-layer pixel and gives 0. The second layer, with a zero
    bias, gives 0 too, so the final 1x1 -- which keeps its ordinary random weights -- returns its bias: one value per side over the
    16 bins (reg_max 16: equal logits, every distance exactly 7.5 cells), or four distances that are exact in binary (reg_max 1).
    The boxes are then exact in every evaluation: bit equality with the float64 reference. What the box bits verify is the decode
    and that all 64 features are exactly zero (any other feature meets a non-zero weight and moves a logit); they do not verify
    the two layers' arithmetic on non-zero sums beyond that -- the value bar of the other cases does."""
    rng = np.random.default_rng(_seed("exact", reg_max))
    lv = _make_levels(rng, MAPS, CINS, reg_max=reg_max)
    for L in lv:
        cin, coff = L["cin"], L["coff"]
        v = rng.integers(1, 4, cin).astype(F32)
        v[-1] = 1
        L["feat"][..., coff:coff + cin] = v
        w1 = rng.integers(-8, 9, (64, 3, 3, cin)).astype(F32)
        w1[..., -1] = -(w1[..., :-1] * v[:-1]).sum(-1)                   # every tap: sum_c w v = 0
        w1[:, 1, 1, 0] += rng.integers(-5, 6, 64).astype(F32)            # the centre tap sums to S = this * v[0]
        assert np.abs(w1).max() < 2**13                                  # integers of at most 13 bits: hi + lo hold them exactly at any scale
        L["w1"] = w1
        L["b1"] = -(w1[:, 1, 1] * v).sum(-1).astype(F32)
        L["w2"] = rng.integers(-8, 9, (64, 3, 3, 64)).astype(F32)
        L["b2"] = np.zeros(64, F32)
        L["bb"] = np.repeat(rng.integers(-3, 4, 4), 16).astype(F32) if reg_max == 16 else np.array([2.5, -0.75, 7.0, 0.125], F32)
        assert np.abs(L["wb"]).min() > 0                                 # the ordinary final weights stay: a feature that is not 0 moves a box
    case = Case(lv, reg_max, vary=False)
    for L in lv:
        f, z1 = _layers(L, F64)
        assert (z1 == 0).all() and (f == 0).all()
    np.testing.assert_array_equal(case.r64.astype(F32).astype(F64), case.r64)
    per_image = [[rng.permutation(_level_anchors(case, l)).tolist() for l in range(4)] for _ in range(2)]
    filed = _file(case, rng, per_image)
    box, sat = _run(case, filed)
    assert sat == 0
    _, anchor, _, lvl_list = filed
    for b in range(2):
        for l in range(4):
            e = lvl_list[b, l, :len(per_image[b][l])]
            np.testing.assert_array_equal(_bits(box[b, e]), _bits(case.r64[b, anchor[b, e]].astype(F32)), err_msg=f"exact reg_max={reg_max} level {l}")
            if reg_max == 16:
                la = anchor[b, e] - case.begin[l]
                w, s = MAPS[l][1], lv[l]["stride"]
                want = np.stack([(la % w - 7.0) * s, (la // w - 7.0) * s, (la % w + 8.0) * s, (la // w + 8.0) * s], -1)
                np.testing.assert_array_equal(box[b, e], want.astype(F32))           # the cell centre -/+ 7.5 cells


def _halfway(y1):
    """First-layer values (hi + lo as float32, as the dense hook hands them back) that lie exactly half-way between two fp16
    numbers: the kernel held (lower, +half an ulp) or (upper, -half an ulp), the host cannot tell which, and splitting hi + lo again
    rounds to even. One float32 ulp up gives the hook's split the upper pair, one down the lower pair (the remainder, half an fp16
    ulp less 2^-13 of it, is itself a tie that rounds to the half). Values below fp16's normal range are `tiny`: left alone."""
    return (_bits(y1) & 0x1FFF) == 0x1000, np.abs(y1) < 2.0**-13


def _window_count(flag, h, w):
    """Per pixel [n, h * w]: how many flagged values its 3 x 3 window holds."""
    c = np.pad(flag.sum(-1), ((0, 0), (1, 1), (1, 1)))
    return sum(c[:, dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)).reshape(flag.shape[0], h * w)


@pytest.mark.parametrize("reg_max", [16, 1])
def test_against_the_dense_route_bit_for_bit(monkeypatch, reg_max):
    """The same layers through the dense hooks with GTX_K32=1 -- conv2d_fused(split=True), conv2d_fused(out_plain=True), head_boxes /
    head_boxes_r1 -- give the sparse launch's boxes bit for bit: the claim in the headers of head_sparse.hip and head_device.hpp, on
    every anchor of 5 x 7, 3 x 4, 2 x 2 and 1 x 1 maps with 96, 32, 128 and 64 input channels; no shape had to be dropped. That
    both dense layers ran the 16x16x32 form is shown as test_conv2d_k32_split_meets_the_fp32_bar shows it: GTX_K32=0 gives other bits.
    The two hook calls take the first layer's map through the host as hi + lo, and a value exactly half-way between two fp16 numbers
    has two (hi, lo) pairs; splitting it again may give the one the kernel did not hold (gtx_ops.cpp says so where it keeps
    post_separate on the device). About one value in 1100 is such a value, so the second dense layer runs twice, with every half-way
    value split to the upper pair and to the lower pair (_halfway). An entry with no such value among the 9 x 64 it reads must
    equal both runs; an entry with one must equal one of them, bit for bit: the dense route with the pair the kernel held. Entries
    with two or more (neither run need hold their combination), or with a value below fp16's normal range, are left to the value
    bar of test_every_anchor; they are counted and printed: every level must have entries that were compared (the 2 x 2 map's four
    anchors read the same pixels, and the 1 x 1 map has one entry per image), and over the levels they must be the majority."""
    from geotrax_amd import ops

    case = _base(reg_max)
    rng = np.random.default_rng(_seed("dense", reg_max))
    per_image = [[rng.permutation(_level_anchors(case, l)).tolist() for l in range(4)] for _ in range(case.n)]
    filed = _file(case, rng, per_image)
    box, _ = _run(case, filed)
    routes, halves = ([], []), []
    for l, L in enumerate(case.levels):
        kw = dict(split=True, in_coff=L["coff"], cin=L["cin"])
        monkeypatch.setenv("GTX_K32", "0")
        direct = ops.conv2d_fused(L["feat"], L["w1"], L["b1"], **kw)
        monkeypatch.setenv("GTX_K32", "1")
        y1 = ops.conv2d_fused(L["feat"], L["w1"], L["b1"], **kw)
        assert not np.array_equal(y1, direct), f"level {l}: the dense hook did not run the 16x16x32 form"
        half, tiny = _halfway(y1)
        h, w = MAPS[l]
        halves.append(_window_count(half, h, w) + 2 * _window_count(tiny, h, w))
        for route, to in zip(routes, (np.inf, -np.inf)):
            y2 = ops.conv2d_fused(np.where(half, np.nextafter(y1, F32(to)), y1), L["w2"], L["b2"], split=True, out_plain=True)
            route.append(dict(feat=y2, cb=64, cc=0, stride=L["stride"], wb=L["wb"], bb=L["bb"]))
        k32_2 = ops.conv2d_fused(y1, L["w2"], L["b2"], split=True, out_plain=True)
        monkeypatch.setenv("GTX_K32", "0")                               # the second layer ran the 16x16x32 form too
        direct_2 = ops.conv2d_fused(y1, L["w2"], L["b2"], split=True, out_plain=True)
        monkeypatch.setenv("GTX_K32", "1")
        assert not np.array_equal(k32_2, direct_2), f"level {l}: the dense hook did not run the second layer on the 16x16x32 form"
    A = int(case.begin[-1])
    every = np.tile(np.arange(A, dtype=np.int32), (case.n, 1))
    up, down = ((ops.head_boxes if reg_max == 16 else ops.head_boxes_r1)(r, np.full(case.n, A, np.int32), every) for r in routes)
    _, anchor, _, lvl_list = filed
    compared = uncompared = 0
    for l in range(4):
        both = one = left = 0
        for b in range(case.n):
            e = lvl_list[b, l, :len(per_image[b][l])]
            a = anchor[b, e]
            k = halves[l][b, a - case.begin[l]]
            is_up, is_down = (_bits(box[b, e]) == _bits(up[b, a])).all(-1), (_bits(box[b, e]) == _bits(down[b, a])).all(-1)
            assert (is_up & is_down)[k == 0].all(), f"dense route reg_max={reg_max} level {l} image {b}: entries {e[(k == 0) & ~(is_up & is_down)]}"
            assert (is_up | is_down)[k == 1].all(), f"dense route reg_max={reg_max} level {l} image {b}: entries {e[(k == 1) & ~(is_up | is_down)]}"
            both += int((k == 0).sum()); one += int((k == 1).sum()); left += int((k > 1).sum())
        print(f"dense route reg_max={reg_max} level {l}: {both} entries bit-equal, {one} bit-equal with their half-way value's upper or lower pair, "
              f"{left} left to the value bar")
        assert both + one > 0
        compared += both + one; uncompared += left
    assert compared > uncompared


def _sat_case(tap, hot, cands, reg_max=16):
    """A 5 x 7 level whose output channel 0 has weight 1 on `tap` (ky, kx) for every input channel, and one input pixel `hot` at
    3000 on all 32 channels: the first-layer pixel that reads `hot` through `tap` reaches 96 000, beyond fp16's 65 504; asserted on
    the CPU: it is the only one, and every other first-layer value stays below 30 000."""
    rng = np.random.default_rng(_seed("sat", tap, hot, tuple(cands)))
    lv = _make_levels(rng, [(5, 7)], [32], n=1, reg_max=reg_max)
    L = lv[0]
    L["w1"][0, tap[0], tap[1], :] = 1.0
    L["feat"][0, hot[0], hot[1], L["coff"]:L["coff"] + 32] = 3000.0
    x = np.zeros((1, 7, 9, 32), F64)
    x[:, 1:-1, 1:-1] = _pairs(L["feat"][..., L["coff"]:L["coff"] + 32])
    z = np.zeros((7, 9, 64)) + L["b1"].astype(F64)                       # the first layer one pixel beyond the map on every side
    xp = np.pad(x[0], ((1, 1), (1, 1), (0, 0)))
    for ky in range(3):
        for kx in range(3):
            z += xp[ky:ky + 7, kx:kx + 9] @ L["w1"].astype(F64)[:, ky, kx].T
    py, px = hot[0] + 1 - tap[0], hot[1] + 1 - tap[1]                    # the pixel that reads `hot` through `tap`
    over = np.argwhere(np.abs(_silu(z)) > 65504)
    assert [tuple(o) for o in over] == [(py + 1, px + 1, 0)], over
    zz = np.abs(_silu(z)); zz[py + 1, px + 1, 0] = 0
    assert zz.max() < 30000
    case = Case(lv, reg_max, vary=False)
    per_image = [[[cy * 7 + cx for cy, cx in cands], [], [], []]]
    filed = _file(case, rng, per_image, cap=8, lvl_cap=4)
    box, sat = _run(case, filed)
    return case, filed, per_image, box, sat, (py, px)


def test_saturation_flag():
    """A first-layer pixel driven over the fp16 range by the input's magnitude (no NaN, no Inf).
    Inside a candidate's 3 x 3 window: sat = 1. Two cells from the only candidate, a corner: sat = 0 and the box meets the bar.
    The cases the kernel excludes on purpose: a first-layer pixel outside the map is second-layer padding -- its accumulator is
    computed (here it reaches 96 000 through the tap that reads the row above) and must be zeroed before the flag looks at it; and MFMA
    columns 9..15 repeat window pixel 8, so they can see nothing pixel 8 does not: with pixel 8 cold (and, for the corner candidate,
    outside the map) and no hot pixel in the window the flag stays 0 whatever those columns hold."""
    centre = (1, 1)
    case, filed, per_image, box, sat, at = _sat_case(centre, (2, 2), [(3, 3)])
    assert at == (2, 2) and sat == 1                                     # window pixel 0 of candidate (3, 3)
    case, filed, per_image, box, sat, at = _sat_case(centre, (2, 2), [(1, 3)])
    assert sat == 1                                                      # window pixel 6
    case, filed, per_image, box, sat, at = _sat_case(centre, (2, 2), [(0, 0)])
    assert at == (2, 2) and sat == 0                                     # two cells away on both axes; window pixel 8 = (1, 1) is cold
    _check("sat: hot pixel two cells away", case, filed, box, per_image)
    case, filed, per_image, box, sat, at = _sat_case((0, 1), (4, 6), [(4, 6), (4, 5)])
    assert at == (5, 6) and sat == 0                                     # the hot accumulator belongs to a pixel below the map
    _check("sat: hot accumulator outside the map", case, filed, box, per_image)
    case, filed, per_image, box, sat, at = _sat_case((0, 1), (3, 6), [(4, 6)])
    assert at == (4, 6) and sat == 1                                     # the same tap, one row up: inside the map, window pixel 4


def test_refusals_then_a_valid_call():
    """One call per host refusal of the hook, each answered with its message before anything is launched; a valid call still works."""
    from geotrax_amd import ops
    from geotrax_amd._lib import GtxError

    rng = np.random.default_rng(_seed("refusals"))
    good = Case(_make_levels(rng, [(2, 2)], [32], n=1), 16)
    per_image = [[[0, 3, 1], [], [], []]]
    filed = _file(good, rng, per_image, cap=8, lvl_cap=4)
    count, anchor, lvl_count, lvl_list = filed

    def level(cin=32, coff=8, room=24, c1out=64, hw=(2, 2), n=1):
        return _make_levels(rng, [hw], [cin], n=n, coff=min(coff, 8), room=room, c1out=c1out)[0] | dict(coff=coff)

    def refused(msg, levels=None, c=count, a=anchor, lc=lvl_count, ll=lvl_list, reg_max=16):
        with pytest.raises(GtxError, match=msg):
            ops.head_sparse_box(levels or good.levels, c, a, lc, ll, reg_max=reg_max if levels is None else levels[0]["wb"].shape[1] // 4)

    refused("multiple of 32", [level(cin=48)])
    refused("multiple of 32", [level(cin=16)])
    refused("coff must be a multiple of 8", [level(coff=4)])
    refused("do not fit", [level(coff=32)])
    five = [level() for _ in range(5)]
    refused("at most 4 levels", five)
    refused("lvl_cap >= 1", ll=np.zeros((1, 4, 0), np.int32))
    neg = lvl_count.copy(); neg[0, 0] = -1
    refused("negative lvl_count", lc=neg)
    for bad in (8, -1):
        out = lvl_list.copy(); out[0, 0, 2] = bad
        refused(r"outside \[0, cap\)", ll=out)
    wrong = anchor.copy(); wrong[0, lvl_list[0, 0, 1]] = 4
    refused("not inside the level", a=wrong)
    two = [good.levels[0], level()]
    lc2 = lvl_count.copy(); lc2[0, 1] = 1                                # level 1's list names entry 0... whose anchor is level 0's or beyond
    a2 = anchor.copy(); a2[0, 0] = 2
    refused("not inside the level", two, a=a2, lc=lc2)
    refused("bad sizes", [level(n=65)], c=np.zeros(65, np.int32), a=np.zeros((65, 8), np.int32), lc=np.zeros((65, 4), np.int32),
            ll=np.zeros((65, 4, 4), np.int32))
    refused("c1out", [dict(level(), w1=np.zeros((96, 3, 3, 32), F32), b1=np.zeros(96, F32))])
    box, sat = _run(good, filed)
    assert sat == 0
    _check("after the refusals", good, filed, box, per_image)
