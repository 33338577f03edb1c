"""The ORB stabilizer's kernels at the edges its one synthetic scene never reaches (csrc/stabilizer.hip; the RANSAC kernel: csrc/homography.hip).

Extract: the pyramid levels, the candidate sets after FAST + 3x3 maximum test + mask, the per-level counts and the keypoints of a
pass are read back (Stabilizer.keep_pass / level / candidates) and compared with oracle.stabilo_ref.extract bit for bit, on images
that overflow the former candidate lists, that send a level through the radix selection, that leave levels empty, at ragged sizes,
with every pyramid grouping, few levels, a level that wants nothing, and masks. Matcher and RANSAC kernel run one launch at a time
(ops.orb_match / ops.orb_ransac) against oracle.stabilo_ref.match + a plain numpy 2-NN, and oracle.stabilo_ref.ransac_hypotheses.
Every case first asserts, from the oracle alone, the property that makes it an edge case.

Frames are gray images stacked three times into BGR (the gray conversion then returns the byte) at downsample_ratio 1.0, so the
working image is the frame. Everything up to and including matching is integer work: array_equal, no tolerance."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BASE = dict(downsample_ratio=1.0, max_features=500, ref_multiplier=1.0, filter_ratio=0.9, ransac_threshold=2.0, mask_use=True,
            mask_margin_ratio=0.15, fast_threshold=20, n_levels=8, scale_factor=1.2, seed=0)
OLD_SORT_CAP = 8192            # eligible candidates one level's in-LDS sort takes; more go through the radix selection


# ------------------------------------------------------------------ images
@functools.lru_cache(maxsize=None)
def _image(name: str) -> np.ndarray:
    if name == "noise":
        g = np.random.default_rng(0).integers(0, 256, (480, 640), dtype=np.uint8)
    elif name in ("dots5", "dots4"):
        g = np.zeros((480, 640), np.uint8)
        p = int(name[-1])
        g[::p, ::p] = 255
    else:                                                   # "scene_<h>x<w>": the synthetic scene rendered at that size
        from geotrax_amd.synth import make_scene
        from oracle.stabilo_ref import bgr2gray

        h, w = (int(v) for v in name.split("_")[1].split("x"))
        g = bgr2gray(make_scene(seed=3, h=h, w=w).render(0), False)
    g.setflags(write=False)
    return g


def _bgr(gray):
    return np.ascontiguousarray(np.repeat(gray[:, :, None], 3, axis=2))


@functools.lru_cache(maxsize=None)
def _pattern():
    from oracle.stabilo_ref import brief_pattern

    return brief_pattern()


def _cfg(**over):
    return dict(BASE, **over)


@functools.lru_cache(maxsize=None)
def _oracle(name: str, boxes_key=None, **over):
    """(keypoints, per-level stages) of the oracle for a named image; computed once per configuration, never modified."""
    from oracle.stabilo_ref import extract

    cfg = _cfg(**over)
    stages = []
    boxes = None if boxes_key is None else np.asarray(boxes_key, np.float32).reshape(-1, 4)
    kp = extract(_image(name), boxes, cfg, cfg["max_features"], _pattern(), stages=stages)
    return kp, stages


def _make(gtx_ctx, hw, **over):
    from geotrax_amd.stabilizer import Stabilizer

    c = _cfg(**over)
    st = Stabilizer(hw, downsample_ratio=c["downsample_ratio"], max_features=c["max_features"], ref_multiplier=c["ref_multiplier"],
                    filter_ratio=c["filter_ratio"], ransac_epipolar_threshold=c["ransac_threshold"], mask_use=c["mask_use"],
                    mask_margin_ratio=c["mask_margin_ratio"], fast_threshold=c["fast_threshold"], n_levels=c["n_levels"],
                    scale_factor=c["scale_factor"], seed=c["seed"], ctx=gtx_ctx)
    st.keep_pass()
    return st


def _gpu_pass(st, gray, boxes=None, n_levels=8):
    st.set_ref_frame(_bgr(gray), boxes)
    return dict(kp=st.keypoints("ref"), levels=[st.level("ref", i) for i in range(n_levels)],
                cands=[st.candidates("ref", i) for i in range(n_levels)])


def _assert_pass_equals_oracle(got, kp, stages):
    assert len(got["levels"]) == len(stages)
    for i, (img, c, o) in enumerate(zip(got["levels"], got["cands"], stages)):
        np.testing.assert_array_equal(img, o["img"], err_msg=f"pyramid level {i}")
        assert c["dropped"] == 0, (i, c["dropped"])
        order = np.argsort(c["pix"], kind="stable")
        np.testing.assert_array_equal(c["pix"][order], o["pix"], err_msg=f"candidate pixels of level {i}")      # the oracle lists them in pixel order
        np.testing.assert_array_equal(c["score"][order], o["score"], err_msg=f"candidate scores of level {i}")
        if o["n_want"] > 0:
            assert c["n_elig"] == o["n_elig"], (i, c["n_elig"], o["n_elig"])
        assert c["n_kp"] == o["n_kp"], (i, c["n_kp"], o["n_kp"])
    g = got["kp"]
    assert len(g["bin"]) == len(kp["bin"])
    np.testing.assert_array_equal(g["level"], kp["level"])
    np.testing.assert_array_equal(g["xy"], kp["xy"])
    np.testing.assert_array_equal(g["bin"], kp["bin"])
    np.testing.assert_array_equal(g["desc"], kp["desc"])


# ------------------------------------------------------------------ extract
def test_noise_fills_more_than_the_former_candidate_lists(gtx_ctx):
    """Uniform noise: level 0 keeps more corners than max(4096, w * h / 16), the size the candidate lists used to have; what was
    dropped then depended on the order the atomics arrived in. Nothing is dropped, twice the same, all equal to the oracle."""
    kp, stages = _oracle("noise")
    h, w = _image("noise").shape
    assert len(stages[0]["pix"]) > max(4096, w * h // 16), len(stages[0]["pix"])
    print(f"level 0: {len(stages[0]['pix'])} corners, former cap {max(4096, w * h // 16)}")
    st = _make(gtx_ctx, (h, w))
    a = _gpu_pass(st, _image("noise"))
    b = _gpu_pass(st, _image("noise"))
    _assert_pass_equals_oracle(a, kp, stages)
    _assert_pass_equals_oracle(b, kp, stages)
    for k in ("xy", "level", "bin", "desc"):
        np.testing.assert_array_equal(a["kp"][k], b["kp"][k])


def test_saturated_dots_go_through_the_radix_selection(gtx_ctx):
    """255 on every fifth pixel: every dot scores 255 and has the same Harris response, so stage 1 hands all of them (more than
    8192) to stage 2, which is then the radix selection with its pixel-index tie-break on every element: the kept keypoints of
    level 0 are the first n_want dots in pixel order."""
    kp, stages = _oracle("dots5")
    assert stages[0]["n_elig"] > OLD_SORT_CAP and (stages[0]["score"] == 255).all(), stages[0]["n_elig"]
    h, w = _image("dots5").shape
    got = _gpu_pass(_make(gtx_ctx, (h, w)), _image("dots5"))
    _assert_pass_equals_oracle(got, kp, stages)
    n0 = stages[0]["n_kp"]
    assert n0 == stages[0]["n_want"] > 50
    first = stages[0]["pix"][:n0]
    np.testing.assert_array_equal(got["kp"]["xy"][:n0], np.stack([first % w, first // w], 1).astype(np.float32))


def test_one_level_wants_more_than_2048_from_the_radix_selection(gtx_ctx):
    """n_levels 1 puts all of max_features on level 0; with more than 8192 eligible dots the radix selection has to deliver 3000
    keypoints (it used to stop at 2048 without a word)."""
    kp, stages = _oracle("dots5", n_levels=1, max_features=3000)
    assert stages[0]["n_elig"] > OLD_SORT_CAP and stages[0]["n_want"] == 3000 and len(kp["bin"]) == 3000
    h, w = _image("dots5").shape
    got = _gpu_pass(_make(gtx_ctx, (h, w), n_levels=1, max_features=3000), _image("dots5"), n_levels=1)
    print(f"keypoints: {len(got['kp']['bin'])} of {stages[0]['n_want']} wanted")
    _assert_pass_equals_oracle(got, kp, stages)


def test_dots_of_period_4_and_the_overflow_count(gtx_ctx):
    """255 on every fourth pixel: a corner in every other 2x2 block (15 k of them on level 0). The pass reports how many candidates
    found their list full: none."""
    kp, stages = _oracle("dots4")
    assert len(stages[0]["pix"]) > 15000 and stages[0]["n_elig"] > OLD_SORT_CAP
    h, w = _image("dots4").shape
    got = _gpu_pass(_make(gtx_ctx, (h, w)), _image("dots4"))
    assert sum(c["dropped"] for c in got["cands"]) == 0
    _assert_pass_equals_oracle(got, kp, stages)


@pytest.mark.parametrize("group", [None, "1", "4"])
@pytest.mark.parametrize("size", ["487x653", "96x131"])
def test_ragged_sizes_and_empty_levels_under_every_pyramid_grouping(gtx_ctx, monkeypatch, size, group):
    """Level widths that are no multiple of 4 (the resize kernel's byte tail) and, at 96 x 131, levels narrower than twice the
    31-pixel border, which hold no keypoint although they want some. GTX_PYR_GROUP unset (groups of 3 and 4), 1 (a launch per
    level) and 4 must all produce the oracle's bytes."""
    if group is None:
        monkeypatch.delenv("GTX_PYR_GROUP", raising=False)
    else:
        monkeypatch.setenv("GTX_PYR_GROUP", group)
    name = f"scene_{size}"
    kp, stages = _oracle(name)
    h, w = _image(name).shape
    assert any(s["img"].shape[1] % 4 for s in stages[1:])
    empty = [i for i, s in enumerate(stages) if min(s["img"].shape) <= 62]
    if size == "96x131":
        assert empty and all(stages[i]["n_want"] > 0 and len(stages[i]["pix"]) == 0 for i in empty), empty
        assert len(kp["bin"]) > 0
    else:
        assert not empty and len(kp["bin"]) > 200
    got = _gpu_pass(_make(gtx_ctx, (h, w)), _image(name))
    _assert_pass_equals_oracle(got, kp, stages)


@pytest.mark.parametrize("n_levels,scale_factor,max_features", [(1, 1.2, 500), (2, 1.2, 500), (8, 1.2, 500), (1, 1.5, 500), (2, 1.5, 500),
                                                                (8, 1.5, 500), (8, 1.2, 8), (8, 1.5, 8)])
def test_level_counts_scale_factors_and_a_level_that_wants_nothing(gtx_ctx, n_levels, scale_factor, max_features):
    """1, 2 and 8 levels at scale factors 1.2 and 1.5; with 8 features over 8 levels the last level (at 1.5 the last three) wants
    none."""
    over = dict(n_levels=n_levels, scale_factor=scale_factor, max_features=max_features)
    kp, stages = _oracle("scene_487x653", **over)
    assert len(stages) == n_levels
    if max_features == 8:
        assert stages[-1]["n_want"] == 0 and sum(s["n_want"] for s in stages) == 8
        assert any(s["n_want"] == 0 and len(s["pix"]) > 0 for s in stages)               # corners are there, none is wanted
    h, w = _image("scene_487x653").shape
    got = _gpu_pass(_make(gtx_ctx, (h, w), **over), _image("scene_487x653"), n_levels=n_levels)
    _assert_pass_equals_oracle(got, kp, stages)


def test_mask_over_the_whole_frame_leaves_nothing(gtx_ctx):
    """One box over the whole frame: no candidate survives on any level, no keypoint, and a frame matched against that yields no
    match and no transform."""
    name = "scene_487x653"
    h, w = _image(name).shape
    boxes = ((w / 2, h / 2, float(w), float(h)),)
    kp, stages = _oracle(name, boxes_key=boxes)
    assert len(kp["bin"]) == 0 and all(len(s["pix"]) == 0 for s in stages)
    st = _make(gtx_ctx, (h, w))
    b = np.asarray(boxes, np.float32)
    got = _gpu_pass(st, _image(name), b)
    _assert_pass_equals_oracle(got, kp, stages)
    st.stabilize(_bgr(_image(name)), b)
    assert st.get_cur_num_keypoints() == (0, 0) and st.get_cur_num_matches() == 0
    assert st.get_cur_trans_matrix(raw=True) is None and not st.registered


def test_mask_boxes_clipped_at_all_four_frame_edges(gtx_ctx):
    name = "scene_487x653"
    h, w = _image(name).shape
    boxes = ((10.0, 200.0, 120.0, 90.0), (w - 5.0, 300.0, 150.0, 80.0), (300.0, 4.0, 100.0, 140.0), (350.0, h - 3.0, 180.0, 110.0),
             (w - 1.0, h - 1.0, 90.0, 90.0), (0.0, 0.0, 200.0, 160.0))
    kp, stages = _oracle(name, boxes_key=boxes)
    kp_free, _ = _oracle(name)
    assert 100 < len(kp["bin"]) and not np.array_equal(kp["xy"], kp_free["xy"])            # the boxes do remove keypoints
    got = _gpu_pass(_make(gtx_ctx, (h, w)), _image(name), np.asarray(boxes, np.float32))
    _assert_pass_equals_oracle(got, kp, stages)


# ------------------------------------------------------------------ matcher
NONE = 1 << 30


def _two_nn(dq, dt):
    """Plain 2-NN: (best_idx, best_d, second_d) per query; lowest index among equals; -1 / 2^30 where there is no neighbour."""
    nq, nt = len(dq), len(dt)
    bi, bd, sd = np.full(nq, -1, np.int32), np.full(nq, NONE, np.int32), np.full(nq, NONE, np.int32)
    if nt == 0:
        return bi, bd, sd
    a, b = np.unpackbits(dq, axis=1).astype(np.float32), np.unpackbits(dt, axis=1).astype(np.float32)
    d = (a.sum(1)[:, None] + b.sum(1)[None, :] - 2.0 * (a @ b.T)).astype(np.int32)          # exact: every term is an integer <= 256
    bi = d.argmin(1).astype(np.int32)
    bd = d[np.arange(nq), bi]
    if nt > 1:
        d[np.arange(nq), bi] = NONE
        sd = d.min(1)
    return bi, bd.astype(np.int32), sd.astype(np.int32)


def _assert_match_equals_oracle(gtx_ctx, dq, dt, ratio, keep_all=False, **slots):
    from geotrax_amd import ops
    from oracle.stabilo_ref import match

    rng = np.random.default_rng(len(dq) * 7919 + len(dt))
    xq, xt = rng.uniform(0, 1000, (len(dq), 2)).astype(np.float32), rng.uniform(0, 1000, (len(dt), 2)).astype(np.float32)
    got = ops.orb_match(dq, dt, ratio, keep_all=keep_all, xy_q=xq, xy_t=xt if len(dt) else None, ctx=gtx_ctx, **slots)
    bi, bd, sd = _two_nn(dq, dt)
    np.testing.assert_array_equal(got["best_idx"], bi)
    np.testing.assert_array_equal(got["best_d"], bd)
    np.testing.assert_array_equal(got["second_d"], sd)
    q, t, d = match(dq, dt, ratio, keep_all=keep_all)
    np.testing.assert_array_equal(got["q"], q)
    np.testing.assert_array_equal(got["t"], t)
    np.testing.assert_array_equal(got["d"], d)
    np.testing.assert_array_equal(got["pts"], np.concatenate([xq[q], xt[t]], 1).reshape(-1, 4))
    assert all((tail == -1).all() for tail in got["tail"])                                   # nothing is written past the count
    return got


def _random_desc(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


SIZES = [(1, 0), (5, 1), (5, 2), (255, 256), (257, 257), (300, 2049), (700, 2305)]


@pytest.mark.parametrize("keep_all", [False, True])
@pytest.mark.parametrize("nq,nt", SIZES)
def test_match_sizes_around_the_chunk_and_the_merge_width(gtx_ctx, nq, nt, keep_all):
    """No train keypoint, one, two; query and train counts on both sides of 256 (a workgroup / a train chunk); more than eight
    train chunks (the merge takes them eight at a time). Random descriptors, with the ratio test and without."""
    rng = np.random.default_rng(nq * 10007 + nt)
    got = _assert_match_equals_oracle(gtx_ctx, _random_desc(rng, nq), _random_desc(rng, nt), 0.95, keep_all)
    if nt > 2048:
        assert -(-nt // 256) > 8
    if keep_all:
        assert got["n"] == (nq if nt >= 1 else 0)
    elif nt < 2:
        assert got["n"] == 0


@pytest.mark.parametrize("nq,nt,slots_q,slots_t", [(300, 2049, 512, 2560), (5, 2, 600, 4000), (257, 257, 257, 1024)])
def test_match_with_more_slots_than_keypoints(gtx_ctx, nq, nt, slots_q, slots_t):
    """The stabilizer's grid covers the keypoint slots, not the counts: workgroups without queries or without train rows only draw
    a ticket."""
    rng = np.random.default_rng(nq + nt)
    _assert_match_equals_oracle(gtx_ctx, _random_desc(rng, nq), _random_desc(rng, nt), 0.9, slots_q=slots_q, slots_t=slots_t)


def test_match_equal_distances_inside_and_across_chunks(gtx_ctx):
    """Duplicated train rows in one chunk, in two neighbouring chunks and on both sides of the merge's eight-chunk step: the lowest
    index wins and second_d == best_d. Queries identical to a train row have distance 0."""
    rng = np.random.default_rng(11)
    nt = 2305
    assert -(-nt // 256) > 8
    dt = _random_desc(rng, nt)
    dt[40] = dt[33]                  # the same chunk
    dt[300] = dt[5]                  # chunks 0 and 1
    dt[2100] = dt[5]                 # ... and chunk 8, the merge's second round
    dt[2304] = dt[1000]              # chunks 3 and 9 (the last chunk holds one row)
    dq = _random_desc(rng, 300)
    for i, j in enumerate((33, 40, 5, 300, 2100, 1000, 2304)):
        dq[i] = dt[j]                # identical: d = 0
        dq[10 + i] = dt[j]
        dq[10 + i, rng.integers(0, 32, 3)] ^= 1 << 3   # near: d <= 3
    got = _assert_match_equals_oracle(gtx_ctx, dq, dt, 0.9)
    np.testing.assert_array_equal(got["best_idx"][:7], [33, 33, 5, 5, 5, 1000, 1000])
    np.testing.assert_array_equal(got["best_d"][:7], 0)
    np.testing.assert_array_equal(got["second_d"][:7], 0)
    np.testing.assert_array_equal(got["best_idx"][10:17], [33, 33, 5, 5, 5, 1000, 1000])
    np.testing.assert_array_equal(got["second_d"][10:17], got["best_d"][10:17])
    assert not np.isin(np.arange(7), got["q"]).any()             # d1 == d2 never passes the ratio test
    keep = _assert_match_equals_oracle(gtx_ctx, dq, dt, 0.9, keep_all=True)
    assert keep["n"] == 300


def test_match_ties_everywhere(gtx_ctx):
    """Train rows drawn from a pool of 48 distinct descriptors, queries a few bits away from pool members: nearly every query has
    several nearest neighbours at the same distance, in its own chunk and in others."""
    rng = np.random.default_rng(5)
    pool = _random_desc(rng, 48)
    dt = pool[rng.integers(0, 48, 2305)]
    dq = pool[rng.integers(0, 48, 700)].copy()
    dq[np.arange(700), rng.integers(0, 32, 700)] ^= rng.integers(0, 256, 700).astype(np.uint8)
    got = _assert_match_equals_oracle(gtx_ctx, dq, dt, 0.9)
    assert (got["second_d"] == got["best_d"]).mean() > 0.9
    _assert_match_equals_oracle(gtx_ctx, dq, dt, 0.9, keep_all=True)


def _bits(n_set):
    d = np.zeros(256, np.uint8)
    d[:n_set] = 1
    return np.packbits(d)


@pytest.mark.parametrize("d1,accepted", [(48, False), (47, True)])
def test_ratio_test_exactly_on_the_boundary(gtx_ctx, d1, accepted):
    """ratio 0.75, second_d 64: 0.75 * 64 is 48 exactly in fp32, so best_d 48 is NOT below it and is rejected; 47 is accepted.
    Best and second neighbour sit in different chunks."""
    assert np.float32(0.75) * np.float32(64) == np.float32(48)
    rng = np.random.default_rng(2)
    dt = _random_desc(rng, 600)
    dq = np.zeros((1, 32), np.uint8)
    dt[500] = _bits(d1)
    dt[10] = _bits(64)
    bi, bd, sd = _two_nn(dq, dt)
    assert (bi[0], bd[0], sd[0]) == (500, d1, 64)               # every random row is further away
    got = _assert_match_equals_oracle(gtx_ctx, dq, dt, 0.75)
    assert got["n"] == (1 if accepted else 0)


def test_match_ticket_is_rearmed_between_calls(gtx_ctx):
    """The ticket word is written by the host once per context; two calls back to back with different sizes both find it armed."""
    rng = np.random.default_rng(3)
    _assert_match_equals_oracle(gtx_ctx, _random_desc(rng, 300), _random_desc(rng, 700), 0.9)
    _assert_match_equals_oracle(gtx_ctx, _random_desc(rng, 40), _random_desc(rng, 3000), 0.9)
    _assert_match_equals_oracle(gtx_ctx, _random_desc(rng, 300), _random_desc(rng, 700), 0.9)


# ------------------------------------------------------------------ RANSAC kernel
WH = (1280, 720)
H_TRUE = np.array([[1.01, 0.02, 5.0], [-0.015, 0.99, -3.0], [2e-5, -1e-5, 1.0]])
A_TRUE = np.array([[1.01, 0.02, 5.0], [-0.015, 0.99, -3.0], [0.0, 0.0, 1.0]])


def _pairs(n, M, seed, outliers=0.3):
    """n point pairs on the map M, float32, the first round(outliers * n) of them (after a shuffle) replaced by random points."""
    rng = np.random.default_rng(seed)
    p = np.stack([rng.uniform(20, WH[0] - 20, n), rng.uniform(20, WH[1] - 20, n)], 1)
    q = np.c_[p, np.ones(n)] @ M.T
    q = q[:, :2] / q[:, 2:]
    bad = rng.permutation(n)[:int(round(outliers * n))]
    q[bad] = np.stack([rng.uniform(0, WH[0], len(bad)), rng.uniform(0, WH[1], len(bad))], 1)
    return np.concatenate([p, q], 1).astype(np.float32)


def _grid_err(Ha, Hb):
    ys, xs = np.meshgrid(np.linspace(0, WH[1] - 1, 9), np.linspace(0, WH[0] - 1, 16), indexing="ij")
    g = np.stack([xs.ravel(), ys.ravel(), np.ones(xs.size)])
    a, b = Ha @ g, Hb @ g
    return float(np.abs(a[:2] / a[2] - b[:2] / b[2]).max())


def _assert_ransac_equals_oracle(gtx_ctx, pts, n_hyp, seed, affine=False, thr=2.0):
    from geotrax_amd import ops
    from oracle.stabilo_ref import ransac_hypotheses

    best, cost, H = ops.orb_ransac(pts, seed, n_hyp, WH, thr, affine=affine, ctx=gtx_ctx)
    rb, rc, rH = ransac_hypotheses(pts[:, :2], pts[:, 2:], WH, thr, n_hyp, seed, affine=affine)
    n = len(pts)
    print(f"n {n} affine {affine}: winner {best} (oracle {rb}), cost {cost} (oracle {rc})")
    assert best == rb
    assert abs(cost - rc) <= n, (cost, rc)            # every term is rounded once: FMA or not may move each by one unit
    if rb < 0:
        assert cost == 0
        np.testing.assert_array_equal(H, np.zeros((3, 3)))
    else:
        err = _grid_err(H, rH)
        print(f"    H against the oracle's hypothesis {rb}: {err:.3e} px over the 9 x 16 grid")
        assert err < 1e-6, err
        if affine:
            np.testing.assert_array_equal(H[2], [0.0, 0.0, 1.0])
    return best, cost, H


@pytest.mark.parametrize("n", [3, 4, 5, 64, 65, 1000])
def test_ransac_homography_hypotheses(gtx_ctx, n):
    """Pairs on a known homography with 30 % outliers: fewer pairs than a sample (no winner), exactly one sample, and counts on
    both sides of a wave's 64 lanes. 300 hypotheses: 38 workgroups, the last one with four."""
    pts = _pairs(n, H_TRUE, seed=n)
    best, cost, H = _assert_ransac_equals_oracle(gtx_ctx, pts, 300, seed=7)
    assert (best < 0) == (n < 4)
    if n >= 64:
        assert _grid_err(H, H_TRUE) < 0.5 and cost < 0.4 * n * 4096            # an all-inlier sample wins: only the outliers cost


@pytest.mark.parametrize("n", [2, 3, 200])
def test_ransac_affine_hypotheses(gtx_ctx, n):
    pts = _pairs(n, A_TRUE, seed=100 + n)
    best, cost, H = _assert_ransac_equals_oracle(gtx_ctx, pts, 300, seed=9, affine=True)
    assert (best < 0) == (n < 3)
    if n == 200:
        assert _grid_err(H, A_TRUE) < 0.5


@pytest.mark.parametrize("affine", [False, True])
def test_ransac_collinear_points_make_no_hypothesis(gtx_ctx, affine):
    """Every pair on one line (exactly: integer coordinates on y = 2x + 3): no sample has three points in general position."""
    x = np.arange(10, 210, dtype=np.float32)
    pts = np.stack([x, 2 * x + 3, x + 1, 2 * (x + 1) + 3], 1).astype(np.float32)
    best, cost, H = _assert_ransac_equals_oracle(gtx_ctx, pts, 300, seed=1, affine=affine)
    assert best == -1 and not H.any()


def test_ransac_state_is_rearmed_between_calls(gtx_ctx):
    """The state words (best key, tickets) are written by the host once per context: consecutive calls with different inputs, a
    call without a winner in between, all find them armed and leave the next one its own answer."""
    a, b = _pairs(500, H_TRUE, seed=21), _pairs(120, np.linalg.inv(H_TRUE), seed=22)
    ra = _assert_ransac_equals_oracle(gtx_ctx, a, 256, seed=3)
    rb = _assert_ransac_equals_oracle(gtx_ctx, b, 64, seed=4)
    _assert_ransac_equals_oracle(gtx_ctx, a[:3], 256, seed=3)                  # no winner: the key stays armed
    ra2 = _assert_ransac_equals_oracle(gtx_ctx, a, 256, seed=3)
    assert ra[:2] == ra2[:2] and np.array_equal(ra[2], ra2[2]) and ra[0] >= 0 and rb[0] >= 0
    assert _grid_err(rb[2], np.linalg.inv(H_TRUE)) < 0.5
