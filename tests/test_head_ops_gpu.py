"""The detector's post-pass kernels (csrc/det_kernels.hip, csrc/v10_select.hip) one launcher at a time through gtx_op_head_gate,
_head_boxes, _nms, _v10_select, _v10_rows and _obj_feats, each against a float64 reference written here, on the smallest shapes that
reach every path. The whole-detector tests reach these kernels with seeded random weights only, which place no exact tie, no IoU on
the threshold, no suppression chain across a 64-box block and no full buffer, and several of them forgive borderline rows.

Bars.
  Values (scores, boxes, frame rows, appearance vectors): error = max-abs over the float64 reference's max-abs;
  e_kernel < 8 * e_fp32ref + 1e-7 (test_ops_gpu.py's rule), where e_fp32ref is the error of the same recipe in plain float32 on the
  CPU, computed in the test and printed beside e_kernel (pytest -s). fp16 / pair-format inputs: the float64 reference starts from
  the values the format holds.
  Decisions (which anchors pass the gate, class, sort order, kept set, counts, selected entries): exact. The inputs are chosen so
  that float64 alone decides: before any launch the test asserts that no float64 score lies within 1e-5 of conf, that an anchor's
  two best classes are 1e-5 apart or exactly equal (a copied weight row), and that no float64 pair IoU -- on the boxes after the
  float32 class-offset add, ultralytics' own arithmetic -- lies within 1e-5 of iou_thr; it reseeds until that holds. Nothing is
  excluded afterwards: the margin is a condition on the inputs, not a tolerance on the kernel.
  Exact edges use values that are exact in every evaluation: integer boxes with areas below 2^24 (an IoU of exactly 0.5 does not
  suppress at iou_thr = 0.5, and does at nextafter(0.5, 0); those two cases sit on the threshold by construction and are the only ones
  without the IoU margin), zero class weights (score 0.5: nothing passes at conf = 0.5, everything at nextafter(0.5, 0)), DFL logits
  that are all equal (distance 7.5). Bit-equal scores are made by copying a feature vector to another anchor or a weight row to
  another class: equal whatever the kernel's arithmetic is.
  The YOLOv10 selection is checked exactly against the kernel's own scores (its scratch rows, and the gate's scores for stage 1), so
  that the selection logic is separated from the rounding of the sigmoid; the scratch rows themselves are held to the value bar and
  their maximum to bit-equality with the gate's score of the same anchor.
"""
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FULL = (2**64 - 1, 2**64 - 1)
MARGIN = 1e-5
F16, F32 = np.float16, np.float32
SHAPES = [(5, 7), (3, 4), (2, 2)]                    # 35 + 12 + 4 = 51 anchors: not a multiple of 16, levels not square
EDGE_ANCHORS = [0, 34, 35, 46, 47, 50]               # both sides of every anchor_begin, first and last anchor


def _seed(*parts):
    return zlib.crc32(repr(parts).encode())


def _words(classes):
    m = sum(1 << c for c in classes)
    return (m & (2**64 - 1), m >> 64)


def _bit(words, c):
    return (np.array([(words[int(k) >> 6] >> (int(k) & 63)) & 1 for k in np.ravel(c)], bool)).reshape(np.shape(c))


def _value_bar(label, got, ref64, ref32):
    scale = float(np.abs(ref64).max())
    e_k = float(np.abs(np.asarray(got, np.float64) - ref64).max() / scale)
    e_r = float(np.abs(np.asarray(ref32, np.float64) - ref64).max() / scale)
    print(f"{label}: e_kernel {e_k:.3e} e_fp32ref {e_r:.3e} ratio {e_k / max(e_r, 1e-30):.2f}")
    assert e_k < 8 * e_r + 1e-7, (label, e_k, e_r)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---------------------------------------------------------------------------- levels and the class branch's reference
def _levels(rng, dtype, shapes, n, cb, cc, nc, pad=8, wscale=1.0):
    """cstride = cb + cc + pad > cb + cc; per-level weights."""
    lv = []
    for l, (h, w) in enumerate(shapes):
        lv.append(dict(feat=rng.standard_normal((n, h, w, cb + cc + pad)).astype(dtype), cb=cb, cc=cc, stride=float(8 << l),
                       wc=(rng.standard_normal((nc, cc)) * (wscale / np.sqrt(cc))).astype(F32), bc=(0.3 * rng.standard_normal(nc)).astype(F32),
                       wb=(rng.standard_normal((max(cb, 1), 64)) / np.sqrt(max(cb, 1))).astype(F32)[:cb], bb=rng.standard_normal(64).astype(F32)))
    return lv


def _begins(levels):
    return np.cumsum([0] + [lv["feat"].shape[1] * lv["feat"].shape[2] for lv in levels])


def _level_of(levels, a):
    return np.searchsorted(_begins(levels)[1:], a, side="right")


def _cls_scores(levels, prec):
    """[n, A, nc] sigmoid(wc . f + bc) in `prec`, from what the maps hold."""
    out = []
    for lv in levels:
        cb, cc = lv["cb"], lv["cc"]
        f = lv["feat"][..., cb:cb + cc].astype(prec)
        f = f.reshape(f.shape[0], -1, cc)
        z = f @ lv["wc"].astype(prec).T + lv["bc"].astype(prec)
        out.append(prec(1) / (prec(1) + np.exp(-z)))
    return np.concatenate(out, axis=1)


def _rows_of(lv, b):
    """Image b's map as [h * w, cstride] (a view)."""
    f = lv["feat"]
    return f[b].reshape(-1, f.shape[3])


def _score_margins(s64, conf):
    """The float64 scores decide: none within MARGIN of conf, and an anchor's two best classes MARGIN apart or exactly equal."""
    if np.abs(s64 - conf).min() <= MARGIN:
        return False
    if s64.shape[-1] > 1:
        top = np.sort(s64, axis=-1)[..., -2:]
        gap = top[..., 1] - top[..., 0]
        if ((gap <= MARGIN) & (gap != 0)).any():
            return False
    return True


def _conf_in_gap(best, lo=0.3, hi=0.5):
    """A float32 threshold in the widest gap between consecutive sorted best scores inside the [lo, hi] quantile range."""
    s = np.unique(best)
    i0, i1 = int(lo * len(s)), max(int(hi * len(s)), int(lo * len(s)) + 2)
    k = i0 + int(np.argmax(np.diff(s[i0:i1])))
    return float(F32((s[k] + s[k + 1]) / 2))


def _gate_expect(s64, conf, words):
    best_c = s64.argmax(-1)                          # first maximum: the lower class on a tie
    best = s64.max(-1)
    return best, best_c, (best > conf) & _bit(words, best_c)


def _gate_case(dtype, cc, nc, n=2):
    """Levels, conf and the subset mask of a gate case whose decisions float64 alone makes, with every coverage property the case is
    there for asserted on the CPU."""
    sub = None if nc == 1 else _words([2, 70] if nc == 80 else [1, 2])
    for attempt in range(500):
        rng = np.random.default_rng(_seed("gate", np.dtype(dtype).name, cc, nc, attempt))
        lv = _levels(rng, dtype, SHAPES, n, 16, cc, nc)
        for L in lv:
            if nc == 80:
                L["bc"][[0, 70]] += F32(1.5)
            if nc >= 3:                              # class 2 = class 0 bit for bit: a class tie wherever they are the best
                L["wc"][2] = L["wc"][0]
                L["bc"][2] = L["bc"][0]
        s64 = _cls_scores(lv, np.float64)
        b0 = _begins(lv)
        for l, L in enumerate(lv):                   # the level's best anchor copied to its first and last: bit-equal scores that pass
            for b in range(n):
                a = int(s64[b, b0[l]:b0[l + 1]].max(-1).argmax())
                r = _rows_of(L, b)
                r[0, 16:16 + cc] = r[a, 16:16 + cc]
                r[-1, 16:16 + cc] = r[a, 16:16 + cc]
        s64 = _cls_scores(lv, np.float64)
        conf = _conf_in_gap(s64.max(-1))
        if not _score_margins(s64, conf):
            continue
        best, best_c, keep = _gate_expect(s64, conf, FULL)
        ok = keep[:, EDGE_ANCHORS].all() and not keep.all()
        if nc >= 3:
            tie = keep & (best_c == 0) & (s64[..., 0] == s64[..., 2])
            _, _, keep_sub = _gate_expect(s64, conf, sub)
            ok = ok and tie.any() and (tie & ~keep_sub & (s64[..., 2] > conf)).any() and keep_sub.any()   # best class masked, a kept class clears conf
        if nc == 80:
            ok = ok and (keep & (best_c == 70)).any()                                                     # the second mask word keeps something
        if ok:
            return lv, conf, sub
    raise AssertionError("no seed gives a gate case with its margins")


def _check_gate(label, out, s64, s32, conf, words, cap):
    best, best_c, keep = _gate_expect(s64, conf, words)
    got, want, want32 = [], [], []
    for b in range(s64.shape[0]):
        exp = set(np.flatnonzero(keep[b]).tolist())
        assert out["count"][b] == len(exp), (label, b, out["count"][b], len(exp))        # the true number, also above cap
        m = min(cap, len(exp))
        a = out["anchor"][b, :m]
        assert len(set(a.tolist())) == m and set(a.tolist()) <= exp, (label, b)          # exactly m stored, each a passing anchor, none twice
        assert cap < len(exp) or set(a.tolist()) == exp
        assert (out["anchor"][b, m:] == -1).all() and (out["cls"][b, m:] == -1).all() and np.isnan(out["score"][b, m:]).all()
        np.testing.assert_array_equal(out["cls"][b, :m], best_c[b, a], err_msg=label)
        got.append(out["score"][b, :m]); want.append(best[b, a]); want32.append(s32[b].max(-1)[a])
    if sum(len(g) for g in got):
        _value_bar(label, np.concatenate(got), np.concatenate(want), np.concatenate(want32))


@pytest.mark.parametrize("nc", [1, 3, 5, 80])
@pytest.mark.parametrize("cc", [8, 64, 136])
@pytest.mark.parametrize("dtype", [F32, F16], ids=["f32", "f16"])
def test_gate(dtype, cc, nc):
    """One chunk, fewer chunks than lanes, a second pass of the 16-lane stride; a partial group of four classes; a class tie (the
    lower class wins); passing anchors on both sides of every anchor_begin; every class kept, then a subset with the second mask word."""
    from geotrax_amd import ops

    lv, conf, sub = _gate_case(dtype, cc, nc)
    s64, s32 = _cls_scores(lv, np.float64), _cls_scores(lv, F32)
    for words in [FULL] + ([sub] if sub else []):
        out = ops.head_gate(lv, nc, conf, 64, class_mask=words)
        _check_gate(f"gate {np.dtype(dtype).name} cc={cc} nc={nc} mask={'all' if words == FULL else 'subset'}", out, s64, s32, conf, words, 64)


@pytest.mark.parametrize("dtype", [F32, F16], ids=["f32", "f16"])
def test_gate_full_buffer_and_level_lists(dtype):
    """cap below the number that passes: count is the true number, exactly cap entries are stored, each a passing anchor, none twice;
    every stored index below lvl_cap is filed once, under its anchor's level."""
    from geotrax_amd import ops

    lv, conf, _ = _gate_case(dtype, 64, 5)
    s64, s32 = _cls_scores(lv, np.float64), _cls_scores(lv, F32)
    _, _, keep = _gate_expect(s64, conf, FULL)
    assert keep.sum(1).min() > 7
    for cap, lvl_cap in [(7, 5), (64, 64), (7, 9)]:
        out = ops.head_gate(lv, 5, conf, cap, lvl_cap=lvl_cap)
        _check_gate(f"gate cap={cap} lvl_cap={lvl_cap} {np.dtype(dtype).name}", out, s64, s32, conf, FULL, cap)
        for b in range(2):
            m = min(cap, int(out["count"][b]), lvl_cap)
            filed = []
            for l in range(4):
                k = int(out["lvl_count"][b, l])
                idx = out["lvl_list"][b, l, :k]
                assert l < 3 or k == 0
                assert (_level_of(lv, out["anchor"][b, idx]) == l).all(), (cap, lvl_cap, b, l)
                filed += idx.tolist()
            assert sorted(filed) == list(range(m)), (cap, lvl_cap, b, filed)


@pytest.mark.parametrize("dtype", [F32, F16], ids=["f32", "f16"])
def test_gate_score_exactly_on_conf(dtype):
    """Zero class weights and bias: every score is exactly 0.5. conf = 0.5 passes nothing (strict >), nextafter(0.5, 0) everything."""
    from geotrax_amd import ops

    lv = _levels(np.random.default_rng(1), dtype, SHAPES, 2, 16, 64, 3)
    for L in lv:
        L["wc"][:] = 0
        L["bc"][:] = 0
    out = ops.head_gate(lv, 3, 0.5, 64)
    assert (out["count"] == 0).all() and (out["anchor"] == -1).all()
    out = ops.head_gate(lv, 3, float(np.nextafter(F32(0.5), F32(0))), 64)
    assert (out["count"] == 51).all()
    for b in range(2):
        assert sorted(out["anchor"][b, :51].tolist()) == list(range(51))
        assert (out["score"][b, :51] == 0.5).all() and (out["cls"][b, :51] == 0).all()


# ---------------------------------------------------------------------------- DFL decode
def _boxes_ref(levels, b, anchors, prec):
    """xyxy in network pixels of image b's anchors, in `prec`, by head_boxes_kernel's recipe (softmax expectation per side,
    dist2bbox to xywh times the stride, xywh2xyxy)."""
    out = np.zeros((len(anchors), 4), prec)
    b0 = _begins(levels)
    lvl = _level_of(levels, anchors)
    bins = np.arange(16).astype(prec)
    for l, L in enumerate(levels):
        sel = np.flatnonzero(lvl == l)
        if not len(sel):
            continue
        la = anchors[sel] - b0[l]
        f = _rows_of(L, b)[la, :L["cb"]].astype(prec)
        z = (f @ L["wb"].astype(prec) + L["bb"].astype(prec)).reshape(-1, 4, 16)
        e = np.exp(z - z.max(-1, keepdims=True))
        d = (e * bins).sum(-1) / e.sum(-1)
        w = L["feat"].shape[2]
        ax, ay = (la % w).astype(prec) + prec(0.5), (la // w).astype(prec) + prec(0.5)
        x1, y1, x2, y2 = ax - d[:, 0], ay - d[:, 1], ax + d[:, 2], ay + d[:, 3]
        s = prec(L["stride"])
        cx, cy, bw, bh = (x1 + x2) * prec(0.5) * s, (y1 + y2) * prec(0.5) * s, (x2 - x1) * s, (y2 - y1) * s
        out[sel] = np.stack([cx - bw / prec(2), cy - bh / prec(2), cx + bw / prec(2), cy + bh / prec(2)], -1)
    return out


def _corner_anchors(levels):
    b0 = _begins(levels)
    out = []
    for l, L in enumerate(levels):
        h, w = L["feat"].shape[1:3]
        out += [b0[l], b0[l] + w - 1, b0[l] + (h - 1) * w, b0[l] + h * w - 1]
    return out


@pytest.mark.parametrize("cb", [16, 64, 72, 128])
@pytest.mark.parametrize("dtype", [F32, F16], ids=["f32", "f16"])
def test_boxes(dtype, cb):
    """Every anchor (the four corner cells of each level, both sides of each level boundary) and more candidates than the grid's 256
    waves; ordinary DFL logits, one bin per side at +80, and all logits equal (distance exactly 7.5); an image whose count exceeds
    cap (only cap decoded, nothing written past them), one with 5 candidates, and counts of 0."""
    from geotrax_amd import ops

    rng = np.random.default_rng(_seed("boxes", np.dtype(dtype).name, cb))
    cap = 300
    anchors = np.zeros((2, cap), np.int32)
    for b in range(2):
        anchors[b] = np.concatenate([rng.permutation(51), rng.integers(0, 51, cap - 51)])
    count = np.array([cap + 50, 5], np.int32)
    for kind in ["ordinary", "peak", "equal"]:
        lv = _levels(rng, dtype, SHAPES, 2, cb, 8, 1)
        assert set(_corner_anchors(lv)) <= set(anchors[0].tolist()) and set(EDGE_ANCHORS) <= set(anchors[0].tolist())
        for L in lv:
            if kind == "peak":
                for side, k in enumerate(rng.integers(0, 16, 4)):
                    L["bb"][side * 16 + k] = 80
            if kind == "equal":
                L["wb"][:] = 0
                L["bb"][:] = F32(0.3)
        box = ops.head_boxes(lv, count, anchors)
        assert np.isnan(box[1, 5:]).all() and not np.isnan(box[0]).any() and not np.isnan(box[1, :5]).any()
        got = np.concatenate([box[0], box[1, :5]])
        r64 = np.concatenate([_boxes_ref(lv, 0, anchors[0], np.float64), _boxes_ref(lv, 1, anchors[1, :5], np.float64)])
        r32 = np.concatenate([_boxes_ref(lv, 0, anchors[0], F32), _boxes_ref(lv, 1, anchors[1, :5], F32)])
        _value_bar(f"boxes {np.dtype(dtype).name} cb={cb} {kind}", got, r64, r32)
        if kind == "equal":
            np.testing.assert_array_equal(got, r64.astype(F32))          # anchor centre -/+ 7.5 cells, exact in every evaluation
    box = ops.head_boxes(lv, np.array([0, 3], np.int32), anchors)
    assert np.isnan(box[0]).all() and np.isnan(box[1, 3:]).all() and not np.isnan(box[1, :3]).any()
    box = ops.head_boxes(lv, np.array([0, 0], np.int32), anchors)
    assert np.isnan(box).all()


# ---------------------------------------------------------------------------- NMS
GEO_RECT = dict(src_hw=(1080, 1920), net_hw=(384, 640), gain=1.0 / 3.0)      # pady = 12, padx = 0
GEO_BIG = dict(src_hw=(2160, 3840), net_hw=(2176, 3840), gain=1.0)          # pady = round(8 - 0.1) = 8, padx = 0
GEO_HALF = dict(src_hw=(714, 1270), net_hw=(384, 640), gain=0.5)            # pady = round(13.5 - 0.1) = 13 (not 14), padx = round(2.5 - 0.1) = 2
SENT = -7.0


def _pads(geo):
    (sh, sw), (nh, nw), g = geo["src_hw"], geo["net_hw"], geo["gain"]
    return round((nw - sw * g) / 2 - 0.1), round((nh - sh * g) / 2 - 0.1)      # ultralytics scale_boxes


def _frame_rows(box, geo, prec):
    padx, pady = _pads(geo)
    g = prec(geo["gain"])
    out = (box.astype(prec) - np.array([padx, pady, padx, pady], prec)) / g
    out[:, [0, 2]] = np.clip(out[:, [0, 2]], 0, prec(geo["src_hw"][1]))
    out[:, [1, 3]] = np.clip(out[:, [1, 3]], 0, prec(geo["src_hw"][0]))
    return out


def _nms_ref(c, iou_thr, agnostic, max_nms=30000, margin=True):
    """Kept candidate slots of one image, in output order: float64 decisions on the boxes after the float32 class-offset add. Asserts
    that no pair's IoU lies within MARGIN of the threshold (margin=False: the two cases that sit on it by construction)."""
    thr = float(F32(iou_thr))
    order = np.lexsort((c["anchor"], -c["score"].astype(np.float64)))[:max_nms]        # score descending, then anchor ascending
    off = F32(0.0 if agnostic else 7680.0) * c["cls"].astype(F32)
    bx = (c["box"].astype(F32) + off[:, None]).astype(np.float64)[order]
    m = len(order)
    area = (bx[:, 2] - bx[:, 0]) * (bx[:, 3] - bx[:, 1])
    over = np.zeros((m, m), bool)
    closest = np.inf
    for r0 in range(0, m, 256):
        a = bx[r0:r0 + 256, None, :]
        iw = np.minimum(a[..., 2], bx[None, :, 2]) - np.maximum(a[..., 0], bx[None, :, 0])
        ih = np.minimum(a[..., 3], bx[None, :, 3]) - np.maximum(a[..., 1], bx[None, :, 1])
        hit = (iw > 0) & (ih > 0)                    # degenerate and disjoint boxes: IoU 0 (or 0 / 0), never above a threshold
        inter = np.where(hit, iw * ih, 0.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            iou = np.where(hit, inter / (area[r0:r0 + 256, None] + area[None, :] - inter), 0.0)
        iou[np.arange(len(a)), np.arange(r0, r0 + len(a))] = 0.0
        closest = min(closest, float(np.abs(iou[hit] - thr).min()) if hit.any() else np.inf)
        over[r0:r0 + 256] = iou > thr
    if margin:
        assert closest > MARGIN and thr > MARGIN, f"a pair IoU lies within {MARGIN} of iou_thr"
    alive = np.ones(m, bool)
    kept = []
    for i in range(m):
        if alive[i]:
            kept.append(i)
            alive &= ~over[i]
    return order[kept]


def _pack(images):
    """Per-image candidate dicts (score, anchor, cls, box of their own length) -> the hook's [n, cap] arrays."""
    n, cap = len(images), max(max(len(c["score"]) for c in images), 1)
    out = dict(count=np.array([len(c["score"]) for c in images], np.int32), score=np.full((n, cap), 0.5, F32), anchor=np.zeros((n, cap), np.int32),
               cls=np.zeros((n, cap), np.int32), box=np.zeros((n, cap, 4), F32))
    for b, c in enumerate(images):
        k = len(c["score"])
        for key in ("score", "anchor", "cls", "box"):
            out[key][b, :k] = c[key]
    return out


def _run_nms(label, images, kept, which, max_det, *, iou_thr, agnostic=False, max_nms=30000, nms_cap=None, geo=GEO_BIG):
    """One launch against the reference's kept lists; returns the rows. Images the chosen path leaves to the other one must come
    back untouched (which = 2) or with out_n = 0 (which = 1)."""
    from geotrax_amd import ops

    p = _pack(images)
    n = len(images)
    if nms_cap is None:
        nms_cap = max(64, -(-int(p["count"].max()) // 64) * 64)
    rows, on, oa = ops.nms(p["count"], p["score"], p["anchor"], p["cls"], p["box"], iou_thr=iou_thr, max_det=max_det, agnostic=agnostic, max_nms=max_nms,
                           nms_cap=nms_cap, which=which, out_rows=np.full((n, max_det, 6), SENT, F32), **geo)
    got, want, want32 = [], [], []
    for b, c in enumerate(images):
        small = len(c["score"]) <= 4096 and max_det <= 2048
        if (which == 1 and not small) or (which == 2 and small):
            assert on[b] == (0 if which == 1 else -1) and (rows[b] == SENT).all() and (oa[b] == -1).all(), (label, b, on[b])
            continue
        k = kept[b][:max_det]
        assert on[b] == len(k), (label, b, int(on[b]), len(k))
        np.testing.assert_array_equal(oa[b, :len(k)], c["anchor"][k], err_msg=f"{label}: image {b}, kept anchors in output order")
        assert (oa[b, len(k):] == -1).all() and (rows[b, len(k):] == SENT).all(), (label, b)          # rows past out_n keep what they held
        np.testing.assert_array_equal(_bits(rows[b, :len(k), 4]), _bits(c["score"][k]), err_msg=label)
        np.testing.assert_array_equal(rows[b, :len(k), 5], c["cls"][k].astype(F32), err_msg=label)
        got.append(rows[b, :len(k), :4]); want.append(_frame_rows(c["box"][k], geo, np.float64)); want32.append(_frame_rows(c["box"][k], geo, F32))
    if sum(len(g) for g in got):
        _value_bar(f"{label} which={which} max_det={max_det}", np.concatenate(got), np.concatenate(want), np.concatenate(want32))
    return rows, on


def _both_paths(label, images, *, iou_thr, agnostic=False, max_det=300, geo=GEO_BIG, margin=True):
    """The single-workgroup kernel (which = 1) and the general kernels, forced with max_det = 2049 (which = 2), against the same
    reference; the two paths' rows must be identical."""
    kept = [_nms_ref(c, iou_thr, agnostic, margin=margin) for c in images]
    r1, n1 = _run_nms(label, images, kept, 1, max_det, iou_thr=iou_thr, agnostic=agnostic, geo=geo)
    r2, n2 = _run_nms(label, images, kept, 2, 2049, iou_thr=iou_thr, agnostic=agnostic, geo=geo)
    for b in range(len(images)):                     # each path cuts at its own max_det; what both hold is the same bits
        k = min(len(kept[b]), max_det, 2049)
        assert min(n1[b], n2[b]) == k, (label, b, n1[b], n2[b])
        np.testing.assert_array_equal(_bits(r1[b, :k]), _bits(r2[b, :k]), err_msg=f"{label}: the two paths' rows differ")
    return kept


def _grid(rng, cnt, nclass=3, cell=40, cols=96, rows=54, anchors=60000):
    """cnt disjoint boxes, one per 40-pixel cell of a 3840 x 2160 network image; slots, anchors and scores in unrelated orders."""
    cells = rng.permutation(cols * rows)[:cnt]
    x0 = (cells % cols) * cell + rng.uniform(1, 8, cnt)
    y0 = (cells // cols) * cell + rng.uniform(1, 8, cnt)
    w, h = rng.uniform(10, 30, cnt), rng.uniform(10, 30, cnt)
    return dict(score=rng.uniform(0.05, 0.95, cnt).astype(F32), anchor=rng.permutation(anchors)[:cnt].astype(np.int32),
                cls=rng.integers(0, nclass, cnt).astype(np.int32), box=np.stack([x0, y0, x0 + w, y0 + h], -1).astype(F32))


def _cover(c, rng, victim, killer):
    """Move candidate `victim` onto candidate `killer` (same class, IoU around 0.8)."""
    c["box"][victim] = c["box"][killer] + rng.uniform(-1.5, 1.5, (len(np.atleast_1d(victim)), 1)).astype(F32)
    c["cls"][victim] = c["cls"][killer]


def _ranked(c):
    return np.lexsort((c["anchor"], -c["score"].astype(np.float64)))


def _seeded(label, build, **kw):
    """build(rng) -> images, reseeded until the reference's IoU margin holds."""
    for attempt in range(200):
        images = build(np.random.default_rng(_seed(label, attempt)))
        try:
            for c in images:
                _nms_ref(c, kw["iou_thr"], kw.get("agnostic", False), kw.get("max_nms", 30000))
        except AssertionError:
            continue
        return images
    raise AssertionError(f"{label}: no seed gives the IoU margin")


def test_nms_order_and_ties():
    """Slot order shuffled against anchor order; the order is score descending, then anchor ascending: groups of bit-equal scores on
    disjoint boxes, and bit-equal scores on overlapping boxes, where the lower anchor survives."""
    def build(rng):
        c = _grid(rng, 150)
        c["score"][10:18] = c["score"][10]           # a group of eight, a pair, a group of three: disjoint boxes, order by anchor
        c["score"][40:42] = c["score"][40]
        c["score"][60:63] = c["score"][60]
        for v, k in [(100, 101), (102, 103), (104, 105), (106, 107)]:      # equal scores on overlapping boxes, either slot order
            c["score"][v] = c["score"][k]
            _cover(c, rng, v, k)
        c["anchor"][100], c["anchor"][101] = 7, 9    # the lower anchor in the lower slot, and in the higher one
        c["anchor"][102], c["anchor"][103] = 59999 + 2, 59999 + 1
        return [c]

    images = _seeded("ties", build, iou_thr=0.5)
    kept = _both_paths("nms ties", images, iou_thr=0.5)
    k = set(kept[0].tolist())
    assert 100 in k and 101 not in k and 103 in k and 102 not in k and len(k) == 146


def _chain(n_box, rng):
    """Box i overlaps only boxes i - 1 and i + 1 (IoU exactly 1/3), scores descend along the chain: the alternate ones survive."""
    i = np.arange(n_box)
    box = np.stack([10.0 * i, np.full(n_box, 100.0), 10.0 * i + 20, np.full(n_box, 130.0)], -1).astype(F32)
    c = dict(score=(0.95 - 0.004 * i).astype(F32), anchor=rng.permutation(5000)[:n_box].astype(np.int32), cls=np.ones(n_box, np.int32), box=box)
    p = rng.permutation(n_box)                       # slots in no order
    return {k: v[p] for k, v in c.items()}, p


def test_nms_chain_across_blocks():
    """A chain of 200: it crosses three 64-box block boundaries, and the longest chain inside a block is 64, the fixpoint's last round."""
    rng = np.random.default_rng(5)
    c, p = _chain(200, rng)
    kept = _both_paths("nms chain", [c], iou_thr=0.3)
    assert sorted(p[kept[0]].tolist()) == list(range(0, 200, 2))


def test_nms_pipeline_wrap():
    """1 100 candidates: block 16 goes back to wave 0 of the resolve pipeline; a box kept in block 0 suppresses one in block 17; a
    hundred more pairs over every distance."""
    def build(rng):
        c = _grid(rng, 1100)
        r = _ranked(c)
        _cover(c, rng, r[1090:1091], r[5:6])
        lo = rng.permutation(np.arange(300, 1088))[:100]
        hi = rng.integers(0, 300, 100)
        _cover(c, rng, r[lo], r[hi])
        return [c]

    images = _seeded("wrap", build, iou_thr=0.5)
    r = _ranked(images[0])
    kept = _both_paths("nms wrap", images, iou_thr=0.5, max_det=2048)
    assert r[5] in kept[0] and r[1090] not in kept[0] and len(kept[0]) < 1050


@pytest.mark.parametrize("max_det", [1, 64, 100])
def test_nms_max_det_cut(max_det):
    """The cut inside a block, exactly at 64 kept (the single-workgroup kernel's early exit) and at 1: rows past out_n keep what
    out_rows held, out_anchor matches the rows. The general kernels take the same cuts on 4 200 candidates."""
    rng = np.random.default_rng(_seed("cut", max_det))
    c = _grid(rng, 200)
    kept = [_nms_ref(c, 0.5, False)]
    assert len(kept[0]) == 200
    _run_nms("nms cut", [c], kept, 1, max_det, iou_thr=0.5)
    c = _grid(rng, 4200)
    kept = [_nms_ref(c, 0.5, False)]
    _run_nms("nms cut 4200", [c], kept, 2, max_det, iou_thr=0.5)


def test_nms_classes_and_degenerate_boxes():
    """Non-agnostic: two identical boxes of different class both survive, of the same class one does; agnostic: one of either pair.
    Degenerate boxes (zero area, x2 < x1, both) lying on ordinary ones suppress nothing and are not suppressed; disjoint boxes neither."""
    box = np.array([[100, 100, 140, 150]] * 2 + [[300, 100, 340, 150]] * 2 + [[500, 100, 560, 160], [520, 120, 520, 140], [540, 150, 510, 110], [530, 110, 550, 110],
                    [505, 105, 555, 155], [700, 100, 740, 140], [740, 100, 780, 140]], F32)
    c = dict(score=np.array([0.9, 0.8, 0.7, 0.6, 0.5, 0.95, 0.94, 0.93, 0.4, 0.3, 0.2], F32), anchor=np.arange(11, dtype=np.int32)[::-1].copy(),
             cls=np.array([0, 1, 2, 2, 0, 0, 0, 0, 0, 1, 1], np.int32), box=box)
    kept = _both_paths("nms classes", [c], iou_thr=0.5)
    assert sorted(kept[0].tolist()) == [0, 1, 2, 4, 5, 6, 7, 9, 10]
    kept = _both_paths("nms agnostic", [c], iou_thr=0.5, agnostic=True)
    assert sorted(kept[0].tolist()) == [0, 2, 4, 5, 6, 7, 9, 10]


def test_nms_iou_exactly_on_threshold():
    """Integer boxes: intersection 100, union 200. At iou_thr = 0.5 the pair survives (strict >); at nextafter(0.5, 0) the lower
    score goes. These two sit on the threshold by construction: the only cases without the IoU margin."""
    c = dict(score=np.array([0.9, 0.8, 0.7], F32), anchor=np.array([3, 2, 1], np.int32), cls=np.zeros(3, np.int32),
             box=np.array([[0, 0, 20, 10], [0, 0, 10, 10], [100, 100, 120, 120]], F32))
    kept = _both_paths("nms iou == thr", [c], iou_thr=0.5, margin=False)
    assert kept[0].tolist() == [0, 1, 2]
    kept = _both_paths("nms iou > thr", [c], iou_thr=float(np.nextafter(F32(0.5), F32(0))), margin=False)
    assert kept[0].tolist() == [0, 2]


@pytest.mark.parametrize("geo", [GEO_RECT, GEO_HALF], ids=["rect", "half"])
def test_nms_unletterbox_and_clip(geo):
    """Boxes partly and wholly outside the padded area, padx != pady, and a pad whose - 0.1 decides the rounding."""
    rng = np.random.default_rng(_seed("clip"))
    assert _pads(geo)[0] != _pads(geo)[1] and (geo is not GEO_HALF or _pads(geo) == (2, 13))
    c = _grid(rng, 120, cell=40, cols=16, rows=9)
    c["box"][:8] = np.array([[-30, -20, 25, 30], [600, 350, 700, 420], [-50, 100, -10, 140], [650, 100, 690, 140], [100, -60, 140, -10], [100, 390, 140, 450],
                             [0, 0, 640, 11], [300, 372, 340, 384]], F32)
    c["cls"][:8] = 5                                 # their own class: the rest keep their disjoint cells
    images = [c]
    _nms_ref(c, 0.5, False)
    _both_paths("nms clip", images, iou_thr=0.5, geo=geo)


@pytest.mark.parametrize("cnt", [0, 1, 64, 65, 4096])
def test_nms_counts(cnt):
    def build(rng):
        c = _grid(rng, cnt)
        if cnt >= 64:
            r = _ranked(c)
            _cover(c, rng, r[cnt - 1:cnt], r[0:1])
            _cover(c, rng, r[40:41], r[20:21])
        return [c]

    images = _seeded(("counts", cnt), build, iou_thr=0.6)
    kept = _both_paths(f"nms count={cnt}", images, iou_thr=0.6, max_det=2048)
    assert len(kept[0]) == (cnt - 2 if cnt >= 64 else cnt)


def test_nms_beyond_the_small_path():
    """4 097 candidates with which = 0: the general kernels take the image (nms_cap = 4160), max_nms = 4000 truncates by score; which
    = 1 alone leaves out_n = 0. Then n = 2 with images of 100 and 4 097 candidates: each path steps aside for the other's image."""
    def build(rng):
        big = _grid(rng, 4097)
        r = _ranked(big)
        _cover(big, rng, r[4050:4051], r[3:4])         # past max_nms = 4000: never a row, truncated or not
        _cover(big, rng, r[3990:3991], r[64:65])
        small = _grid(rng, 100)
        rs = _ranked(small)
        _cover(small, rng, rs[70:71], rs[2:3])
        return [small, big]

    images = _seeded("beyond", build, iou_thr=0.5)
    small, big = images
    kept = [_nms_ref(big, 0.5, False, max_nms=4000)]
    assert len(kept[0]) == 3999
    _run_nms("nms 4097", [big], kept, 0, 2048, iou_thr=0.5, max_nms=4000, nms_cap=4160)
    _run_nms("nms 4097", [big], kept, 0, 300, iou_thr=0.5, max_nms=4000, nms_cap=4160)
    _run_nms("nms 4097", [big], kept, 1, 300, iou_thr=0.5, max_nms=4000, nms_cap=4160)
    kept = [_nms_ref(small, 0.5, False), _nms_ref(big, 0.5, False)]
    assert len(kept[0]) == 99 and len(kept[1]) == 4095
    _run_nms("nms 100 + 4097", images, kept, 0, 300, iou_thr=0.5, nms_cap=4160)
    _run_nms("nms 100 + 4097", images, kept, 1, 300, iou_thr=0.5, nms_cap=4160)
    _run_nms("nms 100 + 4097", images, kept, 2, 300, iou_thr=0.5, nms_cap=4160)


def test_nms_anchor_width():
    """Anchors on both sides of 2^19 and up to 2^20 - 1 (a P2 model at a 4K input has 693 600): bit-equal scores and scores that
    differ in the last mantissa bits only, on disjoint boxes and on overlapping ones. Both paths must give the reference's order."""
    rng = np.random.default_rng(11)
    c = _grid(rng, 40)
    c["anchor"] = (2000 + rng.permutation(40)).astype(np.int32)
    c["anchor"][:12] = [700000, 524288, 524287, 5, 1048575, 524289, 262144, 786432, 600000, 524286, 1, 1000000]
    s = F32(0.625)
    c["score"][:6] = s                               # six bit-equal scores: the order is the anchors'
    c["score"][6:12] = (s.view(np.uint32) + np.array([1, 2, 3, 1, 2, 3], np.uint32)).view(F32)   # last bits only, with ties among them
    c["score"][20:22] = F32(0.7)                     # equal scores on one box: 524290 must survive 700001
    c["anchor"][20:22] = [700001, 524290]
    _cover(c, rng, 20, 21)
    c["score"][22:24] = F32(0.71)
    c["anchor"][22:24] = [524285, 524291]
    _cover(c, rng, 23, 22)
    assert len(set(c["anchor"].tolist())) == 40
    kept = _both_paths("nms anchor width", [c], iou_thr=0.5)
    k = kept[0].tolist()
    assert 21 in k and 20 not in k and 22 in k and 23 not in k
    tied = [i for i in k if i < 6]
    assert c["anchor"][tied].tolist() == sorted(c["anchor"][:6].tolist())
    print("nms anchor width: reference anchor order", c["anchor"][kept[0]][:16].tolist())


# ---------------------------------------------------------------------------- the YOLOv10 cut
V10_SHAPES = [(40, 40), (20, 20), (10, 10)]          # 2 100 anchors: the 1024-thread stride loops run more than once


def _order(score, index):
    """Positions sorted by score descending (bit patterns: the scores are positive), then index ascending."""
    return np.lexsort((index, -_bits(score).astype(np.int64)))


def _v10_levels(dtype, nc, attempt, stress=False):
    rng = np.random.default_rng(_seed("v10", np.dtype(dtype).name, nc, attempt, stress))
    lv = _levels(rng, dtype, V10_SHAPES, 1, 8, 16, nc, wscale=1e-7 if stress else 1.0)
    for L in lv:
        if stress:
            L["bc"][:] = 0                           # every logit within 1e-6 of 0: every score within a few ulps of 0.5
        elif nc >= 3:
            L["bc"][[0, 1, 2]] += F32(2.0)           # classes 0 and 1 are one weight row, class 2 is its own: pairs and singles at the top
            L["wc"][1] = L["wc"][0]
            L["bc"][1] = L["bc"][0]
    return lv


def _v10_case(dtype, nc, cnt):
    """Levels and conf so that exactly cnt anchors pass the gate by float64's decision; beyond 300, a copied feature vector puts a
    bit-equal pair of best scores across the 300th place of stage 1; with classes to choose from and every anchor a candidate, the
    300th place of stage 2 falls inside a pair of bit-equal entries."""
    for attempt in range(500):
        lv = _v10_levels(dtype, nc, attempt)
        s64 = _cls_scores(lv, np.float64)[0]
        if cnt > 300:                                # the 300th anchor's features onto the last-ranked anchor of its level
            best = s64.max(-1)
            r = np.lexsort((np.arange(2100), -best))
            a = r[299]
            l = int(_level_of(lv, a))
            b0 = _begins(lv)
            same = [x for x in r[::-1] if b0[l] <= x < b0[l + 1] and x != a]
            rows = _rows_of(lv[l], 0)
            rows[same[0] - b0[l], 8:24] = rows[a - b0[l], 8:24]
            s64 = _cls_scores(lv, np.float64)[0]
        best = s64.max(-1)
        srt = np.sort(best)[::-1]
        if cnt == 0:
            conf = float(F32(min(srt[0] + 0.01, 0.9999)))
        elif cnt == 2100:
            conf = 1e-4
        else:
            conf = float(F32((srt[cnt - 1] + srt[cnt]) / 2))
        if not _score_margins(s64[None], conf) or (best > conf).sum() != cnt:
            continue
        if cnt > 300:
            r = np.lexsort((np.arange(2100), -best))
            if best[r[299]] != best[r[300]]:
                continue
        if cnt == 2100 and nc >= 3:
            top = np.flatnonzero(np.isin(np.arange(2100), r[:300]))
            e = s64[top].ravel()
            eo = np.lexsort((np.arange(e.size), -e))
            if e[eo[299]] != e[eo[300]]:
                continue
        return lv, conf
    raise AssertionError("no seed gives a v10 case with its margins")


def _check_v10(label, lv, nc, conf, want_count=None, gate_decides=True):
    from geotrax_amd import ops

    s64, s32 = _cls_scores(lv, np.float64)[0], _cls_scores(lv, F32)[0]
    g = ops.head_gate(lv, nc, conf, 2100)
    cnt = int(g["count"][0])
    if gate_decides:
        _check_gate(label + " gate", g, s64[None], s32[None], conf, FULL, 2100)
    else:                                            # the stress case: every anchor passes, which class is best is the rounding's
        assert sorted(g["anchor"][0, :cnt].tolist()) == list(range(2100))
    assert want_count is None or cnt == want_count
    ga, gs = g["anchor"][0, :cnt], g["score"][0, :cnt]
    out = ops.v10_select(lv, nc, conf, g["count"], g["score"], g["anchor"], sel_cap=304, lvl_cap=304)
    # stage 1 on the gate's own scores: the 300 best, ties to the lower anchor
    K = min(cnt, 300)
    s1 = _order(gs, ga)[:K]
    rows_a = out["score_anchor"][0]
    assert (rows_a[K:] == -1).all() and np.isnan(out["scores"][0, K:]).all()
    assert sorted(rows_a[:K].tolist()) == sorted(ga[s1].tolist()), f"{label}: stage 1 kept other anchors"
    kept = int(out["count"][0])
    if K == 0:
        assert kept == 0 and (out["anchor"][0] == -1).all()
        return out
    sc = out["scores"][0, :K]
    _value_bar(label + " scores", sc, s64[rows_a[:K]], s32[rows_a[:K]])
    gate_score = dict(zip(ga.tolist(), _bits(gs).tolist()))
    np.testing.assert_array_equal(_bits(sc.max(-1)), np.array([gate_score[a] for a in rows_a[:K].tolist()], np.uint32),
                                  err_msg=f"{label}: a row's maximum is not the gate's score of that anchor, bit for bit")
    # stage 2 on the kernel's own rows: the 300 best entries above conf, ties to the lower flat index anchor * nc + class
    flat = (rows_a[:K, None].astype(np.int64) * nc + np.arange(nc)[None, :]).ravel()
    e = sc.ravel()
    ok = np.flatnonzero(e > F32(conf))
    o = ok[_order(e[ok], flat[ok])][:300]
    assert kept == len(o), (label, kept, len(o))
    np.testing.assert_array_equal(_bits(out["score"][0, :kept]), _bits(e[o]), err_msg=f"{label}: selected scores, in order")
    np.testing.assert_array_equal(out["anchor"][0, :kept], flat[o] // nc, err_msg=f"{label}: selected anchors, in order")
    np.testing.assert_array_equal(out["cls"][0, :kept], flat[o] % nc, err_msg=f"{label}: selected classes, in order")
    assert (out["anchor"][0, kept:] == -1).all() and (out["cls"][0, kept:] == -1).all() and np.isnan(out["score"][0, kept:]).all()
    filed = []
    for l in range(4):
        k = int(out["lvl_count"][0, l])
        idx = out["lvl_list"][0, l, :k]
        assert (_level_of(lv, out["anchor"][0, idx]) == l).all(), (label, l)
        filed += idx.tolist()
    assert sorted(filed) == list(range(kept)), label
    if len(ok) > 300:
        r = ok[_order(e[ok], flat[ok])]
        print(f"{label}: stage 2 cut between bit-equal entries: {bool(_bits(e[r[299]]) == _bits(e[r[300]]))}")
    return out


@pytest.mark.parametrize("cnt", [0, 299, 300, 301, 2100])
@pytest.mark.parametrize("nc", [1, 3, 80])
@pytest.mark.parametrize("dtype", [F32, F16], ids=["f32", "f16"])
def test_v10_select(dtype, nc, cnt):
    lv, conf = _v10_case(dtype, nc, cnt)
    _check_v10(f"v10 {np.dtype(dtype).name} nc={nc} cnt={cnt}", lv, nc, conf, cnt)


@pytest.mark.parametrize("nc", [3, 80])
@pytest.mark.parametrize("dtype", [F32, F16], ids=["f32", "f16"])
def test_v10_select_radix_stress(dtype, nc):
    """Every logit within 1e-6 of 0, so every score sits within a few ulps of 0.5: many exact ties, and distinct keys that differ only
    in the last byte of the score or only in the index half."""
    lv = _v10_levels(dtype, nc, 0, stress=True)
    z = [np.abs(_rows_of(L, 0)[:, 8:24].astype(np.float64) @ L["wc"].astype(np.float64).T).max() for L in lv]
    assert max(z) < 1e-6
    assert np.abs(_cls_scores(lv, np.float64) - 0.25).min() > MARGIN
    out = _check_v10(f"v10 stress {np.dtype(dtype).name} nc={nc}", lv, nc, 0.25, 2100, gate_decides=False)
    vals = np.unique(_bits(out["scores"][0]))
    print(f"v10 stress: {len(vals)} distinct score bit patterns")
    assert 2 <= len(vals) <= 64 and int(vals.max() - vals.min()) < 256


@pytest.mark.parametrize("geo", [GEO_RECT, GEO_HALF], ids=["rect", "half"])
@pytest.mark.parametrize("max_det", [10, 300])
def test_v10_rows(geo, max_det):
    """`classes` in the second mask word, the max_det cut (the first ten in score order), out_anchor, untouched rows past out_n, boxes
    outside the padded area; n = 2 with a short second image."""
    from geotrax_amd import ops

    rng = np.random.default_rng(_seed("v10rows"))
    n, cap = 2, 304
    count = np.array([300, 37], np.int32)
    score = np.sort(rng.uniform(0.3, 0.9, (n, cap)).astype(F32), axis=1)[:, ::-1].copy()
    anchor = rng.integers(0, 2100, (n, cap)).astype(np.int32)
    cls = rng.choice([2, 70, 5, 64, 127, 63], (n, cap)).astype(np.int32)
    box = np.sort(rng.uniform(-60, 700, (n, cap, 2, 2)), axis=2).reshape(n, cap, 4).astype(F32)      # two corners, sorted: x1 y1 x2 y2
    words = _words([2, 70])
    rows, on, oa = ops.v10_rows(count, score, anchor, cls, box, max_det=max_det, class_mask=words, out_rows=np.full((n, max_det, 6), SENT, F32), **geo)
    got, want, want32 = [], [], []
    for b in range(n):
        k = np.flatnonzero(_bit(words, cls[b, :count[b]]))[:max_det]
        assert len(k) > 0 and on[b] == len(k), (b, int(on[b]), len(k))
        np.testing.assert_array_equal(oa[b, :len(k)], anchor[b, k])
        assert (oa[b, len(k):] == -1).all() and (rows[b, len(k):] == SENT).all()
        np.testing.assert_array_equal(_bits(rows[b, :len(k), 4]), _bits(score[b, k]))
        np.testing.assert_array_equal(rows[b, :len(k), 5], cls[b, k].astype(F32))
        got.append(rows[b, :len(k), :4]); want.append(_frame_rows(box[b, k], geo, np.float64)); want32.append(_frame_rows(box[b, k], geo, F32))
    _value_bar(f"v10 rows max_det={max_det}", np.concatenate(got), np.concatenate(want), np.concatenate(want32))
    rows, on, oa = ops.v10_rows(np.zeros(n, np.int32), score, anchor, cls, box, max_det=max_det, out_rows=np.full((n, max_det, 6), SENT, F32), **geo)
    assert (on == 0).all() and (rows == SENT).all() and (oa == -1).all()


# ---------------------------------------------------------------------------- appearance vectors
def _pairs(a):
    """What the pair format keeps of an fp32 array: hi + lo, as float64 (tests/test_conv_k32s2_gpu.py)."""
    hi = a.astype(F16).astype(F32)
    return hi.astype(np.float64) + (a - hi).astype(F16).astype(np.float64)


@pytest.mark.parametrize("dim", [32, 160])
@pytest.mark.parametrize("fmt", ["f16", "f32", "f32s"])
def test_obj_feats(fmt, dim):
    """Levels of dim, 2 dim and 4 dim channels from a channel offset of 4 (in the pair format, groups on both sides of every 8-group);
    dim = 160 exceeds the 128 threads; kept anchors on both sides of each level boundary; out_n < max_det, the other rows untouched."""
    from geotrax_amd import ops

    rng = np.random.default_rng(_seed("feats", fmt, dim))
    n, max_det, coff = 2, 12, 4
    cs = [dim, 2 * dim, 4 * dim]
    maps = [rng.standard_normal((n, h, w, coff + c + 4)).astype(F16 if fmt == "f16" else F32) for (h, w), c in zip(SHAPES, cs)]
    out_n = np.array([9, 6], np.int32)
    out_anchor = np.full((n, max_det), -1, np.int32)
    out_anchor[0, :9] = EDGE_ANCHORS + [17, 40, 48]
    out_anchor[1, :6] = EDGE_ANCHORS[::-1]
    before = rng.standard_normal((n, max_det, dim)).astype(F32)
    got = ops.obj_feats(maps, cs, dim, out_n, out_anchor, coff=coff, split=fmt == "f32s", out=before)
    b0 = np.cumsum([0] + [h * w for h, w in SHAPES])
    g_all, w64, w32 = [], [], []
    for b in range(n):
        np.testing.assert_array_equal(got[b, out_n[b]:], before[b, out_n[b]:])
        for slot in range(out_n[b]):
            a = int(out_anchor[b, slot])
            l = int(np.searchsorted(b0[1:], a, side="right"))
            v = maps[l][b].reshape(-1, maps[l].shape[3])[a - b0[l], coff:coff + cs[l]]
            held = _pairs(v) if fmt == "f32s" else v.astype(np.float64)
            g = cs[l] // dim
            w64.append(held.reshape(dim, g).mean(1))
            acc = np.zeros(dim, F32)
            for j in range(g):
                acc = acc + held.astype(F32).reshape(dim, g)[:, j]
            w32.append(acc / F32(g))
            g_all.append(got[b, slot])
    _value_bar(f"obj_feats {fmt} dim={dim}", np.stack(g_all), np.stack(w64), np.stack(w32))
