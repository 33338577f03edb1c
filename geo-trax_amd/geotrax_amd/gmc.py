"""Global motion compensation object over the C ABI (gtx_gmc_*), with ultralytics' GMC interface.

Reference behaviour replaced: ultralytics.trackers.utils.gmc.GMC(method='sparseOptFlow', downscale=2)
as BOTSORT.update calls it once per frame inside model.track(..., persist=True)
(geotrax/extract.py:153, tracker block geotrax/cfg/default.yaml:362-374).
"""
from __future__ import annotations

import collections
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, ptr


class GMC:
    wants_frames = False             # works on the detector's half-resolution gray image (EccGMC: on the BGR frames)

    def __init__(self, frame_hw: tuple[int, int], method: str = "sparseOptFlow", downscale: int = 2, seed: int = 0,
                 ctx: _lib.Context | None = None):
        if method in (None, "none", "None"):
            raise ValueError("GMC(method='none'): do not create the object, pass no warp to the tracker")
        if method in ("orb", "sift"):
            raise ValueError(f"GMC(method='{method}'): use gmc.make_gmc (FeatureGMC)")
        if method != "sparseOptFlow":
            raise ValueError(f"GMC(method='{method}'): use gmc.make_gmc ('sparseOptFlow', 'orb', 'sift' and 'ecc' are implemented)")
        if downscale != 2:
            raise NotImplementedError("only downscale=2 (ultralytics' default) is implemented")
        self.ctx = ctx or _lib.default_context()
        h = C.c_void_p()
        check(self.ctx.lib.gtx_gmc_create(self.ctx.handle, int(frame_hw[0]), int(frame_hw[1]), seed, C.byref(h)))
        self.handle = h
        self.frame_hw = (int(frame_hw[0]), int(frame_hw[1]))
        self.stats = np.zeros(3, np.int32)
        self.valid = False

    def close(self):
        if getattr(self, "handle", None):
            self.ctx.lib.gtx_gmc_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset_params(self):                                 # ultralytics' name
        check(self.ctx.lib.gtx_gmc_reset(self.handle))

    def apply(self, raw_frame: np.ndarray, detections=None) -> np.ndarray:
        """2x3 float64 warp previous -> current frame (identity for the first frame)."""
        f = np.ascontiguousarray(raw_frame, np.uint8)
        A, valid = np.zeros(6, np.float64), C.c_int()
        check(self.ctx.lib.gtx_gmc_apply(self.handle, ptr(f), f.shape[0], f.shape[1], ptr(A), C.byref(valid), ptr(self.stats)))
        self.valid = bool(valid.value)
        return A.reshape(2, 3)

    def submit_gray_dev(self, gray_dptr: int, gh: int, gw: int) -> None:
        check(self.ctx.lib.gtx_gmc_submit_gray_dev(self.handle, C.c_void_p(gray_dptr), gh, gw))

    def submit_frame_dev(self, frame_dptr: int, h: int, w: int, restart: bool = False) -> None:
        """A BGR frame in HBM; restart=True opens a new sequence with it (identity warp, next frame is compared with it)."""
        check(self.ctx.lib.gtx_gmc_submit_frame_dev(self.handle, C.c_void_p(frame_dptr), h, w, int(restart)))

    def reset_sequence(self) -> None:
        """The next submitted frame opens a new sequence (identity warp), with frames still in flight: only the
        submitting side's state changes. reset_params() is the blocking variant used between clips."""
        check(self.ctx.lib.gtx_gmc_restart(self.handle))

    def collect(self) -> np.ndarray:
        A, valid = np.zeros(6, np.float64), C.c_int()
        check(self.ctx.lib.gtx_gmc_collect(self.handle, ptr(A), C.byref(valid), ptr(self.stats)))
        self.valid = bool(valid.value)
        return A.reshape(2, 3)

    def points(self, which: int):
        n = C.c_int()
        xy, st = np.zeros((1024, 2), np.float32), np.zeros(1024, np.int32)
        check(self.ctx.lib.gtx_gmc_points(self.handle, which, 1024, C.byref(n), ptr(xy), ptr(st)))
        return xy[:n.value].copy(), st[:n.value].astype(bool)

    def counts(self) -> dict:
        """The corner step's record of the last submitted frame: dict(found, stored, gathered, passes) (gtx_gmc_counts)."""
        c = np.zeros(4, np.int32)
        check(self.ctx.lib.gtx_gmc_counts(self.handle, ptr(c)))
        return dict(zip(("found", "stored", "gathered", "passes"), (int(v) for v in c)))


def estimate_affine_partial(p_xy: np.ndarray, q_xy: np.ndarray, seed: int = 0):
    """cv2.estimateAffinePartial2D(p, q, RANSAC) stand-in (gtx_op_estimate_affine_partial, host C++): 2x3 float64 or None."""
    p = np.ascontiguousarray(p_xy, np.float32).reshape(-1, 2)
    q = np.ascontiguousarray(q_xy, np.float32).reshape(-1, 2)
    A, valid, inl = np.zeros(6, np.float64), C.c_int(), C.c_int()
    check(_lib.load().gtx_op_estimate_affine_partial(ptr(p) if len(p) else None, ptr(q) if len(q) else None, len(p), seed, ptr(A), C.byref(valid), C.byref(inl)))
    return (A.reshape(2, 3), int(inl.value)) if valid.value else (None, 0)


def filter_matches(prev_xy: np.ndarray, cur_xy: np.ndarray, frame_hw) -> np.ndarray:
    """ultralytics GMC.apply_features' two spatial filters on ratio-tested matches: |displacement| < 0.25 x (width, height), then
    displacement - mean < 2.5 x std per axis (one-sided, as upstream writes it). -> boolean mask of the kept matches."""
    d = prev_xy.astype(np.float64) - cur_xy.astype(np.float64)
    keep = (np.abs(d[:, 0]) < 0.25 * frame_hw[1]) & (np.abs(d[:, 1]) < 0.25 * frame_hw[0])
    if keep.sum() == 0:
        return keep
    dk = d[keep]
    inl = ((dk - dk.mean(0)) < 2.5 * dk.std(0)).all(1)
    out = np.zeros(len(d), bool)
    out[np.flatnonzero(keep)[inl]] = True
    return out


class FeatureGMC:
    """ultralytics GMC(method='orb' | 'sift', downscale=2) (`gmc_method: orb` / `sift`, default.yaml:374,419,467): keypoints and
    descriptors of the half-resolution gray image, brute-force 2-NN matching against the previous frame's with Lowe's ratio 0.9,
    the two spatial filters of apply_features, then the RANSAC partial-affine fit. Built from what the path already has:

    * orb: gtx_fgmc_* (csrc/gmc_feat.hip) -- the stabilizer's detector / descriptor / Hamming matcher kernels (csrc/stabilizer.hip, without its
      homography solver, csrc/homography.hip: FAST 20 on an 8-level pyramid, Harris ranking, 256-bit rotated BRIEF; 1000 keypoints per frame), the filters and the RANSAC
      hypotheses as one chain on the object's stream per submitted frame. submit_gray_dev / submit_gray / submit_frame_dev only
      enqueue (frames may be submitted ahead, as with GMC); collect() waits for the oldest frame and refits on the host;
    * sift: csrc/sift.hip's SIFT (plain, not RootSIFT) + the L2 2-NN kernel (csrc/match_l2.hip), the filters in numpy and the fit
      by gtx_op_estimate_affine_partial. SYNCHRONOUS: sift.hip's detect reads its candidate counters back on the host between
      its stages, so a frame's warp is computed when it is collected; the submit calls only queue the image.

    Stated differences from the OpenCV calls upstream makes: the matcher's query is the CURRENT frame (stabilo's rule; upstream
    queries with the previous one), no detection-box mask, SIFT with OpenCV's default thresholds (upstream: contrast 0.02, edge 20).
    Interface of GMC above."""

    wants_frames = False

    def __init__(self, frame_hw: tuple[int, int], method: str = "orb", downscale: int = 2, seed: int = 0, ctx: _lib.Context | None = None,
                 max_features: int = 1000):
        if method not in ("orb", "sift"):
            raise NotImplementedError(f"gmc_method='{method}'")
        if downscale != 2:
            raise NotImplementedError("only downscale=2 (ultralytics' default) is implemented")
        self.method, self.seed = method, seed
        self.ctx = ctx or _lib.default_context()
        self.frame_hw = (int(frame_hw[0]), int(frame_hw[1]))
        self.gh, self.gw = self.frame_hw[0] // 2, self.frame_hw[1] // 2
        self.max_features = int(max_features)
        self.stats = np.zeros(3, np.int32)              # keypoints of the previous frame, matches kept, inliers
        self.valid = False
        self.handle = None
        self._pending = collections.deque()              # orb: host images in flight (kept alive); sift: (kind, image, restart) not yet collected
        self._prev = None
        self._restart_next = False                       # sift: the next submitted frame opens a new sequence
        if method == "orb":
            h = C.c_void_p()
            check(self.ctx.lib.gtx_fgmc_create(self.ctx.handle, self.frame_hw[0], self.frame_hw[1], self.max_features, int(seed), C.byref(h)))
            self.handle = h
            self._n_sub = self._n_col = 0                # frames submitted / collected (one writer each)
        else:
            from .registration import Sift

            self._sift = Sift((self.gh, self.gw), ctx=self.ctx)

    def close(self):
        if getattr(self, "handle", None):
            self.ctx.lib.gtx_fgmc_destroy(self.handle)
            self.handle = None
        if getattr(self, "_sift", None) is not None:
            self._sift.close()
            self._sift = None
            for kind, cur, _ in self._pending:
                if kind == "own":
                    self.ctx.dev_free(cur)
            self._pending.clear()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset_params(self):
        """Forget the previous frame; frames submitted and not collected are dropped. The blocking variant, used between clips."""
        if self.method == "orb":
            A, valid = np.zeros(6, np.float64), C.c_int()
            while self._n_col < self._n_sub:
                check(self.ctx.lib.gtx_fgmc_collect(self.handle, ptr(A), C.byref(valid), None))
                self._n_col += 1
            self._pending.clear()
            check(self.ctx.lib.gtx_fgmc_reset(self.handle))
            return
        self._prev, self._restart_next = None, False
        for kind, cur, _ in self._pending:
            if kind == "own":
                self.ctx.dev_free(cur)
        self._pending.clear()

    def reset_sequence(self) -> None:
        """The next submitted frame opens a new sequence (identity warp), with frames still in flight."""
        if self.method == "orb":
            check(self.ctx.lib.gtx_fgmc_restart(self.handle))
        else:
            self._restart_next = True

    # ---- submission: half-resolution gray images, resident in HBM (the detector's) or on the host, or a BGR frame in HBM
    def submit_gray_dev(self, gray_dptr: int, gh: int, gw: int) -> None:
        if (gh, gw) != (self.gh, self.gw):
            raise ValueError(f"gray image is {gw}x{gh}, the GMC was made for {self.gw}x{self.gh}")
        if self.method == "orb":
            check(self.ctx.lib.gtx_fgmc_submit_gray_dev(self.handle, C.c_void_p(int(gray_dptr)), gh, gw))
            self._pending.append(None)
            self._n_sub += 1
        else:
            self._pending.append(("dev", int(gray_dptr), self._take_restart()))

    def submit_gray(self, gray: np.ndarray) -> None:
        g = np.ascontiguousarray(gray, np.uint8)
        if g.shape != (self.gh, self.gw):
            raise ValueError(f"gray image is {g.shape[1]}x{g.shape[0]}, the GMC was made for {self.gw}x{self.gh}")
        if self.method == "orb":
            check(self.ctx.lib.gtx_fgmc_submit_gray(self.handle, ptr(g), self.gh, self.gw))
            self._pending.append(g)                      # the upload is queued: the image stays alive until its frame is collected
            self._n_sub += 1
        else:
            self._pending.append(("host", g, self._take_restart()))

    def submit_frame_dev(self, frame_dptr: int, h: int, w: int, restart: bool = False) -> None:
        """A BGR frame in HBM (gray + 2x2 mean on the device, the kernel gtx_gmc_submit_frame_dev uses); restart=True opens a new
        sequence with it (identity warp, the next frame is compared with it): how a shard rank primes its GMC."""
        if (int(h), int(w)) != self.frame_hw:
            raise ValueError(f"frame is {w}x{h}, the GMC was made for {self.frame_hw[1]}x{self.frame_hw[0]}")
        if self.method == "orb":
            check(self.ctx.lib.gtx_fgmc_submit_frame_dev(self.handle, C.c_void_p(int(frame_dptr)), int(h), int(w), int(restart)))
            self._pending.append(None)
            self._n_sub += 1
            return
        g = self.ctx.dev_alloc(self.gh * self.gw)        # the frame's buffer may be recycled before the frame is collected: an image of its own
        check(self.ctx.lib.gtx_gray_half_dev(self.ctx.handle, C.c_void_p(int(frame_dptr)), int(h), int(w), C.c_void_p(g)))
        if restart:
            self._restart_next = True
        self._pending.append(("own", g, self._take_restart()))

    def _take_restart(self) -> bool:
        r, self._restart_next = self._restart_next, False
        return r

    def apply(self, raw_frame: np.ndarray, detections=None) -> np.ndarray:
        """2x3 float64 warp previous -> current frame (identity for the first frame). raw_frame: BGR [h, w, 3] uint8."""
        f = np.asarray(raw_frame, np.uint8).astype(np.int32)
        g = (f[..., 0] * 1868 + f[..., 1] * 9617 + f[..., 2] * 4899 + 8192) >> 14          # cv2.cvtColor(BGR2GRAY), then the exact 2x reduction
        g = ((g[0::2, 0::2] + g[0::2, 1::2] + g[1::2, 0::2] + g[1::2, 1::2] + 2) >> 2).astype(np.uint8)
        self.submit_gray(g)
        return self.collect()

    # ---- one step
    def _pairs_sift(self, kind, cur):
        from .ops import match_2nn

        if kind in ("dev", "own"):
            g = np.zeros((self.gh, self.gw), np.uint8)
            self.ctx.dev_download(g, cur)                # waits for the context's stream: the gray pass queued at submit is behind it
            if kind == "own":
                self.ctx.dev_free(cur)
        else:
            g = cur
        k = self._sift.detect_and_compute(np.repeat(g[:, :, None], 3, 2), max_features=self.max_features, root=False)
        cur_f = (k["xy"].astype(np.float32) * 2.0, k["desc"])          # full-resolution pixels
        prev_f, self._prev = self._prev, cur_f
        if prev_f is None or len(prev_f[0]) < 2 or len(cur_f[0]) == 0:
            return None
        self.stats[0] = len(prev_f[0])
        i1, i2, d1, d2 = match_2nn(cur_f[1], prev_f[1], ctx=self.ctx)
        good = (i1 >= 0) & (i2 >= 0) & (d1 < np.float32(0.9) * d2)
        return prev_f[0][i1[good]], cur_f[0][good]

    def collect(self) -> np.ndarray:
        if self.method == "orb":
            A, valid = np.zeros(6, np.float64), C.c_int()
            check(self.ctx.lib.gtx_fgmc_collect(self.handle, ptr(A), C.byref(valid), ptr(self.stats)))
            self._n_col += 1
            self._pending.popleft()
            self.valid = bool(valid.value)
            return A.reshape(2, 3)
        if not self._pending:
            raise RuntimeError("GMC.collect without a submitted frame")
        kind, cur, restart = self._pending.popleft()
        if restart:
            self._prev = None
        H = np.eye(2, 3)
        self.valid = False
        self.stats[:] = 0
        pairs = self._pairs_sift(kind, cur)
        if pairs is None or len(pairs[0]) == 0:
            return H
        prev_xy, cur_xy = pairs
        keep = filter_matches(prev_xy, cur_xy, self.frame_hw)
        self.stats[1] = int(keep.sum())
        if keep.sum() > 4:
            M, inl = estimate_affine_partial(prev_xy[keep], cur_xy[keep], self.seed)
            if M is not None:
                H, self.valid = M, True
                self.stats[2] = inl
        return H

    # ---- parity hooks (orb; nothing may be in flight)
    def kept_pairs(self):
        """(previous-frame points, current-frame points) the filters kept for the frame collected last, full-resolution pixels."""
        n, out = C.c_int(), np.zeros((1024, 4), np.float32)
        check(self.ctx.lib.gtx_fgmc_pairs(self.handle, 1024, C.byref(n), ptr(out)))
        return out[:n.value, :2].copy(), out[:n.value, 2:].copy()

    def raw_matches(self):
        """The matcher's output for the frame submitted last: dict(best_idx, best_d, second_d [n_q], cur_xy [n_q, 2], prev_xy [n_t, 2])."""
        nq, nt = C.c_int(), C.c_int()
        bi, b1, b2 = (np.zeros(1024, np.int32) for _ in range(3))
        q, t = np.zeros((1024, 2), np.float32), np.zeros((1024, 2), np.float32)
        check(self.ctx.lib.gtx_fgmc_matches(self.handle, 1024, C.byref(nq), C.byref(nt), ptr(bi), ptr(b1), ptr(b2), ptr(q), ptr(t)))
        return dict(best_idx=bi[:nq.value].copy(), best_d=b1[:nq.value].copy(), second_d=b2[:nq.value].copy(), cur_xy=q[:nq.value].copy(),
                    prev_xy=t[:nt.value].copy())


class EccGMC:
    """ultralytics GMC(method='ecc', downscale=2) (`gmc_method: ecc`, default.yaml:374,419,467): cv2.findTransformECC with the
    Euclidean motion model, 5000 iterations / 1e-6, on cvtColor -> GaussianBlur(3x3, 1.5) -> resize(1/2) of the frame
    (csrc/ecc.hip over gtx_ecc_*; oracle/ecc_ref.py states the procedure and the OpenCV source it follows). Two properties of the
    upstream method are kept because the reference computes them: every frame is registered against the FIRST frame since
    reset_params() -- upstream never replaces its `prevFrame` for this method --, and the translation stays in half-resolution
    pixels. `last` holds {iters, status, rho} of the frame collected last (status 1 / 2: the two conditions under which
    cv2.findTransformECC raises; upstream catches it and keeps the matrix as the failed call left it, as collect() does).
    `warp`: which of OpenCV's two warpAffine forms takes the bilinear samples -- 'exact' (default; OpenCV >= 4.11, floating-point source
    positions: fits end after 5-30 iterations) or 'fixed' (through 4.10: positions rounded to 1/32 pixel, under which the coefficient
    can dither in its sixth decimal for good and the fit runs to the 5000-iteration cap).
    `replace_template=True` is NOT upstream's behaviour: every collected frame becomes the template of the next one (frame-to-frame
    warps, what a tracker's "previous -> current" compensation expects); off unless a caller asks for it.

    The method needs the BGR frame, not the detector's gray image (the blur comes before the reduction): `wants_frames` tells
    the engine to hand it every frame of a batch when the batch is submitted to a detector, on that detector's stream."""

    wants_frames = True

    def __init__(self, frame_hw: tuple[int, int], method: str = "ecc", downscale: int = 2, seed: int = 0, ctx: _lib.Context | None = None,
                 max_iters: int = 5000, eps: float = 1e-6, replace_template: bool = False, warp: str = "exact"):
        if method != "ecc":
            raise ValueError(f"EccGMC(method='{method}')")
        if downscale != 2:
            raise NotImplementedError("only downscale=2 (ultralytics' default) is implemented")
        self.ctx = ctx or _lib.default_context()
        self.frame_hw = (int(frame_hw[0]), int(frame_hw[1]))
        h = C.c_void_p()
        check(self.ctx.lib.gtx_ecc_create(self.ctx.handle, self.frame_hw[0], self.frame_hw[1], int(max_iters), float(eps), C.byref(h)))
        self.handle = h
        if warp not in ("exact", "fixed"):
            raise ValueError(f"EccGMC(warp='{warp}'): 'exact' (OpenCV >= 4.11's warpAffine) or 'fixed' (through 4.10)")
        if warp == "fixed":
            check(self.ctx.lib.gtx_ecc_exact_positions(h, 0))
        if replace_template:                             # NOT upstream's behaviour: frame-to-frame warps (each collected frame becomes the next template)
            check(self.ctx.lib.gtx_ecc_replace_template(h, 1))
        self.method = "ecc"
        self.valid = False
        self.stats = np.zeros(3, np.int32)               # {iterations, status, 0}: the slot the other methods fill with point counts
        self.last = {}

    def close(self):
        if getattr(self, "handle", None):
            self.ctx.lib.gtx_ecc_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset_params(self):
        check(self.ctx.lib.gtx_ecc_reset(self.handle))

    reset_sequence = reset_params

    def submit_frame_dev(self, frame_dptr: int, h: int, w: int, restart: bool = False, producer: _lib.Context | None = None) -> int:
        """-> the number of warps the call queued. restart=True marks the frame a shard rank primes the other methods with (the one
        before its run): this method registers every frame against the clip's FIRST frame, so it ignores that frame -- nothing is
        queued and there is no warp to collect. What a rank needs instead is the clip's first frame as its template: it submits
        that one like any other frame, once, before its first run, and discards its identity warp."""
        if restart:
            return 0
        check(self.ctx.lib.gtx_ecc_submit_dev(self.handle, producer.handle if producer is not None else None, C.c_void_p(int(frame_dptr)), int(h), int(w)))
        return 1

    def submit_gray_dev(self, gray_dptr: int, gh: int, gw: int) -> None:
        raise NotImplementedError("gmc_method ecc blurs the full-resolution gray image before reducing it: it takes BGR frames (submit_frame_dev / apply)")

    def submit_frame(self, frame: np.ndarray) -> None:
        f = np.ascontiguousarray(frame, np.uint8)
        check(self.ctx.lib.gtx_ecc_submit(self.handle, ptr(f), f.shape[0], f.shape[1]))

    def collect(self) -> np.ndarray:
        A, info, rho = np.zeros(6, np.float64), np.zeros(2, np.int32), C.c_double()
        check(self.ctx.lib.gtx_ecc_collect(self.handle, ptr(A), ptr(info), C.byref(rho)))
        self.last = dict(iters=int(info[0]), status=int(info[1]), rho=float(rho.value))
        self.stats[:2] = info
        self.valid = info[0] > 0 and info[1] == 0
        return A.reshape(2, 3)

    def apply(self, raw_frame: np.ndarray, detections=None) -> np.ndarray:
        """2x3 float64 warp first frame -> this frame in half-resolution pixels (identity for the first frame)."""
        self.submit_frame(raw_frame)
        return self.collect()

    def image(self, which: int = 0) -> np.ndarray:
        out = np.zeros((self.frame_hw[0] // 2, self.frame_hw[1] // 2), np.float32)
        check(self.ctx.lib.gtx_ecc_image(self.handle, int(which), ptr(out)))
        return out


def make_gmc(frame_hw, method: str = "sparseOptFlow", **kw):
    """The GMC object of `gmc_method` (default.yaml:374): sparseOptFlow -> GMC, orb / sift -> FeatureGMC, ecc -> EccGMC."""
    if method in ("orb", "sift"):
        return FeatureGMC(frame_hw, method=method, **kw)
    if method == "ecc":
        return EccGMC(frame_hw, method=method, **kw)
    return GMC(frame_hw, method=method, **kw)
