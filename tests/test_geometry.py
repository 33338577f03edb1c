"""Projective helpers behind gtx_warp_boxes / gtx_perspective_points against the reference's
golden outputs and its own unit-test cases. Host-only entry points: run on CPU."""
import gzip
from pathlib import Path

import numpy as np

from geotrax_amd import geometry as geo

G = Path(__file__).parent / "golden"


def _golden_tracks():
    with gzip.open(G / "U_video_cut.txt.gz", "rt") as f:
        return np.loadtxt(f, delimiter=",")


def test_box_warp_rule_on_golden_clip():
    """K10: raw boxes (cols 2-5) + per-frame homographies (_vid_transf.txt) -> stabilized boxes
    (cols 6-9). The corner-hull rule reproduces every golden box after frame 0 (19 682) to the %g print quantum
    (x >= 1000 px is stored to 0.01 px); frame 0 is copied through (extract.py:178-179)."""
    t = _golden_tracks()
    tr = np.loadtxt(G / "U_video_cut_vid_transf.txt", delimiter=",")
    Hs = {int(r[0]): r[1:].reshape(3, 3) for r in tr}
    assert len(Hs) == 149 and set(Hs) == set(range(1, 150))
    n = 0
    for f in range(150):
        rows = t[t[:, 0] == f]
        if f == 0:
            np.testing.assert_array_equal(rows[:, 6:10], rows[:, 2:6])
            continue
        got = geo.warp_boxes(Hs[f], rows[:, 2:6])
        assert np.abs(got - rows[:, 6:10]).max() < 0.0125
        n += len(rows)
    assert n == len(t) - (t[:, 0] == 0).sum() and n > 19600


def test_perspective_points_on_golden_georeference():
    """K12: Ortho_X/Y of the golden CSV == round(persp(H_geo, x_stab, y_stab), 1) for every row
    the CSV keeps (it drops trajectories shorter than min_traj_length)."""
    t = _golden_tracks()
    Hg = np.loadtxt(G / "U_video_cut_geo_transf.txt", delimiter=",").reshape(3, 3)
    c = np.load(G / "U_video_cut_csv_cols.npz")
    key = {(int(f), int(i)): k for k, (f, i) in enumerate(zip(t[:, 0], t[:, 1]))}
    rows = np.array([key[(int(f), int(i))] for f, i in zip(c["frame"], c["vehicle_id"])])
    ox, oy = geo.apply_homography(t[rows, 6], t[rows, 7], Hg)
    assert len(ox) == 19787
    np.testing.assert_array_equal(np.round(ox, 1), c["ortho_x"])
    np.testing.assert_array_equal(np.round(oy, 1), c["ortho_y"])


def test_apply_homography_reference_cases():
    # tests/test_georeference.py:31-43 of the reference: identity and pure translation
    x, y = np.array([10.0, 20.0, 30.5]), np.array([5.0, 15.0, 25.5])
    ox, oy = geo.apply_homography(x, y, np.eye(3))
    np.testing.assert_allclose(ox, x)
    np.testing.assert_allclose(oy, y)
    Ht = np.array([[1, 0, 7.0], [0, 1, -3.0], [0, 0, 1]])
    ox, oy = geo.apply_homography(x, y, Ht)
    np.testing.assert_allclose(ox, x + 7)
    np.testing.assert_allclose(oy, y - 3)


def test_ortho2geo_reference_case():
    # tests/test_georeference.py:46-51: plain affine
    lat, lon = geo.ortho2geo(np.array([10.0]), np.array([20.0]), (126.0, 37.0, 1e-6, -2e-6, 0.0, 0.0))
    np.testing.assert_allclose(lon, 126.0 + 1e-5)
    np.testing.assert_allclose(lat, 37.0 - 4e-5)


def test_warp_boxes_projective_and_empty():
    H = np.array([[1.01, 0.02, 3.0], [-0.015, 0.99, -2.0], [1e-5, -2e-5, 1.0]])
    b = np.array([[100, 200, 40, 20], [3000, 1500, 90, 45]], dtype=np.float32)
    got = geo.warp_boxes(H, b)
    for (cx, cy, w, h), g in zip(b.astype(np.float64), got):
        cs = np.array([[cx - w / 2, cy - h / 2, 1], [cx + w / 2, cy - h / 2, 1], [cx + w / 2, cy + h / 2, 1], [cx - w / 2, cy + h / 2, 1]]).T
        p = H @ cs
        p = p[:2] / p[2]
        exp = [(p[0].min() + p[0].max()) / 2, (p[1].min() + p[1].max()) / 2, np.ptp(p[0]), np.ptp(p[1])]
        np.testing.assert_allclose(g, exp, rtol=1e-6)
    assert geo.warp_boxes(H, np.zeros((0, 4), np.float32)).shape == (0, 4)


def test_estimate_affine_partial_equals_the_oracle_and_recovers_a_similarity():
    """gtx_op_estimate_affine_partial (host C++; the fit of `gmc_method: orb` / `sift`) == oracle/gmc_ref.estimate_affine_partial on
    seeded matches with 30 % outliers, and both recover the similarity the inliers were made with."""
    from geotrax_amd.gmc import estimate_affine_partial
    from oracle import gmc_ref

    rng = np.random.default_rng(7)
    for n in (5, 60, 800):
        p = rng.uniform(0, 1000, (n, 2)).astype(np.float32)
        a, s = 0.01, 1.002
        M = np.array([[s * np.cos(a), -s * np.sin(a), 12.5], [s * np.sin(a), s * np.cos(a), -7.25]])
        q = (p.astype(np.float64) @ M[:, :2].T + M[:, 2] + 0.3 * rng.standard_normal((n, 2))).astype(np.float32)
        bad = rng.random(n) < 0.3
        q[bad] += rng.uniform(-200, 200, (int(bad.sum()), 2)).astype(np.float32)
        got, inl = estimate_affine_partial(p, q, seed=3)
        want = gmc_ref.estimate_affine_partial(p, q, seed=3)
        assert got is not None and want is not None
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-9)
        if n >= 60:
            assert np.abs(got - M).max() < 0.2 and inl > 0.6 * n
    got, inl = estimate_affine_partial(np.zeros((1, 2), np.float32), np.zeros((1, 2), np.float32))
    assert got is None and inl == 0


_REFIT_FRAME, _REFIT_THR = (1920, 1080), 2.0
_REFIT_CASES = [(False, 4), (False, 5), (False, 60), (False, 800), (True, 3), (True, 60)]      # (affine, n)
_REFIT_BAR = 2.73e-5   # px: ten times the worst distance measured, see the test's docstring


def _refit_pairs(affine, n):
    """n pairs of a 1920x1080 frame under a known map (a mild perspective term unless affine), 0.3 px Gaussian noise, 30 % outliers."""
    w, h = _REFIT_FRAME
    rng = np.random.default_rng(100 * n + affine)
    a, s = 0.01, 1.002
    Ht = np.array([[s * np.cos(a), -s * np.sin(a), 12.5], [s * np.sin(a), s * np.cos(a), -7.25], [0.0, 0.0, 1.0] if affine else [2e-6, -1e-6, 1.0]])
    p = rng.uniform((0, 0), (w, h), (n, 2)).astype(np.float32)
    g = np.concatenate([p.astype(np.float64), np.ones((n, 1))], 1) @ Ht.T
    q = (g[:, :2] / g[:, 2:] + 0.3 * rng.standard_normal((n, 2))).astype(np.float32)
    bad = rng.random(n) < 0.3
    q[bad] += rng.uniform(-200, 200, (int(bad.sum()), 2)).astype(np.float32)
    return p, q, Ht


def _refit_both(p, q, H0, affine):
    from geotrax_amd.ops import homography_refit
    from oracle import stabilo_ref

    w, h = _REFIT_FRAME
    thr = float(np.float32(_REFIT_THR))
    want = stabilo_ref.refine_homography(H0 / H0[2, 2], p.astype(np.float64), q.astype(np.float64), w / 2.0, h / 2.0, 2.0 / w, thr, affine)
    return homography_refit(np.concatenate([p, q], 1), H0, _REFIT_FRAME, thr, affine=affine), want


def test_homography_refit_equals_the_oracle():
    """gtx_op_homography_refit (csrc/homography_refit.cpp, the host tail of every robust homography) == oracle.stabilo_ref.refine_homography
    on the same pairs and the same RANSAC winner (the oracle's, 64 hypotheses): both give a model or both none, the same inlier count,
    and H within the 9 x 16 grid reprojection distance of tests/test_stabilizer_gpu.py. The counts can only be compared exactly when no
    residual sits on the threshold: the oracle's final residuals are first shown to keep 1e-6 px away from it for these seeds.
    The two sides differ in the linear solve (Cholesky here, LU there) and in summation order only. Measured on the CPU this was
    written on: 2.73e-6 px for the five projective pairs (four inliers: the normal matrix is close to singular), at most 9.1e-13 px for
    the other five cases. The bar is ten times the worst, for another libm or BLAS build: 2.73e-5 px, far inside the 1e-3 px that
    test_stabilizer_gpu.py allows end to end for this very pair."""
    from oracle import stabilo_ref
    from test_stabilizer_gpu import _grid_err

    w, h = _REFIT_FRAME
    worst = 0.0
    for affine, n in _REFIT_CASES:
        p, q, _ = _refit_pairs(affine, n)
        _, _, H0 = stabilo_ref.ransac_hypotheses(p, q, _REFIT_FRAME, _REFIT_THR, 64, 0, affine)
        assert H0 is not None, (affine, n)
        (got, got_inl), (want, want_inl) = _refit_both(p, q, H0, affine)
        assert want is not None, (affine, n)
        res = np.sqrt(stabilo_ref._errors(want, p.astype(np.float64), q.astype(np.float64)))
        margin = np.abs(res - float(np.float32(_REFIT_THR))).min()
        assert margin > 1e-6, (affine, n, margin)                     # the oracle alone: no pair on the threshold
        assert got is not None, (affine, n)
        err = _grid_err(got, want, (h, w))
        worst = max(worst, err)
        print(f"homography_refit affine={affine} n={n}: inliers {got_inl} / {want_inl}, nearest residual {margin:.3g} px from the threshold, grid distance {err:.3g} px")
        assert got_inl == want_inl, (affine, n)
        assert err <= _REFIT_BAR, (affine, n, err)
    print(f"homography_refit: worst grid distance {worst:.3g} px, bar {_REFIT_BAR:.3g} px")
    # under-supported: a winner 500 px away from every pair leaves fewer than four pairs within three thresholds
    p, q, Ht = _refit_pairs(False, 60)
    far = Ht.copy()
    far[0, 2] += 500.0
    (got, got_inl), (want, want_inl) = _refit_both(p, q, far, False)
    assert got is None and want is None and got_inl == 0 and want_inl == 0


def _adjugate_inverse_longdouble(H):
    m = np.asarray(H, np.longdouble).ravel()
    a, b, c, d, e, f, g, h, i = m
    adj = np.array([e * i - f * h, -(b * i - c * h), b * f - c * e,
                    -(d * i - f * g), a * i - c * g, -(a * f - c * d),
                    d * h - e * g, -(a * h - b * g), a * e - b * d], np.longdouble)
    return (adj / (a * adj[0] + b * adj[3] + c * adj[6])).reshape(3, 3)


def _camera_like(rng):
    """Rotation up to half a radian, zoom 0.5 .. 2 with 5 % anisotropy, a shift of up to 2000 px, perspective terms up to 1e-4."""
    a, s = rng.uniform(-0.5, 0.5), np.exp(rng.uniform(-0.7, 0.7))
    return np.array([[s * np.cos(a) * rng.uniform(0.95, 1.05), -s * np.sin(a), rng.uniform(-2000, 2000)],
                     [s * np.sin(a), s * np.cos(a) * rng.uniform(0.95, 1.05), rng.uniform(-2000, 2000)],
                     [rng.uniform(-1e-4, 1e-4), rng.uniform(-1e-4, 1e-4), 1.0]])


def test_invert3x3_hook_against_a_longdouble_adjugate():
    """gtx_op_invert3x3 (the inverse gtx_warp_frame hands its kernel) over every matrix of tests/test_warp_ops_gpu.py and 200 seeded
    camera-like ones, against the adjugate formula evaluated in np.longdouble: |inv - ref| <= 16 eps cond_inf(H) max|ref|, elementwise.
    A matrix is kept only if the reference itself is known to sit well inside that bound: its error is at most
    |ref|_inf |I - H ref|_inf (from H^-1 - ref = H^-1 (I - H ref)), the residual taken in longdouble; where that estimate exceeds
    1/8 of the bound (a platform whose longdouble is float64) the matrix is dropped and named in the output."""
    import warp_cases as wc

    eps = np.finfo(np.float64).eps
    rng = np.random.default_rng(2024)
    mats = dict(wc.issue_matrices())
    mats.update({f"camera-like-{k}": _camera_like(rng) for k in range(200)})
    worst, worst_name, dropped = 0.0, None, []
    for name, H in mats.items():
        ref = _adjugate_inverse_longdouble(H)
        Hl = np.asarray(H, np.longdouble)
        norm = lambda m: np.abs(m).sum(1).max()
        bound = 16 * eps * float(norm(Hl) * norm(ref)) * float(np.abs(ref).max())
        ref_err = float(norm(ref) * norm(np.eye(3, dtype=np.longdouble) - Hl @ ref))
        if not ref_err <= bound / 8:
            dropped.append(name)
            continue
        got = wc.hook_inverse(H)
        ratio = float(np.abs(got.astype(np.longdouble) - ref).max()) / bound
        if ratio > worst:
            worst, worst_name = ratio, name
        assert ratio <= 1.0, (name, ratio)
    print(f"gtx_op_invert3x3: {len(mats) - len(dropped)} matrices, largest |inv - ref| / bound = {worst:.3g} ({worst_name}); "
          f"dropped because the reference could not be held: {dropped or 'none'}")
    assert len(dropped) == 0 or np.finfo(np.longdouble).eps >= eps / 2


def test_invert3x3_hook_refuses_singular_and_non_finite_matrices():
    """Singular, NaN and Inf matrices: -1, and the output array is left as it was."""
    from geotrax_amd import _lib

    lib = _lib.load()
    bad = {"zero": np.zeros((3, 3)), "equal rows": np.array([[1.0, 2, 3], [1, 2, 3], [4, 5, 6]]),
           "rank 2": np.array([[1.0, 2, 3], [4, 5, 6], [7, 8, 9]]), "zero column": np.array([[1.0, 0, 3], [4, 0, 6], [7, 0, 10]]),
           "nan": np.array([[1.0, 0, 0], [0, np.nan, 0], [0, 0, 1]]), "inf": np.array([[1.0, 0, np.inf], [0, 1, 0], [0, 0, 1]]),
           "-inf": np.array([[-np.inf, 0, 0], [0, 1, 0], [0, 0, 1]]), "overflowing determinant": np.diag([1e200, 1e200, 1e200])}
    for name, H in bad.items():
        inv = np.full(9, 7.0)
        assert lib.gtx_op_invert3x3(_lib.ptr(np.ascontiguousarray(H.ravel())), _lib.ptr(inv)) == -1, name
        assert b"singular" in lib.gtx_last_error(), name
        np.testing.assert_array_equal(inv, np.full(9, 7.0), err_msg=name)
    inv = np.full(9, 7.0)
    assert lib.gtx_op_invert3x3(_lib.ptr(np.diag([2.0, 4.0, 8.0]).ravel()), _lib.ptr(inv)) == 0
    np.testing.assert_array_equal(inv.reshape(3, 3), np.diag([0.5, 0.25, 0.125]))
