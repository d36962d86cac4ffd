"""CPU checks of the monocular initialiser (Initializer.cpp) — the oracle
(oracle/init_oracle.c) against closed-form two-view geometry, and the host helpers of the C-ABI
(sampler, SelectFeaturesForInit, ComputeParallax, pose composition) against Python restatements.
tests/test_init_reference.py holds the same oracle to an independent f64 restatement of Initializer.cpp
(tests/mono_init_reference.py): that pins the exact null vector of the f32-built system and every
threshold, comparison and convention.  Still not pinned: bit parity with Eigen's f32 JacobiSVD (Eigen is
absent from the image)."""
import numpy as np
import pytest

import init_cases
import oracle_lib
from test_tracker_oracle import py_mt19937_samples


def skew(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])


def run(vio, b1, b2, seed=7, iters=200, **kw):
    P = vio.abi.mono_init_params(ransac_iterations=iters, **kw)
    S = vio.mono_init_samples(seed, len(b1), iters) if iters else np.zeros((0, 8), np.int32)
    return oracle_lib.mono_init(vio, b1, b2, S, P)


def test_sampler_matches_libstdcxx(vio):
    for seed, n in [(0, 300), (99, 8), (2**32 - 1, 1000), (5, 23)]:
        s = vio.mono_init_samples(seed, n, 50)
        assert np.array_equal(s.reshape(-1), py_mt19937_samples(seed, n, 50, k=8))
        assert s.min() >= 0 and s.max() < n
        assert all(len(set(r)) == 8 for r in s.tolist())
    with pytest.raises(vio.VioError):
        vio.mono_init_samples(1, 7, 10)  # the reference's sampler never terminates for n < 8


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_noise_free_two_view_closed_form(vio, seed):
    b1, b2, R, t, P1 = init_cases.make_case(n=400, seed=seed)
    res, mask, X = run(vio, b1, b2)
    assert res["status"] == vio.abi.VIO_INIT_OK, res
    assert mask.all() and res["num_inliers"] == 400
    # E = [t]x R up to scale and sign
    E = res["E"].astype(np.float64)
    Et = skew(t) @ R
    E /= np.linalg.norm(E)
    Et /= np.linalg.norm(Et)
    assert min(np.abs(E - Et).max(), np.abs(E + Et).max()) < 1e-4
    # exact pose: R, and t along the true direction (scale normalised)
    assert np.abs(res["R"] - R).max() < 1e-4
    assert float(res["t"] @ t) / (np.linalg.norm(res["t"]) * np.linalg.norm(t)) > 1 - 1e-6
    # mid-points = landmarks / median distance
    d = np.linalg.norm(P1, axis=1)
    ref = P1 / np.median(d)
    # f32 mid-points at range / baseline up to 33 (points near the baseline direction have no parallax)
    rel = np.linalg.norm(X - ref, axis=1) / np.linalg.norm(ref, axis=1)
    assert np.percentile(rel, 95) < 2e-3 and np.median(rel) < 5e-4, (np.percentile(rel, 95), np.median(rel))
    assert abs(np.median(np.linalg.norm(X, axis=1)) - 1.0) < 1e-4
    assert res["num_triangulated"] == 400 and res["num_valid"] == 400
    assert res["mean_reproj_error"] < 0.05
    # exactly one candidate sees everything in front (the other three fail the reprojection test)
    good = sorted(res["candidate_good"])
    assert good[-1] == 400 and good[-2] < 400


def test_outliers_are_rejected(vio):
    b1, b2, R, t, _ = init_cases.make_case(n=600, seed=11, noise_deg=0.02, outlier_frac=0.2)
    # the reference's 0.1 algebraic threshold lets most gross outliers through (its refit then drifts);
    # a 0.01 threshold separates them on this geometry
    res, mask, X = run(vio, b1, b2, seed=3, ransac_threshold=0.01)
    assert res["status"] == vio.abi.VIO_INIT_OK, res
    assert np.abs(res["R"] - R).max() < 2e-3
    assert float(res["t"] @ t) / (np.linalg.norm(res["t"]) * np.linalg.norm(t)) > 0.999
    assert 0.78 * 600 < res["num_inliers"] <= 0.84 * 600


def test_failure_statuses(vio):
    A = vio.abi
    b1, b2, R, t, _ = init_cases.make_case(n=300, seed=4)
    assert run(vio, b1[:4], b2[:4], iters=0)[0]["status"] == A.VIO_INIT_TOO_FEW_BEARINGS
    assert run(vio, b1, b2, min_features=301)[0]["status"] == A.VIO_INIT_ESSENTIAL_FAILED
    assert run(vio, b1, b2, iters=0)[0]["status"] == A.VIO_INIT_ESSENTIAL_FAILED
    r = run(vio, b1, b2, max_reprojection_error=1e-9)[0]
    assert r["status"] == A.VIO_INIT_VALIDATION and r["num_valid"] < 100  # exact-zero errors still pass
    # pure rotation: no baseline, the rays do not intersect in front of both cameras
    c1, c2, *_ = init_cases.make_case(n=300, seed=5, baseline=0.0)
    r = run(vio, c1, c2)[0]
    assert r["status"] != A.VIO_INIT_OK


def test_select_features_matches_restatement(vio):
    rng = np.random.default_rng(0)
    W, H = 960, 480
    for trial in range(5):
        n = 700
        uv = np.stack([rng.uniform(0, W, n), rng.uniform(0, H, n)], 1).astype(np.float32)
        oc = rng.integers(5, 20, n).astype(np.int32)  # ties on purpose (cells hold <= 16: insertion sort)
        got = vio.init_select_features(uv, oc, W, H, 20, 10, 10, 100)
        cand = [i for i in range(n) if oc[i] >= 10]
        cw, ch = np.float32(W) / np.float32(20), np.float32(H) / np.float32(10)
        cells = {}
        for i in cand:
            c = min(max(int(np.float32(uv[i, 0]) / cw), 0), 19)
            r = min(max(int(np.float32(uv[i, 1]) / ch), 0), 9)
            cells.setdefault(r * 20 + c, []).append(i)
        assert max(len(v) for v in cells.values()) <= 16
        ref = []
        for g in sorted(cells):
            ref += sorted(cells[g], key=lambda i: -oc[i])[:5]  # stable, like libstdc++'s small-range sort
        assert got.tolist() == ref
    assert len(vio.init_select_features(uv, np.zeros(n, np.int32), W, H)) == 0


def test_parallax(vio):
    ids1 = np.array([1, 2, 3, 4, 5], np.int32)
    uv1 = np.zeros((5, 2), np.float32)
    ids2 = np.array([5, 3, 1, 9], np.int32)
    uv2 = np.array([[3, 4], [6, 8], [0, 1], [100, 100]], np.float32)
    assert vio.init_parallax(ids1, uv1, ids2, uv2) == pytest.approx(5.0)  # median of {1, 10, 5}
    assert vio.init_parallax(ids1[:2], uv1[:2], ids2, uv2) == pytest.approx(1.0)
    assert vio.init_parallax(ids1, uv1, np.zeros(0, np.int32), np.zeros((0, 2), np.float32)) == 0.0


def test_compose(vio):
    rng = np.random.default_rng(1)
    T_BC = np.eye(4)
    T_BC[:3, :3] = init_cases.rodrigues(rng.normal(size=3))
    T_BC[:3, 3] = rng.normal(size=3) * 0.1
    R = init_cases.rodrigues(rng.normal(size=3) * 0.1)
    t = rng.normal(size=3)
    X = rng.normal(size=(7, 3))
    T1, T2, Xw = vio.init_compose(T_BC, R, t, X)
    T12 = np.eye(4)
    T12[:3, :3], T12[:3, 3] = R, t
    ref = T_BC @ np.linalg.inv(T12) @ np.linalg.inv(T_BC)
    assert np.array_equal(T1, np.eye(4, dtype=np.float32))
    assert np.abs(T2 - ref).max() < 1e-5
    assert np.abs(Xw - (X @ T_BC[:3, :3].T + T_BC[:3, 3])).max() < 1e-5
