"""GPU checks of vio_mono_init_solve (csrc/mono_init.hip): parity with oracle/init_oracle.c, and the
independent f64 reference of tests/mono_init_reference.py (np.linalg.svd of the f32-built systems, every
threshold and convention of Initializer.cpp restated from the source alone) through the same
check_against_reference() that tests/test_init_reference.py applies to the oracle.  Pinned by the
reference: the exact null vector of the f32-built system, every threshold, comparison and convention.
Not pinned: bit parity with Eigen's f32 JacobiSVD.

Oracle parity:

Initializer::TryMonocularInitialization (src/processing/Initializer.cpp:47-291).  Both sides run the
same f64 Jacobi null vectors / 3x3 SVDs on f32-built systems and the reference's f32 per-point
expressions; the refit sum uses the same fixed order.  Bar (stated here): every integer output
(status, best hypothesis, inlier count and mask, candidate good-point counts, chosen candidate,
triangulated / valid counts) identical; E, R, t, points, scale and the mean reprojection error to
1e-5 relative (device atan2f / asinf vs glibc differ by ulps; the f64 parts are IEEE-exact on both
and agree bitwise in practice).
"""
import ctypes as C
import functools

import numpy as np
import pytest

import init_cases
import mono_init_reference as M
import oracle_lib
from test_init_reference import case_id, ransac_of

pytestmark = pytest.mark.gpu


def compare(vio, ctx, b1, b2, seed=7, iters=200, **kw):
    P = vio.abi.mono_init_params(ransac_iterations=iters, **kw)
    S = vio.mono_init_samples(seed, len(b1), iters) if iters else np.zeros((0, 8), np.int32)
    return compare_samples(vio, ctx, b1, b2, S, P)


def compare_samples(vio, ctx, b1, b2, S, P):
    g, gm, gX = ctx.mono_init(b1, b2, S, P)
    o, om, oX = oracle_lib.mono_init(vio, b1, b2, S, P)
    for k in ("status", "best_hypothesis", "num_inliers", "pose_candidate", "candidate_good",
              "num_triangulated", "num_valid"):
        assert g[k] == o[k], (k, g[k], o[k])
    np.testing.assert_array_equal(gm, om)
    for k in ("E", "R", "t"):
        d = np.abs(g[k].astype(np.float64) - o[k]).max()
        assert d <= 1e-5 * max(1.0, np.abs(o[k]).max()), (k, d)
    assert abs(g["scale_factor"] - o["scale_factor"]) <= 1e-5 * abs(o["scale_factor"])
    assert abs(g["mean_reproj_error"] - o["mean_reproj_error"]) <= 1e-5 * max(1.0, o["mean_reproj_error"])
    nrm = np.maximum(np.linalg.norm(oX, axis=1), 1e-6)
    assert (np.linalg.norm(gX.astype(np.float64) - oX, axis=1) / nrm).max() <= 1e-5
    return g, o, gX, oX


@pytest.mark.parametrize("seed,noise,outl,n", [(1, 0.0, 0.0, 400), (2, 0.05, 0.0, 1000), (3, 0.02, 0.1, 800),
                                               (4, 0.1, 0.3, 2000), (5, 0.0, 0.0, 4096)])
def test_parity_with_oracle(vio, gpu_ctx, seed, noise, outl, n):
    b1, b2, R, t, _ = init_cases.make_case(n=n, seed=seed, noise_deg=noise, outlier_frac=outl)
    g, o, gX, oX = compare(vio, gpu_ctx, b1, b2, seed=seed)
    if outl == 0.0:
        assert g["status"] == vio.abi.VIO_INIT_OK
    assert gpu_ctx.mono_init_kernel_ms() > 0


def test_reference_config_threshold_and_tight_threshold(vio, gpu_ctx):
    b1, b2, *_ = init_cases.make_case(n=600, seed=11, noise_deg=0.02, outlier_frac=0.2)
    compare(vio, gpu_ctx, b1, b2, seed=3)
    g, *_ = compare(vio, gpu_ctx, b1, b2, seed=3, ransac_threshold=0.01)
    assert g["status"] == vio.abi.VIO_INIT_OK


def test_failure_paths(vio, gpu_ctx):
    A = vio.abi
    b1, b2, *_ = init_cases.make_case(n=300, seed=4)
    assert compare(vio, gpu_ctx, b1[:4], b2[:4], iters=0)[0]["status"] == A.VIO_INIT_TOO_FEW_BEARINGS
    assert compare(vio, gpu_ctx, b1, b2, min_features=301)[0]["status"] == A.VIO_INIT_ESSENTIAL_FAILED
    assert compare(vio, gpu_ctx, b1, b2, iters=0)[0]["status"] == A.VIO_INIT_ESSENTIAL_FAILED
    # validation failure on noisy bearings (a 1e-9 px bar would compare exact-zero errors, where an ulp
    # of atan2f / asinf decides)
    n1, n2, *_ = init_cases.make_case(n=300, seed=12, noise_deg=0.3)
    assert compare(vio, gpu_ctx, n1, n2, max_reprojection_error=0.05)[0]["status"] == A.VIO_INIT_VALIDATION
    c1, c2, *_ = init_cases.make_case(n=300, seed=5, baseline=0.0)
    compare(vio, gpu_ctx, c1, c2)
    # few hypotheses / tiny n
    compare(vio, gpu_ctx, b1[:8], b2[:8], iters=3, min_features=4)


def test_bad_arguments(vio, gpu_ctx):
    b1, b2, *_ = init_cases.make_case(n=50, seed=6)
    S = vio.mono_init_samples(1, 50, 10)
    S[3, 2] = 50  # out of range: rejected on the host before any launch
    with pytest.raises(vio.VioError):
        gpu_ctx.mono_init(b1, b2, S)
    big = np.zeros((4097, 3), np.float32)
    with pytest.raises(vio.VioError):
        gpu_ctx.mono_init(big, big, np.zeros((1, 8), np.int32))


def test_repeatable(vio, gpu_ctx):
    b1, b2, *_ = init_cases.make_case(n=1000, seed=8, noise_deg=0.05, outlier_frac=0.1)
    S = vio.mono_init_samples(9, 1000, 200)
    a = gpu_ctx.mono_init(b1, b2, S)
    b = gpu_ctx.mono_init(b1, b2, S)
    for k in a[0]:
        assert np.array_equal(np.asarray(a[0][k]), np.asarray(b[0][k])), k
    assert np.array_equal(a[2], b[2])


# ---- the independent reference and the edges of the three kernels -------------------------------
@pytest.mark.parametrize("res", init_cases.RESOLUTIONS, ids=lambda r: "w%d" % r[0])
@pytest.mark.parametrize("case", init_cases.REFERENCE_CASES, ids=case_id)
def test_device_against_reference(vio, gpu_ctx, case, res):
    b1, b2, S, P, _ = init_cases.reference_case(vio, case, *res)
    fig = M.check_against_reference(gpu_ctx.mono_init, b1, b2, S, P, ransac=ransac_of(vio, case))
    print(case, res, fig)
    g, *_ = compare_samples(vio, gpu_ctx, b1, b2, S, P)
    assert g["status"] == init_cases.EXPECTED_STATUS.get((case[0], case[3], res[0]), vio.abi.VIO_INIT_OK)


@pytest.mark.parametrize("iters", [1, 31, 32, 33, 64, 65])
def test_hypothesis_counts(vio, gpu_ctx, iters):
    """One hypothesis, and both sides of the 32-lane workgroup of mono_hyp_kernel."""
    b1, b2, S, P, _ = init_cases.reference_case(vio, init_cases.REFERENCE_CASES[2], iters=iters)
    g, *_ = compare_samples(vio, gpu_ctx, b1, b2, S, P)
    rr = M.ransac_reference(b1, b2, S, P.ransac_threshold)
    if rr["winner_decided"]:
        assert g["best_hypothesis"] == rr["best"]
        assert rr["lo"][rr["best"]] <= g["num_inliers"] <= rr["hi"][rr["best"]]


def test_first_strictly_best(vio, gpu_ctx):
    case = init_cases.REFERENCE_CASES[2]
    b1, b2, S, P, _ = init_cases.reference_case(vio, case)
    rr = ransac_of(vio, case)
    p, q = 17, 40
    assert rr["winner_decided"] and rr["best"] > q
    S2 = S.copy()
    S2[p] = S2[q] = S[rr["best"]]
    assert compare_samples(vio, gpu_ctx, b1, b2, S2, P)[0]["best_hypothesis"] == p
    # noise-free: every row ties at n inliers
    case = init_cases.REFERENCE_CASES[0]
    b1, b2, S, P, _ = init_cases.reference_case(vio, case)
    assert (ransac_of(vio, case)["lo"] == len(b1)).all()
    g, *_ = compare_samples(vio, gpu_ctx, b1, b2, S, P)
    assert g["best_hypothesis"] == 0 and g["num_inliers"] == len(b1)


def test_no_hypothesis_qualifies(vio, gpu_ctx):
    b1, b2, S, P, _ = init_cases.reference_case(vio, init_cases.REFERENCE_CASES[1])
    P = M.with_params(P, ransac_threshold=0.0)
    g, _, gX, _ = compare_samples(vio, gpu_ctx, b1, b2, S, P)
    gm = gpu_ctx.mono_init(b1, b2, S, P)[1]
    assert g["status"] == vio.abi.VIO_INIT_ESSENTIAL_FAILED
    assert g["best_hypothesis"] == -1 and g["num_inliers"] == 0 and not gm.any() and not gX.any()


def _same(a, b):
    for k in a[0]:
        assert np.array_equal(np.asarray(a[0][k]), np.asarray(b[0][k]), equal_nan=True), k
    assert np.array_equal(a[1], b[1]) and a[2].tobytes() == b[2].tobytes()


def test_no_stale_state(vio, gpu_ctx):
    """The context's buffer is reused: a small call after a large one, a failing one, then a good one,
    each bitwise equal to the same call on a fresh context."""
    big = init_cases.reference_case(vio, init_cases.REFERENCE_CASES[4])[:4]
    b1, b2, _, P, _ = init_cases.reference_case(vio, init_cases.REFERENCE_CASES[6])
    small = (b1, b2, vio.mono_init_samples(16, 9, 3), M.with_params(P, ransac_iterations=3))
    fb1, fb2, fS, fP, _ = init_cases.reference_case(vio, init_cases.REFERENCE_CASES[15])
    ok = init_cases.reference_case(vio, init_cases.REFERENCE_CASES[11])[:4]
    calls = [big, small, (fb1, fb2, fS, fP), ok]
    got = [gpu_ctx.mono_init(*c) for c in calls]
    assert [g[0]["status"] for g in got] == [0, 0, vio.abi.VIO_INIT_POSE_FAILED, 0]
    for c, g in zip(calls, got):
        fresh = vio.Context(0)
        try:
            _same(g, fresh.mono_init(*c))
        finally:
            fresh.close()


def test_null_outputs(vio, gpu_ctx):
    """inlier_mask and points are optional in the C-ABI: the result struct does not depend on them."""
    b1, b2, S, P, _ = init_cases.reference_case(vio, init_cases.REFERENCE_CASES[12])
    n = len(b1)
    vp = C.c_void_p

    def p(a):
        return a.ctypes.data_as(vp)

    def call(want_mask, want_points):
        R = vio.abi.VioMonoInitResult()
        m = np.full(n, 7, np.uint8)
        X = np.full((n, 3), 7, np.float32)
        rc = vio.lib().vio_mono_init_solve(gpu_ctx.h, p(b1), p(b2), n, p(S), C.byref(P), C.byref(R),
                                           p(m) if want_mask else None, p(X) if want_points else None)
        assert rc == 0
        return bytes(R), m, X
    full, m, X = call(True, True)
    assert full == call(False, False)[0]
    r1, m1, X1 = call(True, False)
    assert r1 == full and np.array_equal(m1, m) and (X1 == 7).all()
    r2, m2, X2 = call(False, True)
    assert r2 == full and X2.tobytes() == X.tobytes() and (m2 == 7).all()
    g = gpu_ctx.mono_init(b1, b2, S, P)
    assert np.array_equal(g[1], m) and g[2].tobytes() == X.tobytes() and g[0]["status"] == 0


def test_degenerate_bearings(vio, gpu_ctx):
    """An all-zero pair and a NaN pair among the bearings.  Every loop on these paths is bounded (50
    Jacobi sweeps, fixed bitonic passes) and no index derives from bearing data.  By Initializer.cpp the
    NaN pair fails every comparison: out of the mask, zero point.  The zero pair's error is exactly 0,
    which IS < ransac_threshold (:551-557), so the reference keeps it in the mask; its mid-point fails
    (det = 0, :760-763), stays zero and is skipped by :916, so it counts nowhere."""
    b1, b2, *_ = init_cases.make_case(n=300, seed=21, noise_deg=0.02)
    S = vio.mono_init_samples(21, 300, 20)
    free = sorted(set(range(300)) - set(S.ravel().tolist()))
    iz, inan = free[0], free[1]
    b1[iz] = b2[iz] = 0.0
    b1[inan] = b2[inan] = np.nan
    P = vio.abi.mono_init_params(ransac_iterations=20, ransac_threshold=0.01)
    S2 = S.copy()
    S2[0, 0] = iz   # a zero row in one 8-point system
    for samples in (S, S2):
        gr, gm, gX = gpu_ctx.mono_init(b1, b2, samples, P)
        orr, om, oX = oracle_lib.mono_init(vio, b1, b2, samples, P)
        for k in ("status", "best_hypothesis", "num_inliers", "pose_candidate", "candidate_good",
                  "num_triangulated", "num_valid"):
            assert gr[k] == orr[k], (k, gr[k], orr[k])
        np.testing.assert_array_equal(gm, om)
        assert gr["status"] == vio.abi.VIO_INIT_OK
        assert gm[inan] == 0 and not gX[inan].any() and not gX[iz].any()
        assert gm[iz] == 1 and gr["num_valid"] <= gr["num_inliers"] - 1 and gr["num_triangulated"] == 298
        assert np.isfinite(gX).all()
        for k in ("E", "R", "t", "scale_factor", "mean_reproj_error"):
            assert np.isfinite(gr[k]).all(), k
