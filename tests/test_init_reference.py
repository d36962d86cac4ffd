"""CPU checks of the monocular initialiser against an independent f64 two-view reference.

tests/mono_init_reference.py restates Initializer.cpp:458-1048 in numpy float64 (np.linalg.svd of the
f32-built systems themselves, no code shared with oracle/init_oracle.c or the kernels).  Here the
reference is first checked against truth on noise-free cases, then oracle/init_oracle.c is held to
check_against_reference() over init_cases.REFERENCE_CASES at 960x480 and 3840x1920, and to the edges
where a threshold, a tie or a convention decides.  tests/test_init_gpu.py holds the device to the same
checker.  What this pins: the exact null vector of the f32-built system, and every threshold, comparison
and convention of Initializer.cpp.  What it does not: bit parity with Eigen's f32 JacobiSVD."""
import functools

import numpy as np
import pytest

import init_cases
import mono_init_reference as M
import oracle_lib

_ransac = {}


def ransac_of(vio, case):
    """ransac_reference() of a case: independent of the resolution, computed once, never modified."""
    if case not in _ransac:
        b1, b2, S, P, _ = init_cases.reference_case(vio, case)
        _ransac[case] = M.ransac_reference(b1, b2, S, P.ransac_threshold)
    return _ransac[case]


def case_id(case):
    return "seed%d-n%d-thr%g" % (case[0], case[3], case[4])


@pytest.mark.parametrize("case", [c for c in init_cases.REFERENCE_CASES if c[1] == 0.0], ids=case_id)
def test_reference_recovers_truth(vio, case):
    """Noise-free: the only error is the f32 rounding of the bearings, <= 2^-24 sqrt(3) ~ 1e-7 rad each.
    R and the direction of t to 10x that (100x for t: eight points at a 0.3 m baseline see the direction
    of t through the parallax, ~0.03 rad); a depth's relative error is the angular error over
    sin(parallax), so rel * sin(theta) <= 1e-6."""
    b1, b2, S, P, (R, t, P1) = init_cases.reference_case(vio, case)
    own = M.reference_run(b1, b2, S, P, ransac=ransac_of(vio, case))
    assert own["status"] == M.OK and own["best"] == 0 and own["num_inliers"] == len(b1)
    assert np.abs(own["R"] - R).max() <= 1e-6
    assert np.linalg.norm(own["t_unit"] - t / np.linalg.norm(t)) <= 1e-5
    Et = np.cross(np.eye(3), t / np.linalg.norm(t)) @ R   # [t]x R
    assert M._sign_gap(own["E"] / np.linalg.norm(own["E"]), Et / np.linalg.norm(Et)) <= 1e-5
    ref = P1 / np.median(np.linalg.norm(P1, axis=1))
    rel = np.linalg.norm(own["points"] - ref, axis=1) / np.linalg.norm(ref, axis=1)
    assert (rel * np.sqrt(np.abs(own["terms"]["det"]))).max() <= 1e-6
    assert own["num_valid"] == len(b1) and own["mean_reproj_error"] <= 1e-3
    assert sorted(own["candidate_good"])[-2] < len(b1)


def test_constants_are_measured(vio):
    """K_MIDPOINT and PIX_BAND_960 come from the f32 helpers over every case, not from the code under test."""
    kmax = pmax = 0.0
    for case in init_cases.REFERENCE_CASES:
        for W, H in init_cases.RESOLUTIONS:
            b1, b2, S, P, _ = init_cases.reference_case(vio, case, W, H)
            own = M.reference_run(b1, b2, S, P, ransac=ransac_of(vio, case))
            if "R" in own:
                k, p = M.measure_constants(b1, b2, own, W, H)
                kmax, pmax = max(kmax, k), max(pmax, p)
    print("measured K ratio %.2f, pixel deviation %.5f px per 960" % (kmax, pmax))
    assert 0.9 * M.MEASURED_K_RATIO <= kmax <= M.MEASURED_K_RATIO
    assert 0.9 * M.MEASURED_PIX_960 <= pmax <= M.MEASURED_PIX_960
    assert M.K_MIDPOINT == 2.0 ** np.ceil(np.log2(2 * M.MEASURED_K_RATIO))
    assert M.PIX_BAND_960 == 4 * M.MEASURED_PIX_960


@pytest.mark.parametrize("res", init_cases.RESOLUTIONS, ids=lambda r: "w%d" % r[0])
@pytest.mark.parametrize("case", init_cases.REFERENCE_CASES, ids=case_id)
def test_oracle_against_reference(vio, case, res):
    b1, b2, S, P, _ = init_cases.reference_case(vio, case, *res)
    rr = ransac_of(vio, case)
    own = M.reference_run(b1, b2, S, P, ransac=rr)
    assert own["status"] == init_cases.EXPECTED_STATUS.get((case[0], case[3], res[0]), M.OK), own["status"]
    run = functools.partial(oracle_lib.mono_init, vio)
    fig = M.check_against_reference(run, b1, b2, S, P, ransac=rr)
    print(case, res, fig)
    assert run(b1, b2, S, P)[0]["status"] == own["status"]


def test_seam_points_are_not_wrapped(vio):
    """The seam case has mid-points that project across +-pi from their observation, by more than the
    seam band: the reference's error there is a whole image width (:866-870 has no wrap-around), so they
    are decided failures of both pixel tests."""
    case = [c for c in init_cases.REFERENCE_CASES if c[5]][0]
    b1, b2, S, P, _ = init_cases.reference_case(vio, case)
    own = M.reference_run(b1, b2, S, P, ransac=ransac_of(vio, case))
    T = own["terms"]
    crossed = ~T["fuzzy"] & (T["er"] > 0.9 * P.width)
    assert crossed[: case[5]].sum() >= 4 and not crossed[case[5]:].any()
    lo, hi, _, _ = M.count_bounds(T, own["mask"], 5.0, M.pix_band(P.width))
    assert hi <= len(b1) - crossed.sum()
    o = oracle_lib.mono_init(vio, b1, b2, S, P)[0]
    assert lo <= o["num_valid"] <= hi and o["num_valid"] == max(o["candidate_good"])


def test_first_strictly_best(vio):
    """:568 `num_inliers > best_inliers`: of two equal rows the earlier wins; all rows tie -> row 0."""
    case = init_cases.REFERENCE_CASES[2]
    b1, b2, S, P, _ = init_cases.reference_case(vio, case)
    rr = ransac_of(vio, case)
    assert rr["winner_decided"] and rr["best"] > 40
    S2 = S.copy()
    p, q = 17, 40
    S2[p] = S2[q] = S[rr["best"]]
    r2 = M.ransac_reference(b1, b2, S2, P.ransac_threshold)
    assert r2["best"] == p and r2["winner_decided"]
    assert oracle_lib.mono_init(vio, b1, b2, S2, P)[0]["best_hypothesis"] == p
    b1, b2, S, P, _ = init_cases.reference_case(vio, init_cases.REFERENCE_CASES[0])
    rr = ransac_of(vio, init_cases.REFERENCE_CASES[0])
    assert (rr["lo"] == len(b1)).all() and rr["best"] == 0
    assert oracle_lib.mono_init(vio, b1, b2, S, P)[0]["best_hypothesis"] == 0


def test_threshold_is_strict(vio):
    """:554 `error < m_ransac_threshold`: at threshold 0 nothing is an inlier, not even a pair whose
    error is exactly 0 (an all-zero pair), so no hypothesis qualifies."""
    b1, b2, S, P, _ = init_cases.reference_case(vio, init_cases.REFERENCE_CASES[0], iters=20)
    b1, b2 = b1.copy(), b2.copy()
    b1[5] = b2[5] = 0.0
    S = S[~(S == 5).any(1)]
    P = M.with_params(P, ransac_threshold=0.0, ransac_iterations=len(S))
    rr = M.ransac_reference(b1, b2, S, 0.0)
    assert rr["best"] == -1 and (rr["err"][:, 5] == 0.0).all()
    o, m, X = oracle_lib.mono_init(vio, b1, b2, S, P)
    assert o["status"] == M.ESSENTIAL_FAILED and o["best_hypothesis"] == -1 and o["num_inliers"] == 0
    assert not m.any() and not X.any()


@pytest.mark.parametrize("n,seed", [(8, 31), (9, 32), (10, 30), (11, 32)])
def test_median_even_and_odd(vio, n, seed):
    """:1026-1033 on the smallest counts, where the two middle depths are far apart: the bracket of
    check_against_reference (g) separates the mean of the two from either of them."""
    b1, b2, *_ = init_cases.make_case(n=n, seed=seed, noise_deg=0.0)
    S = vio.mono_init_samples(seed, n, 8)
    P = vio.abi.mono_init_params(min_features=4, ransac_iterations=8, ransac_threshold=0.01)
    own = M.reference_run(b1, b2, S, P)
    assert own["status"] == M.OK
    d = np.sort(np.linalg.norm(own["terms"]["X"], axis=1))
    lo, hi = M.scale_bounds(own["terms"]["X"], own["terms"]["det"])
    if n % 2 == 0:   # neither middle value alone lies in the bracket
        assert not lo <= d[n // 2] <= hi and not lo <= d[n // 2 - 1] <= hi
    else:            # nor the mean with a neighbour
        assert not lo <= 0.5 * (d[n // 2] + d[n // 2 - 1]) <= hi
        assert not lo <= 0.5 * (d[n // 2] + d[n // 2 + 1]) <= hi
    M.check_against_reference(functools.partial(oracle_lib.mono_init, vio), b1, b2, S, P)
