"""CPU: the independent preintegration reference (tests/imu_preint_reference.py) checked against
closed forms, and oracle/imu_oracle.c checked against its f64 mode on every case of
tests/imu_preint_cases.py — field by field, interval by interval.

`valid` and `dt_total` must be exact (dt_total is an f64 sum of the same f32 steps in the same
order).  Every other field must lie within
    bound = 4·floor + 4·2⁻²⁴·max|ref_f64 field|,   floor = max|ref_f32 − ref_f64|
per case, field and interval: the floor is what a faithful f32 evaluation of the reference's
expressions loses against the truth, measured on the reference alone; the factor 4 covers the
association order of the 3x3 products (Eigen's, numpy's and the kernel's differ); the second term
keeps an exactly-zero floor from demanding bitwise equality.

Largest error / bound of the C oracle against the f64 reference, per case and field (a ratio above
1 is a failure to investigate, not a tolerance to widen):

    case        ΔR     ΔV     ΔP     J_Rg   J_Vg   J_Va   J_Pg   J_Pa   cov9   cov_bias
    tame        0.219  0.200  0.192  0.249  0.248  0.217  0.248  0.181  0.160  0.217
    aggressive  0.336  0.414  0.321  0.241  0.324  0.429  0.342  0.332  0.399  0.196
    long        0.328  0.517  0.378  0.246  0.276  0.298  0.286  0.269  0.254  0.249
    threshold   0.006  0.191  0.195  0.230  0.213  0.217  0.213  0.030  0.054  0.217
    big_bias    0.330  0.535  0.263  0.247  0.248  0.468  0.231  0.306  0.367  0.217
    noise       0.329  0.288  0.279  0.241  0.227  0.199  0.225  0.192  0.210  0.163
    ranges      0.381  0.445  0.360  0.249  0.248  0.310  0.315  0.503  0.526  0.189

The HIP kernel is bitwise the oracle on every case (tests/test_imu_gpu.py), so these are its ratios
too; they were also measured on the device directly and came out the same.

Hand mutations of imu_oracle.c against test_oracle_matches_f64_reference: the sign of the
(θ − sin θ)/θ·K² term of the right Jacobian flipped fails 5 of 7 cases (J_Rg up to 1100 × bound);
J_Pa accumulated with the old J_Va fails all 7 (J_Pg 1e3-2e5 × bound); dropping the NaN range rule
fails `ranges` on valid.  Using the old ΔR in the covariance's B passes, and has to: Nga is
σ²·I, so B·Nga·Bᵀ = σ²·dt²·ΔR·ΔRᵀ = σ²·dt²·I whichever rotation is used — the covariance does not
depend on ΔR above rounding.

The f32 mode itself is held to the f64 mode on `tame` by a bound from rounding analysis, not from
its own output (test_f32_mode_tracks_f64_mode_on_tame).
"""
import numpy as np
import pytest

import imu_preint_cases as cases
import imu_preint_reference as ref
import oracle_lib

EPS32 = 2.0 ** -24


def _rodrigues_unit_axis(w):
    """Textbook Exp: I + sin θ·K + (1 − cos θ)·K², K the unit-axis skew matrix (f64)."""
    w = np.asarray(w, np.float64)
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def _const_stream(acc, gyr, n=51, rate=200.0):
    s = np.zeros((n, 7))
    s[:, 0] = np.arange(n) / rate
    s[:, 1:4] = acc
    s[:, 4:7] = gyr
    return s


# ---------------------------------------------------------------- reference self-checks
@pytest.mark.parametrize("w", [(0.1, -0.3, 0.8), (12.0, -20.0, 9.0), (2e-3, 1e-3, -1e-3), (1e-5, -2e-5, 5e-6),
                               (0.0, 0.0, 0.0)])
def test_f64_constant_rotation_closed_form(w):
    w = np.array(w, np.float32).astype(np.float64)
    r = ref.preintegrate_one(_const_stream((0, 0, 0), w), 0.0, 0.25)
    assert r["steps"] == 50
    T = r["dt_total"]
    assert abs(T - 50 * float(np.float32(0.005))) < 1e-12
    assert np.abs(r["delta_R"] - _rodrigues_unit_axis(w * T)).max() <= 1e-12
    assert not r["delta_V"].any() and not r["delta_P"].any()


def test_f64_exp_and_right_jacobian():
    rng = np.random.default_rng(0)
    for th in (0.0, 3e-7, 5e-5, 0.99e-4, 1.01e-4, 1e-3, 0.3, 2.0, 3.1):
        u = rng.normal(size=3)
        w = th * u / np.linalg.norm(u)
        R, Jr = ref.exp_jr64(w)
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-15 and abs(np.linalg.det(R) - 1) < 1e-15
        assert np.abs(R - _rodrigues_unit_axis(w)).max() < 1e-15
        # Exp(w + δ) = Exp(w)·Exp(Jr·δ) + O(δ²)
        for k in range(3):
            d = np.zeros(3)
            d[k] = 1e-6
            lhs = ref.exp_jr64(w + d)[0]
            rhs = R @ ref.exp_jr64(Jr @ d)[0]
            assert np.abs(lhs - rhs).max() < 5e-12, (th, k)


def test_f64_constant_acceleration_closed_form():
    a = np.array([0.3, -0.2, 9.81], np.float32).astype(np.float64)
    r = ref.preintegrate_one(_const_stream(a, (0, 0, 0)), 0.0, 0.25)
    n, dt = 50, float(np.float32(0.005))
    T = r["dt_total"]
    assert np.array_equal(r["delta_R"], np.eye(3))
    np.testing.assert_allclose(r["delta_V"], a * T, rtol=1e-12)
    np.testing.assert_allclose(r["delta_P"], 0.5 * a * T * T, rtol=1e-12)
    np.testing.assert_allclose(r["J_Va"], np.eye(3) * T, rtol=1e-12, atol=0)
    # J_Pa accumulates the updated J_Va: Σ_k (k·dt² + ½dt²) = ½T² + T·dt
    np.testing.assert_allclose(r["J_Pa"], np.eye(3) * (0.5 * T * T + T * dt), rtol=1e-12, atol=0)
    np.testing.assert_allclose(r["J_Rg"], -np.eye(3) * dt, rtol=1e-15, atol=0)
    c = r["cov9"]
    assert not c[:3].any() and not c[:, :3].any()
    sa2 = float(np.float32(1e-3) * np.float32(1e-3))
    np.testing.assert_allclose(np.diag(c)[3:6], n * sa2 * dt * dt, rtol=1e-12)
    # ΔR = I: J_Vg = Σ J_Va_old·[a]×·(−dt) = −[a]×·dt²·n(n−1)/2
    ax = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    np.testing.assert_allclose(r["J_Vg"], -ax * dt * dt * n * (n - 1) / 2, rtol=1e-12, atol=1e-18)
    sg2, sb2 = (float(np.float32(x) * np.float32(x)) for x in (1e-6, 1e-5))  # float products, as m_*·m_*
    np.testing.assert_allclose(r["cov_bias"], np.r_[[sg2 * T] * 3, [sb2 * T] * 3], rtol=1e-12)


def test_range_and_dt_rules_of_the_reference():
    s = _const_stream((0, 0, 9.81), (0.1, 0, 0), n=5)
    s[:, 0] = [0.0, 0.0001, 0.1, 0.105, 0.105]
    c = lambda x: float(np.float32(x))  # noqa: E731
    assert ref.preintegrate_one(s, 0.0, 0.2)["dt_total"] == c(0.0005) + c(0.0005) + c(0.02) + c(0.005) + c(0.0005)
    assert ref.preintegrate_one(s, 0.1, 0.101)["dt_total"] == c(0.002)
    assert ref.preintegrate_one(s, 0.0, 0.1)["steps"] == 2
    for t0, t1 in ((0.2, 0.3), (0.105, 0.105), (0.1, 0.0), (float("nan"), 1.0), (0.0, float("nan")),
                   (float("inf"), float("inf")), (0.0, float("-inf"))):
        assert ref.preintegrate_one(s, t0, t1) is None
    assert ref.preintegrate_one(s, float("-inf"), float("inf"))["steps"] == 5
    assert ref.preintegrate_one(np.zeros((0, 7)), 0.0, 1.0) is None


def test_f32_mode_tracks_f64_mode_on_tame(synth):
    """Bound by reasoning.  An n-step chain of f32 updates, each a handful of roundings relative to the
    field's size, drifts at most 8·n·2⁻²⁴ relative to the largest entry.  The gyro-bias Jacobians
    add the reference's own cancellation: 1 − cos θ in f32 is off by up to 2⁻²⁵, so (1 − cos θ)/θ is
    off by 2⁻²⁵/θ per unit-skew entry of Jr; it enters J_Rg = −dRᵀ·Jr·dt, and through it J_Vg and
    J_Pg, at that relative size (factor 4 for the three-term row sums and max-entry vs norm)."""
    p = cases.case("tame", synth)[0]
    r64, r32 = cases.reference("tame", synth, "f64")[0], cases.reference("tame", synth, "f32")[0]
    assert r64["valid"].all() and np.array_equal(r64["valid"], r32["valid"])
    assert np.array_equal(r64["dt_total"], r32["dt_total"])
    g = p["samples"][:, 4:7].astype(np.float32)
    th_min = np.linalg.norm(g, axis=1).min() * 0.005 * 0.99
    assert th_min > 5e-4
    for k in ref.FIELDS:
        for i in range(len(p["t0"])):
            n = r64["steps"][i]
            tol = 8 * n * EPS32 + (4 * 2.0 ** -25 / th_min if k in ("J_Rg", "J_Vg", "J_Pg") else 0.0)
            err = np.abs(r32[k][i] - r64[k][i]).max()
            assert err <= tol * np.abs(r64[k][i]).max(), (k, i, err / np.abs(r64[k][i]).max(), tol)


def test_threshold_case_alternates_branches(synth):
    small, th = cases.threshold_branches(cases.case("threshold", synth)[0])
    assert th.min() > 3e-7 and th.max() < 3e-6
    assert (small[:, 1:] != small[:, :-1]).all()  # from sample to sample inside one interval
    assert (small[1:] != small[:-1]).all()        # neighbouring intervals at the same step
    assert np.abs(th / 1e-6 - 1).min() > 0.3      # no step close enough for a rounding to pick the branch


def test_aggressive_and_long_cases_are_what_they_claim(synth):
    a = cases.case("aggressive", synth)
    assert [round(np.abs(p["samples"][:, 4:7]).max()) for p in a] == [10, 35]
    assert all(np.abs(p["samples"][:, 1:4]).max() > 140 for p in a)
    r = cases.reference("long", synth, "f64")
    assert [int(x["steps"][0]) for x in r] == [400, 1000, 50]
    assert r[2]["dt_total"][0] == 50 * float(np.float32(0.02))
    g = cases.case("long", synth)[0]["samples"][:400, 4:7]
    assert np.linalg.norm(g.mean(0)) * 2.0 > 1.5 * np.pi  # the mean rate alone turns well past π in 2 s


def test_ranges_case_expected_valid(synth):
    parts = cases.case("ranges", synth)
    r = cases.reference("ranges", synth, "f64")
    assert r[0]["valid"].tolist() == [1, 1, 1, 0, 1, 0, 0, 0, 0, 1, 1, 1]
    assert r[0]["steps"].tolist() == [15, 39, 40, 0, 1, 0, 0, 0, 0, 1, 2, 1]
    # non-finite bounds: kept iff t0 ∈ {0.05, −inf} and t1 ∈ {0.15, +inf}; any NaN keeps nothing
    p = parts[1]
    exp = [int((a == 0.05 or a == -np.inf) and (b == 0.15 or b == np.inf)) for a, b in zip(p["t0"], p["t1"])]
    assert len(exp) == 15 and sum(exp) == 3 and r[1]["valid"].tolist() == exp
    assert r[2]["valid"].tolist() == [1, 1, 1, 1, 0, 0] and r[2]["steps"].tolist() == [3, 2, 12, 4, 0, 0]
    assert r[3]["valid"].tolist() == [1, 0, 1, 0, 0, 0, 1, 0]
    assert [len(q["t0"]) for q in parts[4:]] == [1, 6, 7, 8, 13, 14, 15]


# ---------------------------------------------------------------- the C oracle against the f64 reference
def _oracle(vio, synth, name):
    return [oracle_lib.imu_preintegrate(vio, p["samples"], p["t0"], p["t1"], p["bg"], p["ba"], p["noise"])
            for p in cases.case(name, synth)]


@pytest.mark.parametrize("name", cases.NAMES)
def test_oracle_matches_f64_reference(vio, synth, name):
    got = _oracle(vio, synth, name)
    r64 = cases.reference(name, synth, "f64")
    rat = cases.ratios(got, name, synth)
    worst = {k: max((float(d[k].max()) for d in rat if len(d[k])), default=0.0) for k in ref.FIELDS}
    print(name, " ".join(f"{k}={v:.3f}" for k, v in worst.items()))
    for pi, ((rec, valid, _), r, d) in enumerate(zip(got, r64, rat)):
        assert np.array_equal(valid, r["valid"]), (name, pi, valid.tolist(), r["valid"].tolist())
        assert np.array_equal(rec["dt_total"], r["dt_total"]), (name, pi)
        for k in ref.FIELDS:
            assert (d[k] <= 1.0).all(), (name, pi, k, int(d[k].argmax()), float(d[k].max()))


@pytest.mark.parametrize("name", cases.NAMES)
def test_oracle_covariance_properties(vio, synth, name):
    got = _oracle(vio, synth, name)
    for (rec, valid, _), b in zip(got, cases.bounds(name, synth)):
        for i in range(len(valid)):
            c = rec["cov9"][i].astype(np.float64)
            assert not c[:3].any() and not c[:, :3].any()  # B has no gyro columns: rotation rows stay zero
            assert np.abs(c - c.T).max() <= b["cov9"][i]
            assert np.linalg.eigvalsh(0.5 * (c + c.T)).min() >= -b["cov9"][i]
