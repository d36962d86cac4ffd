"""CPU checks of InertialFactorFixedGravity: the C oracle (oracle_imu_factor, and oracle_ba_solve's
iteration 0 on VIBA windows) against tests/inertial_factor_reference.py, a restatement written from the
reference source that shares no code with the oracle or the kernels.

Bars are never constants: per case and per output block 16 * max|evaluate - evaluate_mp| (the float64
reference's own rounding on that input, so an ill-conditioned case gets the bar its conditioning earns)
plus the floor 64 * eps * max|block| (inertial_factor_cases.expected).  The factor of 16 leaves room for
another summation order and FMA contraction; test_mutants_are_caught shows that it stays far below every
one-line deviation of inertial_factor_reference.MUTANTS."""
import numpy as np
import pytest

import inertial_factor_cases as ic
import inertial_factor_reference as ref
import oracle_lib

@pytest.fixture(scope="module")
def oracle_out(vio, synth):
    return oracle_lib.imu_factor(vio, ic.cases(synth))


def test_case_table_conditions(synth):
    """The table holds what its docstring promises (asserted on the reference alone while it is built):
    about 40 uniquely named cases, every listed edge present."""
    table = ic.cases(synth)
    assert 38 <= len(table) <= 48
    ic.check_conditions(table)
    dts = sorted({round(float(c["preint"]["dt_total"]), 2) for c in table})
    assert dts[0] <= 0.06 and dts[-1] >= 0.99, dts
    assert any(not np.any(c["delta_i"]) and not np.any(c["delta_j"]) for c in table)
    assert sum(ref.evaluate(c)["diag"]["corrected"] for c in table) >= 10
    # every case sits on the first admitted draw of its stream (the module docstring's DRAW)
    for name, build in ic._builders():
        first = next(d for d in range(ic.DRAW.get(name, 0) + 1) if ic.admission(ic.build_case(synth, name, build, d))[1])
        assert first == ic.DRAW.get(name, 0), (name, first)


def test_oracle_matches_reference(vio, synth, oracle_out):
    """sqrt_info, r and the four non-zero Jacobian blocks of oracle_imu_factor against evaluate_mp for
    every case; S == I exactly where the information matrix is not positive definite.  (The oracle,
    like the kernels, does not produce the two pose blocks: the reference writes zeros there.)"""
    off, realised = [], {b: [] for b in ref.BLOCKS}
    for f, (c, m, bars) in enumerate(ic.expected(synth)):
        assert not np.any(m["J_pose_i"]) and not np.any(m["J_pose_j"]) and m["J_pose_i"].shape == (9, 6)
        got = ic.split(oracle_out, f)
        for b in ref.BLOCKS:
            err = ref.absdiff(got[b], m[b]).max()
            realised[b].append(bars[b])
            if not err <= bars[b]:
                off.append((c["name"], b, err, bars[b]))
        if c["name"] == "cov_not_pd":
            assert np.array_equal(got["sqrt_info"], np.eye(9))
    for b in ref.BLOCKS:
        print(f"bar {b}: {min(realised[b]):.2e} .. {max(realised[b]):.2e}")
    assert not off, (sorted({o[0] + '/' + o[1] for o in off}), off[:3])


def test_jacobians_by_finite_differences(synth):
    """Central differences of the reference's own residual confirm the blocks that are derivatives: J_ba
    and rows 3-8 of J_bg, on the cases whose bias correction is live and stays live under the step (the
    largest of |dbg|, |dba| is at least 20 steps), where the residual is linear in both biases apart from
    the rotation rows.

    Not derivatives, and therefore checked against the formula only (test_oracle_matches_reference): rows
    0-2 of J_bg, which use right_jacobian(-er)^-1 of the already weighted er; J_vi and J_vj, which apply
    the diagonal blocks of S alone and differ from d r / d v whenever S has off-diagonal blocks; every
    bias block of a case below the 1e-6 threshold, where the residual ignores the biases altogether.

    Tolerance: a central difference of a linear function errs by the rounding of its two residuals only,
    2 * err(r) / (2 h) with err(r) = max|evaluate - evaluate_mp| on that case (at least eps * max|r|);
    4 x that."""
    h, n = 1e-6, 0
    for c, m, bars in ic.expected(synth):
        p = c["preint"]
        live = max(np.linalg.norm(c["bg"] - np.asarray(p["gyro_bias"], np.float64)),
                   np.linalg.norm(c["ba"] - np.asarray(p["accel_bias"], np.float64)))
        if live < 20 * h:
            continue
        n += 1
        e = ref.evaluate(c)
        err_r = max(ref.absdiff(e["r"], m["r"]).max(), ic.EPS * np.abs(e["r"]).max())
        tol = 4.0 * err_r / h
        for key, block, rows in (("ba", "J_ba", slice(0, 9)), ("bg", "J_bg", slice(3, 9))):
            fd = np.zeros((9, 3))
            for j in range(3):
                cp, cm = dict(c), dict(c)
                cp[key], cm[key] = c[key].copy(), c[key].copy()
                cp[key][j] += h
                cm[key][j] -= h
                fd[:, j] = (ref.residual(cp) - ref.residual(cm)) / (cp[key][j] - cm[key][j])
            d = np.abs(fd[rows] - e[block][rows]).max()
            assert d <= tol, (c["name"], block, d, tol)
    assert n >= 10, n


def test_mutants_are_caught(vio, synth, oracle_out):
    """Each one-line deviation of inertial_factor_reference.MUTANTS is told from the oracle by at least one
    case at 10 x the bar or more: the table is strong enough for every quirk, and the bar is not loose."""
    table = ic.expected(synth)
    missed = []
    for mut in ref.MUTANTS:
        best = (0.0, None, None)
        for f, (c, m, bars) in enumerate(table):
            got, e = ic.split(oracle_out, f), ref.evaluate(c, mutant=mut)
            for b in ref.BLOCKS:
                ratio = np.abs(np.asarray(e[b], np.float64) - got[b]).max() / bars[b]
                if ratio > best[0]:
                    best = (ratio, c["name"], b)
        print(f"mutant {mut}: {best[0]:.3g} x bar at {best[1]} / {best[2]}")
        if not best[0] >= 10.0:
            missed.append((mut,) + best)
    assert not missed, missed


@pytest.mark.parametrize("name", ["k3_l12_bias", "k12_l24_gap"])
def test_oracle_iteration0_on_windows(vio, synth, name):
    """initial_cost, fixed_cost and trace[0].gradient_max_norm of oracle_ba_solve on the two VIBA windows
    against window_iter0: the k-1 -> k indexing, the preint_valid gap, the shared-bias and velocity
    slots, gravity and the constant first keyframe, none of which a single factor can show."""
    w = ic.windows(synth)[name]
    m, bars = ic.window_expected(synth, name)
    o = oracle_lib.ba_solve(vio, vio.BaProblem(w, variant=vio.VIO_BA_VI, max_iterations=1, fixed_iterations=1))
    got = {"initial_cost": o["initial_cost"], "fixed_cost": o["fixed_cost"],
           "gradient_max_norm": o["trace"]["gradient_max_norm"][0]}
    for q, bar in bars.items():
        err = float(ref.absdiff(got[q], m[q]))
        print(f"{name} {q}: value {float(m[q]):.6e} error {err:.2e} bar {bar:.2e}")
        assert err <= bar, (q, got[q], float(m[q]), err, bar)
