"""The device's inertial factor against tests/inertial_factor_reference.py: the three device
implementations (the serial imu_eval, the lane-parallel imu_eval_wave and imu_sqrt_info_wave) through
vio_imu_factor_eval on every case of tests/inertial_factor_cases.py in one launch, and iteration 0 of the
real solvers (the three window routes and the global path) on the two VIBA windows.  Bars as in
tests/test_inertial_factor.py: per case and block 16 x the float64 reference's own rounding plus
64 eps max|block|; nothing here is compared with the C oracle."""
import numpy as np
import pytest

import inertial_factor_cases as ic
import inertial_factor_reference as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def device_out(gpu_ctx, synth):
    return gpu_ctx.imu_factor_eval(ic.cases(synth))


@pytest.mark.parametrize("flavour", ["serial", "wave"])
def test_device_factor_matches_reference(synth, device_out, flavour):
    """sqrt_info (imu_sqrt_info_wave: pivot swap, LLT fallback, zero and ill-scaled covariances), r and
    the Jacobian blocks of imu_eval / imu_eval_wave against evaluate_mp on every case."""
    res = device_out if flavour == "serial" else dict(device_out, r=device_out["r_wave"], J=device_out["J_wave"])
    off, worst = [], {b: 0.0 for b in ref.BLOCKS}
    for f, (c, m, bars) in enumerate(ic.expected(synth)):
        got = ic.split(res, f)
        for b in ref.BLOCKS:
            err = ref.absdiff(got[b], m[b]).max()
            worst[b] = max(worst[b], err / bars[b])
            if not err <= bars[b]:
                off.append((c["name"], b, err, bars[b]))
        if c["name"] == "cov_not_pd":
            assert np.array_equal(got["sqrt_info"], np.eye(9))
    print(flavour, "largest error / bar per block:", {b: round(v, 3) for b, v in worst.items()})
    assert not off, (sorted({o[0] + '/' + o[1] for o in off}), off[:3])


def test_serial_and_wave_agree(synth, device_out):
    """imu_eval_wave against imu_eval directly, at the reference's bar.  They are not bit-identical: on an
    MI355X 14 of the 42 cases differ, only in rows 0-2 of J_bg (-S Jr(-er)^-1 J_Rg), by 1 ulp typically and
    332 ulps (4e-14 relative) at most; the same source operations, compiled separately, are not contracted
    to the same multiply-adds.  The residual and every other Jacobian entry were bit-identical."""
    wave = dict(device_out, r=device_out["r_wave"], J=device_out["J_wave"])
    off, differ = [], 0
    for f, (c, m, bars) in enumerate(ic.expected(synth)):
        a, b = ic.split(device_out, f), ic.split(wave, f)
        differ += any(not np.array_equal(a[k], b[k]) for k in ref.BLOCKS)
        off += [(c["name"], k, np.abs(a[k] - b[k]).max(), bars[k]) for k in ref.BLOCKS
                if not np.abs(a[k] - b[k]).max() <= bars[k]]
    print("cases whose serial and wave outputs differ bitwise:", differ)
    assert not off, (sorted({o[0] + '/' + o[1] for o in off}), off[:3])


def _check_iter0(synth, name, g, label):
    m, bars = ic.window_expected(synth, name)
    assert g["iterations"] >= 1 and len(g["trace"]["gradient_max_norm"]) >= 1
    got = {"initial_cost": g["initial_cost"], "fixed_cost": g["fixed_cost"],
           "gradient_max_norm": g["trace"]["gradient_max_norm"][0]}
    for q, bar in bars.items():
        err = float(ref.absdiff(got[q], m[q]))
        print(f"{name} {label} {q}: value {float(m[q]):.6e} error {err:.2e} bar {bar:.2e}")
        assert err <= bar, (label, q, got[q], float(m[q]), err, bar)


@pytest.mark.parametrize("route", ["ROUTE_PHASES", "ROUTE_SINGLE_KERNEL", "ROUTE_CLUSTER"])
def test_window_iteration0(vio, synth, gpu_ctx, route):
    """initial_cost, fixed_cost and trace[0].gradient_max_norm of the (3, 12) window, whose shared gyro bias
    starts 1e-3 off the preintegrations' (the correction is live at the first linearisation), on every
    window route, against window_iter0."""
    w = ic.windows(synth)["k3_l12_bias"]
    p = vio.BaProblem(w, variant=vio.VIO_BA_VI, max_iterations=1, fixed_iterations=1)
    gpu_ctx.set_ba_route(getattr(gpu_ctx, route))
    try:
        g = gpu_ctx.ba_solve([p])[0]
    finally:
        gpu_ctx.set_ba_route(gpu_ctx.ROUTE_AUTO)
    _check_iter0(synth, "k3_l12_bias", g, route)


def test_global_iteration0(vio, synth, gpu_ctx):
    """The same on the global path: 12 keyframes with the factor 5 -> 6 missing (preint_valid[6] = 0)."""
    w = ic.windows(synth)["k12_l24_gap"]
    p = vio.BaProblem(w, variant=vio.VIO_BA_VI, max_iterations=1, fixed_iterations=1)
    assert p.preint_valid[6] == 0 and p.preint_valid[1:].sum() == 10
    _check_iter0(synth, "k12_l24_gap", gpu_ctx.ba_solve([p])[0], "global")
