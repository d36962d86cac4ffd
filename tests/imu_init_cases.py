"""IMU-initialisation cases shared by the CPU tests (oracle against tests/imu_init_reference.py) and the
GPU parity tests of tests/test_imu_init.py.  `build(synth, name)` returns (name, frames, kwargs): frames
for abi.ImuInitProblem, kwargs its keyword arguments (and the reference cost's).  Finite inputs only.

Windows are synth.make_window(K=F, L=20, seed=SEED + F, imu=True) (the landmarks are unused).  One wave
of 64 lanes solves a problem, so the stage-2 width n2 = 3 * (touched frames) + 6 decides how many trips
the kernel's `j = t; j < n2; j += 64` loops take; m2 = 9 * (kept factors) + 6 rows.

TABLE columns: n2, m2, then the relative cost drop (c0 - c1) / c0 that imu_init_reference.polish
reaches from the CPU oracle's answer in stage 1 and in stage 2, measured once on the CPU (None: that
stage does not end with termination 0 = convergence, so nothing is claimed about its end point).  The
stationarity test allows ten times the recorded drop (the margin is for the polisher's own stopping
noise across scipy / BLAS builds) plus the resolution of the cost itself, 1e-12 relative + 1e-20.
Drops of 1e-7 .. 1e-6 are Ceres's function_tolerance 1e-6 ending the solve a step early; the 1e-15
stage-1 drops of the plain windows are rounding (three parameters, converged quadratically).  On
the stationary cases the cost at the answer is 1e-16 .. 1e-15 (the float rounding of delta_V /
delta_P): stage 1 stops on the gradient tolerance, and stage 2 never leaves zero biases, where the
bias correction is off (|db| <= 1e-6) and velocities times scale ~ 1e-9 move nothing: a recorded
0.0 says the polisher found nothing lower either.
"""
import copy

import numpy as np

#  name            n2   m2   stage-1 drop  stage-2 drop
TABLE = {
    # column-loop trips: second trip with 2 / 5 / 8 / 14 live lanes, third (> 128), fourth (> 192)
    "win20":        (66, 177, 2.9e-15, 2.50e-07),
    "win21":        (69, 186, 3.0e-15, 2.35e-07),
    "win22":        (72, 195, 3.4e-15, 2.28e-07),
    "win24":        (78, 213, 5.0e-15, 2.38e-07),
    "win43":        (135, 384, 2.6e-15, 2.23e-07),
    "win64":        (198, 573, 1.9e-15, 2.11e-07),
    # Huber outer branch: three factors far past s = delta^2; long solves, radius moving both ways
    "huber24":      (78, 213, 1.58e-06, 3.85e-07),
    "huber24_d05":  (78, 213, 5.39e-07, 1.80e-06),
    "huber24_cap4": (78, 213, None, None),
    "win24_cap0":   (78, 213, None, None),
    # factors skipped inside the window (dt_total outside [0.001, 2.0])
    "skip_mid":     (75, 195, 3.3e-15, 5.34e-07),
    "skip_first":   (75, 204, 1.3e-14, 3.82e-07),
    "skip_last":    (75, 204, 6.5e-15, 2.29e-07),
    # non-zero linearisation biases, non-default parameters
    "lin_bias":     (78, 213, 1.50e-09, 3.18e-07),
    "gmag1":        (78, 213, 6.11e-07, 1.2e-12),
    "prior100":     (78, 213, 5.0e-15, 2.60e-07),
    "prior0":       (78, 213, 5.0e-15, 8.90e-09),
    # stationary, tilted by 0 (the small-angle branches) / 90 / 150 / 179 degrees
    "stat_tilt0":   (69, 186, 6.5e-14, 0.0),
    "stat_tilt90":  (69, 186, 4.94e-06, 0.0),
    "stat_tilt150": (69, 186, 1.32e-07, 0.0),
    "stat_tilt179": (69, 186, 6.56e-09, 0.0),
}
NAMES = list(TABLE)

_windows = {}


def window(synth, F):
    """The F-frame synthetic window (cached: treat as read-only, `build` hands out copies)."""
    if F not in _windows:
        w = synth.make_window(K=F, L=20, seed=synth.SEED + F, imu=True)
        _windows[F] = {"T_wb": w["T_wb_init"], "preint": w["preint"], "imu_samples": w["imu_samples"]}
    return _windows[F]


def frames_of(synth, F):
    w = window(synth, F)
    return {"T_wb": w["T_wb"].copy(), "preint": copy.deepcopy(w["preint"])}


def _huber(synth):
    fr = frames_of(synth, 24)
    for k, off in ((5, (8.0, -6.0, 5.0)), (11, (-20.0, 3.0, 9.0)), (17, (1.0, 30.0, -4.0))):
        fr["preint"][k]["delta_V"] = (fr["preint"][k]["delta_V"] + np.array(off, np.float32)).astype(np.float32)
    return fr


def _skip(synth, dts):
    fr = frames_of(synth, 24)
    for k, dt in dts.items():
        fr["preint"][k]["dt_total"] = dt
    return fr


def _lin_bias(synth):
    fr = frames_of(synth, 24)
    for p in fr["preint"][1:]:
        p["gyro_bias"] = np.array([0.01, -0.02, 0.005], np.float32)
        p["accel_bias"] = np.array([0.05, 0.1, -0.08], np.float32)
    return fr


def _stationary(deg):
    from test_imu_init import stationary_frames
    return stationary_frames(F=21, tilt_deg=deg, seed=3)[0]


def build(synth, name):
    if name.startswith("win") and "_" not in name:
        return name, frames_of(synth, int(name[3:])), {}
    if name.startswith("stat_tilt"):
        return name, _stationary(float(name[9:])), {}
    made = {
        "huber24": lambda: (_huber(synth), {}),
        "huber24_d05": lambda: (_huber(synth), {"huber_delta": 0.5}),
        "huber24_cap4": lambda: (_huber(synth), {"max_iterations": 4}),
        "win24_cap0": lambda: (frames_of(synth, 24), {"max_iterations": 0}),
        # frame 7 loses both its factors (its velocity stays vinit); frame 8's vinit is zero
        "skip_mid": lambda: (_skip(synth, {7: 2.5, 8: 0.0005}), {}),
        "skip_first": lambda: (_skip(synth, {1: 2.5}), {}),  # first appearance starts at frame 1
        "skip_last": lambda: (_skip(synth, {23: 2.5}), {}),
        "lin_bias": lambda: (_lin_bias(synth), {}),
        "gmag1": lambda: (frames_of(synth, 24), {"gravity_magnitude": 1.0}),
        "prior100": lambda: (frames_of(synth, 24), {"bias_prior_weight": 100.0}),
        "prior0": lambda: (frames_of(synth, 24), {"bias_prior_weight": 0.0}),
    }
    fr, kw = made[name]()
    return name, fr, kw
