"""Named IMU preintegration cases shared by the CPU reference test and the GPU parity test.

A case is a list of parts; a part is one call: a sample stream (M, 7) [t, ax, ay, az, gx, gy, gz],
interval bounds, per-interval biases (or None) and noise parameters (or None = the defaults).
Every case is small (the whole set is ≈ 8 k integration steps); the motion and the ranges are what
is hard, not the size.  `reference(name, synth, mode)` evaluates tests/imu_preint_reference.py once
per case and mode and keeps the result for every test that needs it.
"""
import numpy as np

import imu_preint_reference as ref

NAMES = ("tame", "aggressive", "long", "threshold", "big_bias", "noise", "ranges")
G = 9.81
NAN, INF = float("nan"), float("inf")


def _part(samples, t0, t1, bg=None, ba=None, noise=None, label=""):
    t0 = np.asarray(t0, np.float64).reshape(-1)
    t1 = np.asarray(t1, np.float64).reshape(-1)
    assert t0.shape == t1.shape
    n = len(t0)
    bg = None if bg is None else np.array(np.broadcast_to(np.asarray(bg, np.float32), (n, 3)))
    ba = None if ba is None else np.array(np.broadcast_to(np.asarray(ba, np.float32), (n, 3)))
    return dict(samples=np.asarray(samples, np.float64), t0=t0, t1=t1, bg=bg, ba=ba, noise=noise, label=label)


def _motion(ts, rng, gyro_amp, acc_amp):
    """Three-axis sinusoids of random frequency (0.5-6 Hz) and phase; the accelerometer adds gravity."""
    s = np.zeros((len(ts), 7))
    s[:, 0] = ts
    for k in range(3):
        fa, fg = rng.uniform(0.5, 6.0, 2)
        pa, pg = rng.uniform(0, 2 * np.pi, 2)
        s[:, 1 + k] = acc_amp * np.sin(2 * np.pi * fa * ts + pa)
        s[:, 4 + k] = gyro_amp * np.sin(2 * np.pi * fg * ts + pg)
    s[:, 3] += G
    return s


def _tame(synth):
    w = synth.make_window(K=10, L=20, seed=20251205, imu=True)
    t0 = synth.KF_DT * np.arange(9)
    return [_part(w["imu_samples"], t0, t0 + synth.KF_DT, label="make_window")]


def _aggressive(synth):
    parts = []
    for amp, seed in ((10.0, 11), (35.0, 12)):
        rng = np.random.default_rng(seed)
        k = np.arange(401)
        ts = (k + rng.uniform(-0.3, 0.3, len(k))) / 200.0  # jitter < half a period: still sorted
        s = _motion(ts, rng, amp, 150.0)
        t0 = 0.25 * np.arange(8)
        parts.append(_part(s, t0, t0 + 0.25, rng.normal(0, 1e-2, (8, 3)), rng.normal(0, 5e-2, (8, 3)),
                           label=f"gyro {amp:g} rad/s"))
    return parts


def _long(synth):
    parts = []
    for rate, T, seed in ((200.0, 2.0, 21), (1000.0, 1.0, 22), (50.0, 1.0, 23)):
        rng = np.random.default_rng(seed)
        ts = np.arange(int(round(rate * T)) + 1) / rate
        s = _motion(ts, rng, 1.5, 6.0)
        s[:, 4:7] += [2.5, -1.5, 2.0]  # steady 3.5 rad/s: 7 rad over 2 s, well past π
        parts.append(_part(s, [0.0, 0.0], [T, T], [[0, 0, 0], [0.02, -0.01, 0.03]], [[0, 0, 0], [0.1, 0.2, -0.1]],
                           label=f"{T:g} s at {rate:g} Hz"))
    return parts


def _threshold(synth):
    """ω·dt straddles the reference's θ < 1e-6 switch: at 200 Hz the unbiased rate alternates between
    ≈1e-4 rad/s (θ ≈ 5e-7, small-angle branch) and ≈4e-4 rad/s (θ ≈ 2e-6, Rodrigues branch) from
    sample to sample; odd intervals subtract a 5e-4 rad/s bias along the same axis, which swaps the
    two, so neighbouring intervals of one wave sit in different branches at every step."""
    rng = np.random.default_rng(31)
    ts = np.arange(51) / 200.0
    s = _motion(ts, rng, 0.0, 3.0)
    u = np.array([0.6, -0.48, 0.64])
    mag = np.where(np.arange(len(ts)) % 2 == 0, 1e-4, 4e-4) * rng.uniform(0.9, 1.1, len(ts))
    s[:, 4:7] = mag[:, None] * u
    n = 14
    bg = np.zeros((n, 3))
    bg[1::2] = 5e-4 * u
    return [_part(s, np.zeros(n), np.full(n, 0.25), bg, rng.normal(0, 1e-2, (n, 3)), label="alternating")]


def threshold_branches(part):
    """(n, steps) bool: True where the step's f32 θ is below 1e-6 (every interval covers all samples
    but the last)."""
    F32 = np.float32
    s = part["samples"]
    idx = ref.select(s[:, 0], part["t0"][0], part["t1"][0])
    dts = ref.step_dts(s[idx, 0])
    g = s[idx, 4:7].astype(F32)
    w = (g[None] - part["bg"][:, None, :]) * dts[None, :, None]
    th = np.sqrt((w[..., 0] * w[..., 0] + w[..., 1] * w[..., 1]) + w[..., 2] * w[..., 2])
    assert th.dtype == F32
    return th < F32(1e-6), th


def _big_bias(synth):
    rng = np.random.default_rng(41)
    ts = np.arange(201) / 200.0
    s = _motion(ts, rng, 1.0, 4.0)
    n = 8
    d = rng.normal(size=(2, n, 3))
    d /= np.linalg.norm(d, axis=2, keepdims=True)
    t0 = rng.uniform(0, 0.7, n)
    return [_part(s, t0, t0 + 0.25, 0.5 * d[0], 2.0 * d[1], label="bg 0.5 rad/s, ba 2 m/s^2")]


def _noise(synth):
    rng = np.random.default_rng(51)
    ts = np.arange(101) / 200.0
    s = _motion(ts, rng, 2.0, 8.0)
    t0 = np.array([0.0, 0.1, 0.2, 0.25])
    return [_part(s, t0, t0 + 0.25, noise=(2e-3, 5e-2, 3e-5, 4e-4), label="large noise"),
            _part(s, t0, t0 + 0.25, noise=(0.0, 0.0, 0.0, 0.0), label="zero noise")]


def _ranges(synth):
    rng = np.random.default_rng(61)
    ts = np.arange(40) / 200.0
    s = _motion(ts, rng, 2.0, 5.0)
    t0 = [ts[5], ts[0], -1.0, -1.0, ts[39], 10.0, -2.0, 0.1, 0.05, ts[7], ts[7], ts[38]]
    t1 = [ts[20], ts[39], 10.0, ts[0], 10.0, 11.0, -1.0, 0.05, 0.05, ts[8], ts[9], ts[39]]
    parts = [_part(s, t0, t1, label="bounds on / off the samples")]
    # every combination of NaN / ±inf / finite bounds but finite-finite (covered above)
    vals = [0.05, NAN, INF, -INF]
    combos = [(a, b) for a in vals for b in vals if not (a == 0.05 and b == 0.05)]
    parts.append(_part(s, [c[0] for c in combos], [0.15 if c[1] == 0.05 else c[1] for c in combos],
                       rng.normal(0, 1e-2, (len(combos), 3)), label="non-finite bounds"))
    # runs of identical timestamps (dt = 0 clamps to 0.5 ms)
    td = np.array([0.0, 0.0, 0.0, 0.005, 0.005, 0.01, 0.01, 0.01, 0.01, 0.015, 0.02, 0.02])
    sd = _motion(td, rng, 2.0, 5.0)
    sd[:, 1:] += rng.normal(0, 0.1, (len(td), 6))  # equal times, different readings
    parts.append(_part(sd, [0.0, 0.005, 0.0, 0.01, 0.02, 0.0], [0.005, 0.01, 1.0, 0.010001, 0.02, 0.0],
                       label="identical timestamps"))
    # a single sample in the whole stream
    s1 = _motion(np.array([0.5]), rng, 2.0, 5.0)
    parts.append(_part(s1, [0.0, 0.5, 0.5, 0.6, NAN, 0.0, -INF, 0.5000001],
                       [1.0, 0.5, 0.6, 1.0, 1.0, NAN, INF, 1.0], label="n_imu = 1"))
    # block tails: 7 intervals per 64-lane block
    for n in (1, 6, 7, 8, 13, 14, 15):
        a = rng.uniform(-0.01, 0.15, n)
        parts.append(_part(s, a, a + rng.uniform(0.0, 0.06, n), rng.normal(0, 1e-2, (n, 3)),
                           rng.normal(0, 5e-2, (n, 3)), label=f"{n} intervals"))
    return parts


_BUILDERS = {"tame": _tame, "aggressive": _aggressive, "long": _long, "threshold": _threshold,
             "big_bias": _big_bias, "noise": _noise, "ranges": _ranges}
_cases, _refs = {}, {}


def case(name, synth):
    if name not in _cases:
        _cases[name] = _BUILDERS[name](synth)
    return _cases[name]


def reference(name, synth, mode):
    """List (one per part) of imu_preint_reference.preintegrate outputs; computed once."""
    if (name, mode) not in _refs:
        _refs[name, mode] = [ref.preintegrate(p["samples"], p["t0"], p["t1"], p["bg"], p["ba"], p["noise"], mode)
                             for p in case(name, synth)]
    return _refs[name, mode]


def bounds(name, synth):
    """Per part: dict field -> (n,) tolerance 4·floor + 4·2⁻²⁴·max|f64 field|, with
    floor = max|ref_f32 − ref_f64| per interval — from the reference alone."""
    out = []
    for r64, r32 in zip(reference(name, synth, "f64"), reference(name, synth, "f32")):
        b = {}
        for k in ref.FIELDS:
            n = len(r64[k])
            floor = np.abs(r32[k] - r64[k]).reshape(n, -1).max(1) if n else np.zeros(0)
            mx = np.abs(r64[k]).reshape(n, -1).max(1) if n else np.zeros(0)
            b[k] = 4.0 * floor + 4.0 * 2.0 ** -24 * mx
        out.append(b)
    return out


def ratios(got, name, synth):
    """error / bound per part, field and interval of a result list [(records, valid, cov_bias)] in
    the layout of Context.imu_preintegrate, against the f64 reference.  A field that is exactly
    equal to the reference has ratio 0 (also where the bound is 0)."""
    out = []
    for (rec, _, cb), r64, b in zip(got, reference(name, synth, "f64"), bounds(name, synth)):
        d = {}
        for k in ref.FIELDS:
            g = (cb if k == "cov_bias" else rec[k]).astype(np.float64)
            n = len(g)
            err = np.abs(g - r64[k]).reshape(n, -1).max(1) if n else np.zeros(0)
            with np.errstate(divide="ignore", invalid="ignore"):
                d[k] = np.where(err == 0, 0.0, err / b[k])
        out.append(d)
    return out
