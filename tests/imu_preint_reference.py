"""Independent reference of IMU preintegration — TEST INFRASTRUCTURE ONLY.

Plain numpy, written from the reference's C++ (IMUPreintegrator::Preintegrate :143-197,
IntegrateMeasurement :199-238, UpdateCovariance :240-274, Rodrigues / RightJacobian :322-354), not
from synth.preintegrate nor from oracle/imu_oracle.c.  Two modes share one recurrence:

  mode="f64"  the high-precision truth.  Samples and biases are the f32 values the reference holds,
              dt is the clamped f32 step, everything after that is float64.  Exp and the right
              Jacobian are branch-free in the coefficient form
                  Exp(w) = I + A·[w]× + B·[w]×²,   Jr(w) = I − B·[w]× + C·[w]×²,
                  A = sin θ/θ,  B = (1 − cos θ)/θ² = 2 sin²(θ/2)/θ²,  C = (θ − sin θ)/θ³,
              with three-term series below θ = 1e-4 (truncation < 1e-29).  The reference's own
              small-angle branch (θ < 1e-6: I + [w]×, I − ½[w]×) differs from this by O(θ²) ≤ 1e-12.
  mode="f32"  the same recurrence with every operation rounded to float32 as the C++ writes it,
              including the θ < 1e-6f branch, the unit axis ω/θ, and (1 − cos θ)/θ, (θ − sin θ)/θ
              formed in f32.  It exists to measure how far a faithful f32 evaluation sits from the
              truth (the floor of the tolerance in test_imu_preint_reference.py).  It is not an oracle.

Range rule: a linear pass `ts >= t0 and ts < t1` over all samples, so NaN and ±inf bounds follow from
IEEE comparison semantics (a NaN bound keeps nothing).  First dt: difference to the next filtered
sample, or 0.002 when there is none; later dt: difference to the previous filtered sample; both
cast to f32 and clamped to [0.0005f, 0.02f].
"""
import numpy as np

F32 = np.float32
F64 = np.float64
DEFAULT_NOISE = (1.0e-4, 1.0e-3, 1.0e-6, 1.0e-5)  # gyro, accel, gyro bias walk, accel bias walk
MAT_FIELDS = ("delta_R", "J_Rg", "J_Vg", "J_Va", "J_Pg", "J_Pa")
VEC_FIELDS = ("delta_V", "delta_P")
FIELDS = ("delta_R", "delta_V", "delta_P", "J_Rg", "J_Vg", "J_Va", "J_Pg", "J_Pa", "cov9", "cov_bias")


def _hat(v, T):
    z = T(0)
    return np.array([[z, -v[2], v[1]], [v[2], z, -v[0]], [-v[1], v[0], z]], dtype=T)


def _coeffs64(th):
    """A, B, C of the module docstring in f64, series below 1e-4."""
    if th < 1e-4:
        t2 = th * th
        return (1.0 - t2 / 6.0 + t2 * t2 / 120.0, 0.5 - t2 / 24.0 + t2 * t2 / 720.0,
                1.0 / 6.0 - t2 / 120.0 + t2 * t2 / 5040.0)
    h = np.sin(0.5 * th)
    return np.sin(th) / th, 2.0 * h * h / (th * th), (th - np.sin(th)) / (th * th * th)


def exp_jr64(w):
    """(Exp(w), Jr(w)) in float64, branch-free."""
    w = np.asarray(w, F64)
    W = _hat(w, F64)
    WW = W @ W
    A, B, Cc = _coeffs64(float(np.sqrt(w @ w)))
    I = np.eye(3)
    return I + A * W + B * WW, I - B * W + Cc * WW


def exp_jr32(w):
    """Rodrigues(w), RightJacobian(w) with every operation in f32, as the C++ reads."""
    w = np.asarray(w, F32)
    th = F32(np.sqrt(F32(F32(w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])))
    I = np.eye(3, dtype=F32)
    if th < F32(1e-6):
        S = _hat(w, F32)
        return I + S, I - F32(0.5) * S
    K = _hat(w / th, F32)
    KK = K @ K
    s, c = F32(np.sin(th)), F32(np.cos(th))
    one = F32(1)
    R = (I + s * K) + (one - c) * KK
    Jr = (I - ((one - c) / th) * K) + ((th - s) / th) * KK
    return R.astype(F32), Jr.astype(F32)


def select(ts, t0, t1):
    """Indices of the samples the reference's filter keeps (IEEE comparisons, linear pass)."""
    ts = np.asarray(ts, F64)
    with np.errstate(invalid="ignore"):
        return np.nonzero((ts >= F64(t0)) & (ts < F64(t1)))[0]


def step_dts(ts):
    """The clamped f32 steps of a filtered timestamp list."""
    n = len(ts)
    dts = np.empty(n, F32)
    for i in range(n):
        if i == 0:
            dt = F32(ts[1] - ts[0]) if n > 1 else F32(0.002)
        else:
            dt = F32(ts[i] - ts[i - 1])
        dts[i] = max(F32(0.0005), min(dt, F32(0.02)))
    return dts


def preintegrate_one(samples, t0, t1, bg=None, ba=None, noise=None, mode="f64"):
    """One Preintegrate call.  samples: (M, 7) [t, ax, ay, az, gx, gy, gz].  Returns None where the
    reference returns nullptr, else a dict of the FIELDS plus dt_total (f64) and steps."""
    T = {"f64": F64, "f32": F32}[mode]
    exp_jr = exp_jr64 if mode == "f64" else exp_jr32
    samples = np.asarray(samples, F64).reshape(-1, 7)
    if len(samples) == 0:
        return None
    idx = select(samples[:, 0], t0, t1)
    if len(idx) == 0:
        return None
    sel = samples[idx]
    meas = sel[:, 1:].astype(F32).astype(T)  # IMUData holds floats
    bg = np.zeros(3, T) if bg is None else np.asarray(bg, F32).astype(T)
    ba = np.zeros(3, T) if ba is None else np.asarray(ba, F32).astype(T)
    ng, na, nbg, nba = (F32(x) for x in (DEFAULT_NOISE if noise is None else noise))
    dts = step_dts(sel[:, 0])

    dR = np.eye(3, dtype=T)
    dV = np.zeros(3, T)
    dP = np.zeros(3, T)
    JRg, JVg, JVa, JPg, JPa = (np.zeros((3, 3), T) for _ in range(5))
    cov = np.zeros((15, 15), T)
    Nga = np.zeros((6, 6), T)
    Nga[:3, :3] = np.eye(3, dtype=T) * T(ng * ng)   # m_gyro_noise·m_gyro_noise is a float product
    Nga[3:, 3:] = np.eye(3, dtype=T) * T(na * na)
    nbg2, nba2 = T(nbg * nbg), T(nba * nba)
    half = T(0.5)
    I3 = np.eye(3, dtype=T)
    dt_total = 0.0
    for i in range(len(sel)):
        dt = T(dts[i])
        # IntegrateMeasurement
        acc = meas[i, 0:3] - ba
        gyr = meas[i, 3:6] - bg
        R, V, P = dR, dV, dP
        dRi, Jr = exp_jr(gyr * dt)
        dRi = dRi.astype(T)
        Jr = Jr.astype(T)
        Sa = _hat(acc, T)
        JRg = -dRi.T @ Jr * dt                       # overwritten each step
        JVg = JVg + JVa @ Sa @ JRg                   # old J_Va
        JPg = JPg + JPa @ Sa @ JRg + JVg * dt        # old J_Pa, updated J_Vg
        dR = R @ dRi
        dV = V + R @ acc * dt
        JVa = JVa + R * dt                           # old ΔR
        dP = P + (V * dt + half * R @ acc * dt * dt)
        JPa = JPa + JVa * dt + half * R * dt * dt    # updated J_Va
        # UpdateCovariance, with the updated ΔR
        A = np.eye(9, dtype=T)
        A[6:9, 3:6] = I3 * dt
        B = np.zeros((9, 6), T)
        B[3:6, 3:6] = dR * dt
        B[6:9, 3:6] = half * dR * dt * dt
        cov[:9, :9] = A @ cov[:9, :9] @ A.T + B @ Nga @ B.T
        walk = np.zeros(6, T)
        walk[:3] = nbg2 * dt
        walk[3:] = nba2 * dt
        cov[np.arange(9, 15), np.arange(9, 15)] += walk
        dt_total += float(dts[i])                    # double accumulator of float steps
        assert dR.dtype == T and cov.dtype == T and JPg.dtype == T
    return {"delta_R": dR, "delta_V": dV, "delta_P": dP, "J_Rg": JRg, "J_Vg": JVg, "J_Va": JVa, "J_Pg": JPg,
            "J_Pa": JPa, "cov9": cov[:9, :9].copy(), "cov_bias": np.diag(cov)[9:].copy(), "dt_total": dt_total,
            "steps": len(sel)}


_SHAPES = {"delta_R": (3, 3), "delta_V": (3,), "delta_P": (3,), "J_Rg": (3, 3), "J_Vg": (3, 3), "J_Va": (3, 3),
           "J_Pg": (3, 3), "J_Pa": (3, 3), "cov9": (9, 9), "cov_bias": (6,)}


def preintegrate(samples, t_start, t_end, gyro_bias=None, accel_bias=None, noise=None, mode="f64"):
    """Every interval of one call, in the layout of Context.imu_preintegrate: dict of (n, ...) float64
    arrays keyed by FIELDS, plus dt_total (n,), valid (n,) u8 and steps (n,).  Invalid intervals are
    all zero, as the entry points write them."""
    t_start = np.asarray(t_start, F64).reshape(-1)
    t_end = np.asarray(t_end, F64).reshape(-1)
    n = len(t_start)
    out = {k: np.zeros((n,) + s) for k, s in _SHAPES.items()}
    out["dt_total"] = np.zeros(n)
    out["valid"] = np.zeros(n, np.uint8)
    out["steps"] = np.zeros(n, np.int64)
    for i in range(n):
        bg = None if gyro_bias is None else np.broadcast_to(np.asarray(gyro_bias, F32), (n, 3))[i]
        ba = None if accel_bias is None else np.broadcast_to(np.asarray(accel_bias, F32), (n, 3))[i]
        r = preintegrate_one(samples, t_start[i], t_end[i], bg, ba, noise, mode)
        if r is None:
            continue
        for k in _SHAPES:
            out[k][i] = r[k]
        out["dt_total"][i] = r["dt_total"]
        out["steps"][i] = r["steps"]
        out["valid"][i] = 1
    return out
