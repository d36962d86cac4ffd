"""Independent float64 restatement of the IMU-initialisation cost — TEST INFRASTRUCTURE ONLY.

Written from the reference source alone (InertialGravityScaleFactor, Factors.cpp:981-1293;
BiasPriorFactor, Factors.h:366-396; Optimizer::OptimizeIMUInit, Optimizer.cpp:972-1257; the SO3d
exp / log / projection it calls, LieUtils.cpp:203-288), not from oracle/ba_oracle.c or the kernel, and
it loads neither liboracle.so nor libvio360.so.  It restates what is minimised, not how: there is
no Jacobian and no Levenberg-Marquardt here.  `polish` hands the cost's residuals to a generic
finite-difference least-squares minimiser, so a returned answer can be checked for stationarity
without anybody's derivatives.

What the reference evaluates (and so what is restated):
  * the pose blocks are zero perturbations mapped through SE3d::exp, so every factor sees identity
    poses (R_wbi = R_wbj = I, t = 0); the keyframe poses enter the velocity initialisation only;
  * the factor's square-root information is computed and never applied;
  * a factor is kept for 0.001 <= dt_total <= 2.0; the velocity initialisation asks dt_total > 0.001;
  * HuberLoss(delta) acts per residual block on s = |r|^2: rho(s) = s for s <= delta^2, otherwise
    2 delta sqrt(s) - delta^2; the two BiasPriorFactor blocks (stage 2) carry no loss and their
    residual is weight * bias, so they cost weight^2 |bias|^2 / 2.
"""
import numpy as np
from scipy.optimize import least_squares

DEFAULTS = {"gravity_magnitude": 9.81, "huber_delta": 4.0, "bias_prior_weight": 1.0}


def _f32(p, key):
    """A preintegration field as the reference holds it (float) and reads it (cast to double)."""
    return np.asarray(p[key], np.float32).astype(np.float64)


def kept(frames):
    """Indices i of the factors (frame i -> i + 1) that both stages add (Optimizer.cpp:1068-1077)."""
    pre = frames["preint"]
    return [i for i in range(len(frames["T_wb"]) - 1)
            if pre[i + 1] is not None and not (pre[i + 1]["dt_total"] < 0.001 or pre[i + 1]["dt_total"] > 2.0)]


def touched(frames):
    """Mask of the frames whose velocity some kept factor reads (the free stage-2 velocities)."""
    m = np.zeros(len(frames["T_wb"]), bool)
    for i in kept(frames):
        m[i] = m[i + 1] = True
    return m


def vinit(frames):
    """velocity_world = R_wb_prev * delta_V for dt_total > 0.001, otherwise zero (Optimizer.cpp:1028-1040).
    The product is summed term by term in index order, so it is reproducible to the bit."""
    T = np.asarray(frames["T_wb"], np.float64)
    v = np.zeros((len(T), 3))
    for i in range(1, len(T)):
        p = frames["preint"][i]
        if p is not None and p["dt_total"] > 0.001:
            R, dv = T[i - 1, :3, :3], _f32(p, "delta_V")
            v[i] = R[:, 0] * dv[0] + R[:, 1] * dv[1] + R[:, 2] * dv[2]
    return v


def _hat(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def _so3_log(R):
    th = np.arccos(max(-1.0, min(1.0, (np.trace(R) - 1.0) * 0.5)))
    if th < 1e-10:
        return np.array([R[2, 1], R[0, 2], R[1, 0]])
    s = np.sin(th)
    skew = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    if abs(s) < 1e-10:  # theta ~ pi: the axis from R + I, its sign from the skew part
        k = int(np.argmax(np.diag(R)))
        ax = np.zeros(3)
        ax[k] = np.sqrt((R[k, k] + 1.0) * 0.5)
        for i in range(3):
            if i != k:
                ax[i] = R[k, i] / (2.0 * ax[k])
        if ax @ (skew * 0.5) < 0:
            ax = -ax
        return ax * th
    return th / (2.0 * s) * skew


def gravity_dir_to_rotation(gdir):
    w = np.array([gdir[0], gdir[1], 0.0])
    d2 = w @ w
    d = np.sqrt(d2)
    W = _hat(w)
    if d < 1e-5:
        return np.eye(3) + W + 0.5 * (W @ W)
    return np.eye(3) + W * np.sin(d) / d + (W @ W) * (1.0 - np.cos(d)) / d2


def _kw(kw):
    bad = set(kw) - set(DEFAULTS) - {"max_iterations"}
    assert not bad, bad
    return {k: kw.get(k, DEFAULTS[k]) for k in DEFAULTS}


def _hat_n(w):
    H = np.zeros(w.shape[:-1] + (3, 3))
    H[..., 0, 1], H[..., 0, 2], H[..., 1, 2] = -w[..., 2], w[..., 1], -w[..., 0]
    H[..., 1, 0], H[..., 2, 0], H[..., 2, 1] = w[..., 2], -w[..., 1], w[..., 0]
    return H


def _project_n(R):
    U, _, Vt = np.linalg.svd(R)
    flip = np.linalg.det(U @ Vt) < 0.0
    U[flip, :, 2] *= -1.0
    return U @ Vt


def _so3_exp_n(w):
    th = np.linalg.norm(w, axis=-1)
    small = th < 1e-10
    K = _hat_n(w / np.where(small, 1.0, th)[:, None])
    R = np.eye(3) + np.sin(th)[:, None, None] * K + (1.0 - np.cos(th))[:, None, None] * (K @ K)
    R[small] = np.eye(3) + _hat_n(w[small])
    return _project_n(R)


def _so3_log_n(R):
    th = np.arccos(np.clip((np.trace(R, axis1=-2, axis2=-1) - 1.0) * 0.5, -1.0, 1.0))
    s = np.sin(th)
    odd = (th < 1e-10) | (np.abs(s) < 1e-10)
    skew = np.stack([R[:, 2, 1] - R[:, 1, 2], R[:, 0, 2] - R[:, 2, 0], R[:, 1, 0] - R[:, 0, 1]], -1)
    w = (th / (2.0 * np.where(odd, 1.0, s)))[:, None] * skew
    for k in np.nonzero(odd)[0]:
        w[k] = _so3_log(R[k])
    return w


_FIELDS = ("delta_R", "J_Rg", "J_Vg", "J_Va", "J_Pg", "J_Pa")


def prepare(frames):
    """The kept factors' preintegrations stacked (float -> double once); `residuals` takes either
    the frames or this."""
    idx = kept(frames)
    pre = [frames["preint"][i + 1] for i in idx]
    P = {k: np.array([_f32(p, k).reshape(3, 3) for p in pre]).reshape(-1, 3, 3) for k in _FIELDS}
    for k in ("delta_V", "delta_P", "gyro_bias", "accel_bias"):
        P[k] = np.array([_f32(p, k) for p in pre]).reshape(-1, 3)
    P["dt"] = np.array([float(p["dt_total"]) for p in pre])
    P["i"] = np.array(idx, int)
    return P


def residuals(frames, gdir, scale, vel, bg, ba, stage, **kw):
    """The robustified residual vector: per kept factor the 9 residuals times sqrt(rho(s) / s), then
    (stage 2) the six prior residuals; half its squared norm is `cost`."""
    o = _kw(kw)
    P = frames if "dt" in frames else prepare(frames)
    vel = np.asarray(vel, np.float64)
    bg, ba = np.asarray(bg, np.float64), np.asarray(ba, np.float64)
    g = gravity_dir_to_rotation(gdir) @ np.array([0.0, 0.0, -o["gravity_magnitude"]])
    dt = P["dt"][:, None]
    dR, dV, dP = P["delta_R"], P["delta_V"], P["delta_P"]
    dbg, dba = bg - P["gyro_bias"], ba - P["accel_bias"]
    c = (np.linalg.norm(dbg, axis=1) > 1e-6) | (np.linalg.norm(dba, axis=1) > 1e-6)
    if c.any():  # first-order bias correction of the preintegrated measurement
        def mv(M, v):
            return np.einsum("nij,nj->ni", M, v)
        dR, dV, dP = dR.copy(), dV.copy(), dP.copy()
        dR[c] = dR[c] @ _so3_exp_n(mv(P["J_Rg"][c], dbg[c]))
        dV[c] = dV[c] + mv(P["J_Vg"][c], dbg[c]) + mv(P["J_Va"][c], dba[c])
        dP[c] = dP[c] + mv(P["J_Pg"][c], dbg[c]) + mv(P["J_Pa"][c], dba[c])
    vi, vj = vel[P["i"]], vel[P["i"] + 1]
    U, _, Vt = np.linalg.svd(np.swapaxes(dR, 1, 2))  # log_SO3: normalise by SVD, then SO3d(...).log()
    r = np.concatenate([
        _so3_log_n(_project_n(U @ Vt)),
        (scale * (vj - vi) - g * dt) - dV,
        (scale * (0.0 - vi * dt) - 0.5 * g * dt * dt) - dP], axis=1)
    s = np.einsum("ni,ni->n", r, r)
    b = o["huber_delta"] ** 2
    out = s > b
    r[out] *= np.sqrt((2.0 * o["huber_delta"] * np.sqrt(s[out]) - b) / s[out])[:, None]
    r = r.ravel()
    if stage == 2:
        r = np.concatenate([r, o["bias_prior_weight"] * bg, o["bias_prior_weight"] * ba])
    return r


def cost(frames, gdir, scale, vel, bg, ba, stage, **kw):
    """1/2 sum rho_Huber(|r|^2) over the kept factors (+ the two bias priors in stage 2)."""
    r = residuals(frames, gdir, scale, vel, bg, ba, stage, **kw)
    return 0.5 * float(r @ r)


def cost_initial(frames, **kw):
    """What Ceres reports as stage 1's initial cost: (0, 0), scale 1, vinit, zero biases."""
    return cost(frames, (0.0, 0.0), 1.0, vinit(frames), np.zeros(3), np.zeros(3), 1, **kw)


def cost_at(frames, res, stage, **kw):
    """The stage's cost at a returned answer (stage 1: velocities at vinit, biases at zero)."""
    if stage == 1:
        return cost(frames, res["gravity_dir"], res["scale"], vinit(frames), np.zeros(3), np.zeros(3), 1, **kw)
    return cost(frames, res["gravity_dir"], res["scale"], res["velocities"], res["gyro_bias"], res["accel_bias"], 2, **kw)


def polish(frames, res, stage, **kw):
    """A generic minimiser (trust-region least squares on `residuals`, finite-difference Jacobian)
    started at a returned answer, over the stage's free parameters only: stage 1 (theta_x, theta_y,
    scale); stage 2 the velocities of factor-touched frames and the biases.  Returns
    (cost at the start, lowest cost found) — the second never exceeds the first."""
    v0 = vinit(frames)
    z3 = np.zeros(3)
    P = prepare(frames)
    if stage == 1:
        x0 = np.array([res["gravity_dir"][0], res["gravity_dir"][1], res["scale"]], np.float64)

        def fun(x):
            return residuals(P, x[:2], x[2], v0, z3, z3, 1, **kw)
    else:
        m = touched(frames)
        vel = np.array(res["velocities"], np.float64)
        x0 = np.concatenate([vel[m].ravel(), res["gyro_bias"], res["accel_bias"]])

        def fun(x):
            v = vel.copy()
            v[m] = x[:-6].reshape(-1, 3)
            return residuals(P, res["gravity_dir"], res["scale"], v, x[-6:-3], x[-3:], 2, **kw)
    c0 = 0.5 * float(fun(x0) @ fun(x0))
    sol = least_squares(fun, x0, jac="2-point", method="trf", x_scale="jac", ftol=1e-15, xtol=1e-15, gtol=1e-15,
                        max_nfev=40)
    return c0, min(c0, float(sol.cost))
