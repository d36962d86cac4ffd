"""Independent restatement of InertialFactorFixedGravity — TEST INFRASTRUCTURE ONLY.

Written from the reference source alone (InertialFactorFixedGravity, Factors.cpp:1299-1519; the SO3d /
SE3d construction, exp and composition it calls, LieUtils.cpp:203-219, 275-333 and LieUtils.h:207-209,
268-271; Optimizer::RunVIBA, Optimizer.cpp:493-724, for which blocks a window holds constant), not from
oracle/ba_oracle.c or any kernel, and it loads neither liboracle.so nor libvio360.so.  The formulas are
written once (`_evaluate`) over a small arithmetic backend and evaluated twice: `evaluate` in numpy
float64, `evaluate_mp` in mpmath at 50 digits.  Their difference on one input is the float64 rounding of
these formulas on that input, which is what the tests scale their bars by.

What the reference evaluates (and so what is restated), quirks included:
  * the square-root information is chol((cov9 + 1e-8 I)^-1) TRANSPOSED (upper triangular), cov9 the f32
    covariance block cast to double; identity when the LLT fails (a pivot <= 0; Eigen reads the lower
    triangle only);
  * every SO3d built from a matrix is projected by SVD (U V^T, third column of U flipped for det < 0):
    SE3d(Matrix4d) projects the f32-rounded T_init, SO3d::Exp projects its Rodrigues matrix, and the
    product T_init * exp(delta) projects again;
  * the bias correction is applied only when |dbg| > 1e-6 || |dba| > 1e-6, and then
    delta_R * Exp(J_Rg dbg) is a plain Matrix3d product with the f32-rounded (not orthonormal) delta_R;
  * log_SO3 is the factor's own: (R - R^T)^vee / 2 for theta < 1e-6, no theta ~ pi handling;
  * the two pose Jacobians are identically zero; J_vi and J_vj use the DIAGONAL 3x3 blocks S(3:6,3:6) and
    S(6:9,6:9) only; J_bg's rotation rows use right_jacobian(-er)^-1 with er the ALREADY WEIGHTED
    rotation residual; right_jacobian is the identity for |phi| < 1e-6.

`MUTANTS` names one-line deviations from the above; `evaluate(case, mutant=name)` evaluates one.  The
tests use them to show that the case table tells the reference from each of them.

`window_iter0` sums these factors and the independent reprojection factor of
tests/golden/gen_factor_golden.py into the cost and gradient of a RunVIBA problem at its initial point.
"""
import importlib.util
import math
import os

import mpmath
import numpy as np

MP_DIGITS = 50

MUTANTS = (
    "raw_er_in_Jr",        # right_jacobian of the unweighted rotation residual
    "Jr_plus_er",          # right_jacobian(+er)
    "full_S_in_Jv",        # J_vi / J_vj = S * [...] instead of the diagonal blocks
    "L_not_LT",            # sqrt information = L instead of L^T
    "no_regularisation",   # no 1e-8 on the covariance diagonal
    "and_threshold",       # && instead of || in the bias-correction test
    "always_correct",      # the bias correction always applied
    "R_wbi_for_R_bwi",     # R_wbi where the residuals use its transpose
    "half_g_dt2_sign",     # + 0.5 g dt^2
    "dt_in_J_vj",          # a dt factor in J_vj
    "project_delta_R",     # the corrected delta_R projected like an SO3d product
)


# ---------------------------------------------------------------------------------------------------
# arithmetic backends: column vectors are 3x1 / 9x1 matrices, elements are read as M[i, j]
class _F64:
    name = "f64"
    sin, cos, acos, sqrt = staticmethod(math.sin), staticmethod(math.cos), staticmethod(math.acos), staticmethod(math.sqrt)

    @staticmethod
    def num(x):
        return float(x)

    @staticmethod
    def mat(a):
        return np.array(a, np.float64)

    @staticmethod
    def zeros(m, n):
        return np.zeros((m, n))

    @staticmethod
    def eye(n):
        return np.eye(n)

    @staticmethod
    def mul(a, b):
        return a @ b

    @staticmethod
    def inv(a):
        try:
            return np.linalg.inv(a)
        except np.linalg.LinAlgError:
            return None

    @staticmethod
    def svd(a):
        U, _, Vt = np.linalg.svd(a)
        return U, Vt

    @staticmethod
    def det3(a):
        return float(np.linalg.det(a))

    @staticmethod
    def out(a):
        return np.array(a, np.float64)


class _MP:
    name = "mp"
    sin, cos, acos, sqrt = mpmath.sin, mpmath.cos, mpmath.acos, mpmath.sqrt

    @staticmethod
    def num(x):
        return mpmath.mpf(float(x)) if not isinstance(x, mpmath.mpf) else x

    @staticmethod
    def mat(a):
        a = np.asarray(a)
        return mpmath.matrix([[_MP.num(a[i, j]) for j in range(a.shape[1])] for i in range(a.shape[0])])

    @staticmethod
    def zeros(m, n):
        return mpmath.zeros(m, n)

    @staticmethod
    def eye(n):
        return mpmath.eye(n)

    @staticmethod
    def mul(a, b):
        return a * b

    @staticmethod
    def inv(a):
        try:
            return mpmath.inverse(a)
        except ZeroDivisionError:
            return None

    @staticmethod
    def svd(a):
        U, _, V = mpmath.svd_r(a)  # a = U diag(S) V: V is already the transposed factor
        return U, V

    @staticmethod
    def det3(a):
        return mpmath.det(a)

    @staticmethod
    def out(a):
        o = np.empty((a.rows, a.cols), object)
        for i in range(a.rows):
            for j in range(a.cols):
                o[i, j] = a[i, j]
        return o


def _col(B, v):
    return B.mat(np.asarray(v, np.float64).reshape(-1, 1))


def _norm(B, v):
    return B.sqrt(sum((v[i, 0] * v[i, 0] for i in range(3)), B.num(0)))


def _hat(B, v):
    S = B.zeros(3, 3)
    S[0, 1], S[0, 2] = -v[2, 0], v[1, 0]
    S[1, 0], S[1, 2] = v[2, 0], -v[0, 0]
    S[2, 0], S[2, 1] = -v[1, 0], v[0, 0]
    return S


def _block(B, M, r0, c0, m, n):
    o = B.zeros(m, n)
    for i in range(m):
        for j in range(n):
            o[i, j] = M[r0 + i, c0 + j]
    return o


def _set_block(M, r0, c0, b, m, n):
    for i in range(m):
        for j in range(n):
            M[r0 + i, c0 + j] = b[i, j]


def _so3d(B, M):
    """SO3d(const Matrix3d&) (LieUtils.cpp:275-288)."""
    U, Vt = B.svd(M)
    R = B.mul(U, Vt)
    if B.det3(R) < 0:
        for i in range(3):
            U[i, 2] = -U[i, 2]
        R = B.mul(U, Vt)
    return R


def _so3d_exp(B, w):
    """SO3d::Exp (LieUtils.cpp:203-219), kEpsilonD = 1e-10."""
    th = _norm(B, w)
    if th < 1e-10:
        return _so3d(B, B.eye(3) + _hat(B, w))
    K = _hat(B, w * (1 / th))
    return _so3d(B, B.eye(3) + B.sin(th) * K + (1 - B.cos(th)) * B.mul(K, K))


def _se3d_exp(B, xi):
    """SE3d::exp (LieUtils.cpp:305-333): xi = [rho, phi]."""
    rho, phi = _block(B, xi, 0, 0, 3, 1), _block(B, xi, 3, 0, 3, 1)
    R = _so3d_exp(B, phi)
    th = _norm(B, phi)
    if th < 1e-10:
        return R, rho
    P = _hat(B, phi)
    th2 = th * th
    V = B.eye(3) + ((1 - B.cos(th)) / th2) * P + ((th - B.sin(th)) / (th2 * th)) * B.mul(P, P)
    return R, B.mul(V, rho)


def _pose(B, T_init, delta):
    """SE3d(T_init) * SE3d::exp(delta) (Factors.cpp:1335-1336, LieUtils.cpp:296-299, LieUtils.h:268-271)."""
    T = B.mat(np.asarray(T_init, np.float64)[:3, :4])
    R0, t0 = _so3d(B, _block(B, T, 0, 0, 3, 3)), _block(B, T, 0, 3, 3, 1)
    dR, dt = _se3d_exp(B, _col(B, delta))
    return _so3d(B, B.mul(R0, dR)), t0 + B.mul(R0, dt)


def _llt(B, A):
    """Eigen::LLT on the lower triangle of A: L, or None where a pivot is <= 0 (NumericalIssue)."""
    n = 9
    L = B.zeros(n, n)
    for j in range(n):
        d = A[j, j] - sum((L[j, k] * L[j, k] for k in range(j)), B.num(0))
        if not d > 0:
            return None
        d = B.sqrt(d)
        L[j, j] = d
        for i in range(j + 1, n):
            L[i, j] = (A[i, j] - sum((L[i, k] * L[j, k] for k in range(j)), B.num(0))) / d
    return L


def _sqrt_information(B, cov9, mutant):
    """The constructor (Factors.cpp:1309-1323)."""
    cov = B.mat(np.asarray(cov9, np.float32).astype(np.float64).reshape(9, 9))
    if mutant != "no_regularisation":
        cov = cov + B.eye(9) * B.num(1e-8)
    info = B.inv(cov)
    L = _llt(B, info) if info is not None else None
    if L is None:
        return B.eye(9)
    return L if mutant == "L_not_LT" else L.T


def _log_so3(B, R):
    """InertialFactorFixedGravity::log_SO3 (Factors.cpp:1507-1519)."""
    c = (R[0, 0] + R[1, 1] + R[2, 2] - 1) / 2
    c = max(-1, min(1, c))
    th = B.acos(c)
    v = B.zeros(3, 1)
    v[0, 0], v[1, 0], v[2, 0] = R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]
    if th < 1e-6:
        return v * (1 / B.num(2)), th
    return v * (th / (2 * B.sin(th))), th


def _right_jacobian(B, phi):
    """InertialFactorFixedGravity::right_jacobian_SO3 (Factors.cpp:1495-1505)."""
    th = _norm(B, phi)
    if th < 1e-6:
        return B.eye(3)
    P = _hat(B, phi)
    th2 = th * th
    return B.eye(3) - ((1 - B.cos(th)) / th2) * P + ((th - B.sin(th)) / (th2 * th)) * B.mul(P, P)


def _f32mat(B, p, key, shape):
    """A preintegration field as the reference holds it (float) and reads it (cast to double)."""
    return B.mat(np.asarray(p[key], np.float32).astype(np.float64).reshape(shape))


def _evaluate(B, case, mutant=None):
    assert mutant is None or mutant in MUTANTS, mutant
    p = case["preint"]
    S = _sqrt_information(B, np.asarray(p["cov"])[:9, :9], mutant)
    R_wbi, t_wbi = _pose(B, case["T_i"], case["delta_i"])
    R_wbj, t_wbj = _pose(B, case["T_j"], case["delta_j"])
    R_bwi = R_wbi if mutant == "R_wbi_for_R_bwi" else R_wbi.T
    vi, vj, bg, ba, g = (_col(B, case[k]) for k in ("v_i", "v_j", "bg", "ba", "gravity"))
    dt = B.num(p["dt_total"])
    delta_R, delta_V, delta_P = _f32mat(B, p, "delta_R", (3, 3)), _f32mat(B, p, "delta_V", (3, 1)), _f32mat(B, p, "delta_P", (3, 1))
    J_Rg, J_Vg, J_Va, J_Pg, J_Pa = (_f32mat(B, p, k, (3, 3)) for k in ("J_Rg", "J_Vg", "J_Va", "J_Pg", "J_Pa"))
    dbg = bg - _f32mat(B, p, "gyro_bias", (3, 1))
    dba = ba - _f32mat(B, p, "accel_bias", (3, 1))
    big_g, big_a = _norm(B, dbg) > 1e-6, _norm(B, dba) > 1e-6
    corrected = (big_g and big_a) if mutant == "and_threshold" else (big_g or big_a)
    if corrected or mutant == "always_correct":
        delta_R = B.mul(delta_R, _so3d_exp(B, B.mul(J_Rg, dbg)))
        if mutant == "project_delta_R":
            delta_R = _so3d(B, delta_R)
        delta_V = delta_V + B.mul(J_Vg, dbg) + B.mul(J_Va, dba)
        delta_P = delta_P + B.mul(J_Pg, dbg) + B.mul(J_Pa, dba)
    er_raw, theta = _log_so3(B, B.mul(B.mul(delta_R.T, R_bwi), R_wbj))
    ev = B.mul(R_bwi, vj - vi - g * dt) - delta_V
    half_g = g * (dt * dt / 2)
    ep = B.mul(R_bwi, t_wbj - t_wbi - vi * dt + (half_g if mutant == "half_g_dt2_sign" else -half_g)) - delta_P
    raw = B.zeros(9, 1)
    _set_block(raw, 0, 0, er_raw, 3, 1)
    _set_block(raw, 3, 0, ev, 3, 1)
    _set_block(raw, 6, 0, ep, 3, 1)
    r = B.mul(S, raw)
    er = er_raw if mutant == "raw_er_in_Jr" else _block(B, r, 0, 0, 3, 1)

    S_vv, S_pp = _block(B, S, 3, 3, 3, 3), _block(B, S, 6, 6, 3, 3)
    J_vi, J_vj = B.zeros(9, 3), B.zeros(9, 3)
    _set_block(J_vi, 3, 0, B.mul(S_vv, R_bwi) * -1, 3, 3)
    _set_block(J_vi, 6, 0, B.mul(S_pp, R_bwi) * (-dt), 3, 3)
    _set_block(J_vj, 3, 0, B.mul(S_vv, R_bwi) * (dt if mutant == "dt_in_J_vj" else 1), 3, 3)
    if mutant == "full_S_in_Jv":
        U = B.zeros(9, 3)
        _set_block(U, 3, 0, R_bwi * -1, 3, 3)
        _set_block(U, 6, 0, R_bwi * (-dt), 3, 3)
        J_vi = B.mul(S, U)
        U = B.zeros(9, 3)
        _set_block(U, 3, 0, R_bwi, 3, 3)
        J_vj = B.mul(S, U)
    Jr = _right_jacobian(B, er if mutant == "Jr_plus_er" else er * -1)
    Jr_inv = B.inv(Jr)
    U = B.zeros(9, 3)
    _set_block(U, 0, 0, B.mul(Jr_inv, J_Rg) * -1, 3, 3)
    _set_block(U, 3, 0, J_Vg * -1, 3, 3)
    _set_block(U, 6, 0, J_Pg * -1, 3, 3)
    J_bg = B.mul(S, U)
    U = B.zeros(9, 3)
    _set_block(U, 3, 0, J_Va * -1, 3, 3)
    _set_block(U, 6, 0, J_Pa * -1, 3, 3)
    J_ba = B.mul(S, U)
    out = {"sqrt_info": B.out(S), "r": B.out(r)[:, 0], "J_pose_i": B.out(B.zeros(9, 6)), "J_vi": B.out(J_vi),
           "J_bg": B.out(J_bg), "J_ba": B.out(J_ba), "J_pose_j": B.out(B.zeros(9, 6)), "J_vj": B.out(J_vj)}
    # diagnostics for the case table's own conditions (not outputs of the factor)
    out["diag"] = {"theta_raw": float(theta), "er_weighted_norm": float(_norm(B, _block(B, r, 0, 0, 3, 1))),
                   "corrected": bool(corrected), "Jr": np.array(B.out(Jr), np.float64)}
    return out


BLOCKS = ("sqrt_info", "r", "J_vi", "J_bg", "J_ba", "J_vj")


def evaluate(case, mutant=None):
    """The factor in numpy float64: sqrt_info (9x9), r (9) and the six Jacobian blocks as the reference
    writes them (J_pose_i / J_pose_j are the all-zero 9x6 blocks)."""
    return _evaluate(_F64, case, mutant)


def evaluate_mp(case, mutant=None):
    """The same formulas in mpmath at MP_DIGITS digits; arrays of mpf (dtype object)."""
    with mpmath.workdps(MP_DIGITS):
        return _evaluate(_MP, case, mutant)


def absdiff(a, b):
    """|a - b| elementwise as float64, the subtraction carried out in mpmath (a, b: float or mpf arrays)."""
    with mpmath.workdps(MP_DIGITS):
        fa, fb = np.asarray(a, object).reshape(-1), np.asarray(b, object).reshape(-1)
        d = [abs(mpmath.mpf(x) - mpmath.mpf(y)) for x, y in zip(fa, fb)]
        return np.array([float(x) for x in d]).reshape(np.shape(a))


def residual(case):
    """r alone (float64), for finite differences of the reference's own residual."""
    return evaluate(case)["r"]


# ---------------------------------------------------------------------------------------------------
# a RunVIBA problem at its initial point
_golden = None


def _visual_factor():
    global _golden
    if _golden is None:
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gen_factor_golden.py")
        spec = importlib.util.spec_from_file_location("gen_factor_golden", path)
        _golden = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(_golden)
    return _golden.factor


def window_factor_case(w, k):
    """The inertial factor RunVIBA adds between frames k-1 and k (Optimizer.cpp:611-632): zero pose
    perturbations, the frames' velocities, the shared biases."""
    z = np.zeros(6)
    return {"preint": w["preint"][k], "gravity": w["gravity"], "T_i": w["T_wb_init"][k - 1], "T_j": w["T_wb_init"][k],
            "delta_i": z, "v_i": w["vel"][k - 1], "bg": w.get("bg", np.zeros(3)), "ba": w.get("ba", np.zeros(3)),
            "delta_j": z, "v_j": w["vel"][k]}


def window_iter0(w, huber_delta=1.0, mp=False):
    """initial_cost, fixed_cost and the iteration-0 gradient_max_norm of the RunVIBA problem of window
    dict `w` (the dict a BaProblem of variant VIO_BA_VI is built from) at its initial point.

    Blocks (Optimizer.cpp:524-637): a 6-vector per frame, a 3-vector velocity per frame, the two shared
    3-vector biases, a 3-vector per MapPoint, all Euclidean.  RunVIBA holds constant the first pose (when
    asked to) and nothing else: MapPoints are never constant there, so every residual block keeps a free
    parameter and fixed_cost is zero.  Visual blocks carry HuberLoss(huber_delta), cost 0.5 rho(|r|^2) and
    gradient rho' J^T r; the inertial blocks carry no loss.  A frame without preintegration has no
    factor to its predecessor (:612-616).

    With mp=True the inertial part comes from evaluate_mp and the sums are carried in mpmath (the visual
    part stays float64).  Also returned: cost_abs and grad_abs, the sums of the absolute values of the
    terms of the cost and of the gradient entry that attains the maximum."""
    kf_const = np.asarray(w["kf_const"], bool)
    assert not kf_const[1:].any() and not np.asarray(w["lm_const"], bool).any(), \
        "RunVIBA holds nothing constant but the first pose"
    K, L = len(w["T_wb_init"]), len(w["lm_xyz"])
    ctx = mpmath.workdps(MP_DIGITS) if mp else mpmath.workdps(mpmath.mp.dps)
    with ctx:
        num = (lambda x: mpmath.mpf(float(x)) if not isinstance(x, mpmath.mpf) else x) if mp else float
        zero = num(0.0)
        g = {"pose": np.full((K, 6), zero, object), "lm": np.full((L, 3), zero, object),
             "vel": np.full((K, 3), zero, object), "bg": np.full(3, zero, object), "ba": np.full(3, zero, object)}
        ga = {k: v.copy() for k, v in g.items()}
        cost = zero

        def add(name, idx, J, r, scale):
            J, r = np.asarray(J, object), np.asarray(r, object)
            for c in range(J.shape[1]):
                for i in range(J.shape[0]):
                    t = num(scale) * num(J[i, c]) * num(r[i])
                    g[name][idx + (c,)] += t
                    ga[name][idx + (c,)] += abs(t)

        factor = _visual_factor()
        T_cb = np.asarray(w["T_cb"], np.float64)
        zeros6 = np.zeros(6)
        for o in range(len(w["obs_kf"])):
            k, l = int(w["obs_kf"][o]), int(w["obs_lm"][o])
            uv = np.asarray(w["obs_uv"][o], np.float32).astype(np.float64)
            ok, r, Jp, Jl = factor(np.asarray(w["T_wb_init"][k], np.float64), T_cb, zeros6,
                                   np.asarray(w["lm_xyz"][l], np.float64), uv, float(w["cols"]), float(w["rows"]))
            assert ok
            s = float(r @ r)
            if s <= huber_delta * huber_delta:
                rho, drho = s, 1.0
            else:
                rho, drho = 2.0 * huber_delta * math.sqrt(s) - huber_delta * huber_delta, huber_delta / math.sqrt(s)
            cost += num(0.5 * rho)
            if not kf_const[k]:
                add("pose", (k,), Jp, r, drho)
            add("lm", (l,), Jl, r, drho)
        for k in range(1, K):
            if w["preint"][k] is None:
                continue
            e = (evaluate_mp if mp else evaluate)(window_factor_case(w, k))
            cost += sum((num(x) * num(x) for x in e["r"]), zero) / 2
            # (the two pose blocks: identically zero Jacobians)
            add("vel", (k - 1,), e["J_vi"], e["r"], 1.0)
            add("bg", (), e["J_bg"], e["r"], 1.0)
            add("ba", (), e["J_ba"], e["r"], 1.0)
            add("vel", (k,), e["J_vj"], e["r"], 1.0)
        best, best_abs = zero, zero
        for name in g:
            for x, a in zip(g[name].reshape(-1), ga[name].reshape(-1)):
                if abs(x) > best:
                    best, best_abs = abs(x), a
        return {"initial_cost": cost, "fixed_cost": zero, "gradient_max_norm": best,
                "cost_abs": float(cost), "grad_abs": float(best_abs)}
