"""Independent float64 reference of the absolute-pose RANSAC (vio_pnp_ransac) — TEST INFRASTRUCTURE ONLY.

Written from the geometry alone; numpy only; it loads neither the device library nor any oracle and shares no
code or formulation with csrc/pnp_dev.h (which splits a degenerate conic of the depth pencil):

  * mode A (P3P): with u = l2 / l1, v = l3 / l1 the three distance constraints give two quadratics in u whose
    coefficients are polynomials in v; their resultant is a Grunert-type quartic in v, solved by numpy.roots.
    u follows from the difference of the two quadratics, l1 from the first constraint.  A root is accepted only
    if the three inter-point distances are reproduced after back-substitution and the depths are positive.  The
    pose is the SVD (Kabsch) alignment of the three scaled bearings to the world points.
  * mode B (known rotation): numpy.linalg.solve of N t = -sum (I - y y^T) R p.
  * inlier test: the angle atan2(|b x x|, b . x) against the threshold.
  * refit: numpy.linalg.lstsq on the stacked residuals unit(R p + t) - b, left perturbation, Rodrigues update.

Brackets, in the manner of tests/mono_init_reference.py: a point whose angle lies within a relative band of the
threshold is UNDECIDED; lo = decided passes, hi = lo + undecided.  A row is FRAGILE when the quartic has a complex
root with an imaginary part below ROOT_BAND, two real roots closer than ROOT_BAND, a u denominator below ROOT_BAND,
a depth or a constraint residual at its acceptance limit, or a skip predicate within SKIP_BAND of its threshold.
The winner is decided when lo[best] > hi[:best] and lo[best] >= hi[best+1:].

The angle band: the rule under test compares (b.x)^2 with cos^2(thr) (x.x) for a bearing that is unit only to f32
rounding, |b|^2 = 1 + e with |e| <= 3 * 2^-24 (three squared components, each rounded to f32).  In angle that moves
the threshold by e / (2 tan(thr)) absolute, so relative to thr by at most 3 * 2^-24 / (2 thr tan thr): 1.2e-3 at
0.5 degrees.  angle_band() is that plus 1e-6 for the f64 arithmetic itself.
"""
import numpy as np

OK, TOO_FEW, NO_MODEL, FEW_INLIERS = range(4)  # VIO_PNPR_*

ROOT_BAND = 1e-4    # relative: near-double roots, small denominators, depths near zero
SKIP_BAND = 1e-3    # relative band on the skip predicates' thresholds
COLLINEAR2 = 1e-10  # the header's collinearity bound on sin^2
CONSTRAINT_TOL = 1e-7  # relative residual of the three distances after back-substitution


def angle_band(thr):
    return 1e-6 + 3 * 2.0 ** -24 / (2 * thr * np.tan(thr))


def angles(R, t, P, B):
    """angle between each bearing and R p + t (f64 on the f32 inputs); NaN where anything is not finite"""
    X = P @ R.T + t
    with np.errstate(invalid="ignore"):
        return np.arctan2(np.linalg.norm(np.cross(B, X), axis=1), np.einsum("ij,ij->i", B, X))


def classify(ang, thr, band):
    """(decided inlier, undecided) masks"""
    with np.errstate(invalid="ignore"):
        yes = ang < thr * (1 - band)
        und = (~yes) & (ang <= thr * (1 + band))
    return yes, und


def pair_angle(b1, b2):
    return np.arctan2(np.linalg.norm(np.cross(b1, b2)), np.dot(b1, b2))


def kabsch(Xw, Xc):
    """R, t with Xc ~ R Xw + t (rows are points)"""
    cw, cc = Xw.mean(0), Xc.mean(0)
    U, _, Vt = np.linalg.svd((Xc - cc).T @ (Xw - cw))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))])
    R = U @ D @ Vt
    return R, cc - R @ cw


def p3p(Pw, Y):
    """All poses of three world points Pw (3,3) and unit bearings Y (3,3): list of (R, t), and a fragility flag."""
    a12 = np.sum((Pw[0] - Pw[1]) ** 2)
    a13 = np.sum((Pw[0] - Pw[2]) ** 2)
    a23 = np.sum((Pw[1] - Pw[2]) ** 2)
    b12, b13, b23 = Y[0] @ Y[1], Y[0] @ Y[2], Y[1] @ Y[2]
    P = np.polynomial.polynomial
    # (I)  a13 (1 + u^2 - 2 b12 u) = a12 (1 + v^2 - 2 b13 v):      A2 u^2 + A1 u + A0(v)
    # (II) a13 (u^2 + v^2 - 2 b23 u v) = a23 (1 + v^2 - 2 b13 v):  A2 u^2 + B1(v) u + B0(v)   (ascending in v)
    A2 = np.array([a13])
    A1 = np.array([-2 * a13 * b12])
    A0 = np.array([a13 - a12, 2 * a12 * b13, -a12])
    B1 = np.array([0.0, -2 * a13 * b23])
    B0 = np.array([-a23, 2 * a23 * b13, a13 - a23])
    d0 = P.polysub(P.polymul(A2, B0), P.polymul(A0, A2))
    d1 = P.polysub(P.polymul(A2, B1), P.polymul(A1, A2))
    d2 = P.polysub(P.polymul(A1, B0), P.polymul(A0, B1))
    q = P.polysub(P.polymul(d0, d0), P.polymul(d1, d2))
    q = np.r_[q, np.zeros(5 - len(q))]
    scale = np.abs(q).max()
    if not np.isfinite(scale) or scale == 0:
        return [], True
    roots = np.roots(q[::-1] / scale)
    fragile = len(roots) < 4
    real = []
    for r in roots:
        m = 1 + abs(r.real)
        if r.imag != 0 and abs(r.imag) < ROOT_BAND * m:
            fragile = True
        if abs(r.imag) < 1e-7 * m:
            real.append(r.real)
    real = sorted(real)
    for x, y in zip(real, real[1:]):
        if abs(x - y) < ROOT_BAND * (1 + abs(x)):
            fragile = True
    sols = []
    side = np.sqrt([a12, a13, a23])
    for v in real:
        den = -2 * a13 * (b12 - b23 * v)            # A1 - B1(v)
        num = P.polyval(v, A0) - P.polyval(v, B0)   # A0 - B0
        if abs(den) < ROOT_BAND * a13 * (1 + abs(v)):
            fragile = True
            if den == 0:
                continue
        u = -num / den
        if abs(u) < ROOT_BAND or abs(v) < ROOT_BAND:
            fragile = True
        if not (u > 0 and v > 0):
            continue
        f = 1 + u * u - 2 * b12 * u
        if not f > 0:
            continue
        l1 = np.sqrt(a12 / f)
        lam = np.array([l1, u * l1, v * l1])
        Xc = lam[:, None] * Y
        got = np.array([np.linalg.norm(Xc[0] - Xc[1]), np.linalg.norm(Xc[0] - Xc[2]), np.linalg.norm(Xc[1] - Xc[2])])
        res = np.abs(got - side).max() / side.max()
        if res > CONSTRAINT_TOL / 100:
            fragile = fragile or res < CONSTRAINT_TOL * 100
        if res > CONSTRAINT_TOL:
            continue
        sols.append(kabsch(Pw, Xc))
    return sols, fragile


def known_rotation(R, Pw, Y):
    """t of (I - y y^T)(R p + t) = 0 over two points; (pose list, fragile)"""
    A = Pw @ R.T
    N = np.zeros((3, 3))
    rhs = np.zeros(3)
    for a, y in zip(A, Y):
        M = np.eye(3) - np.outer(y, y)
        N += M
        rhs -= M @ a
    t = np.linalg.solve(N, rhs)
    depth = np.einsum("ij,ij->i", Y, A + t)
    fragile = bool((np.abs(depth) < ROOT_BAND * np.linalg.norm(A + t, axis=1)).any())
    if not np.isfinite(t).all() or not (depth > 0).all():
        return [], fragile
    return [(R, t)], fragile


def so3_exp(w):
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-12:
        return np.eye(3) + K
    return np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * K @ K


def refit(R, t, P, B, iters):
    """Gauss-Newton by lstsq on r = unit(R p + t) - b, x <- x + w x x + v"""
    for _ in range(iters):
        X = P @ R.T + t
        nrm = np.linalg.norm(X, axis=1)
        U = X / nrm[:, None]
        r = (U - B).reshape(-1)
        J = np.zeros((len(P), 3, 6))
        for i in range(len(P)):
            M = (np.eye(3) - np.outer(U[i], U[i])) / nrm[i]
            x = X[i]
            Xx = np.array([[0, -x[2], x[1]], [x[2], 0, -x[0]], [-x[1], x[0], 0]])
            J[i, :, :3] = -M @ Xx
            J[i, :, 3:] = M
        d = np.linalg.lstsq(J.reshape(-1, 6), -r, rcond=None)[0]
        Q = so3_exp(d[:3])
        R, t = Q @ R, Q @ t + d[3:]
    return R, t


def rot_angle(Ra, Rb):
    c = (np.trace(Ra.T @ Rb) - 1) / 2
    return float(np.arccos(np.clip(c, -1, 1))) if c < 0.999999 else float(np.linalg.norm(Ra - Rb) / np.sqrt(2))


class Reference:
    """The whole stage on one input: per-row poses, skip / fragile flags and count brackets, the winner, its
    brackets and masks, the minimal and the refit pose."""

    def __init__(self, points, bearings, samples, thresh, min_pair, R_known=None, min_inliers=10, refit_iters=5,
                 only_row=None):
        self.P = np.asarray(points, np.float32).astype(np.float64).reshape(-1, 3)
        self.B = np.asarray(bearings, np.float32).astype(np.float64).reshape(-1, 3)
        self.S = np.asarray(samples).reshape(-1, 3)
        self.thr, self.min_pair = float(np.float32(thresh)), float(np.float32(min_pair))
        self.Rk = None if R_known is None else np.asarray(R_known, np.float32).astype(np.float64).reshape(3, 3)
        self.band = angle_band(self.thr)
        n, H = len(self.P), len(self.S)
        self.n, self.H = n, H
        used = 2 if self.Rk is not None else 3
        self.launched = n >= used + 1 and H > 0
        self.skipped = np.ones(H, bool)
        self.fragile = np.zeros(H, bool)
        self.lo = -np.ones(H, int)
        self.hi = -np.ones(H, int)
        self.count = -np.ones(H, int)
        self.poses = [[] for _ in range(H)]
        self.sol_lo = [[] for _ in range(H)]
        self.sol_hi = [[] for _ in range(H)]
        self.sol_count = [[] for _ in range(H)]
        self.finite = np.isfinite(self.P).all(1) & np.isfinite(self.B).all(1)
        if self.launched:
            for h in (range(H) if only_row is None else [only_row]):
                self._row(h, used)
        self._select(min_inliers, refit_iters)

    def _row(self, h, used):
        idx = self.S[h, :used]
        if len(set(int(i) for i in idx)) < used or not self.finite[idx].all():
            return
        Pw, Bs = self.P[idx], self.B[idx]
        Y = Bs / np.linalg.norm(Bs, axis=1)[:, None]
        for i in range(used):
            for j in range(i + 1, used):
                ang = pair_angle(Y[i], Y[j])
                if abs(ang - self.min_pair) < SKIP_BAND * self.min_pair:
                    self.fragile[h] = True
                if ang <= self.min_pair:
                    return
        if used == 3:
            e1, e2 = Pw[1] - Pw[0], Pw[2] - Pw[0]
            den = (e1 @ e1) * (e2 @ e2)
            c = np.cross(e1, e2)
            s2 = (c @ c) / den if den > 0 else 0.0
            if abs(s2 - COLLINEAR2) < SKIP_BAND * COLLINEAR2:
                self.fragile[h] = True
            if not s2 > COLLINEAR2:
                return
            sols, frag = p3p(Pw, Y)
        else:
            sols, frag = known_rotation(self.Rk, Pw, Y)
        self.fragile[h] |= frag
        if not sols:
            return
        self.skipped[h] = False
        self.poses[h] = sols
        for R, t in sols:
            yes, und = classify(angles(R, t, self.P, self.B), self.thr, self.band)
            nominal = angles(R, t, self.P, self.B)
            with np.errstate(invalid="ignore"):
                self.sol_count[h].append(int((nominal <= self.thr).sum()))
            self.sol_lo[h].append(int(yes.sum()))
            self.sol_hi[h].append(int(yes.sum() + und.sum()))
        self.lo[h], self.hi[h], self.count[h] = max(self.sol_lo[h]), max(self.sol_hi[h]), max(self.sol_count[h])

    def _select(self, min_inliers, refit_iters):
        self.best = -1
        self.decided = True
        self.status = TOO_FEW if not self.launched else NO_MODEL
        self.best_solution = -1
        self.mask = np.zeros(self.n, bool)
        self.undecided = np.zeros(self.n, bool)
        self.R0 = self.R = np.zeros((3, 3))
        self.t0 = self.t = np.zeros(3)
        self.refit_kept = 0
        self.status_decided = True
        if not self.launched or (self.count < 0).all():
            return
        b = int(np.argmax(self.count))  # the first of the largest
        self.best = b
        self.decided = bool((self.lo[b] > self.hi[:b]).all() and (self.lo[b] >= self.hi[b + 1:]).all())
        slo, shi = np.array(self.sol_lo[b]), np.array(self.sol_hi[b])
        s = int(np.argmax(self.sol_count[b]))
        self.best_solution = s
        self.solution_decided = bool((slo[s] > shi[:s]).all() and (slo[s] >= shi[s + 1:]).all())
        self.win_lo, self.win_hi = int(slo[s]), int(shi[s])
        self.status_decided = self.win_lo >= min_inliers or self.win_hi < min_inliers
        self.status = FEW_INLIERS if self.win_hi < min_inliers else OK
        self.R0, self.t0 = self.poses[b][s]
        ang0 = angles(self.R0, self.t0, self.P, self.B)
        yes0, und0 = classify(ang0, self.thr, self.band)
        self.R, self.t, self.mask, self.undecided = self.R0, self.t0, yes0, und0
        self.final_lo, self.final_hi = self.win_lo, self.win_hi
        self.kept_decided = True
        if refit_iters > 0 and self.win_lo >= 3:
            with np.errstate(invalid="ignore"):
                inl = ang0 <= self.thr
            R1, t1 = refit(self.R0, self.t0, self.P[inl], self.B[inl], refit_iters)
            self.R1, self.t1 = R1, t1
            yes1, und1 = classify(angles(R1, t1, self.P, self.B), self.thr, self.band)
            lo1, hi1 = int(yes1.sum()), int(yes1.sum() + und1.sum())
            self.kept_decided = lo1 >= self.win_hi or hi1 < self.win_lo
            if lo1 >= self.win_lo:
                self.refit_kept = 1
                self.R, self.t, self.mask, self.undecided = R1, t1, yes1, und1
                self.final_lo, self.final_hi = lo1, hi1
        with np.errstate(invalid="ignore"):
            a = angles(self.R, self.t, self.P, self.B)
            self.rms = float(np.sqrt(np.mean(a[self.mask] ** 2))) if self.mask.any() else 0.0


def ulp_cloud(points, bearings, samples, thresh, min_pair, R_known, refit_iters, row, copies=8, seed=0):
    """The reference's winner row on `copies` inputs whose bearings moved by +-1 ulp f32: the spread of the minimal
    and of the refit pose (rotation angle, translation distance) against the unperturbed reference."""
    base = Reference(points, bearings, samples, thresh, min_pair, R_known, 0, refit_iters, only_row=row)
    rng = np.random.default_rng(seed)
    B = np.asarray(bearings, np.float32)
    spread = {"R0": 0.0, "t0": 0.0, "R": 0.0, "t": 0.0}
    for _ in range(copies):
        up = rng.integers(0, 2, B.shape).astype(bool)
        Bc = np.where(up, np.nextafter(B, np.float32(2)), np.nextafter(B, np.float32(-2))).astype(np.float32)
        r = Reference(points, Bc, samples, thresh, min_pair, R_known, 0, refit_iters, only_row=row)
        if r.best != row or len(r.poses[row]) != len(base.poses[row]):
            continue
        spread["R0"] = max(spread["R0"], rot_angle(base.R0, r.R0))
        spread["t0"] = max(spread["t0"], float(np.linalg.norm(base.t0 - r.t0)))
        spread["R"] = max(spread["R"], rot_angle(base.R, r.R))
        spread["t"] = max(spread["t"], float(np.linalg.norm(base.t - r.t)))
    return spread


def assert_preconditions(r, poses=False, max_fragile=0.03):
    """What a comparison against `r` presupposes, asserted on the reference alone."""
    assert r.fragile.mean() <= max_fragile if r.H else True, float(r.fragile.mean())
    if not r.launched or r.best < 0:
        return
    assert r.decided, "the winner is inside the band"
    assert not r.fragile[r.best], "the winner row is fragile"
    assert r.solution_decided and r.status_decided and r.kept_decided
    if poses:
        assert r.win_hi == r.win_lo  # the refit's input set is then the same on both sides
