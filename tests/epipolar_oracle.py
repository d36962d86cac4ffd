"""TEST INFRASTRUCTURE: the known-rotation epipolar RANSAC (include/vio360.h, erp_epi_params) restated in NumPy f32,
every expression in the header's written order (NumPy's f32 element-wise loops do not contract a*b+c).  Bearings and
the rotation stage come from the C oracle (oracle_lib.pixel_to_bearing / rot_ransac / oracle_kabsch_rotation).
Used by tests/test_epipolar.py (against the f64 reference) and tests/test_epipolar_gpu.py (bitwise)."""
import ctypes as C
import math

import numpy as np

import oracle_lib

F = np.float32


def cos_bound(thr):
    """ransac_cos_bound: the smallest float c in [-1, 1] with (float)acos((double)c) < thr, by bisection over the
    floats' order; +inf when none passes.  (Adjacent floats near the crossing differ in acos by ~1e-6, far above a
    double acos' error, so libm's acos decides as the device's does.)"""
    thr = F(thr)

    def passes(c):
        return F(math.acos(float(c))) < thr

    def order(x):
        b = int(F(x).view(np.uint32))
        return (~b & 0xffffffff) if b >> 31 else (b | 0x80000000)

    def unorder(m):
        return np.uint32((m & 0x7fffffff) if m >> 31 else (~m & 0xffffffff)).view(np.float32)

    if not passes(F(1.0)):
        return F(np.inf)
    lo, hi = order(-1.0), order(1.0)
    while lo < hi:
        mid = lo + (hi - lo) // 2
        if passes(unorder(mid)):
            hi = mid
        else:
            lo = mid + 1
    return unorder(hi)


def thresholds(prm):
    """(cmin, cmax, s2_epi, s2_plane): formed once in double, rounded to float"""
    se, sp = math.sin(float(F(prm.epi_thresh_rad))), math.sin(float(F(prm.min_plane_angle_rad)))
    return (cos_bound(prm.rot_thresh_rad), F(math.cos(float(F(prm.max_parallax_rad)))), F(se * se), F(sp * sp))


def bearings(p, W, H):
    p = np.ascontiguousarray(p, np.float32).reshape(-1, 2)
    return np.array([oracle_lib.pixel_to_bearing(float(u), float(v), W, H) for u, v in p], np.float32).reshape(-1, 3)


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(a, q):
    return (a[1] * q[2] - a[2] * q[1], a[2] * q[0] - a[0] * q[2], a[0] * q[1] - a[1] * q[0])


def rot_best(b0, b1, samples, cmin):
    """The rotation RANSAC's best hypothesis as ransac_hyp_kernel / ransac_best form it: (index, R (9,) f32), or
    (-1, None).  Counts are > 0 for a winner; the first strictly greatest wins."""
    L = oracle_lib.load()
    S = np.asarray(samples, np.int32).reshape(-1, 3)
    n = len(b0)
    if n < 3 or len(S) == 0:
        return -1, None
    Hm = np.zeros((len(S), 3, 3), np.float32)
    for s in range(3):
        Hm = Hm + b1[S[:, s]][:, :, None] * b0[S[:, s]][:, None, :]
    Rs = np.zeros((len(S), 9), np.float32)
    for it in range(len(S)):
        h = np.ascontiguousarray(Hm[it].reshape(9))
        L.oracle_kabsch_rotation(h.ctypes.data_as(C.c_void_p), Rs[it].ctypes.data_as(C.c_void_p))
    m = Rs.T
    det = m[0] * (m[4] * m[8] - m[7] * m[5]) - m[3] * (m[1] * m[8] - m[7] * m[2]) + m[6] * (m[1] * m[5] - m[4] * m[2])
    ok = ~(np.abs(det - F(1.0)) > F(0.1))
    x, y, z = b0[:, 0][None, :], b0[:, 1][None, :], b0[:, 2][None, :]
    r = [(Rs[:, 3 * k][:, None] * x + Rs[:, 3 * k + 1][:, None] * y) + Rs[:, 3 * k + 2][:, None] * z for k in range(3)]
    c = (r[0] * b1[:, 0][None, :] + r[1] * b1[:, 1][None, :]) + r[2] * b1[:, 2][None, :]
    c = np.clip(c, F(-1.0), F(1.0))
    counts = np.where(ok, (c >= cmin).sum(axis=1), -1)
    best, bi = 0, -1
    for it, cnt in enumerate(counts):
        if cnt > best:
            best, bi = int(cnt), it
    return bi, (Rs[bi].copy() if bi >= 0 else None)


class Points:
    """the per-point terms under R"""

    def __init__(self, R, b0, b1, cmin, cmax):
        R = np.asarray(R, np.float32).reshape(9)
        x, y, z = b0[:, 0], b0[:, 1], b0[:, 2]
        self.a = [(R[3 * k] * x + R[3 * k + 1] * y) + R[3 * k + 2] * z for k in range(3)]
        q = [b1[:, 0], b1[:, 1], b1[:, 2]]
        self.c = _dot(self.a, q)
        self.nrm = list(_cross(self.a, q))
        self.nn = _dot(self.nrm, self.nrm)
        self.rin = np.clip(self.c, F(-1.0), F(1.0)) >= cmin
        self.par_ok = self.c >= cmax
        self.n = len(b0)

    def model(self, i, j, s2_plane):
        """t, tt of hypothesis (i, j); None when it is skipped"""
        if self.rin[i] or self.rin[j]:
            return None
        t = _cross([v[i] for v in self.nrm], [v[j] for v in self.nrm])
        tt = _dot(t, t)
        if not tt >= s2_plane * (self.nn[i] * self.nn[j]):
            return None
        return t, tt

    def votes(self, t, tt, s2_epi):
        """+1 / -1 / 0 per point"""
        m = _cross(t, self.a)
        mm = _dot(m, m)
        e = _dot(t, self.nrm)
        on_plane = (mm > F(1e-6) * tt) & (e * e < s2_epi * mm)
        s = -_dot(self.nrm, m)
        v = np.where(on_plane & (s > 0), 1, np.where(on_plane & (s < 0), -1, 0))
        return np.where(~self.rin & self.par_ok, v, 0)


def _info(n_rot=0, n_rescued=0, best=-1, model_valid=0, t_dir=None):
    return {"n_rot": int(n_rot), "n_rescued": int(n_rescued), "best": int(best), "model_valid": int(model_valid),
            "t_dir": np.zeros(3, np.float32) if t_dir is None else np.asarray(t_dir, np.float32)}


def run_bearings(b0, b1, R, samples, prm, min_n=2):
    """The rule on bearings with R known -> dict(mask, n_in, counts, info, pts)."""
    cmin, cmax, s2_epi, s2_plane = thresholds(prm)
    S = np.asarray(samples, np.int32).reshape(-1, 3)
    P = Points(R, b0, b1, cmin, cmax)
    n, n_rot = P.n, int(P.rin.sum())
    counts = np.full(len(S), -1, np.int32)
    resc = np.zeros(len(S), np.int32)
    sig = np.ones(len(S), np.int32)
    best, bi = -1, -1
    with np.errstate(all="ignore"):
        if n >= min_n:
            for it, (i, j, _) in enumerate(S):
                mod = P.model(i, j, s2_plane)
                if mod is None:
                    continue
                v = P.votes(mod[0], mod[1], s2_epi)
                pos, neg = int((v > 0).sum()), int((v < 0).sum())
                resc[it], sig[it] = max(pos, neg), (1 if pos >= neg else -1)
                counts[it] = n_rot + resc[it]
                if counts[it] > best:
                    best, bi = int(counts[it]), it
        mask = P.rin.copy()
        info = _info(n_rot, best=bi)
        if bi >= 0 and resc[bi] >= prm.min_support:
            t, tt = P.model(S[bi][0], S[bi][1], s2_plane)
            mask = P.rin | (P.votes(t, tt, s2_epi) == sig[bi])
            nr = np.sqrt(tt)
            d = [(-c if sig[bi] > 0 else c) / nr for c in t]
            info = _info(n_rot, resc[bi], bi, 1, d)
    return {"mask": mask.astype(np.uint8), "n_in": n_rot + info["n_rescued"], "counts": counts, "info": info, "pts": P,
            "evaluated": n >= min_n and len(S) > 0}


def run(p0, p1, W, H, samples, prm, R=None, min_n=2, rot_samples=None):
    """erp_epi_ransac on pixels.  R None: the rotation RANSAC first, on rot_samples (default: samples)."""
    p0 = np.ascontiguousarray(p0, np.float32).reshape(-1, 2)
    p1 = np.ascontiguousarray(p1, np.float32).reshape(-1, 2)
    S = np.asarray(samples, np.int32).reshape(-1, 3)
    n = len(p0)
    none = np.full(len(S), -1, np.int32)
    if n == 0 or (R is None and n < 3):
        return {"mask": np.ones(n, np.uint8), "n_in": n, "counts": none, "info": _info(n), "evaluated": False}
    b0, b1 = bearings(p0, W, H), bearings(p1, W, H)
    if R is None:
        RS = S if rot_samples is None else np.asarray(rot_samples, np.int32).reshape(-1, 3)
        rmask, rnin = oracle_lib.rot_ransac(p0, p1, W, H, RS, float(F(prm.rot_thresh_rad)))
        bi, R = rot_best(b0, b1, RS, cos_bound(prm.rot_thresh_rad))
        if bi < 0:
            return {"mask": rmask, "n_in": rnin, "counts": none, "info": _info(rnin), "evaluated": False}
        out = run_bearings(b0, b1, R, S, prm, min_n)
        # the restated rotation test under the restated best rotation is the C oracle's mask
        assert np.array_equal(out["pts"].rin.astype(np.uint8), rmask) and int(rmask.sum()) == rnin
        out["rot_mask"] = rmask
        return out
    return run_bearings(b0, b1, np.asarray(R, np.float32).reshape(9), S, prm, min_n)
