"""Independent float64 restatement of the two-view initialiser — TEST INFRASTRUCTURE ONLY.

Written from the reference's src/processing/Initializer.cpp alone (ComputeEssentialMatrix :458-621,
RecoverPose :623-697, TriangulatePoints / TriangulateSinglePoint :699-783, TestPoseCandidate :785-835,
ComputeReprojectionErrorInFrame :837-871, ValidateInitialization :889-995, NormalizeScale :997-1048, and
the call order of TryMonocularInitialization :117-166).  numpy only; it loads neither the CPU oracle nor
the device library, and shares no code with them.  It restates WHAT is computed, not how:

  * the epipolar rows are the f32 products b2[r]*b1[c] (the reference's A is a MatrixXf), read as f64;
  * every null vector and every 3x3 SVD is np.linalg.svd of the matrix itself (never A^T A);
  * every per-point quantity (|b2^T E b1|, the mid-point, the no-wrap pixel error, depths, median) is
    f64 arithmetic on the f32 inputs.

So what it pins is the exact null vector of the f32-built system and every threshold, comparison and
convention of Initializer.cpp; what it cannot pin is bit parity with Eigen's f32 JacobiSVD.

Every comparison is made up to what the reference leaves free (E up to sign, the pose candidates as a
set of four), and every thresholded count is bracketed: a point whose f64 value lies within a band of
the threshold is UNDECIDED, and the count under test must lie in [lo, hi] with lo = decided passes,
hi = lo + undecided.  check_against_reference() applies the same bars to the CPU oracle and to the
device.  Every precondition (decided winner, undecided shares, excluded shares, hi - lo) is asserted on
the reference alone, before the result under test is looked at.

Measured constants (measure_constants(), over every case of init_cases.REFERENCE_CASES at
960x480 and 3840x1920, at this reference's own estimated pose rounded to f32; tri32 / reproj32 below
are TriangulateSinglePoint / ComputeReprojectionErrorInFrame in numpy float32, source expression order):

  * mid-point:  max over points of  rel_i * sin^2(theta_i) / 2^-23  of tri32 against the f64 mid-point
    = 55.02 (points with |det| < 1e-6 excluded; the maximum is a gross outlier of the 30 % outlier case
    whose mid-point lies 0.018 baselines from the camera, every other case stays below 17).  Doubled
    and rounded up to a power of two: K = 128.
  * pixel error: max |reproj32(tri32) - reproj f64(tri f64)| per 960 px of width = 0.00945 px (the
    larger of frame 1 and frame 2, over the points both of whose f64 errors are below 10 px: no test
    here has a threshold above 5 px, and a gross outlier's mid-point can sit at a camera centre, where
    its direction means nothing; points with |det| < 1e-6 or on the seam excluded).  ComputeReprojection-
    ErrorInFrame alone, on the same f32 point, deviates by at most 0.0012 px.  Times 4:
    PIX_BAND_960 = 0.0378 px, scaled by width / 960.
tests/test_init_reference.py::test_constants_are_measured repeats the measurement.
"""
import numpy as np

# VIO_INIT_* of include/vio360.h, in the order TryMonocularInitialization returns false (:117-166)
OK, TOO_FEW_BEARINGS, ESSENTIAL_FAILED, POSE_FAILED, TRIANGULATION, VALIDATION = range(6)

EPI_BAND = 1e-5        # on |b2^T E b1| <= 1: ~10x the f32 rounding of E plus the three-term f32 dots
SEAM_BAND = 1e-5       # rad: |theta| this close to pi, observed or projected, is undecided
DET_MIN = 1e-6         # sin^2 of the parallax angle below which a mid-point is not compared
CANDIDATE_PX = 5.0     # kReprojErrThr of TestPoseCandidate (:817)
MEASURED_K_RATIO = 55.02   # measure_constants() over every case, see the docstring
K_MIDPOINT = 128.0         # 2 x 55.02 rounded up to a power of two
MEASURED_PIX_960 = 0.00945
PIX_BAND_960 = 4 * MEASURED_PIX_960
U23 = 2.0 ** -23


# ------------------------------------------------------------------------------------------------
# ComputeEssentialMatrix
def epipolar_rows(b1, b2):
    """(n, 9) rows A(i, 3r + c) = b2[r] * b1[c] (:510-518): f32 products, read as f64."""
    b1 = np.asarray(b1, np.float32)
    b2 = np.asarray(b2, np.float32)
    return (b2[:, :, None] * b1[:, None, :]).reshape(-1, 9).astype(np.float64)


def project_essential(e):
    """:525-538: E <- U diag(s, s, 0) V^T, s = (s0 + s1) / 2, of the row-major 3x3 of e."""
    U, s, Vt = np.linalg.svd(np.asarray(e, np.float64).reshape(3, 3))
    sg = 0.5 * (s[0] + s[1])
    return U @ np.diag([sg, sg, 0.0]) @ Vt


def essential_from_rows(A):
    """V.col(8) of the SVD of A itself (:522-523, :604-605), projected.  Also sigma_8 / sigma_1."""
    _, s, Vt = np.linalg.svd(A, full_matrices=True)
    ratio = s[7] / s[0] if len(s) >= 8 and s[0] > 0 else 0.0
    return project_essential(Vt[8]), ratio


def hypotheses(b1, b2, S):
    """One E per sample row of S (H, 8): (H, 3, 3) and the rows' sigma_8 / sigma_1."""
    S = np.asarray(S).reshape(-1, 8)
    A = epipolar_rows(b1, b2)
    E = np.zeros((len(S), 3, 3))
    ratio = np.zeros(len(S))
    for h, row in enumerate(S):
        E[h], ratio[h] = essential_from_rows(A[row])
    return E, ratio


def epipolar_error(E, b1, b2):
    """|b2^T E b1| (:551) in f64; E (..., 3, 3) -> (..., n)."""
    return np.abs(np.einsum("ni,...ij,nj->...n", np.asarray(b2, np.float64), E, np.asarray(b1, np.float64)))


def split(value, thr, band):
    """value < thr up to a band: (decided pass, undecided)."""
    return value < thr - band, np.abs(value - thr) <= band


def ransac_reference(b1, b2, S, thr):
    """The hypothesis stage and the winner (:483-573) with their brackets, on the reference alone."""
    E, ratio = hypotheses(b1, b2, S)
    err = epipolar_error(E, b1, b2)
    dec, und = split(err, np.float64(np.float32(thr)), EPI_BAND)
    lo = dec.sum(1)
    hi = lo + und.sum(1)
    # first strictly best: the earliest row whose count no later row exceeds and no earlier row reaches
    cnt = (err < np.float64(np.float32(thr))).sum(1)
    best, bc = -1, 0
    for h in range(len(cnt)):
        if cnt[h] > bc:
            best, bc = h, int(cnt[h])
    decided = best < 0 and hi.max(initial=0) == 0
    if best >= 0:
        decided = bool((lo[best] > hi[:best]).all() and (lo[best] >= hi[best + 1:]).all())
    return {"E": E, "ratio": ratio, "err": err, "pass": dec, "undecided": und, "lo": lo, "hi": hi,
            "best": best, "winner_decided": decided}


# ------------------------------------------------------------------------------------------------
# RecoverPose
def pose_candidates(E):
    """The four (R, t) of :631-663, in the reference's order."""
    U, _, Vt = np.linalg.svd(np.asarray(E, np.float64))
    W = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    R1 = U @ W @ Vt
    R2 = U @ W.T @ Vt
    t1 = U[:, 2].copy()
    if np.linalg.det(R1) < 0:
        R1, t1 = -R1, -t1
    if np.linalg.det(R2) < 0:
        R2 = -R2
    t1 = t1 / np.linalg.norm(t1)
    return [(R1, t1), (R1, -t1), (R2, t1), (R2, -t1)]


def triangulate(b1, b2, R, t):
    """TriangulateSinglePoint (:728-783) for every pair, f64.  Returns X (n, 3), ok (n,), det (n,)."""
    b1 = np.asarray(b1, np.float64)
    b2 = np.asarray(b2, np.float64)
    trans_12 = -(R.T @ t)
    b21 = b2 @ R                      # rows R^T b2
    a00 = (b1 * b1).sum(1)
    a10 = (b1 * b21).sum(1)
    a01 = -a10
    a11 = -(b21 * b21).sum(1)
    r0 = b1 @ trans_12
    r1 = b21 @ trans_12
    det = a00 * a11 - a01 * a10
    with np.errstate(divide="ignore", invalid="ignore"):
        l0 = (a11 * r0 - a01 * r1) / det
        l1 = (-a10 * r0 + a00 * r1) / det
        X = (l0[:, None] * b1 + (l1[:, None] * b21 + trans_12)) / 2.0
    ok = ~(np.abs(det) < 1e-10) & np.isfinite(l0) & np.isfinite(l1)
    X = np.where(ok[:, None], X, 0.0)
    return X, ok, det


def reproj(p, b, width, height):
    """ComputeReprojectionErrorInFrame (:837-871), f64, NO wrap-around.  Returns the pixel error and
    whether the observed or the projected longitude lies within SEAM_BAND of +-pi."""
    p = np.asarray(p, np.float64)
    b = np.asarray(b, np.float64)
    L = np.linalg.norm(p, axis=1)
    safe = np.where(L < 1e-6, 1.0, L)
    th_o = np.arctan2(b[:, 0], b[:, 2])
    ph_o = -np.arcsin(np.clip(b[:, 1], -1.0, 1.0))
    q = p / safe[:, None]
    th_p = np.arctan2(q[:, 0], q[:, 2])
    ph_p = -np.arcsin(np.clip(q[:, 1], -1.0, 1.0))
    du = width * (0.5 + th_o / (2.0 * np.pi)) - width * (0.5 + th_p / (2.0 * np.pi))
    dv = height * (0.5 - ph_o / np.pi) - height * (0.5 - ph_p / np.pi)
    e = np.where(L < 1e-6, 1000.0, np.sqrt(du * du + dv * dv))
    seam = (np.pi - np.abs(th_o) <= SEAM_BAND) | (np.pi - np.abs(th_p) <= SEAM_BAND)
    return e, seam


def point_terms(b1, b2, R, t, width, height):
    """Mid-points and both frames' pixel errors under (R, t); `fuzzy` marks the points whose f32
    evaluation may land on either side of any test: vanishing parallax, the seam, a mid-point at the
    origin (the 1e-6 guards of :846 and :916)."""
    X, ok, det = triangulate(b1, b2, R, t)
    er, s1 = reproj(X, b1, width, height)
    X2 = X @ R.T + t
    ec, s2 = reproj(X2, b2, width, height)
    small = (np.linalg.norm(X, axis=1) < 1e-5) | (np.linalg.norm(X2, axis=1) < 1e-5)
    fuzzy = (np.abs(det) < DET_MIN) | s1 | s2 | small
    return {"X": X, "ok": ok, "det": det, "er": er, "ec": ec, "fuzzy": fuzzy}


def count_bounds(T, mask, thr, band):
    """[lo, hi] of the points of `mask` with both pixel errors below thr, and the decided passes."""
    mask = np.asarray(mask, bool)
    dec = mask & ~T["fuzzy"] & T["ok"] & (T["er"] < thr - band) & (T["ec"] < thr - band)
    fail = mask & ~T["fuzzy"] & ((T["er"] > thr + band) | (T["ec"] > thr + band))
    und = mask & ~dec & ~fail
    return int(dec.sum()), int(dec.sum() + und.sum()), dec, und


def pix_band(width):
    return PIX_BAND_960 * width / 960.0


def midpoint_bound(det):
    """Relative bound of an f32 mid-point: K * 2^-23 / sin^2(theta), sin^2(theta) = |det|."""
    with np.errstate(divide="ignore"):
        return K_MIDPOINT * U23 / np.abs(det)


def median(d):
    """:1026-1033: mean of the two middle values for an even count, the middle one for an odd count."""
    d = np.sort(np.asarray(d, np.float64))
    mid = len(d) // 2
    return 0.5 * (d[mid - 1] + d[mid]) if len(d) % 2 == 0 else d[mid]


def scale_bounds(X, det):
    """Bracket of the median depth (:1005-1033) of f32 mid-points that obey midpoint_bound().  A point
    that may or may not enter the depth list (no parallax, or a norm near the 1e-6 / 0.01 guards) enters
    at 0 for the lower and at +inf for the upper bound: the median is monotone in every entry."""
    nrm = np.linalg.norm(X, axis=1)
    dl = midpoint_bound(det)
    free = (np.abs(det) < DET_MIN) | (nrm * (1 - np.minimum(dl, 1.0)) <= 0.01)
    low = np.where(free, 0.0, nrm * (1 - dl))
    high = np.where(free, np.inf, nrm * (1 + dl))
    return median(low), median(high)


# ------------------------------------------------------------------------------------------------
# f32 helpers: used only to measure K_MIDPOINT and PIX_BAND_960
def _dot32(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def tri32(b1, b2, R, t):
    """TriangulateSinglePoint in numpy float32, in the source's expression order."""
    f = np.float32
    b1 = np.asarray(b1, f)
    b2 = np.asarray(b2, f)
    R = np.asarray(R, f)
    t = np.asarray(t, f)
    Rt = R.T
    trans_12 = -np.array([(Rt[r, 0] * t[0] + Rt[r, 1] * t[1]) + Rt[r, 2] * t[2] for r in range(3)], f)
    b21 = np.stack([(Rt[r, 0] * b2[:, 0] + Rt[r, 1] * b2[:, 1]) + Rt[r, 2] * b2[:, 2] for r in range(3)], 1)
    tr = np.broadcast_to(trans_12, b1.shape)
    a00 = _dot32(b1, b1)
    a10 = _dot32(b1, b21)
    a01 = -a10
    a11 = -_dot32(b21, b21)
    r0 = _dot32(b1, tr)
    r1 = _dot32(b21, tr)
    det = a00 * a11 - a01 * a10
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = f(1.0) / det
        l0 = (a11 * inv) * r0 + (-a01 * inv) * r1
        l1 = (-a10 * inv) * r0 + (a00 * inv) * r1
        X = (l0[:, None] * b1 + (l1[:, None] * b21 + tr)) / f(2.0)
    ok = ~(np.abs(det) < f(1e-10)) & np.isfinite(l0) & np.isfinite(l1)
    assert X.dtype == np.float32
    return np.where(ok[:, None], X, f(0.0)), ok


def reproj32(p, b, width, height):
    """ComputeReprojectionErrorInFrame in numpy float32: float angles, the double pixel maps of
    `0.5f + theta / (2.0f * M_PI)` rounded to float, float differences and norm."""
    f = np.float32
    p = np.asarray(p, f)
    b = np.asarray(b, f)
    L = np.sqrt(_dot32(p, p))
    safe = np.where(L < f(1e-6), f(1.0), L)

    def pix(v):
        th = np.arctan2(v[:, 0], v[:, 2])
        ph = -np.arcsin(np.clip(v[:, 1], f(-1.0), f(1.0)))
        u = (width * (0.5 + th.astype(np.float64) / (2.0 * np.pi))).astype(f)
        w = (height * (0.5 - ph.astype(np.float64) / np.pi)).astype(f)
        return u, w
    uo, vo = pix(b)
    up, vp = pix(p / safe[:, None])
    du, dv = uo - up, vo - vp
    e = np.sqrt(du * du + dv * dv)
    assert e.dtype == np.float32
    return np.where(L < f(1e-6), f(1000.0), e)


# ------------------------------------------------------------------------------------------------
# the reference's own end-to-end run (its own mask, E, pose): truth checks, constants, preconditions
def reference_run(b1, b2, S, params, ransac=None):
    n = len(b1)
    W, H = params.width, params.height
    out = {"status": OK, "best": -1, "num_inliers": 0}
    if n < 5:
        out["status"] = TOO_FEW_BEARINGS
        return out
    rr = ransac if ransac is not None else ransac_reference(b1, b2, S, params.ransac_threshold)
    out["ransac"] = rr
    out["best"] = rr["best"]
    if rr["best"] < 0:
        out["status"] = ESSENTIAL_FAILED
        return out
    mask = rr["err"][rr["best"]] < np.float64(np.float32(params.ransac_threshold))
    out["mask"] = mask
    out["num_inliers"] = int(mask.sum())
    if out["num_inliers"] < params.min_features:
        out["status"] = ESSENTIAL_FAILED
        return out
    E, _ = essential_from_rows(epipolar_rows(b1, b2)[mask])
    out["E"] = E
    cands = pose_candidates(E)
    terms = [point_terms(b1, b2, R, t, W, H) for R, t in cands]
    good = [int((mask & T["ok"] & (T["er"] < CANDIDATE_PX) & (T["ec"] < CANDIDATE_PX)).sum()) for T in terms]
    out["candidate_good"] = good
    bi, bc = -1, 0
    for c in range(4):
        if good[c] > bc:
            bi, bc = c, good[c]
    out["pose_candidate"] = bi
    if bi < 0 or bc < params.min_features:
        out["status"] = POSE_FAILED
        return out
    R, t = cands[bi]
    T = terms[bi]
    out["R"], out["t_unit"], out["terms"] = R, t, T
    if int(T["ok"].sum()) < params.min_features:
        out["status"] = TRIANGULATION
        return out
    mx = np.float64(np.float32(params.max_reprojection_error))
    nrm = np.linalg.norm(T["X"], axis=1)
    valid = mask & ~(nrm < 1e-6) & ~(T["er"] > mx) & ~(T["ec"] > mx)
    out["num_valid"] = int(valid.sum())
    out["mean_reproj_error"] = float(np.maximum(T["er"], T["ec"])[valid].mean()) if valid.any() else 0.0
    if out["num_valid"] == 0 or out["num_valid"] < params.min_features:
        out["status"] = VALIDATION
        return out
    d = nrm[~(nrm < 1e-6) & (nrm > 0.01)]
    scale = 1.0 / median(d) if len(d) else 1.0
    out["scale_factor"] = scale
    out["points"] = T["X"] * scale
    out["t"] = t * scale
    return out


def measure_constants(b1, b2, ref, width, height):
    """(K ratio, pixel deviation per 960 px) of the f32 helpers at the reference's pose rounded to f32."""
    R32 = ref["R"].astype(np.float32)
    t32 = ref["t_unit"].astype(np.float32)
    R, t = R32.astype(np.float64), t32.astype(np.float64)
    T = point_terms(b1, b2, R, t, width, height)
    X32, ok32 = tri32(b1, b2, R32, t32)
    use = ~(np.abs(T["det"]) < DET_MIN) & ok32
    rel = np.linalg.norm(X32.astype(np.float64) - T["X"], axis=1) / np.linalg.norm(T["X"], axis=1)
    kr = float((rel * np.abs(T["det"]) / U23)[use].max())
    er32 = reproj32(X32, b1, width, height)
    X2 = ((R32[:, 0] * X32[:, 0:1] + R32[:, 1] * X32[:, 1:2]) + R32[:, 2] * X32[:, 2:3]) + t32
    ec32 = reproj32(X2, b2, width, height)
    # points whose f64 error is beyond twice the largest threshold any test applies (5 px) are decided by
    # a margin no rounding approaches (gross outliers, whose mid-points can sit at the origin of a frame)
    usep = use & ~T["fuzzy"] & (T["er"] < 2 * CANDIDATE_PX) & (T["ec"] < 2 * CANDIDATE_PX)
    dev = np.maximum(np.abs(er32 - T["er"]), np.abs(ec32 - T["ec"]))[usep].max()
    return kr, float(dev) * 960.0 / width


# ------------------------------------------------------------------------------------------------
def with_params(params, **kw):
    q = type(params)()
    for name, _ in params._fields_:
        setattr(q, name, kw.get(name, getattr(params, name)))
    return q


def _sign_gap(E, E_ref):
    return min(np.abs(E - E_ref).max(), np.abs(E + E_ref).max())


def _match_candidates(cands, R, t_unit):
    """Index of the reference candidate within 1e-6 of (R, t_unit), or -1."""
    gap = [max(np.abs(Rc - R).max(), np.abs(tc - t_unit).max()) for Rc, tc in cands]
    j = int(np.argmin(gap))
    return (j, gap[j]) if gap[j] <= 1e-6 else (-1, gap[j])


def check_against_reference(run, b1, b2, S, params, ransac=None, rows=64):
    """Every bar of the module docstring on `run(b1, b2, S, params) -> (result dict, mask, points)`.
    Returns the measured figures.  `ransac` may carry a cached ransac_reference() of the same case."""
    b1 = np.ascontiguousarray(b1, np.float32)
    b2 = np.ascontiguousarray(b2, np.float32)
    S = np.ascontiguousarray(S, np.int32).reshape(-1, 8)
    n, W, H = len(b1), params.width, params.height
    thr = np.float64(np.float32(params.ransac_threshold))
    mx = np.float64(np.float32(params.max_reprojection_error))
    band = pix_band(W)
    fig = {}

    # ---- preconditions, on the reference alone
    rr = ransac if ransac is not None else ransac_reference(b1, b2, S, params.ransac_threshold)
    own = reference_run(b1, b2, S, params, ransac=rr)
    k = min(rows, len(S))
    assert (rr["ratio"][:k] >= 1e-4).all(), ("degenerate sample row: change the seed", rr["ratio"][:k].min())
    fig["hyp_undecided_share"] = float(rr["undecided"][:k].mean())
    assert fig["hyp_undecided_share"] <= 1e-3, fig
    assert rr["winner_decided"], "the reference's winner is not decided: replace the case"
    best = rr["best"]
    lo_w, hi_w = int(rr["lo"][best]), int(rr["hi"][best])
    if own["status"] in (OK, VALIDATION, TRIANGULATION):
        T = own["terms"]
        fig["excluded_share"] = float((np.abs(T["det"]) < DET_MIN).mean())
        assert fig["excluded_share"] <= 5e-3, fig
        vlo, vhi, _, _ = count_bounds(T, own["mask"], mx, band)
        fig["own_valid_gap"] = (vhi - vlo) / max(1, own["num_inliers"])
        assert fig["own_valid_gap"] <= 0.05, fig

    # ---- a. hypothesis stage, one single-row call per sample row
    for h in range(k):
        P1 = with_params(params, ransac_iterations=1, min_features=n + 1)
        res, m, _ = run(b1, b2, S[h][None], P1)
        assert res["status"] == ESSENTIAL_FAILED and res["best_hypothesis"] == 0, (h, res)
        m = np.asarray(m, bool)
        und = rr["undecided"][h]
        assert np.array_equal(m[~und], rr["pass"][h][~und]), ("hypothesis mask", h)
        assert res["num_inliers"] == int(m.sum()), (h, res["num_inliers"], int(m.sum()))

    # ---- b. winner
    res, mask, X = run(b1, b2, S, params)
    mask = np.asarray(mask, bool)
    X = np.asarray(X, np.float64)
    assert res["best_hypothesis"] == best, (res["best_hypothesis"], best)
    assert lo_w <= res["num_inliers"] <= hi_w, (res["num_inliers"], lo_w, hi_w)
    assert res["num_inliers"] == int(mask.sum())
    und = rr["undecided"][best]
    assert np.array_equal(mask[~und], rr["pass"][best][~und]), "winner mask"
    if hi_w < params.min_features:
        assert res["status"] == ESSENTIAL_FAILED, res
        return fig
    if res["status"] == ESSENTIAL_FAILED:
        assert lo_w < params.min_features, res
        return fig

    # ---- c. refit, from the returned mask (a border point cannot move it)
    E = res["E"].astype(np.float64)
    E_ref, _ = essential_from_rows(epipolar_rows(b1, b2)[mask])
    fig["E_gap"] = _sign_gap(E, E_ref) / np.abs(E_ref).max()
    assert fig["E_gap"] <= 1e-6, fig

    # ---- d. pose: the candidate set of the returned E
    cands = pose_candidates(E)
    terms = [point_terms(b1, b2, R, t, W, H) for R, t in cands]
    bounds = [count_bounds(T, mask, CANDIDATE_PX, band)[:2] for T in terms]
    good = list(res["candidate_good"])
    c = res["pose_candidate"]
    best_lo = max(b[0] for b in bounds)
    best_hi = max(b[1] for b in bounds)
    failed = res["status"] == POSE_FAILED
    if best_hi < params.min_features:
        assert failed, res
    if best_lo >= params.min_features:
        assert not failed, res
    # the chosen index is the first with the strictly largest count (:666-684)
    exp_c, bc = -1, 0
    for i in range(4):
        if good[i] > bc:
            exp_c, bc = i, good[i]
    assert c == exp_c, (c, good)
    assert failed == (c < 0 or bc < params.min_features), (res["status"], c, good)

    def fits(j):
        # reference candidates are (R1, t1), (R1, -t1), (R2, t1), (R2, -t1): index c of the run maps
        # to j, and the other three follow by the same structure (c ^ 1: -t, c ^ 2: the other R)
        return all(bounds[j ^ x][0] <= good[c0 ^ x] <= bounds[j ^ x][1] for x in range(4))
    if failed:
        c0 = 0
        assert any(fits(j) for j in range(4)), (good, bounds)
        assert not res["R"].any() and not res["t"].any()
        return fig
    c0 = c
    R = res["R"].astype(np.float64)
    scale = float(res["scale_factor"])
    t = res["t"].astype(np.float64)
    if res["status"] != OK:
        # R and t are only written on success: match through the counts alone
        assert any(fits(j) for j in range(4)), (good, bounds)
        js = [j for j in range(4) if fits(j)]
        assert len(js) == 1, ("ambiguous candidate match", good, bounds)
        j = js[0]
        R, t_unit = cands[j]
        R32, t32 = R.astype(np.float32).astype(np.float64), t_unit.astype(np.float32).astype(np.float64)
        R, t, scale = R32, t32, 1.0
    else:
        assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-6 and abs(np.linalg.det(R) - 1.0) <= 1e-6
        j, gap = _match_candidates(cands, R, t / scale)
        assert j >= 0, ("(R, t / scale) is none of the four candidates", gap)
        fig["pose_gap"] = gap
        assert fits(j), (good, bounds, j)
        assert np.abs(t - cands[j][1] * scale).max() <= 1e-6 * max(1.0, scale)

    # ---- e. points under the returned pose
    tu = t / scale
    T = point_terms(b1, b2, R, tu, W, H)
    excl = np.abs(T["det"]) < DET_MIN
    fig["points_excluded"] = float(excl.mean())
    assert fig["points_excluded"] <= 5e-3, fig
    ntri_lo, ntri_hi = int((T["ok"] & ~excl).sum()), int((T["ok"] | excl).sum())
    assert ntri_lo <= res["num_triangulated"] <= ntri_hi, (res["num_triangulated"], ntri_lo, ntri_hi)
    if ntri_hi < params.min_features:
        assert res["status"] == TRIANGULATION
    if res["status"] == TRIANGULATION:
        assert ntri_lo < params.min_features
        return fig

    # ---- f. validation
    vlo, vhi, dec, und = count_bounds(T, mask, mx, band)
    fig["valid_gap"] = (vhi - vlo) / max(1, int(mask.sum()))
    assert fig["valid_gap"] <= 0.05, fig
    nv = res["num_valid"]
    assert vlo <= nv <= vhi, (nv, vlo, vhi)
    ssum = float(np.maximum(T["er"], T["ec"])[dec].sum())
    assert abs(res["mean_reproj_error"] * nv - ssum) <= int(und.sum()) * mx + nv * band, \
        (res["mean_reproj_error"], nv, ssum)
    bad = nv == 0 or nv < params.min_features
    if vhi < params.min_features or vhi == 0:
        assert res["status"] == VALIDATION, res
    if vlo >= params.min_features and vlo > 0:
        assert res["status"] != VALIDATION, res
    assert (res["status"] == VALIDATION) == bad
    if res["status"] == VALIDATION:
        return fig
    assert res["status"] == OK, res

    # ---- e (continued): the returned points, and g. the scale
    dl = midpoint_bound(T["det"])
    nref = np.linalg.norm(T["X"], axis=1)
    use = ~excl
    rel = np.linalg.norm(X / scale - T["X"], axis=1)[use] / nref[use]
    fig["K_ratio"] = float((rel * np.abs(T["det"][use]) / U23).max())
    assert (rel <= dl[use]).all(), ("mid-point", fig["K_ratio"])
    mlo, mhi = scale_bounds(T["X"], T["det"])
    inv = 1.0 / scale
    assert mlo <= inv <= mhi, (mlo, inv, mhi)
    fig["median_bracket"] = (mhi - mlo) / inv
    return fig
