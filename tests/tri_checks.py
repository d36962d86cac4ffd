"""Assertions shared by the triangulation tests (CPU oracle checks and GPU parity): the bounds come
from the f64 SVD of the f32-built A — the reference — and from the f32 format, never from the code
under test.

Parity bound (relative, per point): 4·(2⁻²⁴·√3 + 2⁻⁵³·σ₁/(σ₃−σ₄)).  Both sides round an f64 null
vector to f32 once per coordinate (√3·2⁻²⁴ on the point); two backward-stable f64 SVDs of the same A
differ in the null direction by ~2⁻⁵³·σ₁/(σ₃−σ₄).  Asserted where (σ₃−σ₄)/σ₁ ≥ 1e-8; a parity case
must not have a candidate below that.

Pixel-error bound: the f32 dot product b·p̂ may be off by δ = 8·2⁻²⁴ between two evaluations, and
acos turns that into min(√(2δ), δ/sin(angle)) radians — ≈0.6 px at W = 3840 near zero angle, the true
resolution of an f32 acos there — plus 1e-3 px for the acos itself.
"""
import math

import numpy as np

EPS32, EPS64 = 2.0 ** -24, 2.0 ** -53
MIN_REL_GAP = 1e-8


def build_A64(tri, case):
    T = np.asarray(case["T"], np.float32)
    T1, T2 = T[case["pairs"][:, 0]], T[case["pairs"][:, 1]]
    with np.errstate(invalid="ignore", over="ignore"):
        return tri.build_A(T1, T2, case["B"][:, :3], case["B"][:, 3:]).astype(np.float64)


def singular_values(tri, case):
    """(n, 4) σ of the f32-built A in f64; rows with a non-finite A are NaN."""
    A = build_A64(tri, case)
    fin = np.isfinite(A).all((1, 2))
    s = np.full((len(A), 4), np.nan)
    if fin.any():
        s[fin] = np.linalg.svd(A[fin], compute_uv=False)
    return s


def rel_gap(s):
    return (s[:, 2] - s[:, 3]) / s[:, 0]


def parity_bound(s):
    with np.errstate(divide="ignore"):
        return 4.0 * (EPS32 * math.sqrt(3.0) + EPS64 * s[:, 0] / (s[:, 2] - s[:, 3]))


def check_parity(tri, case, got, oracle, width):
    """valid exactly equal, every point within parity_bound, pixel errors within the acos bound on
    all valid candidates and within 1e-3 px where the points are bitwise equal.  Returns
    (largest error / bound, share of bitwise-equal points)."""
    (gp, gv, ge), (op, ov, oe) = got, oracle
    s = singular_values(tri, case)
    assert (rel_gap(s) >= MIN_REL_GAP).all(), float(rel_gap(s).min())  # nothing excluded
    np.testing.assert_array_equal(gv, ov)
    assert set(np.unique(gv).tolist()) <= {0, 1}
    ok = ov == 1
    assert np.isfinite(gp).all() and not gp[~ok].any() and not ge[~ok].any()
    nrm = np.maximum(np.linalg.norm(op.astype(np.float64), axis=1), 1e-30)
    rel = np.linalg.norm(gp.astype(np.float64) - op, axis=1) / nrm
    ratio = np.where(ok, rel / parity_bound(s), 0.0)
    assert (ratio <= 1.0).all(), (float(ratio.max()), int(ratio.argmax()))
    check_pixel_errors(tri, case, gp, gv, ge, width)
    same = (gp == op).all(1)
    if same.any():
        assert np.abs(ge[same] - oe[same]).max() < 1e-3
    return float(ratio.max()), float(same.mean())


def check_pixel_errors(tri, case, X, valid, err, width):
    """err against tri_oracle.reproj_px evaluated on the same X, all valid candidates."""
    T = np.asarray(case["T"], np.float32)
    ok = valid == 1
    if not ok.any():
        return
    delta = 8 * EPS32
    for j in range(2):
        Tj = T[case["pairs"][ok, j]]
        ref = tri.reproj_px(Tj, case["B"][ok, 3 * j:3 * j + 3], X[ok], width).astype(np.float64)
        ang = ref * (2.0 * math.pi) / width
        with np.errstate(divide="ignore"):
            tol = width / (2.0 * math.pi) * np.minimum(math.sqrt(2 * delta), delta / np.sin(ang)) + 1e-3
        d = np.abs(err[ok, j].astype(np.float64) - ref)
        assert (d <= tol).all(), (j, float((d / tol).max()), int((d / tol).argmax()))


def check_contract(tri, case, got, got_clean=None):
    """What the entry promises whatever the geometry."""
    gp, gv, ge = got
    assert gv.dtype == np.uint8 and set(np.unique(gv).tolist()) <= {0, 1}
    inv = gv == 0
    assert not gp[inv].any() and not ge[inv].any()
    assert np.isfinite(gp).all() and np.isfinite(ge).all()
    A = build_A64(tri, case)
    fin = np.isfinite(A).all((1, 2))
    s = singular_values(tri, case)
    m = fin & ~inv
    if m.any():
        v = np.concatenate([gp[m].astype(np.float64), np.ones((int(m.sum()), 1))], 1)
        v /= np.linalg.norm(v, axis=1, keepdims=True)
        res = np.linalg.norm(np.einsum("nij,nj->ni", A[m], v), axis=1)
        lim = s[m, 3] + 8 * EPS32 * s[m, 0]
        assert (res <= lim).all(), (float((res / lim).max()), int(np.nonzero(m)[0][(res / lim).argmax()]))
    if "bad" in case:
        bad = case["bad"]
        assert not gv[bad].any()
        cp, cv, ce = got_clean
        assert cv[~bad].all()
        assert np.array_equal(gp[~bad], cp[~bad]) and np.array_equal(gv[~bad], cv[~bad])
        assert np.array_equal(ge[~bad], ce[~bad])
    if case.get("parallel"):
        far = np.linalg.norm(gp.astype(np.float64), axis=1) > 1e6
        assert (inv | far).all(), int((~(inv | far)).sum())
