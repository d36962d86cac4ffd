"""CPU checks of the triangulation oracle (oracle/tri_oracle.py), SURVEY §8 f2:
Estimator::TriangulateSinglePoint (src/processing/Estimator.cpp:1082-1137).  The reference has no
test for it; the oracle is pinned by exact synthetic geometry, on make_case and on the parity cases
of tri_cases.edge_cases() (tiny baselines, shifted origins, far points, b_z = 0, one pose twice,
non-unit bearings) with a bound that follows each candidate's conditioning."""
import importlib.util
import os

import numpy as np
import pytest

import tri_cases
import tri_checks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_oracle():
    spec = importlib.util.spec_from_file_location("tri_oracle", os.path.join(ROOT, "oracle", "tri_oracle.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_exact_bearings_recover_points():
    tri = load_oracle()
    T, pairs, B, X = tri_cases.make_case(n=2000, seed=1)
    P, valid, err = tri.triangulate(T, pairs, B, 3840)
    assert valid.all()
    rel = np.linalg.norm(P - X, axis=1) / np.linalg.norm(X, axis=1)
    assert np.median(rel) < 1e-5 and np.percentile(rel, 99) < 1e-3, (np.median(rel), rel.max())
    assert np.median(err) < 0.05


def test_noisy_bearings_reprojection_error_scale():
    tri = load_oracle()
    T, pairs, B, X = tri_cases.make_case(n=2000, seed=2, noise=1e-3)
    P, valid, err = tri.triangulate(T, pairs, B, 3840)
    # 1 mrad of bearing noise ~ 0.6 px at 3840 px / 2π; the DLT residual stays at that scale
    assert np.median(err) < 2.0


def test_row_construction_matches_reference_expression():
    tri = load_oracle()
    T, pairs, B, _ = tri_cases.make_case(n=4, seed=3)
    A = tri.build_A(T[pairs[:, 0]], T[pairs[:, 1]], B[:, :3], B[:, 3:])
    b = B[0]
    T1 = T[pairs[0, 0]]
    np.testing.assert_array_equal(A[0, 0], np.float32(b[0]) * T1[2] - np.float32(b[2]) * T1[0])
    np.testing.assert_array_equal(A[0, 1], np.float32(b[1]) * T1[2] - np.float32(b[2]) * T1[1])


@pytest.fixture(scope="module")
def edge():
    return tri_cases.edge_cases()


PARITY = [k for k, c in tri_cases.edge_cases().items() if c["kind"] == "parity"]


@pytest.mark.parametrize("name", PARITY)
def test_parity_cases_have_a_unique_null_vector(edge, name):
    """(σ₃−σ₄)/σ₁ ≥ 1e-8 on every candidate of every parity case: nothing is excluded from the GPU
    comparison.  Smallest gaps: 2.5e-8 (baseline 1e-5, exact bearings), 1.0e-7 (origin 1e3)."""
    tri = load_oracle()
    s = tri_checks.singular_values(tri, edge[name])
    assert np.isfinite(s).all()
    assert tri_checks.rel_gap(s).min() >= tri_checks.MIN_REL_GAP, tri_checks.rel_gap(s).min()


@pytest.mark.parametrize("name", PARITY)
def test_oracle_recovers_planted_points_on_parity_cases(edge, name):
    """Conditioning-aware: building A in f32 from f32 bearings and poses perturbs it by
    ‖E‖ ≤ 16·2⁻²⁴·max|A's terms| (plus the planted bearing noise); the null direction then turns by
    at most ε = ‖E‖/(σ₃−σ₄) (Wedin), and X = v₁₋₃/v₄ moves by ‖[X;1]‖·(1+‖X‖)·ε to first order.
    Asserted with a factor 2 for the higher orders wherever ε < 0.1; beyond that the geometry does
    not determine the point and only `valid` is checked."""
    tri = load_oracle()
    c = edge[name]
    P, valid, _ = tri.triangulate(c["T"], c["pairs"], c["B"], 3840)
    assert valid.all()
    s = tri_checks.singular_values(tri, c)
    T = np.abs(c["T"][c["pairs"]].astype(np.float64)).max((1, 2, 3))
    bn = np.abs(c["B"].astype(np.float64)).max(1)
    eps = (16 * tri_checks.EPS32 + 4 * c["noise"]) * bn * np.maximum(T, 1.0) / (s[:, 2] - s[:, 3])
    X = c["X"]
    nx = np.linalg.norm(X, axis=1)
    bound = 2 * np.sqrt(1 + nx * nx) * (1 + nx) * eps
    err = np.linalg.norm(P.astype(np.float64) - X, axis=1)
    m = eps < 0.1
    assert (err[m] <= bound[m] + 4 * tri_checks.EPS32 * nx[m]).all(), float((err[m] / bound[m]).max())
    if name in ("baseline_0.01_exact", "bz0_one_view", "non_unit_bearings", "n_257"):
        assert m.all()  # well-conditioned cases: the bound binds everywhere


def test_oracle_rejects_nonfinite_rows(edge):
    tri = load_oracle()
    c = edge["nonfinite_rows"]
    P, valid, err = tri.triangulate(c["T"], c["pairs"], c["B"], 3840)
    Pc, vc, ec = tri.triangulate(c["clean"]["T"], c["clean"]["pairs"], c["clean"]["B"], 3840)
    tri_checks.check_contract(tri, c, (P, valid, err), (Pc, vc, ec))
    assert c["bad"].sum() > 100 and valid.sum() == (~c["bad"]).sum()


def test_empty():
    tri = load_oracle()
    P, v, e = tri.triangulate(np.eye(4)[None], np.zeros((0, 2)), np.zeros((0, 6)), 960)
    assert P.shape == (0, 3) and v.shape == (0,)
