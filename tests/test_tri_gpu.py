"""GPU parity of vio_triangulate (csrc/triangulate.hip) against oracle/tri_oracle.py.

Estimator::TriangulateSinglePoint (src/processing/Estimator.cpp:1082-1137).  Both sides build A in
f32 with the reference's expressions and take the null vector in f64 (device: one-sided Jacobi,
oracle: LAPACK SVD), so points agree to f32 rounding (tolerance: 1e-5 relative, stated here), the
valid flags exactly; the reprojection pixel errors (:1233-1248) agree to 1e-3 px wherever the two
points are bitwise equal (acos near 1 amplifies one ulp of the dot product).

The edge cases of tri_cases.edge_cases() are held to the bounds of tests/tri_checks.py.  Measured on
an MI355X: every parity case had every point bitwise equal to the oracle's (error / bound 0) except
baseline 1e-5 with exact bearings (98.63 % bitwise equal, largest error / bound 0.193) and points at
1e5 m (99.61 %, 0.097); no candidate fell below the (σ₃−σ₄)/σ₁ ≥ 1e-8 gate (smallest 2.5e-8).
Before this module's non-finite rule the kernel reported valid = 1, with one coordinate exactly 0,
for a pose holding a NaN or an inf in a rotation column (that column of A never rotates, so the
shortest of the other three was taken as the null vector).
"""
import numpy as np
import pytest

import tri_cases
import tri_checks
from test_tri_oracle import load_oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(vio):
    c = vio.Context(0)
    yield c
    c.close()


# share of points bitwise equal to the oracle's on the make_case geometry: measured 1.0 (8192 of 8192)
# for each of the three cases on an MI355X; asserted less a 1 % margin for another LAPACK build
MIN_SAME_SHARE = 0.99


def _compare(g, o):
    (gp, gv, ge), (op, ov, oe) = g, o
    np.testing.assert_array_equal(gv, ov)
    nrm = np.maximum(np.linalg.norm(op, axis=1), 1e-6)
    rel = np.linalg.norm(gp.astype(np.float64) - op, axis=1) / nrm
    assert rel.max() < 1e-5, (rel.max(), int(rel.argmax()))
    same = (gp == op).all(1)
    assert same.mean() >= MIN_SAME_SHARE, same.mean()
    assert np.abs(ge[same] - oe[same]).max() < 1e-3


@pytest.mark.parametrize("noise,seed", [(0.0, 1), (1e-3, 2), (0.0, 3)])
def test_parity_with_oracle(ctx, noise, seed):
    tri = load_oracle()
    T, pairs, B, _ = tri_cases.make_case(n=8192, n_poses=32, seed=seed, noise=noise)
    g = ctx.triangulate(T, pairs, B, 3840)
    _compare(g, tri.triangulate(T, pairs, B, 3840))
    tri_checks.check_pixel_errors(tri, dict(T=T, pairs=pairs, B=B), *g, 3840)  # every valid candidate
    assert ctx.triangulate_kernel_ms() > 0


EDGE = tri_cases.edge_cases()


@pytest.mark.parametrize("name", [k for k, c in EDGE.items() if c["kind"] == "parity"])
def test_edge_parity_with_oracle(ctx, name):
    """Tiny baselines, shifted origins, far points, b_z = 0, one pose twice, non-unit bearings, block
    tails: valid exactly the oracle's, points within tri_checks.parity_bound with no candidate
    excluded, pixel errors within the acos bound on every valid candidate."""
    tri = load_oracle()
    c = EDGE[name]
    ratio, same = tri_checks.check_parity(tri, c, ctx.triangulate(c["T"], c["pairs"], c["B"], 3840),
                                          tri.triangulate(c["T"], c["pairs"], c["B"], 3840), 3840)
    print(name, f"error/bound={ratio:.3f} bitwise-equal share={same:.4f}")


@pytest.mark.parametrize("name", [k for k, c in EDGE.items() if c["kind"] == "contract"])
def test_edge_contract(ctx, name):
    """Geometry without a unique null vector, or inputs LAPACK cannot take: valid ∈ {0, 1}, invalid
    candidates are all zero, NaN / inf rows are invalid and leave their neighbours bitwise untouched,
    every valid point is a smallest singular vector of A (‖A·v‖ ≤ σ₄ + 8·2⁻²⁴·σ₁), parallel rays give
    no point nearer than 1e6 m."""
    tri = load_oracle()
    c = EDGE[name]
    g = ctx.triangulate(c["T"], c["pairs"], c["B"], 3840)
    gc = ctx.triangulate(c["clean"]["T"], c["clean"]["pairs"], c["clean"]["B"], 3840) if "clean" in c else None
    tri_checks.check_contract(tri, c, g, gc)
    tri_checks.check_pixel_errors(tri, c, *g, 3840)
    print(name, "valid share", g[1].mean())


def test_degenerate_inputs_do_not_fault(ctx):
    T = np.tile(np.eye(4, dtype=np.float32), (2, 1, 1))
    b = np.array([0.0, 0.0, 1.0], np.float32)
    B = np.array([np.r_[b, b], np.zeros(6), np.r_[b, -b]], np.float32)  # zero baseline, zero bearings
    P, V, E = ctx.triangulate(T, [[0, 1], [0, 1], [0, 0]], B, 960)
    assert V.dtype == np.uint8 and set(V.tolist()) <= {0, 1}
    assert np.isfinite(P).all() and (P[V == 0] == 0).all()


def test_errors(vio, ctx):
    T = np.eye(4, dtype=np.float32)[None]
    with pytest.raises(vio.VioError):
        ctx.triangulate(T, [[0, 1]], np.zeros((1, 6)), 960)
    P, V, E = ctx.triangulate(T, np.zeros((0, 2)), np.zeros((0, 6)), 960)
    assert len(P) == 0


@pytest.mark.parametrize("row,col,idx", [(0, 0, 3), (0, 0, -1), (-1, 1, 3), (-1, 1, -1)])
def test_out_of_range_pose_index_at_either_end(vio, ctx, row, col, idx):
    T, pairs, B, _ = tri_cases.make_case(n=257, n_poses=3, seed=6)
    pairs = pairs.copy()
    pairs[row, col] = idx
    with pytest.raises(vio.VioError):
        ctx.triangulate(T, pairs, B, 960)


def test_device_entry_without_pixel_errors(ctx):
    """pixel_err = NULL: points and flags are the host entry's, and the kernel writes nowhere else
    (guard rows past n stay 0xFF)."""
    torch = pytest.importorskip("torch")
    c = EDGE["nonfinite_rows"]
    n = len(c["pairs"])
    host = ctx.triangulate(c["T"], c["pairs"], c["B"], 3840)
    dev = torch.device("cuda:0")
    dT = torch.from_numpy(c["T"].reshape(-1, 16)).to(dev)
    dP = torch.from_numpy(c["pairs"]).to(dev)
    dB = torch.from_numpy(c["B"]).to(dev)
    dX = torch.full(((n + 1) * 12,), 0xFF, dtype=torch.uint8, device=dev)
    dV = torch.full((n + 1,), 0xFF, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    ctx.triangulate_device(dT.data_ptr(), len(c["T"]), dP.data_ptr(), dB.data_ptr(), n, 3840, dX.data_ptr(),
                           dV.data_ptr(), None)
    ctx.triangulate_kernel_ms()  # waits for the kernel
    X, V = dX.cpu().numpy(), dV.cpu().numpy()
    assert (X[n * 12:] == 0xFF).all() and V[n] == 0xFF
    assert np.array_equal(X[:n * 12].view(np.float32).reshape(n, 3), host[0])
    assert np.array_equal(V[:n], host[1])


def test_device_entry_matches_host_entry(ctx):
    torch = pytest.importorskip("torch")
    T, pairs, B, _ = tri_cases.make_case(n=5000, seed=4)
    host = ctx.triangulate(T, pairs, B, 3840)
    dev = torch.device("cuda:0")
    dT = torch.from_numpy(T.reshape(-1, 16)).to(dev)
    dP = torch.from_numpy(pairs).to(dev)
    dB = torch.from_numpy(B).to(dev)
    dX = torch.zeros((5000, 3), dtype=torch.float32, device=dev)
    dV = torch.zeros(5000, dtype=torch.uint8, device=dev)
    dE = torch.zeros((5000, 2), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    ctx.triangulate_device(dT.data_ptr(), len(T), dP.data_ptr(), dB.data_ptr(), 5000, 3840, dX.data_ptr(),
                           dV.data_ptr(), dE.data_ptr())
    ctx.triangulate_kernel_ms()  # waits for the kernel
    assert np.array_equal(dX.cpu().numpy(), host[0])
    assert np.array_equal(dV.cpu().numpy(), host[1])
    assert np.array_equal(dE.cpu().numpy(), host[2])
