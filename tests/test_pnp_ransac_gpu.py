"""Absolute-pose RANSAC on the device (vio_pnp_ransac) against the independent f64 reference of
tests/pnp_reference.py, on the committed cases of tests/pnp_cases.py.

Counts are compared through the reference's brackets (a point whose angle lies inside the band of the threshold may
fall either way; fragile rows are excluded), poses against a measured bar: ten times the spread of the reference's
own winner over 8 copies of the case whose bearings moved by +-1 ulp f32 (DESIGN 4.14 lists the spreads).  Every
precondition is asserted on the reference before the device result is looked at."""
import math

import numpy as np
import pytest

import pnp_cases as cases
import pnp_reference as ref

pytestmark = pytest.mark.gpu


def run(vio, ctx, case, **kw):
    s, S, p = cases.case_inputs(vio, case)
    for k, v in kw.items():
        setattr(p, k, v)
    return ctx.pnp_ransac(s["points"], s["bearings"], S, R=s["R_known"], params=p)


def assert_finite(res):
    for k in ("R_cw", "t_cw", "R0_cw", "t0_cw"):
        assert np.isfinite(res[k]).all(), k
    assert math.isfinite(res["rms_angle_rad"])


def check_against_reference(case, r, res, mask, counts):
    ref.assert_preconditions(r, poses=cases.compares_poses(case))
    assert_finite(res)
    assert len(counts) == r.H and len(mask) == r.n
    assert res["status"] == r.status
    assert res["best_hypothesis"] == r.best
    if not r.launched:
        assert (counts == -1).all() and not mask.any() and res["best_solution"] == -1
        return
    nf = ~r.fragile
    np.testing.assert_array_equal((counts < 0)[nf], r.skipped[nf])
    both = nf & ~r.skipped
    assert ((r.lo[both] <= counts[both]) & (counts[both] <= r.hi[both])).all()
    if r.best < 0:
        assert not mask.any() and res["best_solution"] == -1 and not res["R_cw"].any() and not res["t_cw"].any()
        return
    assert r.win_lo <= res["num_inliers_sample"] <= r.win_hi
    assert res["num_inliers_sample"] == counts[r.best]
    assert 0 <= res["best_solution"] < len(r.poses[r.best])
    assert res["refit_kept"] == r.refit_kept
    assert r.final_lo <= res["num_inliers"] <= r.final_hi
    assert res["num_inliers"] == int(mask.sum())
    np.testing.assert_array_equal(mask.astype(bool)[~r.undecided], r.mask[~r.undecided])
    # the pose, coarsely, for every case (the measured bar is test_poses_within_the_measured_bar's)
    scale = max(1.0, float(np.linalg.norm(r.t0)))
    assert ref.rot_angle(res["R0_cw"], r.R0) < 1e-7 and np.linalg.norm(res["t0_cw"] - r.t0) < 1e-6 * scale
    assert ref.rot_angle(res["R_cw"], r.R) < 1e-7 and np.linalg.norm(res["t_cw"] - r.t) < 1e-6 * scale
    if not r.undecided.any():
        assert abs(res["rms_angle_rad"] - r.rms) <= 1e-9 + 1e-6 * r.rms


@pytest.mark.parametrize("case", cases.ALL_CASES, ids=cases.case_id)
def test_counts_winner_status_and_mask(vio, gpu_ctx, case):
    """every committed scene, the sizes n in {3 .. 4096} and the row counts {0 .. 256}, both modes"""
    _, r = cases.reference(vio, case)
    res, mask, counts = run(vio, gpu_ctx, case)
    check_against_reference(case, r, res, mask, counts)
    if case[0] in ("clean", "iters") and r.launched:
        # every solvable row counts every point (a row whose sampled bearings are closer than the pair angle is
        # skipped on both sides), and the tie picks the earliest of them
        assert (counts[~r.skipped] == r.n).all() and res["best_hypothesis"] == int(np.argmin(r.skipped))


@pytest.mark.parametrize("name", cases.POSE_SCENES)
def test_poses_within_the_measured_bar(vio, gpu_ctx, name):
    case = ("scene", name)
    s, S, p = cases.case_inputs(vio, case)
    _, r = cases.reference(vio, case)
    ref.assert_preconditions(r, poses=True)
    spread = ref.ulp_cloud(s["points"], s["bearings"], S, p.inlier_thresh_rad, p.min_pair_angle_rad, s["R_known"],
                           p.refit_iters, r.best)
    res, _, _ = run(vio, gpu_ctx, case)
    got = {"R0": ref.rot_angle(res["R0_cw"], r.R0), "t0": float(np.linalg.norm(res["t0_cw"] - r.t0)),
           "R": ref.rot_angle(res["R_cw"], r.R), "t": float(np.linalg.norm(res["t_cw"] - r.t))}
    print(f"pnp-pose {name}: spread of 8 +-1 ulp copies "
          + " ".join(f"{k}={v:.3e}" for k, v in spread.items()) + " | device - reference "
          + " ".join(f"{k}={v:.3e}" for k, v in got.items()))
    assert res["best_hypothesis"] == r.best and res["refit_kept"] == r.refit_kept
    for k in got:
        assert got[k] <= 10 * spread[k], (k, got[k], spread[k])


def test_min_inliers_at_and_above_the_winner(vio, gpu_ctx):
    case = ("scene", "family-1")
    base, mask0, _ = run(vio, gpu_ctx, case)
    c = base["num_inliers_sample"]
    at, _, _ = run(vio, gpu_ctx, case, min_inliers=c)
    above, mask, _ = run(vio, gpu_ctx, case, min_inliers=c + 1)
    assert at["status"] == vio.VIO_PNPR_OK and above["status"] == vio.VIO_PNPR_FEW_INLIERS
    # the pose and the mask are still reported
    assert np.array_equal(above["R_cw"], base["R_cw"]) and np.array_equal(above["t_cw"], base["t_cw"])
    assert np.array_equal(mask, mask0) and mask.sum() == base["num_inliers"] > 0


def test_tie_picks_the_earlier_row_and_bad_rows_are_skipped(vio, gpu_ctx):
    s = cases.scene("nan3")
    n = len(s["points"])
    S = cases.samples(vio, 5, n)
    _, r = cases.reference(vio, ("scene", "nan3"))
    bad = np.nonzero(~np.isfinite(s["points"]).all(1))[0]
    assert len(bad) == 3
    w = S[r.best]
    # row 0 repeats an index, rows 1..3 sample a NaN point, rows 4 and 5 are the winner twice, row 6 is another row
    T = np.array([[w[0], w[0], w[1]], [bad[0], w[1], w[2]], [w[0], bad[1], w[2]], [w[0], w[1], bad[2]], w, w,
                  S[(r.best + 1) % len(S)]], np.int32)
    res, mask, counts = gpu_ctx.pnp_ransac(s["points"], s["bearings"], T, params=cases.params(vio))
    assert (counts[:4] == -1).all() and counts[4] == counts[5] == counts.max() > 0
    assert res["best_hypothesis"] == 4 and not mask[bad].any()
    assert_finite(res)


def test_refit_off_returns_the_minimal_pose(vio, gpu_ctx):
    for case in (("scene", "family-2"), ("scene", "known-off")):
        res, mask, counts = run(vio, gpu_ctx, case, refit_iters=0)
        assert res["refit_kept"] == 0 and res["num_inliers"] == res["num_inliers_sample"] == int(mask.sum())
        assert np.array_equal(res["R_cw"], res["R0_cw"]) and np.array_equal(res["t_cw"], res["t0_cw"])
        on, _, counts_on = run(vio, gpu_ctx, case)
        assert np.array_equal(counts, counts_on) and np.array_equal(on["R0_cw"], res["R0_cw"])


def test_not_a_rotation_is_rejected(vio, gpu_ctx):
    s, S, p = cases.case_inputs(vio, ("scene", "known-exact"))
    for R in (2.0 * np.eye(3), np.diag([1.0, 1.0, -1.0]), np.full((3, 3), np.nan)):
        with pytest.raises(vio.VioError):
            gpu_ctx.pnp_ransac(s["points"], s["bearings"], S, R=R, params=p)
    with pytest.raises(vio.VioError):
        gpu_ctx.pnp_ransac(s["points"], s["bearings"], S + len(s["points"]), params=p)  # indices out of range


def test_optional_outputs_may_be_null(vio, gpu_ctx):
    s, S, p = cases.case_inputs(vio, ("scene", "planar"))
    full, _, _ = gpu_ctx.pnp_ransac(s["points"], s["bearings"], S, params=p)
    bare, m, c = gpu_ctx.pnp_ransac(s["points"], s["bearings"], S, params=p, want_mask=False, want_counts=False)
    assert m is None and c is None
    for k in full:
        assert np.array_equal(full[k], bare[k]), k
    assert gpu_ctx.pnp_ransac_kernel_ms() > 0.0


def test_bitwise_reproducible_across_calls_and_contexts(vio, gpu_ctx):
    for case in (("scene", "family-1"), ("scene", "known-off"), ("clean", 4096, False)):
        a = run(vio, gpu_ctx, case)
        b = run(vio, gpu_ctx, case)
        ctx = vio.Context(0)
        try:
            c = run(vio, ctx, case)
        finally:
            ctx.close()
        for other in (b, c):
            for k in a[0]:
                assert np.asarray(a[0][k]).tobytes() == np.asarray(other[0][k]).tobytes(), (case, k)
            assert np.array_equal(a[1], other[1]) and np.array_equal(a[2], other[2])


SOLVE = dict(max_iterations=30, fixed_iterations=1)


def rot_angle(Ra, Rb):
    return math.acos(max(-1.0, min(1.0, (np.trace(Ra.T @ Rb) - 1.0) / 2.0)))


def test_seeds_the_pnp_solve_like_the_true_pose(vio, synth, gpu_ctx):
    """correspondences -> vio_pnp_ransac -> vio_pnp_compose -> the VIO_PNP solve: the same answer as that solve
    started from the true pose, to test_ba_gpu.py's PnP bars (|dt| 1e-4 m, 1e-5 rad, cost 1e-6 relative), with equal
    outlier flags.  Both legs run the solve to convergence (30 fixed iterations per outlier round, the mode
    test_ba_gpu.py's trace cases use): the tolerance-terminated default stops each leg inside its own 1e-6 function
    tolerance, and on the CPU oracle that alone leaves |dt| 1.5e-4 m, 3.8e-5 rad and 1.5e-4 of the cost between the
    two legs with identical outlier flags (a property of the stopping rule: a start 40 degrees off lands as far
    away).  Converged, the oracle's two legs differ by 1.8e-9 m and 2.4e-10 of the cost."""
    full = synth.config2()
    w = synth.make_pnp(full, outlier_frac=0.3)
    T_true = np.asarray(full["T_wb_true"])[len(full["T_wb_init"]) - 1]
    P = np.asarray(w["lm_xyz"])[w["obs_lm"]].astype(np.float32)
    uv = np.asarray(w["obs_uv"], np.float64)
    lon = (uv[:, 0] / w["cols"] - 0.5) * 2.0 * np.pi
    lat = -(uv[:, 1] / w["rows"] - 0.5) * np.pi
    B = np.stack([np.cos(lat) * np.sin(lon), -np.sin(lat), np.cos(lat) * np.cos(lon)], 1).astype(np.float32)
    S = cases.samples(vio, 1, len(P))
    res, mask, _ = gpu_ctx.pnp_ransac(P, B, S, params=cases.params(vio))
    assert res["status"] == vio.VIO_PNPR_OK
    T_seed = vio.pnp_compose(res["R_cw"], res["t_cw"], np.asarray(w["T_cb"]).reshape(-1, 4, 4)[0])
    a = gpu_ctx.ba_solve([vio.BaProblem(dict(w, T_wb_init=T_true[None]), variant=vio.VIO_PNP, **SOLVE)])[0]
    b = gpu_ctx.ba_solve([vio.BaProblem(dict(w, T_wb_init=T_seed.astype(np.float64)[None]), variant=vio.VIO_PNP, **SOLVE)])[0]
    dt = float(np.abs(a["T_wb"][0, :3, 3] - b["T_wb"][0, :3, 3]).max())
    dr = rot_angle(a["T_wb"][0, :3, :3], b["T_wb"][0, :3, :3])
    dc = abs(a["final_cost"] - b["final_cost"]) / max(1.0, abs(a["final_cost"]))
    flags = int((a["obs_outlier"] != b["obs_outlier"]).sum())
    print(f"pnp-e2e: ransac inliers {res['num_inliers']} of {len(P)}; true-seeded vs ransac-seeded solve: |dt| {dt:.3e} "
          f"rot {dr:.3e} cost rel {dc:.3e} differing outlier flags {flags}; final cost {a['final_cost']:.6f} "
          f"inliers {a['num_inliers']}")
    assert a["success"] == b["success"] == 1
    assert dt <= 1e-4 and dr <= 1e-5 and dc <= 1e-6
    assert flags == 0
