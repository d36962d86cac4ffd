"""Absolute-pose RANSAC, CPU checks: struct layouts and the parameter check of the C-ABI, the two host helpers
(vio_pnp_correspondences against vio_ba_gather(VIO_PNP), vio_pnp_compose against numpy), and the self-checks of the
independent f64 reference (tests/pnp_reference.py) that the GPU tests compare against, with the preconditions of
every committed case asserted on the reference alone."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pnp_cases as cases
import pnp_reference as ref
from test_gather import PNP, near_boundary, random_graph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vio360.h")


def test_struct_layouts_match_header(vio, tmp_path):
    structs = {"vio_pnp_ransac_params": (vio.abi.VioPnpRansacParams,
                                         ["inlier_thresh_rad", "min_pair_angle_rad", "min_inliers", "refit_iters"]),
               "vio_pnp_ransac_result": (vio.abi.VioPnpRansacResult,
                                         ["status", "best_hypothesis", "best_solution", "num_inliers_sample",
                                          "num_inliers", "refit_kept", "R_cw", "t_cw", "R0_cw", "t0_cw",
                                          "rms_angle_rad"])}
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void){"]
    for cs, (_, fields) in structs.items():
        lines.append(f'printf("%zu\\n", sizeof({cs}));')
        lines += [f'printf("%zu\\n", offsetof({cs}, {f}));' for f in fields]
    lines.append('printf("%d %d %d %d\\n", VIO_PNPR_OK, VIO_PNPR_TOO_FEW, VIO_PNPR_NO_MODEL, VIO_PNPR_FEW_INLIERS);')
    (tmp_path / "pnp.c").write_text("\n".join(lines + ["return 0;}"]))
    subprocess.check_call(["gcc", "-o", str(tmp_path / "pnp"), str(tmp_path / "pnp.c")])
    out = [int(x) for x in subprocess.check_output([str(tmp_path / "pnp")]).split()]
    want = []
    for cls, fields in structs.values():
        want += [C.sizeof(cls)] + [getattr(cls, f).offset for f in fields]
    want += [vio.VIO_PNPR_OK, vio.VIO_PNPR_TOO_FEW, vio.VIO_PNPR_NO_MODEL, vio.VIO_PNPR_FEW_INLIERS]
    assert out == want
    assert vio.lib().vio_abi_version() == 4
    for name in ("vio_pnp_ransac_check", "vio_pnp_ransac", "vio_pnp_ransac_kernel_ms", "vio_pnp_correspondences",
                 "vio_pnp_compose"):
        assert name in vio.EXPORTS and hasattr(vio.lib(), name), name


def test_check_accepts_defaults_and_rejects_each_bad_field(vio):
    L = vio.lib()
    d = vio.default_pnp_ransac_params()
    assert np.allclose(np.rad2deg([d.inlier_thresh_rad, d.min_pair_angle_rad]), [0.5, 1.0], rtol=1e-6)
    assert (d.min_inliers, d.refit_iters) == (10, 5)
    assert L.vio_pnp_ransac_check(C.byref(d), 300, 256) == 0
    assert L.vio_pnp_ransac_check(C.byref(d), 0, 0) == 0
    assert L.vio_pnp_ransac_check(C.byref(d), 4096, 4096) == 0
    assert L.vio_pnp_ransac_check(None, 300, 256) != 0
    for n, iters in ((-1, 1), (4097, 1), (10, -1), (10, 4097)):
        assert L.vio_pnp_ransac_check(C.byref(d), n, iters) != 0, (n, iters)
    bad = [("min_inliers", -1), ("refit_iters", -1), ("refit_iters", 11)]
    for f in ("inlier_thresh_rad", "min_pair_angle_rad"):
        bad += [(f, 0.0), (f, -0.1), (f, float("nan")), (f, float(np.pi / 2)), (f, 2.0), (f, float("inf"))]
    for f, v in bad:
        assert L.vio_pnp_ransac_check(C.byref(cases.params(vio, **{f: v})), 300, 256) != 0, (f, v)
    assert L.vio_pnp_ransac_check(C.byref(cases.params(vio, min_inliers=0, refit_iters=0)), 300, 256) == 0
    assert L.vio_pnp_ransac_check(C.byref(cases.params(vio, refit_iters=10)), 300, 256) == 0


def pixel_to_bearing64(uv, W, H):
    """Camera::PixelToBearing (Camera.cpp:22-47) in f64"""
    uv = np.asarray(uv, np.float64)
    lon = (uv[:, 0] / W - 0.5) * 2.0 * np.pi
    lat = -(uv[:, 1] / H - 0.5) * np.pi
    b = np.stack([np.cos(lat) * np.sin(lon), -np.sin(lat), np.cos(lat) * np.cos(lon)], 1)
    return b / np.linalg.norm(b, axis=1)[:, None]


@pytest.mark.parametrize("seed", range(12))
def test_correspondences_are_the_pnp_gather(vio, seed):
    G = random_graph(seed)
    view = vio.abi.MapView(G)
    fb = G["feat_begin"]
    for frame in range(len(fb) - 1):
        P, B, F = vio.pnp_correspondences(view, frame)
        want = [g for g in range(fb[frame], fb[frame + 1])
                if G["feat_valid"][g] and G["feat_mp"][g] >= 0 and not G["mp_bad"][G["feat_mp"][g]]
                and not near_boundary(G["feat_uv"][g], G["width"], G["height"], G["boundary_margin"])]
        np.testing.assert_array_equal(F, np.array(want, np.int32))
        np.testing.assert_array_equal(P, G["mp_pos"][G["feat_mp"][F]])
        b64 = pixel_to_bearing64(G["feat_uv"][F], G["width"], G["height"]) if len(F) else np.zeros((0, 3))
        ulp = np.spacing(np.abs(b64).astype(np.float32)).astype(np.float64)
        assert (np.abs(B.astype(np.float64) - b64) <= ulp).all()
    # frame 0 against the library's own gather: the same set, the same order, its mp_pos
    g = vio.ba_gather(view, PNP, False, False).result()
    P, B, F = vio.pnp_correspondences(view, 0)
    if g["status"] == 0:
        np.testing.assert_array_equal(F, g["obs_feat"])
        np.testing.assert_array_equal(P.astype(np.float64), g["lm_xyz"][g["obs_lm"]])
    else:
        assert len(F) < 6
    n = C.c_int()
    assert vio.lib().vio_pnp_correspondences(C.byref(view.c), len(fb) - 1, None, None, None, 0, C.byref(n)) != 0
    assert vio.lib().vio_pnp_correspondences(C.byref(view.c), -1, None, None, None, 0, C.byref(n)) != 0


def test_compose_matches_numpy(vio):
    rng = np.random.default_rng(3)
    for _ in range(20):
        R, t = cases.so3_exp(rng.normal(0, 1, 3)), rng.normal(0, 3, 3)
        Tcb = np.eye(4)
        Tcb[:3, :3], Tcb[:3, 3] = cases.so3_exp(rng.normal(0, 1, 3)), rng.normal(0, 0.2, 3)
        Tcb32 = Tcb.astype(np.float32)
        Tcw = np.eye(4)
        Tcw[:3, :3], Tcw[:3, 3] = R, t
        want = np.linalg.inv(Tcw) @ Tcb32.astype(np.float64)
        got = vio.pnp_compose(R, t, Tcb32)
        assert got.dtype == np.float32 and np.array_equal(got[3], [0, 0, 0, 1])
        assert np.abs(got.astype(np.float64) - want).max() <= 4e-7 * max(1.0, np.abs(want).max())
    assert vio.lib().vio_pnp_compose(None, None, None, None) != 0


# ------------------------------------------------------------------------------------------------
# the reference itself
def test_reference_p3p_solutions_satisfy_the_constraints():
    rng = np.random.default_rng(0)
    found = 0
    for _ in range(200):
        R, t = cases.so3_exp(rng.normal(0, 1, 3)), rng.normal(0, 1, 3)
        Pw = rng.uniform(-8, 8, (3, 3))
        Xc = Pw @ R.T + t
        Y = Xc / np.linalg.norm(Xc, axis=1)[:, None]
        sols, _ = ref.p3p(Pw, Y)
        assert 1 <= len(sols) <= 4
        for Rs, ts in sols:
            assert abs(np.linalg.det(Rs) - 1) < 1e-9 and np.abs(Rs @ Rs.T - np.eye(3)).max() < 1e-9
            X = Pw @ Rs.T + ts
            assert (np.einsum("ij,ij->i", X, Y) > 0).all()
            assert np.abs(np.cross(X / np.linalg.norm(X, axis=1)[:, None], Y)).max() < 1e-6
        found += any(ref.rot_angle(Rs, R) < 1e-6 and np.linalg.norm(ts - t) < 1e-5 for Rs, ts in sols)
    assert found >= 198  # (a sample may sit on a double root, where the quartic loses digits)


@pytest.mark.parametrize("known", [False, True])
@pytest.mark.parametrize("n", [5, 65, 300])
def test_reference_clean_scene_finds_the_true_pose(vio, n, known):
    s, r = cases.reference(vio, ("clean", n, known))
    assert r.best == 0 and (r.lo == n).all() and (r.hi == n).all()
    assert any(ref.rot_angle(R, s["R_true"]) < 1e-5 and np.linalg.norm(t - s["t_true"]) < 1e-4 for R, t in r.poses[0])
    assert r.status == ref.OK if n >= 10 else r.status == ref.FEW_INLIERS


@pytest.mark.parametrize("case", cases.ALL_CASES, ids=cases.case_id)
def test_preconditions_of_every_committed_case(vio, case):
    """what the GPU comparison presupposes, on the reference alone: the winner is decided and not fragile, fragile
    rows are at most 3 % of the rows, and where poses are compared the winner's bracket is closed"""
    _, r = cases.reference(vio, case)
    ref.assert_preconditions(r, poses=cases.compares_poses(case))


def test_scene_family_is_what_the_cases_say(vio):
    s, r = cases.reference(vio, ("scene", "family-1"))
    assert 0.3 < 1 - s["inlier"].mean() < 0.5
    assert r.status == ref.OK and r.win_lo > 0.8 * s["inlier"].sum()
    assert 0.2 < r.skipped.mean() < 0.7  # contaminated samples have no admissible solution
    assert ref.rot_angle(r.R, s["R_true"]) < np.deg2rad(0.1) and np.linalg.norm(r.t - s["t_true"]) < 0.05
    s, r = cases.reference(vio, ("scene", "nan3"))
    assert not r.mask[~np.isfinite(s["points"]).all(1)].any()
    _, r = cases.reference(vio, ("collinear",))
    assert r.status == ref.NO_MODEL and r.skipped.all()
