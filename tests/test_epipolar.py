"""Known-rotation epipolar RANSAC, CPU checks: the parameter check and struct layouts of the C-ABI, and the f32
oracle (tests/epipolar_oracle.py, what the GPU tests compare against bit for bit) against an independent f64
evaluation written from the geometry (tests/epipolar_reference.py)."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import epipolar_cases as cases
import epipolar_oracle as eo
import epipolar_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vio360.h")
BAND = 1e-3  # relative band on every threshold inside which f32 and f64 may disagree
ITERS = 256


def test_check_accepts_defaults_and_rejects_each_bad_field(vio):
    L = vio.lib()
    for mode in (vio.VIO_EPI_OFF, vio.VIO_EPI_ON):
        assert L.erp_epi_check(C.byref(vio.default_epi_params(mode))) == 0
    d = vio.default_epi_params()
    assert (d.mode, d.iters, d.min_support) == (vio.VIO_EPI_OFF, 256, 10)
    assert np.allclose(np.rad2deg([d.epi_thresh_rad, d.rot_thresh_rad, d.max_parallax_rad, d.min_plane_angle_rad]),
                       [0.25, 2.0, 20.0, 1.0], rtol=1e-6)
    assert d.rot_thresh_rad == np.float32(vio.ransac_threshold())  # the rotation test's own 2 degrees, same bits
    assert L.erp_epi_check(None) != 0
    bad = [("mode", 2), ("mode", -1), ("iters", -1), ("iters", 65537), ("min_support", -1)]
    for f in ("epi_thresh_rad", "rot_thresh_rad", "max_parallax_rad", "min_plane_angle_rad"):
        bad += [(f, 0.0), (f, -0.1), (f, float("nan")), (f, float(np.pi / 2)), (f, 2.0), (f, float("inf"))]
    for f, v in bad:
        assert L.erp_epi_check(C.byref(cases.params(**{f: v}))) != 0, (f, v)
    assert L.erp_epi_check(C.byref(cases.params(iters=65536, min_support=0))) == 0


def test_struct_layouts_match_header(vio, tmp_path):
    structs = {"erp_epi_params": (vio.abi.ErpEpiParams, ["mode", "iters", "epi_thresh_rad", "rot_thresh_rad",
                                                        "max_parallax_rad", "min_plane_angle_rad", "min_support"]),
               "erp_epi_info": (vio.abi.ErpEpiInfo, ["n_rot", "n_rescued", "best", "model_valid", "t_dir"])}
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void){"]
    for cs, (_, fields) in structs.items():
        lines.append(f'printf("%zu\\n", sizeof({cs}));')
        lines += [f'printf("%zu\\n", offsetof({cs}, {f}));' for f in fields]
    (tmp_path / "epi.c").write_text("\n".join(lines + ["return 0;}"]))
    subprocess.check_call(["gcc", "-o", str(tmp_path / "epi"), str(tmp_path / "epi.c")])
    out = [int(x) for x in subprocess.check_output([str(tmp_path / "epi")]).split()]
    want = []
    for cls, fields in structs.values():
        want += [C.sizeof(cls)] + [getattr(cls, f).offset for f in fields]
    assert out == want
    assert vio.lib().vio_abi_version() == 4


def test_cos_bound_is_the_acos_test():
    thr = np.float32(cases.params().rot_thresh_rad)
    c = eo.cos_bound(thr)
    below = np.nextafter(c, np.float32(-2))
    assert np.float32(np.arccos(np.float64(c))) < thr and not np.float32(np.arccos(np.float64(below))) < thr
    assert eo.cos_bound(0.0) == np.inf


@functools.lru_cache(maxsize=None)
def evaluated(name):
    """a scene, the oracle's result with the perturbed true rotation given, and the f64 reference"""
    s, prm = cases.scene(name), cases.params()
    S = cases.samples(5, len(s["p0"]), ITERS)
    o = eo.run(s["p0"], s["p1"], s["W"], s["H"], S, prm, R=s["R_given"])
    return name, s, S, o, ref.Reference(s["p0"], s["p1"], s["W"], s["H"], s["R_given"], prm), prm


@pytest.mark.parametrize("scene", list(cases.SCENES))
def test_oracle_counts_within_the_f64_band(scene):
    _, _, S, o, R, _ = evaluated(scene)
    assert o["evaluated"]
    for it, (i, j, _k) in enumerate(S):
        lo, hi = R.count(i, j, -BAND)[0], R.count(i, j, +BAND)[0]
        assert lo <= o["counts"][it] <= hi, (it, lo, int(o["counts"][it]), hi)
    assert (o["counts"] >= 0).sum() >= ITERS // 20  # the check is not empty


@pytest.mark.parametrize("scene", list(cases.SCENES))
def test_oracle_mask_is_the_f64_mask_outside_the_band(scene):
    name, s, S, o, R, prm = evaluated(scene)
    info = o["info"]
    assert info["best"] >= 0
    i, j, _ = S[info["best"]]
    _, rescued, sigma = R.count(i, j)
    # (a track on the edge of the rotation test moves between the two sets: the rescued count is not monotone in
    # the band, the total is)
    lo, hi = sorted([R.count(i, j, -BAND)[1], R.count(i, j, +BAND)[1]])
    assert lo >= prm.min_support or hi < prm.min_support, "the support test itself is inside the band"
    if hi < prm.min_support:
        # no model: the rotation mask
        tight, wide, nominal = R.rin(-BAND), R.rin(+BAND), R.rin()
        assert info["model_valid"] == 0
    else:
        tight, wide, nominal = R.mask(i, j, sigma, -BAND), R.mask(i, j, sigma, +BAND), R.mask(i, j, sigma)
        assert info["model_valid"] == 1 and lo <= info["n_rescued"] <= hi
        assert np.dot(R.t_dir(i, j, sigma), info["t_dir"].astype(np.float64)) > 1.0 - 1e-6
    band = tight != wide
    assert band.sum() <= 0.02 * len(band), (name, int(band.sum()))
    assert np.array_equal(o["mask"].astype(bool)[~band], nominal[~band])
    assert o["n_in"] == int(o["mask"].sum()) == info["n_rot"] + info["n_rescued"]


def test_translation_keeps_the_parallax_tracks():
    _, s, _, o, R, _ = evaluated("translation")
    true, rin = ~s["outlier"], o["pts"].rin
    assert np.array_equal(rin, R.rin())  # (with margin: nothing within the band)
    assert o["mask"][true].mean() >= 0.90 and rin[true].mean() <= 0.75
    assert o["mask"][~true].sum() <= rin[~true].sum() + 5
    assert np.dot(o["info"]["t_dir"], s["c"] / np.linalg.norm(s["c"])) > 0.99


def test_pure_rotation_is_the_rotation_mask():
    _, _, _, o, _, _ = evaluated("pure_rotation")
    assert o["info"]["model_valid"] == 0 and np.all(o["info"]["t_dir"] == 0)
    assert np.array_equal(o["mask"].astype(bool), o["pts"].rin)


@pytest.mark.parametrize("name", list(cases.SCENES))
def test_without_a_rotation_the_mask_contains_the_rotation_ransac_mask(name):
    import oracle_lib
    s, prm = cases.scene(name), cases.params()
    S = cases.samples(5, len(s["p0"]), 1000)
    o = eo.run(s["p0"], s["p1"], s["W"], s["H"], S[:ITERS], prm, R=None, rot_samples=S)
    rmask, _ = oracle_lib.rot_ransac(s["p0"], s["p1"], s["W"], s["H"], S, float(np.float32(prm.rot_thresh_rad)))
    assert np.all(o["mask"] >= rmask) and o["info"]["n_rot"] == int(rmask.sum())


def test_sign_and_plane_tests_reject():
    """Three tracks appended to the translation scene (never sampled: the sample stream is drawn for the scene's n),
    each 3 degrees from its rotated bearing a, a perpendicular to the true direction of translation d: away from d
    in the epipolar plane (the flow translation causes: kept), towards d (rejected by the sign), and away from d
    but 3 x epi_thresh across the plane (rejected by the plane test).  An estimated direction delta away from d turns
    these planes about a, which moves a point 3 degrees from a by sin(3 deg) x delta: with delta < 2 degrees
    (asserted: t_dir . d > cos(2 deg)) by 0.11 degrees at most, well inside epi_thresh for the first track and well
    short of the 0.5 degrees the third is beyond it."""
    s, prm = cases.scene("translation"), cases.params()
    W, H, Rg = s["W"], s["H"], s["R_given"].astype(np.float64).reshape(3, 3)
    d = s["c"] / np.linalg.norm(s["c"])
    a = np.cross(d, [0.0, 1.0, 0.0])
    a /= np.linalg.norm(a)
    side = np.cross(d, a)  # unit normal direction across the plane
    th, across = np.deg2rad(3.0), 3.0 * prm.epi_thresh_rad
    away = np.cos(th) * a - np.sin(th) * d
    b1 = np.stack([away, np.cos(th) * a + np.sin(th) * d, np.cos(across) * away + np.sin(across) * side])
    p0 = np.vstack([s["p0"], np.repeat(ref.bearing_to_pixel((Rg.T @ a)[None, :], W, H), 3, axis=0)]).astype(np.float32)
    p1 = np.vstack([s["p1"], ref.bearing_to_pixel(b1, W, H)]).astype(np.float32)
    assert np.all(np.abs(p1[-3:, 1] / H - 0.5) < 0.3)
    S = cases.samples(5, len(s["p0"]), ITERS)
    o = eo.run(p0, p1, W, H, S, prm, R=s["R_given"])
    assert o["info"]["model_valid"] == 1 and np.dot(o["info"]["t_dir"], d) > np.cos(np.deg2rad(2.0))
    assert not o["pts"].rin[-3:].any()
    assert list(o["mask"][-3:]) == [1, 0, 0]
