"""Seeded scenes for the absolute-pose RANSAC tests (tests/test_pnp_ransac.py, tests/test_pnp_ransac_gpu.py).

A scene is a dict: points (n,3) f32 world, bearings (n,3) f32 unit, R_true / t_true (x_c = R x_w + t), R_known
((3,3) f32 or None: mode A), inlier (n,) bool: which pairs are true correspondences.  Bearings are
PixelToBearing of the projected pixel on a W x H equirectangular frame, with pixel noise added before the way back.
"""
import functools

import numpy as np

W, H = 960, 480
ITERS = 256


def so3_exp(w):
    w = np.asarray(w, np.float64)
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-12:
        return np.eye(3) + K
    return np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * K @ K


def bearing_to_pixel(b):
    b = b / np.linalg.norm(b, axis=1)[:, None]
    lon = np.arctan2(b[:, 0], b[:, 2])
    lat = -np.arcsin(np.clip(b[:, 1], -1, 1))
    return np.stack([(lon / (2 * np.pi) + 0.5) * W, (-lat / np.pi + 0.5) * H], 1)


def pixel_to_bearing(uv):
    """Camera::PixelToBearing in f64"""
    lon = (uv[:, 0] / W - 0.5) * 2 * np.pi
    lat = -(uv[:, 1] / H - 0.5) * np.pi
    b = np.stack([np.cos(lat) * np.sin(lon), -np.sin(lat), np.cos(lat) * np.cos(lon)], 1)
    return b / np.linalg.norm(b, axis=1)[:, None]


def random_dirs(rng, n, max_lat=1.2):
    lon = rng.uniform(-np.pi, np.pi, n)
    lat = rng.uniform(-max_lat, max_lat, n)
    return np.stack([np.cos(lat) * np.sin(lon), -np.sin(lat), np.cos(lat) * np.cos(lon)], 1)


def make(seed, n=300, outlier_frac=0.4, noise_px=0.5, depth=(1.0, 20.0), planar=False, t_scale=1.0, known=None,
         nan_points=0):
    rng = np.random.default_rng(seed)
    R = so3_exp(rng.normal(0, 0.6, 3))
    t = rng.normal(0, 1.0, 3) * t_scale
    # points around the camera centre c = -R^T t, in world coordinates
    c = -R.T @ t
    d = random_dirs(rng, n)
    if planar:
        # a plane 4 m in front of the world origin, seen under at most ~60 degrees
        xy = rng.uniform(-6, 6, (n, 2))
        Pw = np.stack([xy[:, 0], xy[:, 1], np.full(n, 4.0)], 1) + c
    else:
        Pw = c + d * rng.uniform(depth[0], depth[1], n)[:, None]
    Pw = Pw.astype(np.float32)
    Xc = Pw.astype(np.float64) @ R.T + t
    uv = bearing_to_pixel(Xc)
    if noise_px > 0:
        uv = uv + rng.normal(0, noise_px, uv.shape)
    B = pixel_to_bearing(uv)
    inl = np.ones(n, bool)
    if outlier_frac > 0:
        bad = rng.uniform(size=n) < outlier_frac
        B[bad] = random_dirs(rng, int(bad.sum()), max_lat=1.5)
        inl &= ~bad
    if nan_points:
        idx = np.nonzero(inl)[0][:nan_points]
        Pw[idx[0]] = np.nan
        Pw[idx[1:], 1] = np.nan
        inl[idx] = False
    Rk = None
    if known is not None:
        Rk = (so3_exp(np.deg2rad(known) * np.array([0.6, -0.64, 0.48])) @ R).astype(np.float32)
    return {"points": Pw, "bearings": B.astype(np.float32), "R_true": R, "t_true": t, "R_known": Rk, "inlier": inl}


SCENES = {
    # the issue's scene family: 300 points at 1-20 m, 40 % random outlier bearings, 0.5 px noise
    "family-1": dict(seed=1),
    "family-2": dict(seed=2),
    "planar": dict(seed=3, planar=True, outlier_frac=0.3),
    # points at 200 m, the camera 0.1 m from the world origin
    "far": dict(seed=4, depth=(200.0, 200.0), t_scale=0.1 / np.sqrt(3.0), outlier_frac=0.3),
    "nan3": dict(seed=5, nan_points=3),
    "known-exact": dict(seed=6, known=0.0),
    "known-off": dict(seed=7, known=0.05),
}
POSE_SCENES = ["family-1", "planar", "far", "known-exact", "known-off"]  # poses compared against the reference


@functools.lru_cache(maxsize=None)
def scene(name):
    return make(**SCENES[name])


@functools.lru_cache(maxsize=None)
def clean(n, seed=11, known=False):
    """no noise, no outliers: every row counts n"""
    return make(seed + n, n=n, outlier_frac=0.0, noise_px=0.0, known=0.0 if known else None)


def collinear(n=40):
    """every world point on one line (exact in f32): every P3P row is degenerate"""
    s = make(21, n=n, outlier_frac=0.0, noise_px=0.0)
    k = np.arange(n, dtype=np.float32)
    s = dict(s, points=np.stack([k, 2 * k, -k], 1).astype(np.float32) + np.float32(1.0))
    return s


def params(vio, **kw):
    p = vio.default_pnp_ransac_params()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def samples(vio, seed, n, iters=ITERS):
    return np.asarray(vio.ransac_samples(seed, n, iters), np.int32).reshape(-1, 3)


# ------------------------------------------------------------------------------------------------
# the committed cases: ("scene", name) | ("clean", n, known) | ("iters", iters, known) | ("collinear",)
SIZES = [3, 4, 5, 63, 64, 65, 255, 256, 257, 300, 4096]
ROWS = [0, 1, 31, 32, 33, 63, 64, 65, 256]   # the hypothesis kernel's workgroup is 64 rows
ALL_CASES = ([("scene", name) for name in SCENES] + [("clean", n, known) for n in SIZES for known in (False, True)] +
             [("iters", it, known) for it in ROWS for known in (False, True)] + [("collinear",)])


def case_id(case):
    return "-".join("B" if x is True else "A" if x is False else str(x) for x in case)


def compares_poses(case):
    return case[0] == "scene" and case[1] in POSE_SCENES


def case_inputs(vio, case):
    """(scene, samples (iters,3), params)"""
    if case[0] == "scene":
        s = scene(case[1])
        return s, samples(vio, 5, len(s["points"])), params(vio)
    if case[0] == "clean":
        s = clean(case[1], known=case[2])
        return s, samples(vio, 7, len(s["points"]), 64), params(vio)
    if case[0] == "iters":
        s = clean(65, known=case[2])
        return s, samples(vio, 9, 65, case[1]), params(vio)
    s = collinear()
    return s, samples(vio, 3, len(s["points"]), 64), params(vio)


_refs = {}


def reference(vio, case):
    """(scene, pnp_reference.Reference) of a committed case, computed once per session"""
    import pnp_reference as ref
    if case not in _refs:
        s, S, p = case_inputs(vio, case)
        _refs[case] = (s, ref.Reference(s["points"], s["bearings"], S, p.inlier_thresh_rad, p.min_pair_angle_rad,
                                        s["R_known"], p.min_inliers, p.refit_iters))
    return _refs[case]
