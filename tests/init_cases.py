"""Synthetic two-view cases for the monocular initialiser (Initializer.cpp): landmarks around the
camera, frame 2 = frame 1 rotated and translated (P2 = R P1 + t, the reference's T_c1c2 convention),
unit f32 bearings, optional angular noise and gross outliers."""
import numpy as np


def rodrigues(w):
    th = np.linalg.norm(w)
    if th < 1e-12:
        return np.eye(3)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def make_case(n=400, seed=0, noise_deg=0.0, outlier_frac=0.0, baseline=0.3, rot_deg=5.0, seam=0, seam_rad=2e-4):
    """seam > 0 moves the first `seam` non-outlier landmarks to longitude pi + 5 seam_rad (just past the
    +-pi seam of the panorama), keeps their exact bearing in frame 2 and observes them in frame 1 at
    pi - seam_rad.  The mid-point moves up to half of the way from the observed ray to the landmark, so
    for most of them it projects on the far side of the seam from its observation, where the reference's
    pixel error (no wrap-around) is a whole image width.  Drawn after everything else, so
    the arrays of seam = 0 do not change."""
    rng = np.random.default_rng(seed)
    # landmarks on a shell around the camera (360 degrees; |lat| <= 60 deg), range 2..10 m
    lon = rng.uniform(-np.pi, np.pi, n)
    lat = rng.uniform(-np.pi / 3, np.pi / 3, n)
    rr = rng.uniform(2.0, 10.0, n)
    P1 = np.stack([np.cos(lat) * np.sin(lon), -np.sin(lat), np.cos(lat) * np.cos(lon)], 1) * rr[:, None]
    R = rodrigues(rng.normal(size=3) * np.deg2rad(rot_deg) / np.sqrt(3))
    t = rng.normal(size=3)
    t = t / np.linalg.norm(t) * baseline
    P2 = P1 @ R.T + t
    b1 = P1 / np.linalg.norm(P1, axis=1, keepdims=True)
    b2 = P2 / np.linalg.norm(P2, axis=1, keepdims=True)
    if noise_deg > 0:
        for b in (b1, b2):
            b += rng.normal(size=b.shape) * np.deg2rad(noise_deg)
            b /= np.linalg.norm(b, axis=1, keepdims=True)
    n_out = int(round(outlier_frac * n))
    if n_out:
        idx = rng.choice(n, n_out, replace=False)
        v = rng.normal(size=(n_out, 3))
        b2[idx] = v / np.linalg.norm(v, axis=1, keepdims=True)
    if seam:
        out = set(idx.tolist()) if n_out else set()
        pick = np.array([i for i in range(n) if i not in out][:seam])

        def at(lon):
            return np.stack([np.cos(lat[pick]) * np.sin(lon), -np.sin(lat[pick]),
                             np.cos(lat[pick]) * np.cos(lon) * np.ones(len(pick))], 1)
        P1[pick] = at(np.pi + 5 * seam_rad) * rr[pick, None]
        q = P1[pick] @ R.T + t
        b2[pick] = q / np.linalg.norm(q, axis=1, keepdims=True)
        b1[pick] = at(np.pi - seam_rad)
    return b1.astype(np.float32), b2.astype(np.float32), R, t, P1


# (seed, noise_deg, outlier_frac, n, ransac_threshold, seam, sample seed, max_reprojection_error): the
# cases of the independent-reference check (tests/mono_init_reference.py), each run at 960x480 and at
# 3840x1920 with 200 sample rows.  The sample seed is the case seed unless one of its first 64 rows is
# near-degenerate (sigma_8 / sigma_1 < 1e-4), where the 8-point answer is arbitrary.
REFERENCE_CASES = [
    (1, 0.0, 0.0, 400, 0.1, 0, 1, 5.0), (2, 0.05, 0.0, 1000, 0.1, 0, 2, 5.0), (3, 0.02, 0.1, 800, 0.1, 0, 3, 5.0),
    (4, 0.1, 0.3, 2000, 0.1, 0, 4, 5.0), (5, 0.0, 0.0, 4096, 0.1, 0, 105, 5.0),
    # size edges: n = 8 / 9, the 64-lane refit stride, the 256-thread workgroup, the bitonic padding
    (15, 0.0, 0.0, 8, 0.01, 0, 15, 5.0), (16, 0.02, 0.0, 9, 0.01, 0, 16, 5.0), (9, 0.02, 0.0, 63, 0.01, 0, 109, 5.0),
    (10, 0.02, 0.0, 64, 0.01, 0, 10, 5.0), (11, 0.02, 0.0, 65, 0.01, 0, 11, 5.0),
    (12, 0.05, 0.1, 255, 0.01, 0, 12, 5.0), (13, 0.05, 0.1, 256, 0.01, 0, 13, 5.0),
    (14, 0.05, 0.1, 257, 0.01, 0, 14, 5.0), (8, 0.02, 0.05, 4095, 0.01, 0, 8, 5.0),
    (5, 0.0, 0.0, 4096, 0.01, 0, 105, 5.0),
    # failure statuses (with max_reprojection_error = 5 px = TestPoseCandidate's own bar, validation
    # cannot fail after the pose stage passed: the second case tightens it)
    (6, 0.05, 0.1, 129, 0.1, 0, 6, 5.0), (7, 0.03, 0.05, 257, 0.1, 0, 7, 2.0),
    # mid-points across the +-pi seam: the reference does not wrap the pixel error
    (17, 0.02, 0.0, 300, 0.01, 12, 17, 5.0),
]
# status the reference must reach: (seed, n, width) -> VIO_INIT_*; every other case ends VIO_INIT_OK
EXPECTED_STATUS = {(6, 129, 960): 3, (6, 129, 3840): 3, (7, 257, 960): 5, (7, 257, 3840): 3}
RESOLUTIONS = [(960, 480), (3840, 1920)]


def reference_case(vio, case, width=960, height=480, iters=200):
    """(b1, b2, S, params, truth) of one REFERENCE_CASES entry."""
    seed, noise, outl, n, thr, seam, sseed, mxe = case
    b1, b2, R, t, P1 = make_case(n=n, seed=seed, noise_deg=noise, outlier_frac=outl, seam=seam)
    S = vio.mono_init_samples(sseed, n, iters)
    mf = 100 if case in REFERENCE_CASES[:5] else min(100, max(4, n // 2))
    P = vio.abi.mono_init_params(width=width, height=height, min_features=mf, ransac_iterations=iters,
                                 ransac_threshold=thr, max_reprojection_error=mxe)
    return b1, b2, S, P, (R, t, P1)
