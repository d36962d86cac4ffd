"""Small window-BA problems at the (K, L) shapes where the walk kernels' lane geometry can go wrong
(tests/test_ba_walk_shapes_gpu.py).  A walk chunk holds LC = 256 // K landmarks, lane t = slot * K + keyframe:

    K   L          chunks
    2   1          one landmark in a chunk of 128 slots
    3   LC = 85    one chunk exactly (lane 255 idle: 3 * 85 = 255)
    3   LC + 1     one landmark over: a second chunk of one
    7   2 LC - 1   71: a ragged last chunk (35 of 36), lanes 252..255 idle
    10  26         LC = 25: one landmark over, lanes 250..255 idle
    16  17         LC = 16: every lane used, one landmark over (visual only: VI windows have K <= 10)

Across them: about a third of the observations missing, gross-noise observations that end flagged as
outliers, constant landmarks, and the constant first keyframe every synthetic window has."""
import numpy as np

ITERS = 10  # fixed LM iterations, the timed mode
# ... but 6 for the two-observation window: its cost reaches 1e-21 at iteration 8, and from there the oracle's
# own accept / reject decisions are made on roundoff (cost changes of 1e-22 and below), so no two correct
# solvers agree on them; through iteration 6 every decision is on a cost change as large as the cost.
# (No K = 2, L = 1 window avoids this: 4 visual + 9 inertial residuals against 21 free parameters, or 4
# against 9 without the IMU, always have an exact zero of the cost whatever the pixel noise.)
ITERS_BY_NAME = {"K2-L1-vi": 6}


def thin(w, frac, seed):
    """drop about `frac` of the observations, keeping at least two of every landmark"""
    rng = np.random.default_rng(seed)
    lm = w["obs_lm"]
    keep = rng.random(len(lm)) >= frac
    for l in np.unique(lm):
        idx = np.nonzero(lm == l)[0]
        if keep[idx].sum() < 2:
            keep[idx[:2]] = True
    out = dict(w)
    for key in ("obs_kf", "obs_lm", "obs_uv"):
        out[key] = np.ascontiguousarray(w[key][keep])
    return out


def const_landmarks(w, which):
    out = dict(w)
    c = w["lm_const"].copy()
    c[list(which)] = 1
    out["lm_const"] = c
    return out


def build(vio, synth):
    """[(name, window, variant)] in batch order, and the batches as index lists (sizes 3, 2, 1)"""
    mk = synth.make_window
    LC = {k: 256 // k for k in (3, 7, 10, 16)}
    cases = [
        ("K3-L85-local", mk(K=3, L=LC[3], seed=31, all_visible=False), vio.VIO_BA_LOCAL),
        ("K3-L86-vi", const_landmarks(mk(K=3, L=LC[3] + 1, seed=32, imu=True, all_visible=False), (0, 85)),
         vio.VIO_BA_VI),
        ("K2-L1-vi", mk(K=2, L=1, seed=33, imu=True), vio.VIO_BA_VI),
        ("K7-L71-full", const_landmarks(thin(mk(K=7, L=2 * LC[7] - 1, seed=34, outlier_frac=0.06,
                                                 all_visible=False), 1.0 / 3.0, 1), (3, 36, 70)), vio.VIO_BA_FULL),
        ("K10-L26-vi", thin(mk(K=10, L=26, seed=36, imu=True, outlier_frac=0.05, all_visible=False), 1.0 / 3.0, 2),
         vio.VIO_BA_VI),
        ("K16-L17-local", thin(mk(K=16, L=17, seed=36, outlier_frac=0.05, all_visible=False), 1.0 / 3.0, 3),
         vio.VIO_BA_LOCAL),
    ]
    return cases, [[0, 1, 2], [3, 4], [5]]


def problems(vio, cases):
    return [vio.BaProblem(w, variant=var, max_iterations=ITERS_BY_NAME.get(name, ITERS), fixed_iterations=1)
            for name, w, var in cases]
