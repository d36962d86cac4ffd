"""Diagnostic: the device time of the absolute-pose RANSAC (vio_pnp_ransac_kernel_ms: its three launches) beside the
VIO_PNP solve it seeds.

  stage   n = 300 / 256 rows and n = 4096 / 1024 rows, mode A (P3P) and mode B (known rotation), on the scene family
          of tests/pnp_cases.py (40 % outlier bearings, 0.5 px noise): median and minimum of the timed calls.
  solve   one VIO_PNP solve (reference options) of the same 300 correspondences from the stage's pose:
          vio_ba_batch_kernel_ms of a one-window batch.
Usage: pnp_time.py [timed calls per configuration, default 100]"""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402,F401

import pnp_cases as cases  # noqa: E402

vio = importlib.import_module("360_visual_inertial_odometry_amd")
timed = int(sys.argv[1]) if len(sys.argv) > 1 else 100
ctx = vio.Context(0)


def median(v):
    return sorted(v)[len(v) // 2]


prm = cases.params(vio)
seed_pose = None
for n, iters in ((300, 256), (4096, 1024)):
    for known in (False, True):
        s = cases.make(1, n=n, known=0.0 if known else None)
        S = cases.samples(vio, 5, n, iters)
        for _ in range(5):
            res, _, _ = ctx.pnp_ransac(s["points"], s["bearings"], S, R=s["R_known"], params=prm)
        ms = []
        for _ in range(timed):
            ctx.pnp_ransac(s["points"], s["bearings"], S, R=s["R_known"], params=prm)
            ms.append(ctx.pnp_ransac_kernel_ms())
        print(f"vio_pnp_ransac n={n} rows={iters} mode {'B (known rotation)' if known else 'A (P3P)'}: kernel_ms median "
              f"of {timed}: {median(ms):.4f} (min {min(ms):.4f}); inliers {res['num_inliers']} status {res['status']}",
              flush=True)
        if n == 300 and not known:
            seed_pose = (s, res)

# the VIO_PNP solve of the same 300 correspondences, seeded with the stage's pose
s, res = seed_pose
n = len(s["points"])
uv = cases.bearing_to_pixel(s["bearings"].astype(np.float64)).astype(np.float32)
w = {"cols": cases.W, "rows": cases.H, "T_cb": np.eye(4)[None],
     "T_wb_init": vio.pnp_compose(res["R_cw"], res["t_cw"], np.eye(4, dtype=np.float32)).astype(np.float64)[None],
     "kf_const": np.zeros(1, np.uint8), "lm_const": np.zeros(n, np.uint8), "lm_marg": np.zeros(n, np.uint8),
     "lm_xyz": s["points"].astype(np.float64), "obs_kf": np.zeros(n, np.int32), "obs_lm": np.arange(n, dtype=np.int32),
     "obs_uv": uv}
batch = vio.BaBatch(ctx, [vio.BaProblem(w, variant=vio.VIO_PNP)])
ms = []
for k in range(5 + timed):
    batch.run()
    batch.sync()
    if k >= 5:
        ms.append(batch.kernel_ms()[0])
out = batch.download()[0]
print(f"VIO_PNP solve of the same {n} correspondences: kernel_ms median of {timed}: {median(ms):.4f} (min {min(ms):.4f}); "
      f"iterations {out['iterations']} inliers {out['num_inliers']} final cost {out['final_cost']:.4f}", flush=True)
batch.close()
ctx.close()
