"""Diagnostic: what the known-rotation epipolar stage costs the tracker pipeline, and its one-shot entry point.

  pipeline   960x480, 300 corners of the first frame of synth.erp_translation_sequence (a camera moving past near and
             far columns while it yaws 3 columns), erp_tracker_stage_ms with the stage markers: the median `ransac`
             interval (sampler + rotation hypotheses + selection + epipolar kernels + discs) and the median total of
             200 timed runs after warm-up, for three configurations taken in alternating blocks of 20 runs:
               mode off                    today's fused RANSAC tail
               mode on, no prediction      rotation RANSAC (1000 hypotheses), unfused selection, 256 plane hypotheses
               mode on, with a prediction  erp_tracker_set_rotation before every run: no rotation hypothesis
             (the prediction also seeds LK: the `lk` interval is printed beside it)
  one-shot   erp_epi_ransac on 1000 synthetic tracks, wall clock around the blocking call (it creates and destroys its
             scratch tracker): given rotation / rotation RANSAC first, beside erp_rot_ransac on the same tracks.
A library without the entry points (VIO360_LIB = an older build, for A/B) gives the mode-off figures only.
Usage: epi_time.py [timed runs per configuration, default 200]"""
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402,F401

vio = importlib.import_module("360_visual_inertial_odometry_amd")
synth = importlib.import_module("360_visual_inertial_odometry_amd.synth")
timed = int(sys.argv[1]) if len(sys.argv) > 1 else 200
BLOCK = 20
HAS_EPI = hasattr(vio.lib(), "erp_epi_ransac")
ctx = vio.Context(0)


def median(v):
    return sorted(v)[len(v) // 2]


W, H = 960, 480
a, b = synth.erp_translation_sequence(W, H, 2, 0.05, 3)
R = synth.rot_yaw_pitch(3 * 360.0 / W, 0.0).astype(np.float32)
region = np.zeros((H, W), np.uint8)
region[int(np.float32(H) * np.float32(0.15)):int(np.float32(H) * np.float32(0.85)), 20:W - 20] = 255
pts = ctx.gftt(a, region, 300, float(np.float32(0.01)), 20.0)
prm = vio.default_tracker_params(max_corners=300, seed=1)
t = vio.Tracker(ctx, W, H, max_points=512, max_corners=512)
t.upload(0, a)
t.upload(1, b)
t.set_points(pts)
t.set_stage_timing(True)
configs = [("mode off", False, False)]
if HAS_EPI:
    configs += [("mode on, no prediction", True, False), ("mode on, with a prediction", True, True)]


def one(on, predicted):
    if HAS_EPI:
        t.set_epipolar(vio.default_epi_params(vio.VIO_EPI_ON if on else vio.VIO_EPI_OFF))
    if predicted:
        t.set_rotation(R)
    t.run(prm)
    t.sync()
    return t.stage_ms()


for _, on, predicted in configs:  # warm-up: every configuration's kernels
    for _ in range(5):
        one(on, predicted)
series = {name: [] for name, _, _ in configs}
for _ in range((timed + BLOCK - 1) // BLOCK):
    for name, on, predicted in configs:
        series[name] += [one(on, predicted) for _ in range(BLOCK)]
for name, on, predicted in configs:
    s = series[name][:timed]
    one(on, predicted)
    kept = int(t.download()["kept"].sum())
    info = t.download_epi() if on else None
    print(f"pipeline {W}x{H} {len(pts)} points, {name}: median of {len(s)} runs: ransac_ms "
          f"{median([x['ransac'] for x in s]):.4f} (min {min(x['ransac'] for x in s):.4f})  total_ms "
          f"{median([x['total'] for x in s]):.4f} (min {min(x['total'] for x in s):.4f})  lk_ms "
          f"{median([x['lk'] for x in s]):.4f}; kept {kept}"
          + (f", rotation inliers {info['n_rot']}, rescued {info['n_rescued']}" if info else ""), flush=True)
t.close()

# one-shot: 1000 tracks of a translating camera (depths 0.8 .. 15 m, 0.3 m step, 3 degrees), 25 % gross outliers
rng = np.random.default_rng(1)
n = 1000
lon, lat = rng.uniform(-3.0, 3.0, n), rng.uniform(-0.9, 0.9, n)
X0 = rng.uniform(0.8, 15.0, n)[:, None] * np.stack([np.cos(lat) * np.sin(lon), -np.sin(lat), np.cos(lat) * np.cos(lon)], 1)
Rt = synth.so3_exp(np.deg2rad(3.0) * np.array([0.3, 0.9, 0.3]) / np.linalg.norm([0.3, 0.9, 0.3]))
X1 = X0 @ Rt.T - np.array([0.2, 0.1, 0.2])
p0, p1 = synth.erp_project(X0, W, H), synth.erp_project(X1, W, H)
bad = rng.uniform(size=n) < 0.25
p1[bad] += rng.uniform(-40, 40, (n, 2))[bad]
S = vio.ransac_samples(3, n, 1000)
calls = [("erp_rot_ransac, 1000 hypotheses", lambda: ctx.rot_ransac(p0, p1, W, H, S))]
if HAS_EPI:
    epi = vio.default_epi_params(vio.VIO_EPI_ON)
    calls += [("erp_epi_ransac, R given, 256 hypotheses", lambda: ctx.epi_ransac(p0, p1, W, H, S[:3 * 256], R=Rt, params=epi)),
              ("erp_epi_ransac, R = NULL, 1000 rows", lambda: ctx.epi_ransac(p0, p1, W, H, S, params=epi))]
for name, fn in calls:
    for _ in range(5):
        out = fn()
    ms = []
    for _ in range(timed):
        t0 = time.perf_counter()
        out = fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    print(f"one-shot {n} points, {name}: wall ms of the blocking call, median of {timed}: {median(ms):.4f} "
          f"(min {min(ms):.4f}); inliers {int(out[1])}", flush=True)
ctx.close()
