"""Diagnostic: device time of the region-mask build and what a mask costs the tracker pipeline.

  build      erp_mask_build_device, device buffers, erp_mask_kernel_ms (device events), median of `steps`:
             3840x1920 -> 960x480 and 960x480 -> 960x480, r = 10, X_WRAP, a 12 % operator mask; beside the HBM
             bound: source bytes read + dW dH / 8 bytes of plane written, at 8.0 TB/s.  (The 0 / 255 image the entry
             point also writes, dW dH bytes, is not in the bound: a tracker keeps the plane.)
  pipeline   erp_tracker_stage_ms total without stage markers on the 960x480 pair and on the config-1 pair
             (3840x1920, 300 corners, bench.py's erp_klt leg), with the mask and without it: `runs` runs of `steps`
             pipeline runs each, a run's figure is its median; median and range over the runs, and
             erp_tracker_gftt_fallbacks after a download.
A library without the mask entry points (VIO360_LIB = an older build, for A/B) gives the maskless pipeline only.
Usage: mask_time.py [steps] [runs] [frames.npz: the rendered pairs are kept there between calls]"""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

vio = importlib.import_module("360_visual_inertial_odometry_amd")
synth = importlib.import_module("360_visual_inertial_odometry_amd.synth")
steps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
runs = int(sys.argv[2]) if len(sys.argv) > 2 else 5
cache = sys.argv[3] if len(sys.argv) > 3 else None
PEAK = 8.0e12
HAS_MASK = hasattr(vio.lib(), "erp_mask_build_device")
ctx = vio.Context(0)


def operator_mask(W, H):
    """an ellipse of about 12 % of the frame, low centre, and a pole across the seam (tests/test_mask_gpu.py)"""
    y, x = np.mgrid[0:H, 0:W]
    m = np.full((H, W), 255, np.uint8)
    m[((x - W * 0.5) / (W * 0.23)) ** 2 + ((y - H * 0.84) / (H * 0.17)) ** 2 <= 1] = 0
    m[int(H * 0.3):int(H * 0.62), :int(W * 0.04)] = 0
    m[int(H * 0.3):int(H * 0.62), W - int(W * 0.03):] = 0
    return m


def median(v):
    return sorted(v)[len(v) // 2]


if HAS_MASK:
    dW, dH = 960, 480
    p = vio.mask_params(10, vio.VIO_MASK_X_WRAP)
    dst = torch.zeros((dH, dW), dtype=torch.uint8, device="cuda:0")
    for sW, sH in [(3840, 1920), (960, 480)]:
        src = torch.from_numpy(operator_mask(sW, sH)).to("cuda:0")
        torch.cuda.synchronize()
        ms = []
        for i in range(3 + steps):
            ctx.mask_build_device(src.data_ptr(), sW, sH, sW, dW, dH, p, dst.data_ptr(), dW)
            ms.append(ctx.mask_kernel_ms())
        ms = ms[3:]
        alg = sW * sH + dW * dH // 8
        bound = alg / PEAK * 1e3
        print(f"build {sW}x{sH} -> {dW}x{dH} r=10 wrap: {median(ms):.4f} ms (min {min(ms):.4f}, max {max(ms):.4f}, "
              f"median of {steps}); {alg / 1e6:.2f} MB: HBM bound {bound:.5f} ms = {100 * bound / median(ms):.1f} % "
              f"of the time", flush=True)

frames = {}
if cache and os.path.exists(cache):
    frames = dict(np.load(cache))
for W, H in [(960, 480), (3840, 1920)]:
    if f"a{W}" not in frames:
        frames[f"a{W}"], frames[f"b{W}"], _ = synth.config1(W, H)
if cache and not os.path.exists(cache):
    np.savez(cache, **frames)

for W, H in [(960, 480), (3840, 1920)]:
    a, b = frames[f"a{W}"], frames[f"b{W}"]
    region = np.zeros((H, W), np.uint8)
    region[int(np.float32(H) * np.float32(0.15)):int(np.float32(H) * np.float32(0.85)), 20:W - 20] = 255
    pts = ctx.gftt(a, region, 300, float(np.float32(0.01)), 30.0)
    prm = vio.default_tracker_params(max_corners=300, seed=1)
    t = vio.Tracker(ctx, W, H, max_points=512, max_corners=512)
    t.upload(0, a)
    t.upload(1, b)
    t.set_points(pts)
    t.set_stage_timing(False)
    cases = [("no mask", None)] + ([(f"12 % mask, r={10 * W // 960} wrap", operator_mask(W, H))] if HAS_MASK else [])
    for name, m in cases:
        if HAS_MASK:
            t.set_mask(m, vio.mask_params(10 * W // 960, vio.VIO_MASK_X_WRAP))
        for _ in range(3):
            t.run(prm)
        t.sync()
        per_run = []
        for _ in range(runs):
            tot = []
            for _ in range(steps):
                t.run(prm)
                t.sync()
                tot.append(t.stage_ms()["total"])
            per_run.append(median(tot))
        t.set_stage_timing(True)  # where the time goes: a second series with the stage markers (a few us each)
        st = []
        for _ in range(3 + steps):
            t.run(prm)
            t.sync()
            st.append(t.stage_ms())
        t.set_stage_timing(False)
        stage = {k: median([s[k] for s in st[3:]]) for k in st[0]}
        fb0 = t.gftt_fallbacks()
        t.run(prm)
        res = t.download()
        fb1 = t.gftt_fallbacks()
        print(f"pipeline {W}x{H} {name}: total ms median {median(per_run):.4f} range [{min(per_run):.4f}, "
              f"{max(per_run):.4f}] over {runs} runs of {steps} ({' '.join('%.4f' % v for v in per_run)}); "
              f"one download: fallbacks (exact tail, full sort) +{fb1[0] - fb0[0]} +{fb1[1] - fb0[1]}, "
              f"kept {int(res['kept'].sum())} of {len(pts)}, corners {len(res['corners'])}; with stage markers: "
              + "  ".join(f"{k} {v:.4f}" for k, v in stage.items()), flush=True)
    t.close()
ctx.close()
