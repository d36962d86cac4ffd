"""Diagnostic: what the round-trip check costs the LK stage, fused against composed.

One process, the config-1 pair (3840x1920, 300 corners, bench.py's erp_klt leg), erp_tracker_stage_ms's lk_ms, the
median of `steps` pipeline runs after `warm`:
  (a) the check off
  (b) the check on: the fused instance, forward search + backward search + test in one launch
  (c) the composition from the entry points that exist without the check: (a) plus the lk_ms of a run with the
      frames swapped, points = the forward-found next, set_guess = their previous positions (the status fold a
      composition also needs is not counted)
Prints the three medians and (b)/(a), (b)/(c).
Usage: fb_lk_times.py [steps] [warm]"""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402,F401

vio = importlib.import_module("360_visual_inertial_odometry_amd")
synth = importlib.import_module("360_visual_inertial_odometry_amd.synth")
steps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
warm = int(sys.argv[2]) if len(sys.argv) > 2 else 5
W, H = 3840, 1920
ctx = vio.Context(0)
a, b, _ = synth.config1(W, H)
mask = np.zeros((H, W), np.uint8)
mask[int(np.float32(H) * np.float32(0.15)):int(np.float32(H) * np.float32(0.85)), 20:W - 20] = 255
pts = ctx.gftt(a, mask, 300, float(np.float32(0.01)), 30.0)
prm = vio.default_tracker_params(max_corners=300, seed=1)
klt = vio.default_klt_params()


def lk_ms(t, before_run=None):
    out = []
    for i in range(warm + steps):
        if before_run:
            before_run()
        t.run(prm, klt)
        t.sync()
        if i >= warm:
            out.append(t.stage_ms()["lk"])
    return float(np.median(out)), float(min(out)), float(max(out))


t = vio.Tracker(ctx, W, H, max_points=512, max_corners=512)
t.upload(0, a)
t.upload(1, b)
t.set_points(pts)
off = lk_ms(t)
res = t.download()
nxt, found = res["next"].copy(), res["status"] == 1
t.set_fb(vio.default_fb_params())
on = lk_ms(t)
state = t.download_fb()[1]
t.set_fb(vio.ErpFbParams(vio.VIO_FB_OFF, 0.5))
t.upload(0, b)
t.upload(1, a)
t.set_points(nxt[found])
back = lk_ms(t, lambda: t.set_guess(pts[found]))
t.close()
ctx.close()
print("points %d, forward found %d, pass %d, back lost %d, too far %d" %
      (len(pts), int(found.sum()), int((state == 1).sum()), int((state == 2).sum()), int((state == 3).sum())))
for name, v in (("(a) check off", off), ("(b) check on, fused", on), ("    backward run alone", back)):
    print("%-24s lk_ms median %.4f  (min %.4f, max %.4f)" % (name, *v))
c = off[0] + back[0]
print("(c) composed = (a) + backward  %.4f" % c)
print("(b)/(a) %.3f   (b)/(c) %.3f" % (on[0] / off[0], on[0] / c))
