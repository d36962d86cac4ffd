"""CPU checks of the round-trip check's reference (tests/klt_fb_oracle.py) and of the host-only parts of the feature:

  1. erp_fb_check, the new exports, the header's declarations and the Python mirrors;
  2. the reference on the occluded pair of tests/fb_cases.py reproduces DESIGN 4.12's table, and the check is worth
     having: it rejects the wrong tracks, keeps the right ones, and empties the pipeline's `kept` of wrong tracks;
  3. the front-end sequence exercises the check in both seam modes;
  4. the check survives a gyro-seeded search beyond the pyramid's reach.
Nothing here touches a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fb_cases as fc
import guess_cases as gc
import klt_fb_oracle as fbo
import klt_guess_oracle as ko
import seam_oracle as so

EINVAL = -22
MODES = (ko.CUT, ko.WRAP)
NEW = ["erp_fb_check", "erp_klt_track_fb", "erp_tracker_set_fb", "erp_tracker_download_fb", "erp_frontend_set_fb",
       "erp_frontend_fb_stats"]
# DESIGN 4.12's table, (W, mode) -> forward found, of them wrong, pass, back lost, too far, wrong that pass, right
# that are rejected; and the forward-found / passing counts of the plain pair
TABLE = {(512, ko.CUT): (268, 26, 231, 7, 30, 0, 11), (512, ko.WRAP): (272, 27, 236, 0, 36, 0, 9),
         (328, ko.CUT): (274, 57, 183, 6, 85, 1, 35), (328, ko.WRAP): (275, 59, 187, 0, 88, 1, 30)}
PLAIN = {(512, ko.CUT): (268, 265), (512, ko.WRAP): (272, 272), (328, ko.CUT): (273, 263), (328, ko.WRAP): (275, 275)}
# the pipeline oracle (max_corners 100, seed 21): wrong tracks in `kept` without the check, `kept` without / with it
PIPELINE = {(512, ko.CUT): (3, 225, 214), (512, ko.WRAP): (5, 247, 233), (328, ko.CUT): (4, 202, 172),
            (328, ko.WRAP): (4, 217, 183)}


def test_fb_check_and_the_new_entry_points(vio):
    L = vio.lib()
    for n in NEW:
        assert hasattr(L, n) and n in vio.EXPORTS, n
    assert L.vio_abi_version() == 4
    fb = vio.default_fb_params()
    assert (fb.mode, fb.max_dist) == (vio.VIO_FB_ON, 0.5) and C.sizeof(fb) == 8
    assert vio.default_fb_params(2.0).max_dist == 2.0
    assert L.erp_fb_check(C.byref(fb)) == 0
    assert L.erp_fb_check(C.byref(vio.ErpFbParams(vio.VIO_FB_OFF, 0.5))) == 0
    assert L.erp_fb_check(C.byref(vio.ErpFbParams(vio.VIO_FB_ON, 0.0))) == 0
    assert L.erp_fb_check(None) == EINVAL
    for mode, dist in ((2, 0.5), (-1, 0.5), (1, -1.0), (1, float("nan")), (1, float("inf")), (0, -1.0)):
        assert L.erp_fb_check(C.byref(vio.ErpFbParams(mode, dist))) == EINVAL, (mode, dist)
    # the header declares every new entry point, the struct and the enumerators
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "vio360.h")) as f:
        header = f.read()
    for n in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % n, header), n
    assert re.search(r"typedef struct erp_fb_params\s*\{\s*int32_t mode;[^}]*float max_dist;[^}]*\}", header)
    for name, value in (("VIO_FB_OFF", 0), ("VIO_FB_ON", 1), ("VIO_FB_NOT_RUN", 0), ("VIO_FB_PASS", 1),
                        ("VIO_FB_BACK_LOST", 2), ("VIO_FB_TOO_FAR", 3)):
        assert re.search(r"\b%s = %d\b" % (name, value), header) and getattr(vio, name) == value, name
    for n in ("set_fb", "download_fb"):
        assert hasattr(vio.Tracker, n)
    for n in ("set_fb", "fb_stats"):
        assert hasattr(vio.Frontend, n)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("W,H", fc.SIZES)
def test_reference_on_the_occluded_pair(vio, W, H, mode):
    """regenerates DESIGN 4.12's table (printed), and holds the bars: of the wrong forward tracks at least 90 % are
    rejected (reference: 100, 100, 98.2, 98.3 %); on the plain pair at least 95 % of the forward-found pass
    (98.9, 100, 96.3, 100 %)"""
    klt = vio.default_klt_params()
    pts, tr = fc.points(W, H), fc.truth(W, H)
    assert len(pts) == (272 if W == 512 else 275)
    prev, curr = fc.occluded(W, H)
    fwd = ko.klt_track(prev, curr, pts, klt, None, mode)
    r = fbo.fb_track(prev, curr, pts, klt, None, mode, 0.5)
    # the composition: next / err are the forward search's, status = forward AND pass
    assert np.array_equal(r[0], fwd[0]) and np.array_equal(r[2], fwd[2])
    assert np.array_equal(r[1], (fwd[1] == 1) & (r[4] == fbo.PASS))
    assert np.array_equal(r[4] == fbo.NOT_RUN, fwd[1] == 0)
    assert not r[3][r[4] == fbo.NOT_RUN].any() and not r[5][(r[4] == fbo.NOT_RUN) | (r[4] == fbo.BACK_LOST)].any()
    found = fwd[1] == 1
    wrong = found & (fc.error_px(fwd[0], tr, W) > fc.WRONG_PX)
    checked, back_lost, too_far = fbo.counts(r[4])
    row = (int(found.sum()), int(wrong.sum()), int((r[1] == 1).sum()), back_lost, too_far,
           int((wrong & (r[1] == 1)).sum()), int((found & ~wrong & (r[1] == 0)).sum()))
    print("occluded %dx%d mode %d:" % (W, H, mode), row)
    assert checked == row[0]
    assert row == TABLE[(W, mode)]
    assert row[1] >= 20 and (row[1] - row[5]) >= 0.9 * row[1]
    p0, p1 = fc.plain(W, H)
    f2 = ko.klt_track(p0, p1, pts, klt, None, mode)
    r2 = fbo.fb_track(p0, p1, pts, klt, None, mode, 0.5)
    n_found, n_pass = int((f2[1] == 1).sum()), int((r2[1] == 1).sum())
    print("plain    %dx%d mode %d: found %d pass %d" % (W, H, mode, n_found, n_pass))
    assert (n_found, n_pass) == PLAIN[(W, mode)]
    assert n_pass >= 0.95 * n_found


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("W,H", fc.SIZES)
def test_pipeline_oracle_keeps_no_wrong_track(vio, W, H, mode):
    """LK, filter, RANSAC, discs, GFTT: `kept` holds at least 3 wrong tracks without the check and none with it"""
    from test_tracker_gpu import pipeline_oracle
    klt = vio.default_klt_params()
    prm = vio.default_tracker_params(max_corners=100, seed=21)
    pts, tr = fc.points(W, H), fc.truth(W, H)
    prev, curr = fc.occluded(W, H)

    def run(step):
        with ko.klt_step(step):
            if mode == ko.WRAP:
                return so.pipeline_oracle(vio, prev, curr, pts, prm, klt)[:4]
            return pipeline_oracle(vio, prev, curr, pts, prm, klt)

    off = run(lambda a, b, p, k, m: ko.klt_track(a, b, p, k, None, m)[:3])
    on = run(fbo.fb_step(0.5))
    wrong = [int(((r[2] == 1) & (fc.error_px(r[0], tr, W) > fc.WRONG_PX)).sum()) for r in (off, on)]
    got = (wrong[0], int(off[2].sum()), int(on[2].sum()))
    print("pipeline %dx%d mode %d: wrong kept without %d with %d, kept %d -> %d" % (W, H, mode, wrong[0], wrong[1],
                                                                                  got[1], got[2]))
    assert wrong[0] >= 3 and wrong[1] == 0
    assert got == PIPELINE[(W, mode)]


@pytest.mark.parametrize("mode", MODES)
def test_front_end_sequence_exercises_the_check(vio, mode):
    """measured: too_far sums to 8 (CUT) and 10 (WRAP) over the five frames, back_lost to 0"""
    W, H = fc.SIZES[0]
    fe = fbo.fb_frontend(vio, W, H, vio.default_frontend_params(seed=3), mode, 0.5)
    stats = []
    for img in fc.frontend_sequence():
        fe.track(img)
        stats.append(fe.fb_stats)
    print("front-end oracle mode", mode, "fb stats per frame", stats)
    assert stats[0] == (0, 0, 0) and all(s[0] > 0 for s in stats[1:])
    assert sum(s[2] for s in stats) >= 1
    assert (sum(s[2] for s in stats), sum(s[1] for s in stats)) == ((8, 0) if mode == ko.CUT else (10, 0))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("W,H", gc.SIZES)
def test_check_survives_a_guided_search(vio, W, H, mode):
    """yaw 120 px, pitch 10 degrees, the forward search seeded by the (slightly wrong) gyro rotation: of the points
    the guided search brings within 1.5 px of the truth, at least 90 % pass the check -- the backward search starts at
    the previous position, so the displacement's size does not matter.  Measured share: DESIGN 4.12."""
    prev, curr, pts, truth, R_seed = gc.large("yaw120_pitch10", W, H)
    pts, truth = fc.few(pts), fc.few(truth)
    klt = vio.default_klt_params()
    guess = ko.predict(pts, R_seed, W, H)[0].astype(np.float32)
    r = fbo.fb_track(prev, curr, pts, klt, guess, mode, 0.5)
    fwd = ko.klt_track(prev, curr, pts, klt, guess, mode)
    right = (fwd[1] == 1) & (gc.error_px(fwd[0], truth, W) < 1.5)
    share = float((r[1][right] == 1).mean())
    print("guided + check %dx%d mode %d: right %d of %d, of them pass %.4f" % (W, H, mode, right.sum(), len(pts), share))
    assert right.sum() >= 100
    assert share >= 0.90
