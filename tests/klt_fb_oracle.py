"""klt_fb_oracle.py — TEST INFRASTRUCTURE ONLY (parity checker, never shipped).

The reference of the round-trip check (include/vio360.h "Round-trip check"): two calls of the guided
restatement klt_guess_oracle.klt_track -- forward, then (curr, prev, next[found], guess = pts[found]) -- and the
distance test in np.float32 (NumPy rounds every f32 operation on its own: no contraction).

  fb_track(prev, curr, pts, klt, guess, seam, max_dist) -> (next, status, err, back, fb_state, fb_d2)
      = judge(round_trip(...), max_dist), split so that one pair of searches serves several distances
  fb_step(max_dist, guess=None, log=None)   fb_track as the KLT step of klt_guess_oracle.klt_step; log collects every
                                            call's fb_track result
  fb_frontend(vio, W, H, params, seam, max_dist)   the front-end oracle with that step; .fb_stats after each track
"""
import numpy as np

import frontend_oracle as fo
import klt_guess_oracle as ko
import seam_oracle as so

CUT, WRAP = ko.CUT, ko.WRAP
NOT_RUN, PASS, BACK_LOST, TOO_FAR = 0, 1, 2, 3
F32 = np.float32


def round_trip(prev, curr, pts, klt, guess=None, seam=CUT):
    """the two searches and the distance, everything of the check that does not depend on max_dist ->
    (next, forward status, err, back, backward status, d2), the last three zero where the backward search was not
    run"""
    prev, curr = np.asarray(prev, np.uint8), np.asarray(curr, np.uint8)
    W = prev.shape[1]
    pts = np.ascontiguousarray(pts, F32).reshape(-1, 2)
    n = len(pts)
    nxt, fwd, err, _ = ko.klt_track(prev, curr, pts, klt, guess, seam)
    back, bst, d2 = np.zeros((n, 2), F32), np.zeros(n, np.uint8), np.zeros(n, F32)
    f = np.nonzero(fwd == 1)[0]
    if len(f):
        back[f], bst[f] = ko.klt_track(curr, prev, nxt[f], klt, pts[f], seam)[:2]
        with np.errstate(invalid="ignore", over="ignore"):
            dx, dy = back[f, 0] - pts[f, 0], back[f, 1] - pts[f, 1]
            if seam == WRAP:  # the short way round
                Wf, half = F32(W), F32(W) * F32(0.5)
                dx = np.where(dx > half, dx - Wf, np.where(dx < -half, dx + Wf, dx))
            d2[f] = dx * dx + dy * dy
    return nxt, fwd, err, back, bst, d2


def judge(trip, max_dist):
    """the test and the results of the header's steps 3 and 4 on a round_trip"""
    nxt, fwd, err, back, bst, d2 = trip
    with np.errstate(invalid="ignore"):
        ok = (fwd == 1) & (bst == 1) & (d2 <= F32(max_dist) * F32(max_dist))  # (a NaN fails)
    state = np.where(fwd != 1, NOT_RUN, np.where(bst != 1, BACK_LOST, np.where(ok, PASS, TOO_FAR))).astype(np.uint8)
    return nxt, ok.astype(np.uint8), err, back, state, np.where(bst == 1, d2, F32(0)).astype(F32)


def fb_track(prev, curr, pts, klt, guess=None, seam=CUT, max_dist=0.5):
    return judge(round_trip(prev, curr, pts, klt, guess, seam), max_dist)


def counts(state):
    """(checked, back_lost, too_far) as erp_frontend_fb_stats reports them"""
    state = np.asarray(state)
    return int((state != NOT_RUN).sum()), int((state == BACK_LOST).sum()), int((state == TOO_FAR).sum())


def fb_step(max_dist=0.5, guess=None, log=None):
    def step(prev, curr, pts, klt, seam):
        r = fb_track(prev, curr, pts, klt, guess, seam, max_dist)
        if log is not None:
            log.append(r)
        return r[:3]
    return step


def fb_frontend(vio, W, H, params, seam, max_dist=0.5):
    base = so.SeamFrontendOracle if seam == WRAP else fo.FrontendOracle

    class Checked(base):
        fb_stats = (0, 0, 0)

        def track(self, img):
            log = []
            with ko.klt_step(fb_step(max_dist, None, log)):
                out = super().track(img)
            assert len(log) <= 1
            self.fb_stats = counts(log[0][4]) if log else (0, 0, 0)
            return out

    return Checked(vio, W, H, params)
