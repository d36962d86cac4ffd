"""seam_oracle.py — TEST INFRASTRUCTURE ONLY (parity checker, never shipped).

The seam wrap mode (VIO_SEAM_WRAP, include/vio360.h) restated on the CPU oracle, unchanged: every operation is the
flat operation on the horizontally periodic continuation of the frame, so the references run oracle_lib on frames
extended by columns from the other side and shift the coordinates back.

  KLT       oracle_lib.klt_track on extend(prev), extend(curr) at x + left; next.x - left, folded into [0, W).  With
            left = 0 the coordinates are the frame's own: the arithmetic is bit for bit that of the wrapped kernels
            (the right seam band).  With left > 0 every coordinate is rounded at another offset: equal up to f32
            rounding (the left seam band).
  GFTT      the candidate list (masked maximum, 3x3 NMS, scan, tie order) from oracle_lib.gftt on the extended frame
            with a mask that is zero on the aprons, no cap and no minimum distance; then a greedy pass here with
            the distance on the cylinder.
  pipeline  these two, the filter without a left / right margin, oracle_lib.rot_ransac on the folded points and
            CreateFeatureMask's discs with columns modulo W.
"""
import numpy as np

import frontend_oracle as fo
import oracle_lib

CUT, WRAP = 0, 1
APRON = 128   # columns of continuation for LK: the window, its margins and any flow of the tests
GF_APRON = 8  # for detection: Sobel + box + NMS reach 3 columns


def extend(F, left, right):
    """the frame with `left` columns of its right end before it and `right` columns of its left end after it"""
    F = np.asarray(F)
    W = F.shape[1]
    assert 0 <= left <= W and 0 <= right <= W
    return np.ascontiguousarray(np.concatenate([F[:, W - left:], F, F[:, :right]], axis=1))


def fold_x(x, W):
    """x (float32) folded into [0, W) by one f32 +-W; a fold that rounds to W gives 0"""
    x = np.asarray(x, np.float32).copy()
    Wf = np.float32(W)
    lo, hi = x < 0, x >= Wf
    x[lo] = x[lo] + Wf
    x[hi] = x[hi] - Wf
    x[x == Wf] = 0
    return x


def klt_track(prev, curr, pts, klt, left=0, right=APRON):
    """-> (next with x folded, status, err) of the periodic continuation, computed at column offset `left`"""
    W = prev.shape[1]
    p = np.asarray(pts, np.float32).reshape(-1, 2).copy()
    p[:, 0] += np.float32(left)
    nxt, st, err = oracle_lib.klt_track(extend(prev, left, right), extend(curr, left, right), p, klt)
    nxt[:, 0] = fold_x(nxt[:, 0] - np.float32(left), W)
    return nxt, st, err


def gftt_candidates(F, mask, quality):
    """every candidate of the wrapped detection in the order the greedy pass takes them: (n, 2) float32"""
    H, W = F.shape
    P = GF_APRON
    m = np.zeros((H, W + 2 * P), np.uint8)
    m[:, P:P + W] = 255 if mask is None else np.asarray(mask, np.uint8)
    c = oracle_lib.gftt(extend(F, P, P), m, 0, quality, 0.0)
    c[:, 0] -= np.float32(P)
    assert ((c[:, 0] >= 0) & (c[:, 0] < W)).all()
    return c


def greedy(cand, W, max_corners, min_dist, wrapped=True):
    """goodFeaturesToTrack's min-distance pass with the distance on the cylinder -> (accepted indices, for each
    rejected candidate whether only the wrapped distance rejected it)"""
    if min_dist < 1:
        n = len(cand) if max_corners <= 0 else min(len(cand), max_corners)
        return list(range(n)), []
    md2 = float(min_dist) * float(min_dist)
    acc, ax, ay, seam_only = [], [], [], []
    for i, (x, y) in enumerate(np.asarray(cand, np.int64)):
        if acc:
            dx = np.abs(np.array(ax) - x)
            dy = np.array(ay) - y
            flat = (dx * dx + dy * dy < md2).any()
            dxw = np.minimum(dx, W - dx) if wrapped else dx
            if (dxw * dxw + dy * dy < md2).any():
                seam_only.append(not flat)
                continue
        acc.append(i)
        ax.append(x)
        ay.append(y)
        if max_corners > 0 and len(acc) == max_corners:
            break
    return acc, seam_only


def gftt(F, mask, max_corners, quality, min_dist):
    """the wrapped goodFeaturesToTrack -> (k, 2) float32"""
    cand = gftt_candidates(F, mask, quality)
    acc, _ = greedy(cand, F.shape[1], max_corners, min_dist)
    return cand[acc].copy()


def gftt_stats(F, mask, max_corners, quality, min_dist):
    """(corners, accepted corners within min_dist of the seam, rejections only the wrapped distance makes)"""
    W = F.shape[1]
    cand = gftt_candidates(F, mask, quality)
    acc, seam_only = greedy(cand, W, max_corners, min_dist)
    c = cand[acc]
    near = int(((c[:, 0] < min_dist) | (c[:, 0] >= W - min_dist)).sum())
    return c.copy(), near, int(sum(seam_only))


def region_mask(W, H, polar):
    """the analytic detection mask in wrap mode: the polar rows, no left / right margin"""
    m = np.zeros((H, W), np.uint8)
    m[int(np.float32(H) * np.float32(polar)):int(np.float32(H) * (np.float32(1.0) - np.float32(polar)))] = 255
    return m


def discs(mask, centres, r):
    """cv::circle(filled) around every (cx, cy) of `centres`, cx in [0, W], with its columns taken modulo W: drawn
    on three copies of the frame side by side (r < W: no span leaves them), then folded onto the mask"""
    H, W = mask.shape
    assert 0 <= r < W
    wide = np.full((H, 3 * W), 255, np.uint8)
    for cx, cy in centres:
        assert 0 <= cx <= W
        fo.cv_circle_fill(wide, cx + W, cy, r)
    mask &= wide[:, :W] & wide[:, W:2 * W] & wide[:, 2 * W:]


def keep_filter(nxt, st, W, H, margin, polar):
    """status AND NOT polar AND NOT (top / bottom margin): the wrap-mode filter on folded points"""
    vr = nxt[:, 1] / np.float32(H)
    pol = (vr < np.float32(polar)) | (vr > np.float32(1.0) - np.float32(polar))
    m = np.float32(margin)
    nearb = (nxt[:, 1] < m) | (nxt[:, 1] > np.float32(H) - m)
    return (st == 1) & ~pol & ~nearb


def pipeline_oracle(vio, prev, curr, pts, prm, klt):
    """erp_tracker_run in wrap mode composed from the oracle pieces -> (next, status, kept, corners, number of kept
    points whose disc crosses the seam).  Bitwise for points the right-band KLT reference covers (x + flow >= 0)."""
    H, W = prev.shape
    nxt, st, _ = klt_track(prev, curr, pts, klt)
    good = np.nonzero(keep_filter(nxt, st, W, H, prm.boundary_margin, prm.polar_ratio))[0]
    kept = np.zeros(len(pts), np.uint8)
    if len(good) >= 3:
        s = vio.ransac_samples(prm.ransac_seed, len(good), prm.ransac_iters)
        mk, _ = oracle_lib.rot_ransac(np.asarray(pts, np.float32)[good], nxt[good], W, H, s, prm.ransac_thresh_rad)
        kept[good] = mk
    else:
        kept[good] = 1
    mask = region_mask(W, H, prm.polar_ratio)
    r = int(prm.min_dist)
    centres = [(int(np.rint(nxt[i, 0])), int(np.rint(nxt[i, 1]))) for i in np.nonzero(kept)[0]]
    discs(mask, centres, r)
    crossing = sum(int(cx - r < 0 or cx + r >= W) for cx, _ in centres)
    return nxt, st, kept, gftt(curr, mask, prm.max_corners, prm.quality, prm.min_dist), crossing


class SeamFrontendOracle(fo.FrontendOracle):
    """FrontendOracle in wrap mode: LK on the continuation (both aprons: left-band points are exact only up to f32
    rounding of the offset), the filter without a left / right margin, wrapped discs and detection.  The grid
    assignment, RemoveClusteredFeatures and LimitFeaturesPerGrid stay flat."""

    def _base_mask(self):
        return region_mask(self.W, self.H, 0.15)

    def _detect(self, img, with_discs):
        m = self._base_mask()
        if with_discs:
            discs(m, [(int(np.rint(np.float32(f["x"]))), int(np.rint(np.float32(f["y"])))) for f in self.feats],
                  int(self.p.min_distance))
        return gftt(img, m, self.p.max_features, float(np.float32(self.p.quality_level)),
                    float(np.float32(self.p.min_distance)))

    def track(self, img):
        p, W, H = self.p, self.W, self.H
        if self.frame == 0 or not self.feats:
            return super().track(img)  # detection only: the mode enters through _detect
        prev = np.array([[f["x"], f["y"]] for f in self.feats], np.float32)
        nxt, st, _ = klt_track(self.prev, img, prev, self.vio.default_klt_params(), APRON, APRON)
        good = list(np.nonzero(keep_filter(nxt, st, W, H, p.boundary_margin, 0.15))[0])
        inl = np.ones(len(good), np.uint8)
        if len(good) >= 3:
            s = self.vio.ransac_samples((p.ransac_seed + self.frame) & 0xffffffff, len(good), 1000)
            inl, _ = oracle_lib.rot_ransac(prev[good], nxt[good], W, H, s, self.vio.ransac_threshold())
        cur = []
        for j, i in enumerate(good):
            if inl[j]:
                f = self.feats[i]
                cur.append(dict(id=f["id"], x=float(nxt[i, 0]), y=float(nxt[i, 1]), tc=f["tc"] + 1, age=f["age"] + 1))
        self.feats = cur
        self.num_tracked = len(cur)
        if p.remove_clustered:
            self.feats = fo.remove_clustered(self.feats, W, H, p.clustered_std_ratio)
        self.feats = fo.assign_and_limit(self.feats, W, H, p.grid_cols, p.grid_rows, p.max_features_per_grid)
        if len(self.feats) < p.max_features:
            c = self._detect(img, True)
            self.feats += [dict(id=self.next_id + i, x=float(x), y=float(y), tc=0, age=0) for i, (x, y) in enumerate(c)]
            self.next_id += len(c)
            self.num_detected = len(c)
            self.feats = fo.assign_and_limit(self.feats, W, H, p.grid_cols, p.grid_rows, p.max_features_per_grid)
        else:
            self.num_detected = 0
        self.prev = img
        self.frame += 1
        return {"ids": np.array([f["id"] for f in self.feats], np.int32),
                "xy": np.array([[f["x"], f["y"]] for f in self.feats], np.float32).reshape(-1, 2),
                "track_count": np.array([f["tc"] for f in self.feats], np.int32),
                "age": np.array([f["age"] for f in self.feats], np.int32),
                "num_tracked": self.num_tracked, "num_detected": self.num_detected}
