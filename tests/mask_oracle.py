"""mask_oracle.py — TEST INFRASTRUCTURE ONLY (parity checker, never shipped).

numpy restatement of the region masks (erp_mask_*, include/vio360.h).  A mask is a u8 image, nonzero = usable;
every function here returns 0 / 255.

  reduce   per axis the footprint of destination index d is the set of source indices with a tap (d, si, alpha) in
           resize_general_oracle.area_tab(ssize, dsize); a destination pixel is usable iff every source pixel of
           footprint_x x footprint_y is
  erode    usable'(x, y) = AND of usable(x + dx, y + dy), |dx|, |dy| <= r; rows outside count as usable, columns
           outside count as usable (X_CLAMP) or are taken modulo W (X_WRAP)
  warp     a warp pixel is usable iff its map entry is valid and its four taps are usable: columns modulo sW under
           X_WRAP, rows clamped under Y_REPLICATE, a tap outside the source under a CONSTANT border is not usable
and the tracker pipeline / front end with the mask's two effects: detection mask and tracked-point filter.
"""
import numpy as np

import frontend_oracle as fo
import oracle_lib
import resize_general_oracle as rgo
import warp_oracle as wo

X_CLAMP, X_WRAP = 0, 1


def _u8(usable):
    return np.where(usable, 255, 0).astype(np.uint8)


def footprint(ssize, dsize):
    """list over d of the sorted source indices that area_tab gives destination index d"""
    di, si, _ = rgo.area_tab(ssize, dsize)
    return [np.unique(si[di == d]) for d in range(dsize)]


def reduce(mask, dW, dH):
    u = np.asarray(mask) != 0
    sH, sW = u.shape
    assert 0 < dW <= sW and 0 < dH <= sH
    fx, fy = footprint(sW, dW), footprint(sH, dH)
    h = np.stack([u[:, f].all(axis=1) for f in fx], axis=1)      # (sH, dW)
    return _u8(np.stack([h[f].all(axis=0) for f in fy], axis=0))  # (dH, dW)


def erode(mask, r, border_x=X_CLAMP):
    u = np.asarray(mask) != 0
    H, W = u.shape
    assert 0 <= r <= 255 and border_x in (X_CLAMP, X_WRAP)
    x = np.arange(W)
    h = np.ones_like(u)
    for dx in range(-r, r + 1):
        if border_x == X_WRAP:
            h &= u[:, (x + dx) % W]
        else:
            inside = (x + dx >= 0) & (x + dx < W)
            h &= np.where(inside[None, :], u[:, np.clip(x + dx, 0, W - 1)], True)
    y = np.arange(H)
    v = np.ones_like(u)
    for dy in range(-r, r + 1):
        inside = (y + dy >= 0) & (y + dy < H)
        v &= np.where(inside[:, None], h[np.clip(y + dy, 0, H - 1)], True)
    return _u8(v)


def build(mask, dW, dH, r=0, border_x=X_CLAMP):
    """erp_mask_build"""
    return erode(reduce(mask, dW, dH), r, border_x)


def warp_usable(src_mask, map_x, map_y, sW, sH, border_x, border_y):
    """src_mask (sH, sW) u8 or None, maps (wH, wW) float32 -> (wH, wW) 0 / 255"""
    u = np.ones((sH, sW), bool) if src_mask is None else np.asarray(src_mask) != 0
    assert u.shape == (sH, sW)
    qx, vx = wo.quantize(map_x, sW, border_x)
    qy, vy = wo.quantize(map_y, sH, border_y)
    ix, iy = qx >> 5, qy >> 5

    def tap(xx, yy):
        inside = np.ones(xx.shape, bool)
        if border_x == wo.X_WRAP:
            xx = xx % sW
        else:
            inside &= (xx >= 0) & (xx < sW)
        if border_y == wo.Y_REPLICATE:
            yy = np.clip(yy, 0, sH - 1)
        else:
            inside &= (yy >= 0) & (yy < sH)
        return inside & u[np.clip(yy, 0, sH - 1), np.clip(xx, 0, sW - 1)]

    return _u8(vx & vy & tap(ix, iy) & tap(ix + 1, iy) & tap(ix, iy + 1) & tap(ix + 1, iy + 1))


def build_warped(src_mask, map_x, map_y, sW, sH, border_x, border_y, dW=None, dH=None, r=0, mask_border_x=X_CLAMP):
    """erp_mask_build_warped: the warp's usable pixels, reduced to (dW, dH), then eroded"""
    m = warp_usable(src_mask, map_x, map_y, sW, sH, border_x, border_y)
    wH, wW = m.shape
    return erode(reduce(m, wW if dW is None else dW, wH if dH is None else dH), r, mask_border_x)


def region_mask(W, H, margin, polar):
    m = np.zeros((H, W), np.uint8)
    m[int(np.float32(H) * np.float32(polar)):int(np.float32(H) * (np.float32(1.0) - np.float32(polar))),
      margin:W - margin] = 255
    return m


def usable_at(usable, x, y):
    """the filter's mask term for float32 positions: the pixel (rint(x), rint(y)), half to even; outside: False"""
    u = np.asarray(usable) != 0
    H, W = u.shape
    xi = np.rint(np.asarray(x, np.float32)).astype(np.int64)
    yi = np.rint(np.asarray(y, np.float32)).astype(np.int64)
    inside = (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)
    return inside & u[np.clip(yi, 0, H - 1), np.clip(xi, 0, W - 1)]


def pipeline_oracle_masked(vio, prev, curr, pts, prm, klt, usable):
    """test_tracker_gpu.pipeline_oracle with a usable-region mask (0 / 255 at the frame's size) -> (next, status,
    kept, corners, number of points that only the mask term dropped)"""
    H, W = prev.shape
    nxt, st, _ = oracle_lib.klt_track(prev, curr, pts, klt)
    vr = nxt[:, 1] / np.float32(H)
    polar = (vr < np.float32(prm.polar_ratio)) | (vr > np.float32(1.0) - np.float32(prm.polar_ratio))
    m = np.float32(prm.boundary_margin)
    nearb = (nxt[:, 0] < m) | (nxt[:, 0] > np.float32(W) - m) | (nxt[:, 1] < m) | (nxt[:, 1] > np.float32(H) - m)
    base = (st == 1) & ~polar & ~nearb
    ok = usable_at(usable, nxt[:, 0], nxt[:, 1])
    good = np.nonzero(base & ok)[0]
    kept = np.zeros(len(pts), np.uint8)
    if len(good) >= 3:
        s = vio.ransac_samples(prm.ransac_seed, len(good), prm.ransac_iters)
        mk, _ = oracle_lib.rot_ransac(pts[good], nxt[good], W, H, s, prm.ransac_thresh_rad)
        kept[good] = mk
    else:
        kept[good] = 1
    mask = region_mask(W, H, prm.boundary_margin, prm.polar_ratio) & np.asarray(usable, np.uint8)
    r = int(prm.min_dist)
    for i in np.nonzero(kept)[0]:
        fo.cv_circle_fill(mask, int(np.rint(nxt[i, 0])), int(np.rint(nxt[i, 1])), r)
    corners = oracle_lib.gftt(curr, mask, prm.max_corners, prm.quality, prm.min_dist)
    return nxt, st, kept, corners, int((base & ~ok).sum())


class MaskedFrontendOracle(fo.FrontendOracle):
    """FrontendOracle with a usable-region mask (0 / 255 at the front end's size): polar AND boundary AND usable
    in _base_mask, the extra term in the tracked-point filter.  mask_dropped counts the points of the last frame
    that only the mask term dropped."""

    def __init__(self, vio, W, H, params, usable):
        super().__init__(vio, W, H, params)
        self.usable = np.asarray(usable, np.uint8)
        assert self.usable.shape == (H, W)
        self.mask_dropped = 0

    def _base_mask(self):
        return super()._base_mask() & self.usable

    def track(self, img):
        p, W, H = self.p, self.W, self.H
        self.mask_dropped = 0
        if self.frame == 0 or not self.feats:
            return super().track(img)  # detection only: the mask enters through _base_mask
        prev = np.array([[f["x"], f["y"]] for f in self.feats], np.float32)
        nxt, st, _ = oracle_lib.klt_track(self.prev, img, prev, self.vio.default_klt_params())
        m = np.float32(p.boundary_margin)
        ok = usable_at(self.usable, nxt[:, 0], nxt[:, 1])
        good = []
        for i in range(len(prev)):
            x, y = nxt[i]
            vr = np.float32(y / np.float32(H))
            polar = vr < np.float32(0.15) or vr > np.float32(1.0) - np.float32(0.15)
            nearb = x < m or x > np.float32(W) - m or y < m or y > np.float32(H) - m
            if st[i] and not polar and not nearb:
                if ok[i]:
                    good.append(i)
                else:
                    self.mask_dropped += 1
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
