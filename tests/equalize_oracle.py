"""equalize_oracle.py — TEST INFRASTRUCTURE ONLY (parity checker, never shipped).

numpy restatement of the contrast equalisation (erp_equalize*, include/vio360.h): cv::equalizeHist and
cv::CLAHE::apply (8-bit).  All float arithmetic is float32 arrays / scalars, so every operation is rounded on its own
and nothing is fused; division is numpy's correctly rounded one; round() is np.rint (half to even), then a clamp to
[0, 255].

  HIST    hist over the frame, i0 the first non-empty bin; hist[i0] == W H: every pixel is i0; else scale = 255 /
          (W H - hist[i0]), lut[i <= i0] = 0, lut[i > i0] = round(sum_{i0 < j <= i} hist[j] * scale); dst = lut[src]
  CLAHE   tiles over the frame, or over the frame extended right / bottom with BORDER_REFLECT_101 when a size is not
          divisible (then both axes grow, a divisible one by a whole tiles count); per tile: histogram, clip at c =
          max(int(clip * area / 256), 1) with the excess spread (batch to every bin, the residual to bins 0, step,
          2 step, ...), lut = round(cumsum * (255 / area)); per pixel: bilinear interpolation of the four nearest
          tiles' LUTs at the pixel's value, tile indices clamped at the borders (X_WRAP: wrapped horizontally)
OpenCV is not available to the tests: parity with it is unpinned; pinned here by closed forms (tests/test_equalize.py).
"""
import numpy as np

NONE, HIST, CLAHE = 0, 1, 2
X_CLAMP, X_WRAP = 0, 1
F = np.float32


def saturate(f):
    """float32 array -> u8: round half to even, clamp"""
    return np.clip(np.rint(np.asarray(f, F)), 0, 255).astype(np.uint8)


def histogram(a):
    return np.bincount(np.asarray(a, np.uint8).reshape(-1), minlength=256).astype(np.int64)


def hist_lut(hist, total):
    """the frame rule: 256 counts of a frame of `total` pixels -> u8[256]"""
    h = np.asarray(hist, np.int64)
    i0 = int(np.flatnonzero(h)[0])
    if h[i0] == total:
        return np.full(256, i0, np.uint8)
    scale = F(255) / F(total - h[i0])
    s = np.cumsum(h) - h[i0]
    lut = saturate(s.astype(F) * scale)
    lut[:i0 + 1] = 0
    return lut


def clahe_clip(hist, area, clip_limit):
    """the clip and redistribution of one tile -> (clipped counts, {c, excess, batch, resid})"""
    h = np.asarray(hist, np.int64).copy()
    info = {"c": 0, "excess": 0, "batch": 0, "resid": 0}
    if clip_limit > 0:
        c = max(int(clip_limit * area / 256), 1)
        excess = int(np.maximum(h - c, 0).sum())
        h = np.minimum(h, c)
        batch = excess // 256
        resid = excess - 256 * batch
        info = {"c": c, "excess": excess, "batch": batch, "resid": resid}
        h += batch
        if resid > 0:
            step = max(256 // resid, 1)
            i = 0
            while i < 256 and resid > 0:
                h[i] += 1
                i += step
                resid -= 1
    return h, info


def clahe_lut(hist, area, clip_limit):
    """the tile rule: 256 counts of a tile of `area` pixels -> u8[256]"""
    h, _ = clahe_clip(hist, area, clip_limit)
    return saturate(np.cumsum(h).astype(F) * (F(255) / F(area)))


def extended(img, tiles_x, tiles_y):
    """the tiled image: img itself, or its BORDER_REFLECT_101 extension to the right and the bottom"""
    a = np.asarray(img, np.uint8)
    H, W = a.shape
    if W % tiles_x == 0 and H % tiles_y == 0:
        return a
    ex, ey = tiles_x - W % tiles_x, tiles_y - H % tiles_y

    def idx(n, e):
        i = np.arange(n + e)
        return np.where(i < n, i, 2 * n - 2 - i)

    return a[idx(H, ey)][:, idx(W, ex)]


def tile_luts(img, tiles_x, tiles_y, clip_limit):
    """(tiles_y, tiles_x, 256) u8 LUTs, and the tile size (tw, th)"""
    e = extended(img, tiles_x, tiles_y)
    th, tw = e.shape[0] // tiles_y, e.shape[1] // tiles_x
    L = np.zeros((tiles_y, tiles_x, 256), np.uint8)
    for ty in range(tiles_y):
        for tx in range(tiles_x):
            L[ty, tx] = clahe_lut(histogram(e[ty * th:(ty + 1) * th, tx * tw:(tx + 1) * tw]), tw * th, clip_limit)
    return L, tw, th


def _axis(n, t, tiles, wrap):
    """per pixel index of one axis: (t1, t2, a, a1)"""
    f = np.arange(n).astype(F) * (F(1) / F(t)) - F(0.5)
    fl = np.floor(f)
    a = f - fl
    a1 = F(1) - a
    t1 = fl.astype(np.int64)
    t2 = t1 + 1
    if wrap:
        t1, t2 = np.where(t1 < 0, tiles - 1, t1), np.where(t2 >= tiles, 0, t2)
    else:
        t1, t2 = np.maximum(t1, 0), np.minimum(t2, tiles - 1)
    assert a.dtype == F and a1.dtype == F
    return t1, t2, a, a1


def clahe(img, tiles_x=8, tiles_y=8, clip_limit=3.0, border_x=X_CLAMP):
    a = np.asarray(img, np.uint8)
    H, W = a.shape
    assert 1 <= tiles_x <= W // 2 and 1 <= tiles_y <= H // 2
    assert border_x == X_CLAMP or (W % tiles_x == 0 and H % tiles_y == 0)
    L, tw, th = tile_luts(a, tiles_x, tiles_y, clip_limit)
    Lf = L.astype(F)
    tx1, tx2, xa, xa1 = _axis(W, tw, tiles_x, border_x == X_WRAP)
    ty1, ty2, ya, ya1 = _axis(H, th, tiles_y, False)
    v = a.astype(np.int64)
    ty1, ty2, ya, ya1 = ty1[:, None], ty2[:, None], ya[:, None], ya1[:, None]
    tx1, tx2, xa, xa1 = tx1[None, :], tx2[None, :], xa[None, :], xa1[None, :]
    top = Lf[ty1, tx1, v] * xa1 + Lf[ty1, tx2, v] * xa
    bot = Lf[ty2, tx1, v] * xa1 + Lf[ty2, tx2, v] * xa
    res = top * ya1 + bot * ya
    assert res.dtype == F
    return saturate(res)


def equalize_hist(img):
    a = np.asarray(img, np.uint8)
    return hist_lut(histogram(a), a.size)[a]


def equalize(img, mode, tiles_x=8, tiles_y=8, clip_limit=3.0, border_x=X_CLAMP):
    if mode == NONE:
        return np.asarray(img, np.uint8).copy()
    if mode == HIST:
        return equalize_hist(img)
    assert mode == CLAHE
    return clahe(img, tiles_x, tiles_y, clip_limit, border_x)
