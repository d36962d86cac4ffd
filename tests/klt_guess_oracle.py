"""klt_guess_oracle.py — TEST INFRASTRUCTURE ONLY (parity checker, never shipped).

The reference of the guided LK search (erp_klt_track_guess / erp_klt_track_rot, include/vio360.h "Guided LK").  The C
oracle (oracle_klt_track) cannot take a guess, so this is a NumPy restatement of its lk_point / oracle_klt_track
(oracle/tracker_oracle.c:139-277), operation by operation in f32 and integer arithmetic: np.float32 arrays (NumPy
rounds every f32 operation on its own, nothing is fused), np.rint for rintf, int64 window sums.  All points run
together, one array row per point; the pyramids come from oracle_lib.pyr_down.  With guess=None, and with
guess == pts, it must equal oracle_lib.klt_track bit for bit (tests/test_klt_guess.py): that pins everything here
except the one line a guess changes, the start position at the top level.

  klt_track(prev, curr, pts, klt, guess=None, seam=CUT)
      seam=WRAP is built like seam_oracle.klt_track with left = 0: the pyramids are those of the frame extended to the
      right by half its width (so no wrapped pyrDown is assumed), the coordinates are the frame's own, and column X of
      level l is read at X mod (W >> l), taken in [Wl / 4, Wl / 4 + Wl) of the extended level -- away from both of its
      ends, whose few columns the REFLECT_101 border of the extension reaches.
  start_positions(pts, guess, W, H, seam)    the fold and the bad-guess rule
  predict(pts, R, W, H)                      the rotation predictor in f64
  klt_step(fn)                               runs the pinned pipeline / front-end oracles with fn as their KLT step
"""
import contextlib

import numpy as np

import frontend_oracle as fo
import oracle_lib
import seam_oracle as so

CUT, WRAP = 0, 1
W_BITS = 14
F32 = np.float32
FLT_SCALE = F32(1.0) / F32(1 << 20)
FLT_EPSILON = F32(np.finfo(np.float32).eps)


def reflect101(p, n):
    """tracker_oracle.c reflect101 on an integer array"""
    p = np.asarray(p, np.int64)
    if n == 1:
        return np.zeros_like(p)
    period = 2 * n - 2
    p = np.mod(p, period)
    return np.where(p >= n, period - p, p)


def start_positions(pts, guess, W, H, seam=CUT):
    """the position every point's search starts from at the top level, in level-0 pixels (f32): its guess; its
    previous position when the guess is not finite or lies outside [-W, 2W) x [-H, 2H); under WRAP the guess's x
    folded into [0, W) by one f32 +-W (a fold that rounds to W gives 0)"""
    pts = np.asarray(pts, F32).reshape(-1, 2)
    if guess is None:
        return pts.copy()
    g = np.asarray(guess, F32).reshape(-1, 2).copy()
    assert g.shape == pts.shape
    Wf, Hf = F32(W), F32(H)
    with np.errstate(invalid="ignore"):
        ok = (g[:, 0] >= -Wf) & (g[:, 0] < F32(2) * Wf) & (g[:, 1] >= -Hf) & (g[:, 1] < F32(2) * Hf)
    if seam == WRAP:
        g[ok, 0] = so.fold_x(g[ok, 0], W)
    g[~ok] = pts[~ok]
    return g


def bearings(pts, W, H):
    """Camera::PixelToBearing (Camera.cpp:22-47) in f64"""
    p = np.asarray(pts, np.float64).reshape(-1, 2)
    lon = (p[:, 0] / W - 0.5) * 2.0 * np.pi
    lat = -(p[:, 1] / H - 0.5) * np.pi
    return np.stack([np.cos(lat) * np.sin(lon), -np.sin(lat), np.cos(lat) * np.cos(lon)], -1)


def predict(pts, R_cur_prev, W, H):
    """-> (guesses (n, 2) f64 = BearingToPixel(R PixelToBearing(pts)), the rotated bearings (n, 3) f64)
    (Camera.cpp:49-67: theta = atan2(x, z), phi = -asin(y / |b|), u = W (0.5 + theta / 2pi), v = H (0.5 - phi / pi))"""
    d = bearings(pts, W, H) @ np.asarray(R_cur_prev, np.float64).reshape(3, 3).T
    theta = np.arctan2(d[:, 0], d[:, 2])
    phi = -np.arcsin(np.clip(d[:, 1] / np.linalg.norm(d, axis=1), -1.0, 1.0))
    return np.stack([W * (0.5 + theta / (2.0 * np.pi)), H * (0.5 - phi / np.pi)], -1), d


def angle_to(px, d, W, H):
    """the angle (rad, f64) between the bearing of every pixel of px and the unit vector of the same row of d"""
    b = bearings(px, W, H)
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    return np.arctan2(np.linalg.norm(np.cross(b, d), axis=1), (b * d).sum(1))


# ---------------------------------------------------------------------------------------------
# pyramids

def lk_top_level(W, H, win, max_level):
    """build_pyramid's `levels`: buildOpticalFlowPyramid stops when the next level would be <= winSize"""
    w, h, top = W, H, 0
    for l in range(max_level + 1):
        top = l
        nw, nh = (w + 1) // 2, (h + 1) // 2
        if nw <= win or nh <= win:
            break
        w, h = nw, nh
    return top


def pyramid(img, top):
    lv = [np.ascontiguousarray(img, np.uint8)]
    for _ in range(top):
        lv.append(oracle_lib.pyr_down(lv[-1]))
    return lv


def scharr(img):
    """calcSharrDeriv: (dx, dy) int16, REFLECT_101 inside the image"""
    p = np.pad(img.astype(np.int32), 1, mode="reflect")
    r0, r1, r2 = p[:-2], p[1:-1], p[2:]
    t0 = (r0 + r2) * 3 + r1 * 10
    t1 = r2 - r0
    dx = t0[:, 2:] - t0[:, :-2]
    dy = (t1[:, 2:] + t1[:, :-2]) * 3 + t1[:, 1:-1] * 10
    return dx.astype(np.int16), dy.astype(np.int16)


class _Level:
    """one pyramid level of one frame: img_at / der_at of tracker_oracle.c on index arrays.  w, h are the tracked
    frame's level sizes; under WRAP the arrays are the extended frame's level and columns are periodic in w."""

    def __init__(self, img, w, h, wrap, deriv):
        self.img, self.w, self.h, self.wrap = img, w, h, wrap
        self.dx, self.dy = scharr(img) if deriv else (None, None)

    def cols(self, X):
        if not self.wrap:
            return reflect101(X, self.w)
        c = np.mod(np.asarray(X, np.int64), self.w)
        return np.where(c < self.w // 4, c + self.w, c)

    def img_at(self, X, Y):
        return self.img[reflect101(Y, self.h), self.cols(X)].astype(np.int32)

    def der_at(self, X, Y):
        inside = (Y >= 0) & (Y < self.h)
        if not self.wrap:
            inside = inside & (X >= 0) & (X < self.w)
        yy, xx = reflect101(Y, self.h), self.cols(X)
        gx = np.where(inside, self.dx[yy, xx].astype(np.int32), 0)
        gy = np.where(inside, self.dy[yy, xx].astype(np.int32), 0)
        return gx, gy


def _levels(frame, W, H, top, wrap, deriv):
    if wrap:
        assert W % (1 << top) == 0, "erp_seam_check: W must be divisible by 2^top"
        frame = so.extend(frame, 0, W // 2)
    out, w, h = [], W, H
    for img in pyramid(frame, top):
        assert img.shape[0] == h and (img.shape[1] == w or wrap)
        out.append(_Level(img, w, h, wrap, deriv))
        w, h = (w + 1) // 2, (h + 1) // 2
    return out


# ---------------------------------------------------------------------------------------------
# LKTrackerInvoker, all points at once

def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _weights(a, b):
    """(iw00, iw01, iw10, iw11) int32 arrays from the f32 fractions a, b"""
    one, s = F32(1), F32(1 << W_BITS)
    iw00 = np.rint((one - a) * (one - b) * s).astype(np.int32)
    iw01 = np.rint(a * (one - b) * s).astype(np.int32)
    iw10 = np.rint((one - a) * b * s).astype(np.int32)
    return iw00, iw01, iw10, (1 << W_BITS) - iw00 - iw01 - iw10


def _bilinear(L, ix, iy, wts, win, shift):
    """DESCALE of the four-tap interpolation of L's pixels over every point's win x win window at (ix, iy)"""
    g = np.arange(win, dtype=np.int64)
    X = ix[:, None, None] + g[None, None, :]
    Y = iy[:, None, None] + g[None, :, None]
    w00, w01, w10, w11 = (w[:, None, None] for w in wts)
    return _descale(L.img_at(X, Y) * w00 + L.img_at(X + 1, Y) * w01 + L.img_at(X, Y + 1) * w10 +
                    L.img_at(X + 1, Y + 1) * w11, shift)


def _outside(ix, iy, L, win):
    out = (iy < -win) | (iy >= L.h)
    if not L.wrap:
        out = out | (ix < -win) | (ix >= L.w)
    return out


def _lk_level(I, J, level, top, pts, start, nxt, status, err, win, max_iters, eps2, min_eig_thr):
    """lk_point for every point at `level` (updates nxt, status, err in place)"""
    n = len(pts)
    hw = F32((win - 1) * 0.5)
    sc = F32(1.0 / (1 << level))
    px, py = pts[:, 0] * sc, pts[:, 1] * sc
    if level == top:
        nx, ny = start[:, 0] * sc, start[:, 1] * sc  # the one line a guess changes (unguided: start == pts)
    else:
        nx, ny = nxt[:, 0] * F32(2), nxt[:, 1] * F32(2)
    nxt[:, 0], nxt[:, 1] = nx, ny
    px, py = px - hw, py - hw
    ipx, ipy = np.floor(px).astype(np.int64), np.floor(py).astype(np.int64)
    out = _outside(ipx, ipy, I, win)
    if level == 0:
        status[out] = 0
        err[out] = 0
    idx = np.nonzero(~out)[0]
    if not len(idx):
        return
    ipx, ipy = ipx[idx], ipy[idx]
    wts = _weights(px[idx] - ipx.astype(F32), py[idx] - ipy.astype(F32))
    Iw = _bilinear(I, ipx, ipy, wts, win, W_BITS - 5).astype(np.int16).astype(np.int64)
    g = np.arange(win, dtype=np.int64)
    X = ipx[:, None, None] + g[None, None, :]
    Y = ipy[:, None, None] + g[None, :, None]
    w00, w01, w10, w11 = (w[:, None, None] for w in wts)
    g00, g01, g10, g11 = I.der_at(X, Y), I.der_at(X + 1, Y), I.der_at(X, Y + 1), I.der_at(X + 1, Y + 1)
    dIx = _descale(g00[0] * w00 + g01[0] * w01 + g10[0] * w10 + g11[0] * w11, W_BITS).astype(np.int16).astype(np.int64)
    dIy = _descale(g00[1] * w00 + g01[1] * w01 + g10[1] * w10 + g11[1] * w11, W_BITS).astype(np.int16).astype(np.int64)
    A11 = (dIx * dIx).sum((1, 2)).astype(F32) * FLT_SCALE
    A12 = (dIx * dIy).sum((1, 2)).astype(F32) * FLT_SCALE
    A22 = (dIy * dIy).sum((1, 2)).astype(F32) * FLT_SCALE
    D = A11 * A22 - A12 * A12
    min_eig = (A22 + A11 - np.sqrt((A11 - A22) * (A11 - A22) + F32(4) * A12 * A12)) / F32(2 * win * win)
    bad = (min_eig < F32(min_eig_thr)) | (D < FLT_EPSILON)
    if level == 0:
        status[idx[bad]] = 0
    keep = ~bad
    idx, Iw, dIx, dIy = idx[keep], Iw[keep], dIx[keep], dIy[keep]
    A11, A12, A22 = A11[keep], A12[keep], A22[keep]
    with np.errstate(divide="ignore"):
        D = F32(1) / D[keep]
    m = len(idx)
    cx, cy = nx[idx] - hw, ny[idx] - hw  # the iteration's position (window corner), f32
    pdx, pdy = np.zeros(m, F32), np.zeros(m, F32)
    live = np.ones(m, bool)
    for j in range(max_iters):
        k = np.nonzero(live)[0]
        if not len(k):
            break
        inx, iny = np.floor(cx[k]).astype(np.int64), np.floor(cy[k]).astype(np.int64)
        gone = _outside(inx, iny, J, win)
        if level == 0:
            status[idx[k[gone]]] = 0
        live[k[gone]] = False
        k, inx, iny = k[~gone], inx[~gone], iny[~gone]
        if not len(k):
            break
        wj = _weights(cx[k] - inx.astype(F32), cy[k] - iny.astype(F32))
        diff = _bilinear(J, inx, iny, wj, win, W_BITS - 5).astype(np.int64) - Iw[k]
        b1 = (diff * dIx[k]).sum((1, 2)).astype(F32) * FLT_SCALE
        b2 = (diff * dIy[k]).sum((1, 2)).astype(F32) * FLT_SCALE
        ddx = (A12[k] * b2 - A22[k] * b1) * D[k]
        ddy = (A12[k] * b1 - A11[k] * b2) * D[k]
        cx[k] = cx[k] + ddx
        cy[k] = cy[k] + ddy
        ox, oy = cx[k] + hw, cy[k] + hw
        small = ddx.astype(np.float64) * ddx.astype(np.float64) + ddy.astype(np.float64) * ddy.astype(np.float64) <= eps2
        osc = np.zeros(len(k), bool)
        if j > 0:
            osc = (~small & (np.abs((ddx + pdx[k]).astype(np.float64)) < 0.01) &
                   (np.abs((ddy + pdy[k]).astype(np.float64)) < 0.01))
            ox = np.where(osc, ox - ddx * F32(0.5), ox)
            oy = np.where(osc, oy - ddy * F32(0.5), oy)
        nxt[idx[k], 0], nxt[idx[k], 1] = ox, oy
        live[k[small | osc]] = False
        pdx[k], pdy[k] = ddx, ddy
    if level == 0:
        k = np.nonzero(status[idx] == 1)[0]
        if len(k):
            fx, fy = nxt[idx[k], 0] - hw, nxt[idx[k], 1] - hw
            ix, iy = np.floor(fx).astype(np.int64), np.floor(fy).astype(np.int64)
            gone = _outside(ix, iy, J, win)
            status[idx[k[gone]]] = 0
            k, fx, fy, ix, iy = k[~gone], fx[~gone], fy[~gone], ix[~gone], iy[~gone]
            if len(k):
                wf = _weights(fx - ix.astype(F32), fy - iy.astype(F32))
                diff = _bilinear(J, ix, iy, wf, win, W_BITS - 5).astype(np.int64) - Iw[k]
                err[idx[k]] = np.abs(diff).sum((1, 2)).astype(F32) * (F32(1) / F32(32 * win * win))


def klt_track(prev, curr, pts, klt, guess=None, seam=CUT):
    """oracle_klt_track with OPTFLOW_USE_INITIAL_FLOW -> (next, status, err, the start positions used).
    seam=WRAP: on the periodic continuation, next.x folded into [0, W) as lk_kernel folds it."""
    prev, curr = np.asarray(prev, np.uint8), np.asarray(curr, np.uint8)
    H, W = prev.shape
    pts = np.ascontiguousarray(pts, F32).reshape(-1, 2)
    n = len(pts)
    win = klt.win
    max_iters = min(max(klt.max_iters, 0), 100)
    eps = min(max(float(F32(klt.epsilon)), 0.0), 10.0)
    top = lk_top_level(W, H, win, klt.max_level)
    wrap = seam == WRAP
    I = _levels(prev, W, H, top, wrap, True)
    J = _levels(curr, W, H, top, wrap, False)
    start = start_positions(pts, guess, W, H, seam)
    nxt, status, err = np.zeros((n, 2), F32), np.ones(n, np.uint8), np.zeros(n, F32)
    for level in range(top, -1, -1):
        _lk_level(I[level], J[level], level, top, pts, start, nxt, status, err, win, max_iters, eps * eps,
                  klt.min_eig_threshold)
    if wrap:
        nxt[:, 0] = so.fold_x(nxt[:, 0], W)
        with np.errstate(invalid="ignore"):
            lost = ~((nxt[:, 0] >= 0) & (nxt[:, 0] < F32(W)))  # more than a turn away, or not a number
        nxt[lost, 0], status[lost], err[lost] = 0, 0, 0
    return nxt, status, err, start


# ---------------------------------------------------------------------------------------------
# the pinned pipeline / front-end oracles with another KLT step

@contextlib.contextmanager
def klt_step(fn):
    """Inside the block, the KLT step of test_tracker_gpu.pipeline_oracle, seam_oracle.pipeline_oracle,
    frontend_oracle.FrontendOracle (all three call oracle_lib.klt_track(prev, curr, pts, klt)) and of
    seam_oracle.SeamFrontendOracle (seam_oracle.klt_track(prev, curr, pts, klt, left, right)) is
    fn(prev, curr, pts, klt, seam) -> (next, status, err); everything else of those oracles runs as it is."""
    flat, wrapped = oracle_lib.klt_track, so.klt_track
    oracle_lib.klt_track = lambda prev, curr, pts, klt: fn(prev, curr, pts, klt, CUT)
    so.klt_track = lambda prev, curr, pts, klt, left=0, right=so.APRON: fn(prev, curr, pts, klt, WRAP)
    try:
        yield
    finally:
        oracle_lib.klt_track, so.klt_track = flat, wrapped


def guided_frontend(vio, W, H, params, seam, guess_fn):
    """A FrontendOracle / SeamFrontendOracle whose track(img) runs the guided restatement as its KLT step, started
    from guess_fn(prev_img, img, pts) (a return of None: unguided).  Everything but that step is the base oracle."""
    base = so.SeamFrontendOracle if seam == WRAP else fo.FrontendOracle

    class Guided(base):
        def track(self, img):
            def step(prev, curr, pts, klt, _seam):
                g = guess_fn(prev, curr, pts)
                return klt_track(prev, curr, pts, klt, g, seam)[:3]
            with klt_step(step):
                return super().track(img)

    return Guided(vio, W, H, params)
