"""warp_oracle.py — TEST INFRASTRUCTURE ONLY (parity checker, never shipped).

numpy restatement of the lens-to-ERP warp (erp_warp_*, include/vio360.h): cv::remap(..., INTER_LINEAR) in exact
integer arithmetic on the grey image that tests/ingest_oracle.py's luma makes of a packed frame, and the three map
generators in float64.

  quantisation   q = rint(float64(s) * 32) (half to even), i = q >> 5 (floor), a = q & 31; X_WRAP reduces q to
                 [0, 32 S), the other modes clamp it to [-32, 32 S]; a non-finite coordinate makes the pixel invalid
  borders        X_WRAP: tap columns modulo sW; Y_REPLICATE: tap rows clamped to [0, sH); CONSTANT: a tap outside the
                 source reads border_value; an invalid pixel is border_value whatever the modes
  pixel          ((32-a)(32-b) p00 + a(32-b) p01 + (32-a)b p10 + ab p11 + 512) >> 10
OpenCV is not available to the tests: parity with it is unpinned; pinned here by closed forms (tests/test_warp.py).
"""
import numpy as np

import ingest_oracle as io

X_CONSTANT, X_WRAP = 0, 1
Y_CONSTANT, Y_REPLICATE = 0, 2


def quantize(s, S, border_mode):
    """float32 coordinates of one axis of size S -> (q int64, valid bool), q = 0 where invalid"""
    s = np.asarray(s, np.float32)
    valid = np.isfinite(s)
    d = np.rint(np.where(valid, s, np.float32(0)).astype(np.float64) * 32.0)
    M = 32.0 * S
    if border_mode == X_WRAP:
        d = np.fmod(d, M)  # exact
        d = np.where(d < 0, d + M, d)
    else:
        assert border_mode in (X_CONSTANT, Y_REPLICATE)
        d = np.clip(d, -32.0, M)
    return np.where(valid, d, 0.0).astype(np.int64), valid


def remap_grey(grey, map_x, map_y, border_x, border_y, border_value=0):
    """grey (sH, sW) u8, maps (dH, dW) float32 -> (dH, dW) u8"""
    g = np.asarray(grey, np.uint8).astype(np.int64)
    sH, sW = g.shape
    qx, vx = quantize(map_x, sW, border_x)
    qy, vy = quantize(map_y, sH, border_y)
    ix, a = qx >> 5, qx & 31
    iy, b = qy >> 5, qy & 31

    def tap(xx, yy):
        inside = np.ones(xx.shape, bool)
        if border_x == X_WRAP:
            xx = xx % sW
        else:
            inside &= (xx >= 0) & (xx < sW)
        if border_y == Y_REPLICATE:
            yy = np.clip(yy, 0, sH - 1)
        else:
            inside &= (yy >= 0) & (yy < sH)
        return np.where(inside, g[np.clip(yy, 0, sH - 1), np.clip(xx, 0, sW - 1)], border_value)

    v = ((32 - a) * (32 - b) * tap(ix, iy) + a * (32 - b) * tap(ix + 1, iy) + (32 - a) * b * tap(ix, iy + 1) +
         a * b * tap(ix + 1, iy + 1) + 512) >> 10
    return np.where(vx & vy, v, border_value).astype(np.uint8)


def remap(img, fmt, rule, map_x, map_y, border_x, border_y, border_value=0):
    """a packed frame of format fmt (tests/ingest_oracle.py) -> the warp of its luma"""
    return remap_grey(io.luma(img, fmt, rule), map_x, map_y, border_x, border_y, border_value)


# ---- map generators, float64 ----

def rot_x(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[1, 0, 0], [0, c, -s], [0, s, c]], np.float64)


def rot_y(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], np.float64)


def dst_bearings(dW, dH, R_dst=None):
    """(dH, dW, 3): Camera::PixelToBearing at (u, v) = (x, y), rotated by R_dst"""
    x, y = np.meshgrid(np.arange(dW, dtype=np.float64), np.arange(dH, dtype=np.float64))
    lon = (x / dW - 0.5) * 2.0 * np.pi
    lat = -(y / dH - 0.5) * np.pi
    b = np.stack([np.cos(lat) * np.sin(lon), -np.sin(lat), np.cos(lat) * np.cos(lon)], axis=-1)
    return b if R_dst is None else b @ np.asarray(R_dst, np.float64).reshape(3, 3).T


def map_erp(sW, sH, dW, dH, R_dst=None):
    """Camera::BearingToPixel into the sW x sH source -> float64 (sx, sy)"""
    b = dst_bearings(dW, dH, R_dst)
    theta = np.arctan2(b[..., 0], b[..., 2])
    phi = -np.arcsin(np.clip(b[..., 1] / np.linalg.norm(b, axis=-1), -1.0, 1.0))
    return sW * (0.5 + theta / (2.0 * np.pi)), sH * (0.5 - phi / np.pi)


def fisheye_angles(lenses, dW, dH, R_dst=None):
    """(n, dH, dW) theta of every pixel in every lens, and the lens-frame bearings (n, dH, dW, 3)"""
    b = dst_bearings(dW, dH, R_dst)
    bl = np.stack([b @ np.asarray(l["R"], np.float64).reshape(3, 3).T for l in lenses])
    return np.arctan2(np.hypot(bl[..., 0], bl[..., 1]), bl[..., 2]), bl


def map_fisheye(lenses, dW, dH, R_dst=None):
    """equidistant lenses -> float64 (sx, sy), NaN where no lens sees the pixel"""
    theta, bl = fisheye_angles(lenses, dW, dH, R_dst)
    tmax = np.array([l["theta_max"] for l in lenses], np.float64)[:, None, None]
    cost = np.where(theta <= tmax, theta, np.inf)
    k = np.argmin(cost, axis=0)  # the first of equal minima: the lowest index
    seen = np.isfinite(np.min(cost, axis=0))
    yy, xx = np.indices(k.shape)
    th, v = theta[k, yy, xx], bl[k, yy, xx]
    h = np.hypot(v[..., 0], v[..., 1])
    hs = np.where(h == 0, 1.0, h)
    cx, cy, f = (np.array([l[n] for l in lenses], np.float64)[k] for n in ("cx", "cy", "f"))
    sx = np.where(h == 0, cx, cx + f * th * v[..., 0] / hs)
    sy = np.where(h == 0, cy, cy + f * th * v[..., 1] / hs)
    return np.where(seen, sx, np.nan), np.where(seen, sy, np.nan)


def cube_depths(faces, dW, dH, R_dst=None):
    """(n, dH, dW) z of every pixel in every face frame, and the face-frame bearings"""
    b = dst_bearings(dW, dH, R_dst)
    bf = np.stack([b @ np.asarray(f["R"], np.float64).reshape(3, 3).T for f in faces])
    return bf[..., 2], bf


def map_cubemap(faces, eac, dW, dH, R_dst=None):
    """cubemap / EAC faces -> float64 (sx, sy), NaN where no face has positive depth"""
    z, bf = cube_depths(faces, dW, dH, R_dst)
    k = np.argmax(z, axis=0)  # the first of equal maxima: the lowest index
    yy, xx = np.indices(k.shape)
    v = bf[k, yy, xx]
    seen = v[..., 2] > 0
    zs = np.where(seen, v[..., 2], 1.0)
    u, w = v[..., 0] / zs, v[..., 1] / zs
    if eac:
        u, w = (4.0 / np.pi) * np.arctan(u), (4.0 / np.pi) * np.arctan(w)
    x0, y0, fw, fh = (np.array([f[n] for f in faces], np.float64)[k] for n in ("x0", "y0", "w", "h"))
    sx = np.clip(x0 + (u + 1.0) * fw / 2.0 - 0.5, x0, x0 + fw - 1)
    sy = np.clip(y0 + (w + 1.0) * fh / 2.0 - 0.5, y0, y0 + fh - 1)
    return np.where(seen, sx, np.nan), np.where(seen, sy, np.nan)


# ---- the coordinates and geometries of the tests ----

def special_coordinates(S):
    """float32 coordinates of an axis of size S that the quantisation must get right: integers, ties, both borders,
    values far outside, non-finite ones"""
    return np.array([0, 1, S - 1, S, 5 + 1 / 64, 5 + 3 / 64, -1, -0.5, S - 1, S - 0.5, S, 1e9, -1e9, np.inf, -np.inf,
                     np.nan, -1 - 1 / 64, S + 1 / 64, 3e38, -3e38, -0.0], np.float32)


def dual_fisheye(theta_max_deg, circle=32):
    """two back-to-back lenses, `circle`-pixel image circles side by side in a (2 circle) x circle source, the
    circle's rim at 95 degrees whatever theta_max"""
    f = (circle / 2.0) / np.deg2rad(95.0)
    t = np.deg2rad(theta_max_deg)
    c = (circle - 1) / 2.0
    return [{"R": np.eye(3), "cx": c, "cy": c, "f": f, "theta_max": t},
            {"R": rot_y(np.pi), "cx": circle + c, "cy": c, "f": f, "theta_max": t}]


def cube_faces_3x2(n=16):
    """six axis faces of n pixels in a 3 x 2 layout: +Z +X -Z over -X +Y -Y (R: rig -> face, the face along +Z)"""
    Rs = [np.eye(3), rot_y(-np.pi / 2), rot_y(np.pi), rot_y(np.pi / 2), rot_x(np.pi / 2), rot_x(-np.pi / 2)]
    return [{"R": R, "x0": (k % 3) * n, "y0": (k // 3) * n, "w": n, "h": n} for k, R in enumerate(Rs)]
