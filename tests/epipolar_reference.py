"""TEST INFRASTRUCTURE: an f64 evaluation of the known-rotation epipolar test written from the geometry (angles by
arcsin / arccos on unit vectors), independent of the f32 operation order of tests/epipolar_oracle.py, and a synthetic
two-view scene generator.  Used by tests/test_epipolar.py.

Geometry.  a = R b0 is the previous bearing in the current frame.  Without translation b1 = a.  With the camera
moving along the unit vector d (current frame), b1 lies in the plane through d and a, displaced from a *away* from
d.  Two correspondences whose planes differ fix d up to sign: d is on the line of intersection of the two planes.
"""
import numpy as np


def pixel_to_bearing(p, W, H):
    """Camera::PixelToBearing in f64 on (n, 2) pixels"""
    p = np.asarray(p, np.float64).reshape(-1, 2)
    lon = (p[:, 0] / W - 0.5) * 2.0 * np.pi
    lat = -(p[:, 1] / H - 0.5) * np.pi
    return np.stack([np.cos(lat) * np.sin(lon), -np.sin(lat), np.cos(lat) * np.cos(lon)], axis=1)


def bearing_to_pixel(b, W, H):
    b = np.asarray(b, np.float64)
    b = b / np.linalg.norm(b, axis=1, keepdims=True)
    lon = np.arctan2(b[:, 0], b[:, 2])
    lat = -np.arcsin(np.clip(b[:, 1], -1.0, 1.0))
    return np.stack([(lon / (2.0 * np.pi) + 0.5) * W, (0.5 - lat / np.pi) * H], axis=1)


def rodrigues(axis, angle):
    k = np.asarray(axis, np.float64)
    k = k / np.linalg.norm(k)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * (K @ K)


def make_scene(seed, n=300, W=960, H=480, step=0.3, rot_deg=3.0, outliers=0.25, noise_px=0.2, depth=(0.8, 15.0),
               r_err_deg=0.05, t_axis=None):
    """n points at depths in `depth` seen from two poses: X_cur = R X_prev - c with |c| = step and a rotation of
    rot_deg about a random axis; pixel noise on both views; a share `outliers` of the tracks is displaced by a gross
    error of 6..40 px in a random direction.  Returns p0, p1 (f32 pixels), the true R, the rotation handed to the
    stage (R perturbed by r_err_deg about another axis), c, and the outlier flags."""
    rng = np.random.default_rng(seed)
    lon = rng.uniform(-np.pi, np.pi, n) * 0.97
    lat = rng.uniform(-1.0, 1.0, n) * np.deg2rad(55.0)
    d = rng.uniform(depth[0], depth[1], n)
    X0 = d[:, None] * np.stack([np.cos(lat) * np.sin(lon), -np.sin(lat), np.cos(lat) * np.cos(lon)], axis=1)
    R = rodrigues(rng.normal(size=3), np.deg2rad(rot_deg))
    ax = rng.normal(size=3) if t_axis is None else np.asarray(t_axis, np.float64)
    c = step * ax / np.linalg.norm(ax)
    X1 = X0 @ R.T - c
    p0 = bearing_to_pixel(X0, W, H) + rng.normal(scale=noise_px, size=(n, 2))
    p1 = bearing_to_pixel(X1, W, H) + rng.normal(scale=noise_px, size=(n, 2))
    bad = rng.uniform(size=n) < outliers
    ang = rng.uniform(0, 2 * np.pi, n)
    mag = rng.uniform(6.0, 40.0, n)
    p1[bad] += (mag[:, None] * np.stack([np.cos(ang), np.sin(ang)], axis=1))[bad]
    R_given = rodrigues(rng.normal(size=3), np.deg2rad(r_err_deg)) @ R
    return {"p0": p0.astype(np.float32), "p1": p1.astype(np.float32), "R": R, "R_given": R_given.astype(np.float32),
            "c": c, "outlier": bad, "W": W, "H": H}


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


class Reference:
    """The test on f64 bearings of the f32 pixels, under the f32 rotation the stage is handed.  `grow` scales every
    threshold by (1 + grow) in the direction that lets more tracks pass (grow > 0) or fewer (grow < 0)."""

    def __init__(self, p0, p1, W, H, R, prm):
        self.b0, self.b1 = pixel_to_bearing(p0, W, H), pixel_to_bearing(p1, W, H)
        self.a = _unit(self.b0 @ np.asarray(R, np.float64).reshape(3, 3).T)
        self.theta = np.arccos(np.clip(np.sum(self.a * self.b1, axis=1), -1.0, 1.0))  # rotation residual
        self.plane = np.cross(self.a, self.b1)  # |.| = sin(theta)
        self.prm = prm
        self.n = len(self.b0)

    def rin(self, grow=0.0):
        return self.theta < self.prm.rot_thresh_rad * (1.0 + grow)

    def direction(self, i, j):
        """the line both sample planes contain, and the angle between the planes"""
        ni, nj = _unit(self.plane[i]), _unit(self.plane[j])
        t = np.cross(ni, nj)
        s = np.linalg.norm(t)
        return t / s if s > 0 else t, np.arcsin(min(s, 1.0))

    def skipped(self, i, j, grow=0.0):
        """grow > 0: fewer hypotheses are skipped (a sample must not be a rotation inlier: that test shrinks)"""
        rin = self.rin(-grow)
        if rin[i] or rin[j]:
            return True
        _, ang = self.direction(i, j)
        return not ang >= self.prm.min_plane_angle_rad * (1.0 - grow)

    def votes(self, d, grow=0.0, rin_grow=None):
        """+1 / -1 / 0 per point that is not a rotation inlier: on its epipolar plane through d, displaced towards
        +d (+1) or towards -d (-1)"""
        a, b1 = self.a, self.b1
        m = np.cross(d, a)
        sin_to_epipole = np.linalg.norm(m, axis=1)  # sin of the angle between a and the line of d
        with np.errstate(all="ignore"):
            off = np.arcsin(np.clip(np.abs(np.sum(b1 * m, axis=1)) / sin_to_epipole, 0.0, 1.0))  # b1 to the plane
        tangent = d[None, :] - np.sum(a * d, axis=1)[:, None] * a  # at a, towards +d
        flow = np.sum((b1 - a) * tangent, axis=1)
        ok = (sin_to_epipole > 1e-3 * (1.0 - grow)) & (off < self.prm.epi_thresh_rad * (1.0 + grow))
        ok &= self.theta <= self.prm.max_parallax_rad * (1.0 + grow)
        ok &= ~self.rin(grow if rin_grow is None else rin_grow)
        return np.where(ok, np.sign(flow), 0).astype(int)

    def count(self, i, j, grow=0.0):
        """count of hypothesis (i, j): -1 when skipped.  With grow > 0 an upper bound of the nominal count, with
        grow < 0 a lower bound: a track that turns from rescued into a rotation inlier stays counted, so the count
        rin + max(pos, neg) is monotone in every threshold taken in its passing direction."""
        if self.skipped(i, j, grow):
            return -1, 0, 1
        d, _ = self.direction(i, j)
        v = self.votes(d, grow)
        pos, neg = int((v > 0).sum()), int((v < 0).sum())
        return int(self.rin(grow).sum()) + max(pos, neg), max(pos, neg), (1 if pos >= neg else -1)

    def mask(self, i, j, sigma, grow=0.0):
        d, _ = self.direction(i, j)
        return self.rin(grow) | (self.votes(d, grow) == sigma)

    def t_dir(self, i, j, sigma):
        d, _ = self.direction(i, j)
        return -sigma * d
