"""Synthetic two-view triangulation cases (shared by the CPU oracle test and the GPU parity test)."""
import numpy as np


def _rot(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def make_case(n=4096, n_poses=16, seed=0, baseline=0.5, noise=0.0):
    """Keyframes on a short track (world-to-camera f32), random points 2-20 m away, exact (or
    noisy) unit bearings; candidate i pairs two random distinct keyframes."""
    rng = np.random.default_rng(seed)
    T = np.zeros((n_poses, 4, 4), np.float32)
    centers = np.cumsum(rng.normal(0, baseline, (n_poses, 3)), 0)
    for k in range(n_poses):
        R = _rot(rng)
        T[k, :3, :3] = R
        T[k, :3, 3] = -R @ centers[k]
        T[k, 3, 3] = 1
    pairs = np.zeros((n, 2), np.int32)
    pairs[:, 0] = rng.integers(0, n_poses, n)
    pairs[:, 1] = (pairs[:, 0] + rng.integers(1, n_poses, n)) % n_poses
    mid = 0.5 * (centers[pairs[:, 0]] + centers[pairs[:, 1]])
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    X = mid + d * rng.uniform(2, 20, (n, 1))
    B = np.zeros((n, 6), np.float32)
    for j in range(2):
        Tj = T[pairs[:, j]].astype(np.float64)
        pc = np.einsum("nij,nj->ni", Tj[:, :3, :3], X) + Tj[:, :3, 3]
        pc += rng.normal(0, noise, pc.shape) * np.linalg.norm(pc, axis=1, keepdims=True)
        B[:, 3 * j:3 * j + 3] = (pc / np.linalg.norm(pc, axis=1, keepdims=True)).astype(np.float32)
    return T, pairs, B, X


# --------------------------------------------------------------------------------------------
# Named edge cases (n = 1024 unless the name says otherwise).  Parity cases have a unique null
# vector, so the kernel must match oracle/tri_oracle.py; contract cases do not (or the LAPACK
# oracle cannot run on them), so only the entry's contract is asserted.
def _poses(rng, centers):
    T = np.zeros((len(centers), 4, 4), np.float32)
    for k, c in enumerate(centers):
        R = _rot(rng)
        T[k, :3, :3] = R
        T[k, :3, 3] = -R @ c
        T[k, 3, 3] = 1
    return T


def _bearings(T, pairs, X, rng, noise=0.0):
    B = np.zeros((len(pairs), 6), np.float32)
    for j in range(2):
        Tj = T[pairs[:, j]].astype(np.float64)
        pc = np.einsum("nij,nj->ni", Tj[:, :3, :3], X) + Tj[:, :3, 3]
        pc += rng.normal(0, noise, pc.shape) * np.linalg.norm(pc, axis=1, keepdims=True)
        B[:, 3 * j:3 * j + 3] = (pc / np.linalg.norm(pc, axis=1, keepdims=True)).astype(np.float32)
    return B


def _two_view(rng, n, baseline, dist, origin=0.0, noise=0.0, n_rigs=8):
    """n_rigs camera pairs `baseline` apart with random orientations around `origin`·(1,1,1)/√3;
    candidate i sees a point `dist` (lo, hi) metres from its pair's midpoint, 45°-135° off the baseline
    (a point on the baseline has no parallax at any baseline)."""
    o = origin * np.ones(3) / np.sqrt(3.0)
    mids = o + rng.normal(0, 1.0, (n_rigs, 3))
    u = rng.normal(size=(n_rigs, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    centers = np.empty((2 * n_rigs, 3))
    centers[0::2] = mids - 0.5 * baseline * u
    centers[1::2] = mids + 0.5 * baseline * u
    T = _poses(rng, centers)
    rig = rng.integers(0, n_rigs, n)
    pairs = np.stack([2 * rig, 2 * rig + 1], 1).astype(np.int32)
    flip = rng.random(n) < 0.5
    pairs[flip] = pairs[flip][:, ::-1]
    # direction = cos a · u + sin a · (unit vector ⟂ u), a in [45°, 135°]
    a = rng.uniform(np.pi / 4, 3 * np.pi / 4, n)
    w = rng.normal(size=(n, 3))
    w -= (w * u[rig]).sum(1, keepdims=True) * u[rig]
    w /= np.linalg.norm(w, axis=1, keepdims=True)
    d = np.cos(a)[:, None] * u[rig] + np.sin(a)[:, None] * w
    X = mids[rig] + d * rng.uniform(dist[0], dist[1], (n, 1))
    return dict(T=T, pairs=pairs, B=_bearings(T, pairs, X, rng, noise), X=X, noise=noise)


def _bz0(rng, n, both):
    """The point lies in the z = 0 plane of view 1 (and of view 2 when `both`): b_z is exactly 0."""
    c = _two_view(rng, n, 0.5, (2, 20))
    T, pairs = c["T"], c["pairs"]
    R1 =T[pairs[:, 0], :3, :3].astype(np.float64)
    c1 = -np.einsum("nji,nj->ni", R1, T[pairs[:, 0], :3, 3].astype(np.float64))
    phi = rng.uniform(0, 2 * np.pi, n)
    pc1 = np.stack([np.cos(phi), np.sin(phi), np.zeros(n)], 1) * rng.uniform(2, 20, (n, 1))
    X = c1 + np.einsum("nji,nj->ni", R1, pc1)
    B = _bearings(T, pairs, X, rng)
    B[:, 2] = 0.0
    if both:
        B[:, 5] = 0.0
    return dict(T=T, pairs=pairs, B=B, X=None if both else X, noise=0.0)


def edge_cases():
    """dict name -> case (T (m,4,4) f32, pairs (n,2) i32, B (n,6) f32, X planted (n,3) f64 or None,
    kind 'parity' | 'contract'; contract cases may add `bad` (rows holding NaN / inf), `clean`
    (the same case without them) and `parallel`)."""
    out = {}

    def add(name, kind, case, **extra):
        out[name] = dict(case, kind=kind, **extra)

    for bi, b in enumerate((1e-2, 1e-3, 1e-4, 1e-5)):
        for noise in (0.0, 1e-3):
            rng = np.random.default_rng(100 + 2 * bi + (noise > 0))
            add(f"baseline_{b:g}_{'noisy' if noise else 'exact'}", "parity", _two_view(rng, 1024, b, (2, 20), noise=noise))
    add("origin_1e2", "parity", _two_view(np.random.default_rng(110), 1024, 0.5, (2, 20), origin=1e2))
    add("origin_1e3", "parity", _two_view(np.random.default_rng(111), 1024, 0.5, (2, 20), origin=1e3))
    add("far_1e3", "parity", _two_view(np.random.default_rng(112), 1024, 0.5, (1e3, 1e3)))
    add("far_1e5", "parity", _two_view(np.random.default_rng(113), 1024, 0.5, (1e5, 1e5)))
    add("bz0_one_view", "parity", _bz0(np.random.default_rng(114), 1024, both=False))
    # the same pose twice with two distinct bearings: the rays meet in the camera centre
    rng = np.random.default_rng(115)
    c = _two_view(rng, 1024, 0.5, (2, 20))
    c["pairs"][:, 1] = c["pairs"][:, 0]
    Tc = c["T"][c["pairs"][:, 0]].astype(np.float64)
    c["X"] = -np.einsum("nji,nj->ni", Tc[:, :3, :3], Tc[:, :3, 3])
    add("same_pose_two_bearings", "parity", c)
    rng = np.random.default_rng(116)
    c = _two_view(rng, 1024, 0.5, (2, 20))
    s = 10.0 ** rng.uniform(-1, 1, (1024, 2))
    c["B"] = (c["B"].reshape(1024, 2, 3) * s[:, :, None].astype(np.float32)).reshape(1024, 6).astype(np.float32)
    add("non_unit_bearings", "parity", c, scale=s)
    for n in (1, 255, 256, 257):
        T, pairs, B, X = make_case(n=n, n_poses=8, seed=120 + n)
        add(f"n_{n}", "parity", dict(T=T, pairs=pairs, B=B, X=X, noise=0.0))

    # ---- contract cases
    add("bz0_both_views", "contract", _bz0(np.random.default_rng(130), 1024, both=True))
    rng = np.random.default_rng(131)
    c = _two_view(rng, 1024, 0.5, (2, 20))
    c["pairs"][:, 1] = c["pairs"][:, 0]
    c["B"][:, 3:] = c["B"][:, :3]
    c["X"] = None
    add("same_pose_same_bearing", "contract", c)
    rng = np.random.default_rng(132)
    c = _two_view(rng, 1024, 0.5, (2, 20))
    # both cameras of a rig get the same f32 rotation and the candidate the same f32 bearing twice:
    # the two rays are parallel exactly, not to rounding, and meet at infinity
    for k in range(0, len(c["T"]), 2):
        R = c["T"][k, :3, :3]
        ck = -c["T"][k + 1, :3, :3].astype(np.float64).T @ c["T"][k + 1, :3, 3].astype(np.float64)
        c["T"][k + 1, :3, :3] = R
        c["T"][k + 1, :3, 3] = -R.astype(np.float64) @ ck
    c["B"][:, 3:] = c["B"][:, :3]
    c["X"] = None
    add("parallel_bearings", "contract", c, parallel=True)
    add("origin_1e4", "contract", _two_view(np.random.default_rng(133), 1024, 0.5, (2, 20), origin=1e4))
    add("far_1e7", "contract", _two_view(np.random.default_rng(134), 1024, 0.5, (1e7, 1e7)))
    rng = np.random.default_rng(135)
    c = _two_view(rng, 1024, 0.5, (2, 20))
    c["B"][0::3] = 0.0          # both bearings zero
    c["B"][1::3, :3] = 0.0      # one bearing zero
    c["X"] = None
    add("zero_bearings", "contract", c)
    # NaN / ±inf rows between good candidates of the same wave
    rng = np.random.default_rng(136)
    clean = _two_view(rng, 1024, 0.5, (2, 20))
    c = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in clean.items()}
    m = len(c["T"])
    extra = np.repeat(c["T"][:1], 4, 0).copy()
    extra[0, 0, 1] = np.nan      # NaN in a rotation entry
    extra[1, 1, 3] = np.inf      # +inf translation
    extra[2, 2, 3] = -np.inf     # −inf translation
    extra[3, 2, 2] = np.inf      # inf in the row every A row uses
    c["T"] = np.concatenate([c["T"], extra])
    clean["T"] = np.concatenate([clean["T"], np.repeat(clean["T"][:1], 4, 0)])  # same pose count
    bad = np.zeros(1024, bool)
    idx = np.r_[np.arange(3, 1024, 7), [0, 63, 64, 255, 256, 1023]]
    vals = [np.nan, np.inf, -np.inf]
    for j, i in enumerate(idx):
        bad[i] = True
        if j % 2 == 0:
            c["B"][i, j % 6] = vals[(j // 2) % 3]
        else:
            c["pairs"][i, (j // 2) % 2] = m + (j // 2) % 4
    c["X"] = None
    add("nonfinite_rows", "contract", c, bad=bad, clean=clean)
    return out
