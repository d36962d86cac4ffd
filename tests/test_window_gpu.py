"""GPU leg of the window bookkeeping: vio_window_triangulate (candidates -> device vio_triangulate ->
commit) gives the same graph as the host halves around the numpy/LAPACK oracle triangulation
(test_window.py's path): identical MapPoint handles, flags and observation lists, positions within
the triangulation bar of test_tri_gpu.py (1e-5 relative)."""
import numpy as np
import pytest

from test_tri_oracle import load_oracle
from test_window import make_sequence

pytestmark = pytest.mark.gpu


def run(vio, frames, tri_fn, max_kf=4):
    W = vio.Window(max_kf)
    prev = None
    for fr in frames:
        mp = [-1] * len(fr["fid"]) if prev is None else \
            W.link_mappoints(prev["fid"], prev["valid"], prev["mp"], fr["fid"]).tolist()
        W.add_keyframe(fr["id"], fr["T"], np.eye(4), fr["fid"], fr["bearing"], fr["valid"], mp, tracks=fr["tracks"])
        if prev is not None:
            tri_fn(W, prev["id"], fr["id"])
        prev = dict(id=fr["id"], fid=fr["fid"], valid=fr["valid"].tolist(), mp=W.frame_mappoints(fr["id"]))
    return W


def low_parallax_sequence(rng, n_frames=12, n_tracks=80, feats=60):
    """make_sequence's tracks on a geometrically consistent scene: every track is a point 4-15 m away,
    the camera (identity rotation) steps 0.2 m, 0 (zero baseline), 1e-3 m and 1e-4 m (low parallax) in
    turn, and the bearings are the true directions with 1e-3 of noise — so a zero-baseline pair still
    has two distinct rays (they meet in the camera centre) and the null vector stays unique."""
    frames = make_sequence(rng, n_frames=n_frames, n_tracks=n_tracks, feats=feats)
    d = rng.normal(size=(n_tracks, 3))
    pts = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(4, 15, (n_tracks, 1))
    x = np.cumsum(np.resize([0.2, 0.0, 1e-3, 1e-4], n_frames))
    for f, fr in enumerate(frames):
        c = np.array([x[f], 0.0, 0.0])
        fr["T"][:3, 3] = c
        b = pts[fr["fid"]] - c
        b /= np.linalg.norm(b, axis=1, keepdims=True)
        b += rng.normal(0, 1e-3, b.shape)
        fr["bearing"] = (b / np.linalg.norm(b, axis=1, keepdims=True)).astype(np.float32)
    return frames


def _device_and_host_graphs_match(vio, gpu_ctx, frames):
    tri = load_oracle()

    def host(W, a, b):
        pairs, bear, T = W.triangulation_candidates(a, b)
        if len(pairs):
            X, V, _ = tri.triangulate(T, np.tile([0, 1], (len(pairs), 1)), bear, 960)
            W.commit_triangulation(a, b, pairs, X.astype(np.float32), V.astype(np.uint8))

    Wh = run(vio, frames, host)
    Wd = run(vio, frames, lambda W, a, b: W.triangulate(gpu_ctx, a, b))
    assert Wh.keyframes() == Wd.keyframes()
    assert Wh.num_mappoints() == Wd.num_mappoints() > 0
    for h in range(Wh.num_mappoints()):
        a, b = Wh.mappoint(h), Wd.mappoint(h)
        assert (a["bad"], a["marg"], a["tri"], a["ref"], a["obs"]) == (b["bad"], b["marg"], b["tri"], b["ref"], b["obs"])
        nrm = max(float(np.linalg.norm(a["pos"])), 1e-6)
        assert np.linalg.norm(a["pos"].astype(np.float64) - b["pos"]) / nrm < 1e-5
    return Wh


def test_device_triangulation_matches_host_path(vio, gpu_ctx):
    _device_and_host_graphs_match(vio, gpu_ctx, make_sequence(np.random.default_rng(3), n_frames=12, n_tracks=80,
                                                              feats=60))


def test_device_triangulation_matches_host_path_at_low_parallax(vio, gpu_ctx):
    """Zero-baseline and 1e-3 / 1e-4 m pairs among the candidates: the device and host graphs still
    match handle for handle, and the zero-baseline pairs did produce MapPoints (at the camera)."""
    frames = low_parallax_sequence(np.random.default_rng(4))
    W = _device_and_host_graphs_match(vio, gpu_ctx, frames)
    centres = np.array([fr["T"][:3, 3] for fr in frames], np.float64)
    pos = np.array([W.mappoint(h)["pos"] for h in range(W.num_mappoints())], np.float64)
    near = np.linalg.norm(pos[:, None] - centres[None], axis=2).min(1)
    assert (near < 1e-2).any() and (near > 1.0).any()
