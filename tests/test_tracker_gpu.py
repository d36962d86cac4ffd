"""GPU parity of the HIP ERP tracker (libvio360.so via the C-ABI) against the CPU oracle.

The HIP kernels implement the oracle's integer / float definitions literally (exact int64 LK sums,
-ffp-contract=off), so the bar is BITWISE: tracked positions, status, RANSAC masks, corner lists.
"""
import numpy as np
import pytest

import oracle_lib

pytestmark = pytest.mark.gpu

W, H = 960, 480


@pytest.fixture(scope="module")
def pair(synth):
    return synth.config1(W, H)


def region_mask(W, H, margin=20, polar=0.15):
    m = np.zeros((H, W), np.uint8)
    m[int(np.float32(H) * np.float32(polar)):int(np.float32(H) * (np.float32(1.0) - np.float32(polar))),
      margin:W - margin] = 255
    return m


def test_klt_bitwise(vio, gpu_ctx, pair):
    a, b, _ = pair
    pts = oracle_lib.gftt(a, region_mask(W, H), 300, float(np.float32(0.01)), 30.0)
    # add hard cases: image corners, outside the image, the polar rows
    extra = np.array([[0, 0], [959.9, 479.9], [-30, 100], [1000, 20], [480, 5], [3.5, 240.25], [955.2, 300.7]],
                     np.float32)
    pts = np.concatenate([pts, extra])
    prm = vio.default_klt_params()
    g = gpu_ctx.klt_track(a, b, pts, prm)
    o = oracle_lib.klt_track(a, b, pts, prm)
    assert np.array_equal(g[1], o[1])
    assert np.array_equal(g[0], o[0])
    assert np.array_equal(g[2][o[1] == 1], o[2][o[1] == 1])


def test_klt_params_and_levels(vio, gpu_ctx, pair):
    a, b, _ = pair
    pts = oracle_lib.gftt(a, None, 100, 0.01, 20.0)
    for win, lv, it in [(15, 2, 10), (21, 0, 30), (9, 4, 5)]:
        prm = vio.abi.ErpKltParams(win, lv, it, 0.01, 1e-4, 0)
        g = gpu_ctx.klt_track(a, b, pts, prm)
        o = oracle_lib.klt_track(a, b, pts, prm)
        assert np.array_equal(g[1], o[1]) and np.array_equal(g[0], o[0]), (win, lv, it)
    g = gpu_ctx.klt_track(a, b, np.zeros((0, 2), np.float32))
    assert len(g[0]) == 0


def test_gftt_bitwise(vio, gpu_ctx, pair):
    a = pair[1]
    q = float(np.float32(0.01))
    m = region_mask(W, H)
    m[200:260, 300:420] = 0
    for mask, maxc, md in [(m, 300, 30.0), (None, 1000, 10.0), (m, 0, 5.0), (None, 50, 0.0), (m, 2000, 1.0)]:
        g = gpu_ctx.gftt(a, mask, maxc, q, md)
        o = oracle_lib.gftt(a, mask, maxc, q, md)
        assert np.array_equal(g, o), (maxc, md, len(g), len(o))


def test_gftt_odd_sizes(vio, gpu_ctx, synth):
    rng = np.random.default_rng(0)
    for (h, w) in [(37, 53), (129, 257), (64, 65)]:
        img = synth.render_erp(w, h)
        img = np.clip(img.astype(int) + rng.integers(-20, 20, img.shape), 0, 255).astype(np.uint8)
        g = gpu_ctx.gftt(img, None, 0, 0.01, 3.0)
        o = oracle_lib.gftt(img, None, 0, 0.01, 3.0)
        assert np.array_equal(g, o), (h, w)


def test_rot_ransac_bitwise(vio, gpu_ctx):
    from test_tracker_oracle import planted_rotation
    thr = vio.ransac_threshold()
    for seed, frac, n in [(5, 0.2, 300), (9, 0.6, 120), (1, 0.0, 50), (3, 0.3, 1500)]:
        p0, p1, inl = planted_rotation(n=n, outlier_frac=frac, seed=seed)
        s = vio.ransac_samples(seed, len(p0), 1000)
        g = gpu_ctx.rot_ransac(p0, p1, W, H, s, thr)
        o = oracle_lib.rot_ransac(p0, p1, W, H, s, thr)
        assert np.array_equal(g[0], o[0]) and g[1] == o[1]
    m, k = gpu_ctx.rot_ransac(np.zeros((2, 2)), np.zeros((2, 2)), W, H, np.zeros(0, np.int32), thr)
    assert m.tolist() == [1, 1] and k == 2


def cv_circle_fill(mask, cx, cy, r):
    """OpenCV drawing.cpp Circle(fill=1), LINE_8: the midpoint loop painting its spans."""
    h, w = mask.shape
    err, dx, dy, plus, minus = 0, r, 0, 1, (r << 1) - 1
    while dx >= dy:
        for (yy, xl, xr) in ((cy - dy, cx - dx, cx + dx), (cy + dy, cx - dx, cx + dx),
                             (cy - dx, cx - dy, cx + dy), (cy + dx, cx - dy, cx + dy)):
            if 0 <= yy < h:
                mask[yy, max(xl, 0):min(xr, w - 1) + 1] = 0
        dy += 1
        err += plus
        plus += 2
        msk = (err <= 0) - 1
        err -= minus & msk
        dx += msk
        minus -= msk & 2


def pipeline_oracle(vio, prev, curr, pts, prm, klt):
    """TrackFeatures' numeric path composed from the oracle pieces."""
    H, W = prev.shape
    nxt, st, _ = oracle_lib.klt_track(prev, curr, pts, klt)
    vr = nxt[:, 1] / np.float32(H)
    polar = (vr < np.float32(prm.polar_ratio)) | (vr > np.float32(1.0) - np.float32(prm.polar_ratio))
    m = np.float32(prm.boundary_margin)
    nearb = (nxt[:, 0] < m) | (nxt[:, 0] > np.float32(W) - m) | (nxt[:, 1] < m) | (nxt[:, 1] > np.float32(H) - m)
    good = np.nonzero((st == 1) & ~polar & ~nearb)[0]
    kept = np.zeros(len(pts), np.uint8)
    if len(good) >= 3:
        s = vio.ransac_samples(prm.ransac_seed, len(good), prm.ransac_iters)
        mk, _ = oracle_lib.rot_ransac(pts[good], nxt[good], W, H, s, prm.ransac_thresh_rad)
        kept[good] = mk
    else:
        kept[good] = 1
    mask = region_mask(W, H, prm.boundary_margin, prm.polar_ratio)
    r = int(prm.min_dist)
    for i in np.nonzero(kept)[0]:
        cv_circle_fill(mask, int(np.rint(nxt[i, 0])), int(np.rint(nxt[i, 1])), r)
    corners = oracle_lib.gftt(curr, mask, prm.max_corners, prm.quality, prm.min_dist)
    return nxt, st, kept, corners


def test_pipeline_bitwise(vio, gpu_ctx, pair):
    a, b, _ = pair
    pts0 = oracle_lib.gftt(a, region_mask(W, H), 300, float(np.float32(0.01)), 30.0)
    rng = np.random.default_rng(2)
    bad = np.stack([rng.uniform(30, 930, 20), rng.uniform(80, 400, 20)], -1).astype(np.float32)
    pts = np.concatenate([pts0, bad])  # weak points: some fail LK / become RANSAC outliers
    prm = vio.default_tracker_params(max_corners=300, seed=77)
    klt = vio.default_klt_params()
    t = vio.Tracker(gpu_ctx, W, H, max_points=1024, max_corners=1024)
    t.upload(0, a)
    t.upload(1, b)
    t.set_points(pts)
    t.run(prm, klt)
    res = t.download()
    st_ms = t.stage_ms()
    t.close()
    nxt, st, kept, corners = pipeline_oracle(vio, a, b, pts, prm, klt)
    assert np.array_equal(res["status"], st)
    assert np.array_equal(res["next"], nxt)
    assert np.array_equal(res["kept"], kept)
    assert kept.sum() > 200
    assert np.array_equal(res["corners"], corners)
    assert st_ms["total"] > 0


def test_pipeline_full_size_config1(vio, gpu_ctx, synth):
    """Config 1 at its BASELINE size (3840x1920, 300 corners): LK against the analytic flow, the
    pipeline against the oracle composition."""
    a, b, R21 = synth.config1()
    Wf, Hf = 3840, 1920
    pts = oracle_lib.gftt(a, region_mask(Wf, Hf), 300, float(np.float32(0.01)), 30.0)
    assert len(pts) == 300
    prm = vio.default_tracker_params(max_corners=300, seed=1)
    klt = vio.default_klt_params()
    t = vio.Tracker(gpu_ctx, Wf, Hf, max_points=512, max_corners=512)
    t.upload(0, a)
    t.upload(1, b)
    t.set_points(pts)
    t.run(prm, klt)
    res = t.download()
    fb = t.gftt_fallbacks()
    t.close()
    assert fb == (0, 0)  # the bench's configuration: decided by the presorted greedy pass on the device
    truth = synth.erp_flow_truth(pts, Wf, Hf, R21)
    ok = res["status"] == 1
    assert ok.mean() > 0.95
    e = np.linalg.norm(res["next"] - truth, axis=1)[ok]
    assert np.median(e) < 0.05
    nxt, st, kept, corners = pipeline_oracle(vio, a, b, pts, prm, klt)
    assert np.array_equal(res["next"], nxt) and np.array_equal(res["kept"], kept)
    assert np.array_equal(res["corners"], corners)


@pytest.mark.parametrize("npts,max_corners,quality,tail", [(300, 1000, 0.01, 1), (300, 300, 0.3, 1), (300, 4, 0.01, 1),
                                                            (100, 20, 0.01, 0), (40, 4, 0.01, 0)])
def test_pipeline_presel_cases_bitwise(vio, gpu_ctx, pair, npts, max_corners, quality, tail):
    """The pipeline's GFTT greedy pass runs over the presorted strongest local maxima (side stream, before the
    discs exist) and hands frames it cannot decide to the exact tail.  On this 960x480 pair 300 tracked points'
    discs cover the prefix's keys (~2.7 k) but one, so every 300-point case takes the exact tail (more corners
    than the frame holds, a high quality level, a small max_corners); 100 and 40 points leave enough of the
    prefix outside the discs to decide on the device.  All give the oracle's corners bit for bit (the expected
    paths follow a CPU emulation of the prefix: the oracle's eigenvalue map, the bucket cut, the discs)."""
    a, b, _ = pair
    pts = oracle_lib.gftt(a, region_mask(W, H), 300, float(np.float32(0.01)), 30.0)[:npts]
    prm = vio.default_tracker_params(max_corners=max_corners, seed=5)
    prm.quality = float(np.float32(quality))
    klt = vio.default_klt_params()
    t = vio.Tracker(gpu_ctx, W, H, max_points=1024, max_corners=1024)
    t.upload(0, a)
    t.upload(1, b)
    t.set_points(pts)
    t.run(prm, klt)
    res = t.download()
    fb = t.gftt_fallbacks()
    t.close()
    nxt, st, kept, corners = pipeline_oracle(vio, a, b, pts, prm, klt)
    assert np.array_equal(res["kept"], kept)
    assert np.array_equal(res["corners"], corners)
    assert fb == (tail, 0)


PRESEL_CASES = [(300, 1000, 0.01), (300, 300, 0.3), (300, 4, 0.01), (100, 20, 0.01), (40, 4, 0.01)]


def test_download_is_idempotent(vio, gpu_ctx, pair):
    """A second download() of the same run launches nothing more and counts nothing again: the (300, 1000, 0.01)
    case takes the exact tail on its first download, and both downloads give the oracle's corners with one
    fallback counted.  The same for a detection on the local-maximum route without a presort (Context.gftt
    with the analytic mask), asked twice."""
    a, b, _ = pair
    npts, max_corners, quality = PRESEL_CASES[0]
    pts = oracle_lib.gftt(a, region_mask(W, H), 300, float(np.float32(0.01)), 30.0)[:npts]
    prm = vio.default_tracker_params(max_corners=max_corners, seed=5)
    prm.quality = float(np.float32(quality))
    klt = vio.default_klt_params()
    corners = pipeline_oracle(vio, a, b, pts, prm, klt)[3]
    t = vio.Tracker(gpu_ctx, W, H, max_points=1024, max_corners=1024)
    t.upload(0, a)
    t.upload(1, b)
    t.set_points(pts)
    t.run(prm, klt)
    for _ in range(2):
        res = t.download()
        assert np.array_equal(res["corners"], corners)
        assert t.gftt_fallbacks() == (1, 0)
    t.close()
    o = oracle_lib.gftt(b, None, 1000, float(np.float32(0.01)), 10.0)
    for _ in range(2):
        assert np.array_equal(gpu_ctx.gftt(b, None, 1000, float(np.float32(0.01)), 10.0), o)


_PRESEL_VARIANT_CHILD = r"""
import importlib, sys, numpy as np
sys.path.insert(0, sys.argv[1])
vio = importlib.import_module("360_visual_inertial_odometry_amd")
ref = np.load(sys.argv[2])
ctx = vio.Context(0)
klt = vio.default_klt_params()
for i in range(int(ref["n_cases"])):
    prm = vio.default_tracker_params(max_corners=int(ref["max_corners"][i]), seed=5)
    prm.quality = float(ref["quality"][i])
    t = vio.Tracker(ctx, 960, 480, max_points=1024, max_corners=1024)
    t.upload(0, ref["a"])
    t.upload(1, ref["b"])
    t.set_points(ref["pts%d" % i])
    t.run(prm, klt)
    r = t.download()
    print("CASE", i, np.array_equal(r["kept"], ref["kept%d" % i]), np.array_equal(r["corners"], ref["corners%d" % i]),
          *t.gftt_fallbacks())
    t.close()
ctx.close()
"""


@pytest.fixture(scope="module")
def presel_default_npz(vio, gpu_ctx, pair, tmp_path_factory):
    """kept / corners of the five presel cases on the default route (this process), for the variants' children"""
    a, b, _ = pair
    pts0 = oracle_lib.gftt(a, region_mask(W, H), 300, float(np.float32(0.01)), 30.0)
    klt = vio.default_klt_params()
    d = {"a": a, "b": b, "n_cases": len(PRESEL_CASES), "max_corners": [c[1] for c in PRESEL_CASES],
         "quality": np.array([c[2] for c in PRESEL_CASES], np.float32)}
    for i, (npts, max_corners, quality) in enumerate(PRESEL_CASES):
        prm = vio.default_tracker_params(max_corners=max_corners, seed=5)
        prm.quality = float(np.float32(quality))
        t = vio.Tracker(gpu_ctx, W, H, max_points=1024, max_corners=1024)
        t.upload(0, a)
        t.upload(1, b)
        t.set_points(pts0[:npts])
        t.run(prm, klt)
        res = t.download()
        t.close()
        d["pts%d" % i], d["kept%d" % i], d["corners%d" % i] = pts0[:npts], res["kept"], res["corners"]
    path = str(tmp_path_factory.mktemp("presel") / "default.npz")
    np.savez(path, **d)
    return path


@pytest.mark.parametrize("var,fallbacks", [
    ("VIO_TRK_PRESEL", ["0 0"] * 5),
    ("VIO_TRK_PRESEL_FLAG", ["1 0", "1 0", "1 0", "0 0", "0 0"]),
])
def test_pipeline_retained_alternates_bitwise(presel_default_npz, var, fallbacks):
    """The two alternates kept as fallbacks -- VIO_TRK_PRESEL=0 (the masked-maximum tail instead of the presort)
    and VIO_TRK_PRESEL_FLAG=0 (the presort handed over through the stream join) -- give the default route's kept
    flags and corners bit for bit on the five presel cases.  One child process per variant (the environment is
    read once per process).  The expected fallback pairs were taken from a run of this test body on the commit
    before the GfttPlan refactor."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _PRESEL_VARIANT_CHILD, root, presel_default_npz],
                       env=dict(os.environ, **{var: "0"}), capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    print(r.stdout)
    cases = [x.split() for x in r.stdout.split("\n") if x.startswith("CASE")]
    assert len(cases) == len(PRESEL_CASES), r.stdout
    for i, c in enumerate(cases):
        assert c[1:4] == [str(i), "True", "True"], r.stdout
    assert [" ".join(c[4:6]) for c in cases] == fallbacks, r.stdout


_PRESEL_TIMEOUT_CHILD = r"""
import importlib, sys, numpy as np
sys.path.insert(0, sys.argv[1])
vio = importlib.import_module("360_visual_inertial_odometry_amd")
synth = importlib.import_module("360_visual_inertial_odometry_amd.synth")
W, H = 3840, 1920
a, b, _ = synth.config1(W, H)
ctx = vio.Context(0)
mask = np.zeros((H, W), np.uint8)
mask[int(np.float32(H) * np.float32(0.15)):int(np.float32(H) * np.float32(0.85)), 20:W - 20] = 255
pts = ctx.gftt(a, mask, 300, float(np.float32(0.01)), 30.0)
t = vio.Tracker(ctx, W, H, max_points=512, max_corners=512)
t.upload(0, a)
t.upload(1, b)
t.set_points(pts)
prm = vio.default_tracker_params(max_corners=300, seed=1)
res = []
for _ in range(2):
    t.run(prm)
    r = t.download()
    res.append({k: r[k].copy() for k in ("next", "kept", "corners")})
    print("FALLBACKS", *t.gftt_fallbacks())
print("SAME", all(np.array_equal(res[0][k], res[1][k]) for k in res[0]), len(res[0]["corners"]))
t.close()
ctx.close()
"""


def test_presel_handoff_timeout_takes_the_exact_tail():
    """The greedy pass's wait for the presort (a device counter polled under a 2 s wall-clock bound) never hangs
    and never returns a wrong corner set: a one-shot hook makes the first run's target unreachable; that run's
    pass reports `incomplete`, the download runs the exact tail (one fallback counted) and its corners equal the
    second, normal run's (decided on the device: no further fallback)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _PRESEL_TIMEOUT_CHILD, root],
                       env=dict(os.environ, VIO_TRK_TEST_PRESEL_TIMEOUT="1"), capture_output=True, text=True,
                       timeout=100)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.split("\n")
    fb = [x for x in lines if x.startswith("FALLBACKS")]
    assert fb == ["FALLBACKS 1 0", "FALLBACKS 1 0"], r.stdout
    same = [x for x in lines if x.startswith("SAME")][0].split()
    assert same[1] == "True" and int(same[2]) > 0, r.stdout


def test_pipeline_graph_replay_bitwise(vio, gpu_ctx, synth):
    """Runs without stage markers (the bench's timed mode), repeated on the same tracker, give bitwise
    the outputs of a run with them, also after the parameter set and the point count change (config-1
    pair at 1920x960).  (The name is from when such runs could be captured into a graph and replayed.)"""
    a, b, _ = synth.config1(1920, 960)
    Wf, Hf = 1920, 960
    pts = oracle_lib.gftt(a, region_mask(Wf, Hf), 200, float(np.float32(0.01)), 30.0)
    klt = vio.default_klt_params()
    t = vio.Tracker(gpu_ctx, Wf, Hf, max_points=512, max_corners=512)
    t.upload(0, a)
    t.upload(1, b)

    def run(prm, p, markers):
        t.set_points(p)
        t.set_stage_timing(markers)
        t.run(prm, klt)
        t.sync()
        r = t.download()
        return {k: r[k].copy() for k in ("next", "status", "kept", "corners")}

    prm = vio.default_tracker_params(max_corners=200, seed=1)
    ref = run(prm, pts, True)
    for _ in range(3):
        g = run(prm, pts, False)
        for k in ref:
            assert np.array_equal(ref[k], g[k]), k
    prm2 = vio.default_tracker_params(max_corners=150, seed=3)
    ref2 = run(prm2, pts[:120], True)
    g2 = run(prm2, pts[:120], False)
    for k in ref2:
        assert np.array_equal(ref2[k], g2[k]), k
    t.close()


def test_pipeline_on_device_resized_frames(vio, gpu_ctx, synth):
    """The demo frame path (app/main.cpp:199-204): 3840x1920 camera frames INTER_AREA-resized on the
    device into the tracker's 960x480 slots give bitwise the pipeline on oracle-resized frames."""
    from test_dataset import load_resize_oracle
    ro = load_resize_oracle()
    A, B, _ = synth.config1()  # 3840 x 1920
    a, b = ro.resize_area(A, W, H), ro.resize_area(B, W, H)
    pts = oracle_lib.gftt(a, region_mask(W, H), 300, float(np.float32(0.01)), 30.0)
    prm = vio.default_tracker_params(max_corners=300, seed=78)
    klt = vio.default_klt_params()
    res = []
    for resized_on_device in (True, False):
        t = vio.Tracker(gpu_ctx, W, H, max_points=1024, max_corners=1024)
        if resized_on_device:
            t.upload_resized(0, A)
            t.upload_resized(1, B)
        else:
            t.upload(0, a)
            t.upload(1, b)
        t.set_points(pts)
        t.run(prm, klt)
        res.append(t.download())
        t.close()
    for k in ("status", "next", "kept", "corners"):
        assert np.array_equal(res[0][k], res[1][k]), k
    assert res[0]["kept"].sum() > 200
