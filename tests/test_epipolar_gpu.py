"""GPU parity of the known-rotation epipolar RANSAC (csrc/epipolar.hip: erp_epi_ransac, the tracker pipeline's and
the front end's stage) against tests/epipolar_oracle.py, which tests/test_epipolar.py pins to an f64 reference.
Bitwise throughout: mask, n_inliers, every hypothesis' count, and the info including the bits of t_dir."""
import contextlib

import numpy as np
import pytest

import epipolar_cases as cases
import epipolar_oracle as eo
import epipolar_reference as ref
import klt_guess_oracle as ko
import oracle_lib
from test_seam_gpu import padded

pytestmark = pytest.mark.gpu

FRAMES = [(64, 32), (960, 480)]
SIZES = [0, 1, 2, 3, 63, 64, 65, 300, 1000]


def stream(seed, n, iters):
    """sample rows for n points: the reference's stream from n = 3, the only pair for n = 2"""
    if n >= 3:
        return cases.samples(seed, n, iters)
    return np.tile(np.int32([[0, 1, 0], [1, 0, 1]]), ((iters + 1) // 2, 1))[:iters] if n == 2 else np.zeros((iters, 3), np.int32)


def same_info(g, o):
    assert (g["n_rot"], g["n_rescued"], g["best"], g["model_valid"]) == \
        (o["n_rot"], o["n_rescued"], o["best"], o["model_valid"]), (g, o)
    assert np.array_equal(g["t_dir"].view(np.uint32), o["t_dir"].view(np.uint32)), (g, o)


def check(gpu_ctx, p0, p1, W, H, S, prm, R, what=None):
    g = gpu_ctx.epi_ransac(p0, p1, W, H, S, R=R, params=prm)
    o = eo.run(p0, p1, W, H, S, prm, R=R)
    assert np.array_equal(g[0], o["mask"]), what
    assert g[1] == o["n_in"], what
    assert np.array_equal(g[2], o["counts"]), what
    same_info(g[3], o["info"])
    return o


@pytest.mark.parametrize("given", [True, False])
@pytest.mark.parametrize("W,H", FRAMES)
def test_one_shot_sizes(gpu_ctx, W, H, given):
    prm = cases.params()
    valid = 0
    for n in SIZES:
        s = cases.sized(n, W, H, seed=100 + n)
        o = check(gpu_ctx, s["p0"], s["p1"], W, H, stream(7, n, 256), prm, s["R_given"] if given else None, (W, n))
        valid += o["info"]["model_valid"]
        if n >= 300 and given:
            assert o["info"]["model_valid"] == 1 and o["info"]["n_rescued"] >= n // 10
    assert valid >= 2


@pytest.mark.parametrize("given", [True, False])
def test_one_shot_iters(gpu_ctx, given):
    s, prm = cases.scene("translation"), cases.params()
    for iters in (0, 1, 4, 5, 256):
        S = cases.samples(5, 300, 256)[:iters]
        check(gpu_ctx, s["p0"], s["p1"], s["W"], s["H"], S, prm, s["R_given"] if given else None, iters)


def test_scenes_and_the_rotation_ransac_route(gpu_ctx):
    prm = cases.params()
    for name in cases.SCENES:
        s = cases.scene(name)
        check(gpu_ctx, s["p0"], s["p1"], s["W"], s["H"], cases.samples(5, 300, 256), prm, s["R_given"], name)
        # R == NULL: 1000 rotation hypotheses, every row also a plane hypothesis
        o = check(gpu_ctx, s["p0"], s["p1"], s["W"], s["H"], cases.samples(5, 300, 1000), prm, None, name)
        assert np.all(o["mask"] >= o["rot_mask"])


def test_every_hypothesis_skipped(gpu_ctx):
    """a pure rotation without noise or outliers: every point is a rotation inlier, no pair may be sampled"""
    s = ref.make_scene(seed=3, step=0.0, rot_deg=5.0, outliers=0.0, noise_px=0.0, r_err_deg=0.0)
    for R in (s["R_given"], None):
        o = check(gpu_ctx, s["p0"], s["p1"], s["W"], s["H"], cases.samples(5, 300, 256), cases.params(), R)
        assert np.all(o["counts"] == -1) and o["info"]["best"] == -1 and o["mask"].all()


def test_point_at_the_epipole(gpu_ctx):
    """an exact scene (no noise, no outliers, the true rotation): every hypothesis' direction is the true one to f32
    rounding, and the appended track starts 0.005 degrees from it -- inside the mm guard (0.057 degrees) -- and ends
    3 degrees away: never on a plane, whatever the hypothesis"""
    s = ref.make_scene(seed=4, outliers=0.0, noise_px=0.0, r_err_deg=0.0)
    W, H, Rg = s["W"], s["H"], s["R_given"].astype(np.float64).reshape(3, 3)
    d = s["c"] / np.linalg.norm(s["c"])
    side = np.cross(d, [1.0, 0.0, 0.0])
    side /= np.linalg.norm(side)
    a = np.cos(np.deg2rad(0.005)) * d + np.sin(np.deg2rad(0.005)) * side
    b1 = np.cos(np.deg2rad(3.0)) * d + np.sin(np.deg2rad(3.0)) * side
    p0 = np.vstack([s["p0"], ref.bearing_to_pixel((Rg.T @ a)[None, :], W, H)]).astype(np.float32)
    p1 = np.vstack([s["p1"], ref.bearing_to_pixel(b1[None, :], W, H)]).astype(np.float32)
    o = check(gpu_ctx, p0, p1, W, H, cases.samples(5, 300, 256), cases.params(), s["R_given"])
    P, S = o["pts"], cases.samples(5, 300, 256)
    assert o["info"]["model_valid"] == 1 and not P.rin[-1] and P.par_ok[-1] and o["mask"][-1] == 0
    t, tt = P.model(*S[o["info"]["best"]][:2], eo.thresholds(cases.params())[3])
    m = eo._cross(t, [v[-1] for v in P.a])
    assert not eo._dot(m, m) > np.float32(1e-6) * tt  # the guard, not the plane test, rejected it


def test_support_floor(gpu_ctx):
    s = cases.scene("translation")
    S = cases.samples(5, 300, 256)
    r = eo.run(s["p0"], s["p1"], s["W"], s["H"], S, cases.params(), R=s["R_given"])["info"]["n_rescued"]
    assert r >= 10
    below = check(gpu_ctx, s["p0"], s["p1"], s["W"], s["H"], S, cases.params(min_support=r + 1), s["R_given"])
    assert below["info"]["model_valid"] == 0 and below["info"]["best"] >= 0
    assert np.array_equal(below["mask"].astype(bool), below["pts"].rin)
    at = check(gpu_ctx, s["p0"], s["p1"], s["W"], s["H"], S, cases.params(min_support=r), s["R_given"])
    assert at["info"]["model_valid"] == 1 and at["info"]["n_rescued"] == r


def test_tie_picks_the_earlier(gpu_ctx):
    s, prm = cases.scene("translation"), cases.params()
    S = cases.samples(5, 300, 256)
    bi = eo.run(s["p0"], s["p1"], s["W"], s["H"], S, prm, R=s["R_given"])["info"]["best"]
    first = check(gpu_ctx, s["p0"], s["p1"], s["W"], s["H"], np.vstack([S[bi:bi + 1], S]), prm, s["R_given"])
    assert first["info"]["best"] == 0 and first["counts"][0] == first["counts"][bi + 1]
    last = check(gpu_ctx, s["p0"], s["p1"], s["W"], s["H"], np.vstack([S, S[bi:bi + 1]]), prm, s["R_given"])
    assert last["info"]["best"] == bi and last["counts"][bi] == last["counts"][len(S)]


def test_errors_launch_nothing(vio, gpu_ctx):
    s = cases.scene("translation")
    S = cases.samples(5, 300, 8)
    for bad in (dict(params=cases.params(epi_thresh_rad=0.0)), dict(R=2.0 * np.eye(3)),
                dict(samples=np.full((8, 3), 300, np.int32))):
        kw = dict(samples=S, R=s["R_given"], params=cases.params())
        kw.update(bad)
        with pytest.raises(vio.VioError):
            gpu_ctx.epi_ransac(s["p0"], s["p1"], s["W"], s["H"], kw["samples"], R=kw["R"], params=kw["params"])


# ---- the tracker pipeline and the front end: their oracles with the RANSAC step swapped ----

@contextlib.contextmanager
def epipolar_step(prm, rotation, log):
    """Inside the block, the RANSAC step of test_tracker_gpu.pipeline_oracle and frontend_oracle.FrontendOracle (both
    call oracle_lib.rot_ransac on the filtered points with the stage's sample stream) is the epipolar oracle under
    rotation() (None: the rotation RANSAC's best over every row); the plane hypotheses are the first prm.iters rows."""
    plain = oracle_lib.rot_ransac

    def step(p0, p1, W, H, samples, _thresh):
        S = np.asarray(samples, np.int32).reshape(-1, 3)
        iters = min(prm.iters, len(S))
        oracle_lib.rot_ransac = plain  # (the epipolar oracle's own rotation stage)
        try:
            o = eo.run(p0, p1, W, H, S[:iters], prm, R=rotation(), min_n=3, rot_samples=S)
        finally:
            oracle_lib.rot_ransac = step
        log.append(o["info"])
        return o["mask"], o["n_in"]

    oracle_lib.rot_ransac = step
    try:
        yield
    finally:
        oracle_lib.rot_ransac = plain


def pipeline_inputs(W, H):
    # (a step that gives the near columns a few pixels of parallax at either size)
    prev, curr = cases.translation_sequence(W, H, 2, step=0.12 if W < 400 else 0.05, yaw_px=3)
    q = float(np.float32(0.01))
    pts = oracle_lib.gftt(prev, None, 0, q, 12.0 if W < 400 else 24.0)
    pts = pts[(pts[:, 1] > 0.2 * H) & (pts[:, 1] < 0.8 * H) & (pts[:, 0] > 24) & (pts[:, 0] < W - 24)][:300]
    return prev, curr, pts


@pytest.mark.parametrize("W,H", [(328, 164), (960, 480)])
def test_tracker_pipeline(vio, gpu_ctx, synth, W, H):
    from test_tracker_gpu import pipeline_oracle
    prev, curr, pts = pipeline_inputs(W, H)
    dev = padded if W == 328 else (lambda a: a)
    R = synth.rot_yaw_pitch(3 * 360.0 / W, 0.0).astype(np.float32)
    prm = vio.default_tracker_params(max_corners=150, seed=31)
    prm.min_dist = 12.0 if W < 400 else 30.0
    klt, epi = vio.default_klt_params(), cases.params()

    def device(t, rotation, on):
        t.set_epipolar(epi if on else vio.default_epi_params())
        if rotation is not None:
            t.set_rotation(rotation)
        t.run(prm, klt)
        res = {k: v.copy() for k, v in t.download().items()}
        res["used"] = t.download_guess() if rotation is not None else None
        if on:
            res["info"] = t.download_epi()
        else:
            with pytest.raises(vio.VioError):
                t.download_epi()
        return res

    def oracle(used, rotation, on):
        log = []
        with contextlib.ExitStack() as es:
            if used is not None:
                es.enter_context(ko.klt_step(lambda a, b, p, k, _m: ko.klt_track(a, b, p, k, used, ko.CUT)[:3]))
            if on:
                es.enter_context(epipolar_step(epi, lambda: rotation, log))
            return pipeline_oracle(vio, prev, curr, pts, prm, klt), log

    t = vio.Tracker(gpu_ctx, W, H, max_points=512, max_corners=256)
    never = vio.Tracker(gpu_ctx, W, H, max_points=512, max_corners=256)
    for x in (t, never):
        x.upload(0, dev(prev))
        x.upload(1, dev(curr))
        x.set_points(pts)
    rescued = []
    for rotation in (None, R):
        g = device(t, rotation, True)
        want, log = oracle(g["used"], rotation, True)
        for k, w in zip(("next", "status", "kept", "corners"), want):
            assert np.array_equal(g[k], w), (W, rotation is not None, k)
        same_info(g["info"], log[0])
        assert int(g["kept"].sum()) == log[0]["n_rot"] + log[0]["n_rescued"]
        rescued.append(log[0]["n_rescued"])
        # the mode off after it was on: a tracker that never had it on, and the plain oracle
        off, plain = device(t, rotation, False), device(never, rotation, False)
        for k, w in zip(("next", "status", "kept", "corners"), oracle(off["used"], rotation, False)[0]):
            assert np.array_equal(off[k], w) and np.array_equal(plain[k], w), (W, rotation is not None, k)
    print("pipeline", W, "rescued without / with the rotation", rescued)
    assert max(rescued) >= epi.min_support
    t.close()
    never.close()


def test_frontend_sequence(vio, gpu_ctx, synth):
    """six frames of the translating scene with a yaw of 6 columns per frame; the exact yaw is predicted before
    frames 2..5, frame 1 takes the rotation RANSAC's best"""
    W, H, d, n = 512, 256, 6, 6
    seq = cases.translation_sequence(W, H, n, step=0.1, yaw_px=d)
    R = synth.rot_yaw_pitch(d * 360.0 / W, 0.0).astype(np.float32)
    prm, klt, epi = vio.default_frontend_params(seed=3), vio.default_klt_params(), cases.params()
    given = [False] + [False] + [True] * 4  # per frame: a prediction before it
    state = {"R": None}
    guess = lambda a, b, p: gpu_ctx.klt_track(a, b, p, klt, seam=ko.CUT, rot=state["R"])[3] if state["R"] is not None else None
    oracle = ko.guided_frontend(vio, W, H, prm, ko.CUT, guess)
    plain = ko.guided_frontend(vio, W, H, prm, ko.CUT, guess)
    fe, fe_off = vio.Frontend(gpu_ctx, W, H, prm), vio.Frontend(gpu_ctx, W, H, prm)
    fe.set_epipolar(epi)
    rescued, valid = [], []
    for f, img in enumerate(seq):
        state["R"] = R if given[f] else None
        for x in (fe, fe_off):
            if given[f]:
                x.predict_rotation(R)
        log = []
        with epipolar_step(epi, lambda: state["R"], log):
            o = oracle.track(img)
        g = fe.track(img)
        for k in ("ids", "xy", "track_count", "age"):
            assert np.array_equal(g[k], o[k]), (f, k)
        assert (g["num_tracked"], g["num_detected"]) == (o["num_tracked"], o["num_detected"])
        same_info(fe.epi_stats(), log[0] if log else eo._info())
        rescued.append(log[0]["n_rescued"] if log else 0)
        valid.append(log[0]["model_valid"] if log else 0)
        if valid[-1]:
            assert log[0]["t_dir"][1] > 0.99, f  # the camera moves along +Y
        g0, o0 = fe_off.track(img), plain.track(img)  # the mode off: today's oracle
        for k in ("ids", "xy", "track_count", "age"):
            assert np.array_equal(g0[k], o0[k]), (f, k, "off")
        same_info(fe_off.epi_stats(), eo._info())
    fe.close()
    fe_off.close()
    print("front end: rescued per frame", rescued, "model valid", valid)
    assert max(rescued) >= epi.min_support
