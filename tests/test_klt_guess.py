"""CPU checks of the guided-LK reference (tests/klt_guess_oracle.py) and of the host-only parts of the feature:

  1. the NumPy restatement with guess=None, and with guess == pts, is the C oracle bit for bit -- everything in it
     except the one line a guess changes;
  2. the large cases of tests/guess_cases.py are worth having: the unguided oracle loses them, the guided reference
     follows them;
  3. erp_predict_from_preint;
  4. the fold and bad-guess rules of the reference;
  5. the new symbols exist and the ABI version stays 4.
Nothing here touches a GPU."""
import ctypes as C

import numpy as np
import pytest

import guess_cases as gc
import klt_guess_oracle as ko
import oracle_lib
import seam_cases as sc
import seam_oracle as so


def klt_params(vio, max_level=3, win=21):
    k = vio.default_klt_params()
    k.max_level, k.win = max_level, win
    return k


def same(a, b):
    """next, status bitwise; err where status is 1"""
    return np.array_equal(a[1], b[1]) and np.array_equal(a[0], b[0]) and np.array_equal(a[2][b[1] == 1], b[2][b[1] == 1])


@pytest.mark.parametrize("flow", sc.FLOWS)
@pytest.mark.parametrize("W,H", sc.SIZES)
def test_restatement_is_the_c_oracle(vio, W, H, flow):
    prev, curr = sc.pair(W, H, flow)
    for name, pts in gc.point_sets(W, H).items():
        assert len(pts) >= 10, name
        for max_level in (0, 1, 3):
            klt = klt_params(vio, max_level)
            want = oracle_lib.klt_track(prev, curr, pts, klt)
            assert same(ko.klt_track(prev, curr, pts, klt), want), (name, max_level, "no guess")
            got = ko.klt_track(prev, curr, pts, klt, guess=pts)
            assert same(got, want), (name, max_level, "guess == pts")
            assert np.array_equal(got[3], pts)
    # the seam variant at the frame's own coordinates is seam_oracle's right-band reference
    klt = klt_params(vio)
    pts = sc.right_band(W, H)
    want = so.klt_track(prev, curr, pts, klt, 0, so.APRON)
    assert same(ko.klt_track(prev, curr, pts, klt, None, ko.WRAP), want)
    assert same(ko.klt_track(prev, curr, pts, klt, pts, ko.WRAP), want)
    assert want[1].mean() > 0.9


def test_restatement_small_window(vio):
    W, H = sc.SIZES[1]
    prev, curr = sc.pair(W, H, sc.FLOWS[1])
    pts = sc.corners(W, H)
    for max_level in (1, 3):
        klt = klt_params(vio, max_level, 9)
        assert same(ko.klt_track(prev, curr, pts, klt, guess=pts), oracle_lib.klt_track(prev, curr, pts, klt))


@pytest.mark.parametrize("name", list(gc.LARGE))
@pytest.mark.parametrize("W,H", gc.SIZES)
def test_large_cases_need_the_guess(vio, W, H, name):
    """measured (fraction within 1.5 px of the true flow; unguided status == 1 share in brackets):
         512 x 256   yaw80 0.004 -> 1.000 (0.918)   yaw120_pitch10 0.000 -> 0.979 (0.901)   third 0.000 -> 0.950 (0.916)
         328 x 160   yaw80 0.002 -> 1.000 (0.972)   yaw120_pitch10 0.000 -> 0.983 (0.961)   third 0.000 -> 0.966 (0.959)"""
    prev, curr, pts, truth, R_seed = gc.large(name, W, H)
    klt = vio.default_klt_params()
    assert len(pts) >= 300
    un = so.klt_track(prev, curr, pts, klt, 0, so.APRON)
    flat = oracle_lib.klt_track(prev, curr, pts, klt)
    guess = ko.predict(pts, R_seed, W, H)[0].astype(np.float32)
    # the seed alone is not the answer: a gyro off by (0.5, 0.3) degrees is more than 0.5 px away
    assert np.median(gc.error_px(guess, truth, W)) > 0.5
    g = ko.klt_track(prev, curr, pts, klt, guess, ko.WRAP)
    f_un = max(float((gc.error_px(un[0], truth, W) < 1.5).mean()), float((gc.error_px(flat[0], truth, W) < 1.5).mean()))
    f_g = float(((gc.error_px(g[0], truth, W) < 1.5) & (g[1] == 1)).mean())
    print(name, W, "unguided within 1.5 px", f_un, "status==1", float(flat[1].mean()), "guided", f_g)
    assert flat[1].mean() > 0.9  # LK itself still reports the lost points as found
    assert f_un <= 0.05
    assert f_g >= 0.90


def rot_zyx(a, b, c):
    def r(axis, t):
        m = np.eye(3)
        i, j = [(1, 2), (0, 2), (0, 1)][axis]
        m[i, i] = m[j, j] = np.cos(t)
        m[i, j], m[j, i] = -np.sin(t), np.sin(t)
        return m
    return r(2, a) @ r(1, b) @ r(0, c)


def test_predict_from_preint(vio, synth):
    T = np.eye(4)
    assert np.array_equal(vio.predict_from_preint(np.eye(3), T), np.eye(3, dtype=np.float32))
    dR = synth.rot_yaw_pitch(17.0, 0.0)
    T[:3, :3] = rot_zyx(0.4, -1.1, 2.0)
    T[:3, 3] = [0.1, -0.2, 0.05]
    dR32, T32 = dR.astype(np.float32), T.astype(np.float32)
    want = T32[:3, :3].astype(np.float64).T @ dR32.astype(np.float64).T @ T32[:3, :3].astype(np.float64)
    got = vio.predict_from_preint(dR, T)
    assert got.dtype == np.float32 and np.abs(got - want).max() <= 1e-6
    assert np.abs(got - np.eye(3)).max() > 0.1
    # a full record goes the same way
    pre = vio.abi.preint_from_delta_R(dR)
    assert np.array_equal(vio.predict_from_preint(pre, T), got)
    # not a rotation: a scaled matrix, a reflection, a NaN; in delta_R or in T_BC
    out = np.zeros(9, np.float32)
    for bad in (1.01 * dR, np.diag([1.0, 1.0, -1.0]), np.full((3, 3), np.nan)):
        with pytest.raises(vio.VioError):
            vio.predict_from_preint(bad, T)
        Tb = T.copy()
        Tb[:3, :3] = bad
        with pytest.raises(vio.VioError):
            vio.predict_from_preint(dR, Tb)
    L = vio.lib()
    assert L.erp_predict_from_preint(None, T32.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)) == -22
    assert L.erp_predict_from_preint(C.byref(pre), None, out.ctypes.data_as(C.c_void_p)) == -22
    assert L.erp_predict_from_preint(C.byref(pre), T32.ctypes.data_as(C.c_void_p), None) == -22


def test_fold_and_bad_guess_rules(vio):
    W, H = sc.SIZES[0]
    prev, curr = sc.pair(W, H, sc.FLOWS[2])
    klt = vio.default_klt_params()
    pts = sc.interior(W, H)[:40]
    flow = np.float32(sc.FLOWS[2])
    good = pts + flow
    base = {m: ko.klt_track(prev, curr, pts, klt, good, m) for m in (ko.CUT, ko.WRAP)}
    un = {m: ko.klt_track(prev, curr, pts, klt, None, m) for m in (ko.CUT, ko.WRAP)}
    bads = [(np.nan, 100.0), (50.0, np.nan), (np.inf, 100.0), (-np.inf, 100.0), (50.0, np.inf), (2.0 * W, 100.0),
            (-W - 1.0, 100.0), (50.0, 2.0 * H), (50.0, -H - 1.0)]
    for m in (ko.CUT, ko.WRAP):
        g = good.copy()
        g[:len(bads)] = np.float32(bads)
        r = ko.klt_track(prev, curr, pts, klt, g, m)
        k = len(bads)
        for q in range(3):  # the bad guesses give the unguided result for their points only
            assert np.array_equal(r[q][:k], un[m][q][:k]) and np.array_equal(r[q][k:], base[m][q][k:])
        assert np.array_equal(r[3][:k], pts[:k]) and np.array_equal(r[3][k:], good[k:])
    # the edges of the admitted range are guesses like any other
    edge = np.float32([[-W, -H], [np.nextafter(np.float32(2 * W), np.float32(0)), np.nextafter(np.float32(2 * H), np.float32(0))]])
    assert np.array_equal(ko.start_positions(pts[:2], edge, W, H, ko.CUT), edge)
    assert np.array_equal(ko.start_positions(pts[:2], edge, W, H, ko.WRAP)[:, 0], np.float32([0, W - 2.0 ** -14]))  # (the f32 below 2W is 2W - 2^-14 at W = 512)
    # WRAP: a guess a turn to either side is the guess itself
    for shift in (np.float32(W), np.float32(-W)):
        g = good.copy()
        g[:, 0] += shift
        r = ko.klt_track(prev, curr, pts, klt, g, ko.WRAP)
        back = g.copy()
        back[:, 0] -= shift  # one f32 operation: x in [W, 2W) equals x - W
        assert ((back[:, 0] >= 0) & (back[:, 0] < W)).all() and np.abs(back - good).max() < 1e-4
        assert np.array_equal(r[3], back) and same(r, ko.klt_track(prev, curr, pts, klt, back, ko.WRAP))
    # CUT: it is taken as it is, and the search ends outside the frame
    g = good.copy()
    g[:, 0] += np.float32(W)
    r = ko.klt_track(prev, curr, pts, klt, g, ko.CUT)
    assert np.array_equal(r[3], g) and not r[1].any()


def test_abi_has_the_guided_entry_points(vio):
    L = vio.lib()
    names = ["erp_klt_track_guess", "erp_klt_track_rot", "erp_tracker_set_guess", "erp_tracker_set_rotation",
             "erp_tracker_download_guess", "erp_frontend_predict_rotation", "erp_predict_from_preint"]
    for n in names:
        assert hasattr(L, n) and n in vio.EXPORTS, n
    assert L.vio_abi_version() == 4
    for n in ("set_guess", "set_rotation", "download_guess"):
        assert hasattr(vio.Tracker, n)
    assert hasattr(vio.Frontend, "predict_rotation")


def test_guided_front_end_oracle_follows_a_fast_yaw(vio, synth):
    """the property test of tests/test_klt_guess_gpu.py on the reference alone: 80 px of yaw per frame, wrap mode;
    measured 72 of 72 frame-1 features alive with track_count 3 at frame 4 with the prediction, none without"""
    W, H, d = 512, 256, 80
    base = sc.pair(W, H, sc.FLOWS[0])[0]
    seq = [np.roll(base, d * f, axis=1) for f in range(4)]
    R = synth.rot_yaw_pitch(d * 360.0 / W, 0.0)
    prm = vio.default_frontend_params(seed=3)
    share = {}
    for guided in (True, False):
        fe = ko.guided_frontend(vio, W, H, prm, ko.WRAP,
                                (lambda p, c, pts: ko.predict(pts, R, W, H)[0].astype(np.float32)) if guided
                                else (lambda p, c, pts: None))
        outs = [fe.track(img) for img in seq]
        first = set(outs[0]["ids"].tolist())
        alive = [i for i, tc in zip(outs[3]["ids"], outs[3]["track_count"]) if int(i) in first and tc == 3]
        share[guided] = len(alive) / len(first)
    print("front-end oracle: share alive", share)
    assert share[True] >= 0.8 and share[False] == 0.0
