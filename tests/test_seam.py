"""Seam wrap mode (VIO_SEAM_WRAP), the part that needs no GPU: erp_seam_check, and the references of
tests/seam_oracle.py on the inputs of tests/test_seam_gpu.py -- every one of them must be a case in which the seam
matters (the reference differs from the flat oracle), or the GPU tests would show nothing."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib
import seam_cases as sc
import seam_oracle as so

OK, EINVAL = 0, -22


def test_constants_and_exports(vio):
    assert (vio.VIO_SEAM_CUT, vio.VIO_SEAM_WRAP) == (so.CUT, so.WRAP) == (0, 1)
    lib = C.CDLL(vio.LIB_PATH)
    for name in ("erp_seam_check", "erp_klt_track_seam", "erp_gftt_seam", "erp_tracker_set_seam",
                 "erp_frontend_set_seam"):
        assert name in vio.EXPORTS and hasattr(lib, name), name
    assert vio.lib().vio_abi_version() == 4  # additive: the version stays


def test_seam_check(vio):
    assert vio.seam_check(512, 256, 21, 3, 30.0) == OK
    assert vio.seam_check(520, 256, 21, 3, 30.0) == OK        # 8 x 65
    assert vio.seam_check(328, 160, 21, 3, 30.0) == OK        # the rows stop the pyramid at level 2: 328 = 4 x 82
    assert vio.seam_check(516, 256, 21, 3, 30.0) == EINVAL    # 4 x 129: level 3 would be odd
    assert vio.seam_check(516, 256, 21, 2, 30.0) == OK        # ... and is not used at max_level 2
    assert vio.seam_check(144, 256, 21, 3, 30.0) == EINVAL    # top level (2) is 36 columns: under the 38 of the tiles
    assert vio.seam_check(152, 256, 21, 3, 30.0) == OK        # 38 columns
    assert vio.seam_check(512, 256, 21, 3, 256.0) == EINVAL   # W <= 2 min_dist
    assert vio.seam_check(512, 256, 21, 3, 255.5) == OK
    for bad in ((0, 256, 21, 3, 30.0), (512, 0, 21, 3, 30.0), (512, 256, 2, 3, 30.0), (512, 256, 22, 3, 30.0),
                (512, 256, 21, -1, 30.0), (512, 256, 21, 8, 30.0), (512, 256, 21, 3, -1.0),
                (512, 256, 21, 3, float("nan"))):
        assert vio.seam_check(*bad) == EINVAL, bad


@pytest.mark.parametrize("W,H", sc.SIZES)
def test_extension_is_the_rolled_frame(W, H):
    """the constructions the references rest on: pyrDown (through the levels LK uses at this size: 3 and 2) and the
    min-eigenvalue map of an extended frame equal those of the frame rolled by W / 2 on the seam band, bit for bit"""
    F = sc.pair(W, H, sc.FLOWS[0])[0]
    P = 64
    e, r = so.extend(F, P, P), np.roll(F, W // 2, axis=1)
    np.testing.assert_array_equal(oracle_lib.min_eig_map(e)[:, P - 40:P + 40],
                                  oracle_lib.min_eig_map(r)[:, W // 2 - 40:W // 2 + 40])
    for lv in range(1, 4 if H == 256 else 3):
        e, r = oracle_lib.pyr_down(e), oracle_lib.pyr_down(r)
        p, w, b = P >> lv, W >> lv, 40 >> lv
        np.testing.assert_array_equal(e[:, p - b:p + b], r[:, w // 2 - b:w // 2 + b])


@pytest.mark.parametrize("flow", sc.FLOWS)
@pytest.mark.parametrize("W,H", sc.SIZES)
def test_klt_inputs_need_the_seam(vio, W, H, flow):
    """on both seam bands the flat oracle loses or moves some of the points the reference tracks"""
    prev, curr = sc.pair(W, H, flow)
    klt = vio.default_klt_params()
    for pts, left in ((sc.right_band(W, H), 0), (sc.left_band(W, H), so.APRON)):
        assert len(pts) >= 40
        assert ((pts[:, 0] >= W - sc.BAND) if left == 0 else (pts[:, 0] < sc.BAND)).all()
        ref = so.klt_track(prev, curr, pts, klt, left, so.APRON)
        assert ref[1].mean() > 0.95
        flat = oracle_lib.klt_track(prev, curr, pts, klt)
        d = np.abs(so.fold_x(flat[0][:, 0], W) - ref[0][:, 0])
        d = np.minimum(d, W - d)
        lost = (flat[1] == 0) & (ref[1] == 1)
        moved = (flat[1] == 1) & (ref[1] == 1) & (d > 0.05)
        assert lost.sum() + moved.sum() >= 1, (W, flow, left)
    crossed = np.abs(ref[0][:, 0] - pts[:, 0]) > W / 2
    assert crossed.any() or flow[0] < 0  # (left band: the flows that point left take points across the seam)


@pytest.mark.parametrize("flow", sc.FLOWS)
@pytest.mark.parametrize("W,H", sc.SIZES)
def test_klt_offset_spread(vio, W, H, flow):
    """the reference at column offset APRON against the reference at offset W / 2 (the rolled pair) on the left band:
    equal statuses, positions within 5e-4 px -- the f32 rounding of coordinates at another offset, which bounds
    what the GPU test of the left band may ask (7 x the largest spread: tests/test_seam_gpu.py)"""
    prev, curr = sc.pair(W, H, flow)
    klt = vio.default_klt_params()
    pts = sc.left_band(W, H)
    a = so.klt_track(prev, curr, pts, klt, so.APRON, so.APRON)
    p2 = pts.copy()
    p2[:, 0] += np.float32(W // 2)
    n2, s2, _ = oracle_lib.klt_track(np.roll(prev, W // 2, axis=1), np.roll(curr, W // 2, axis=1), p2, klt)
    assert np.array_equal(a[1], s2)
    ok = s2 == 1
    dx = np.abs(so.fold_x(n2[:, 0] - np.float32(W // 2), W) - a[0][:, 0])[ok]
    dx = np.minimum(dx, W - dx)
    dy = np.abs(n2[:, 1] - a[0][:, 1])[ok]
    print("offset spread", W, flow, float(dx.max()), float(dy.max()))
    assert max(dx.max(), dy.max()) <= 5e-4


def test_interior_points_exist():
    for (W, H) in sc.SIZES:
        assert len(sc.interior(W, H)) >= 10, (W, H)


@pytest.mark.parametrize("W,H,mask,cap,md", sc.gftt_cases())
def test_gftt_cases_exercise_the_seam(W, H, mask, cap, md):
    """each case: a corner accepted within min_dist of the seam, a rejection only the wrapped distance makes, and a
    result that differs from the flat oracle's"""
    img = sc.pair(W, H, sc.FLOWS[0])[0]
    m = sc.gftt_mask(W, H, mask)
    c, near, seam_only = so.gftt_stats(img, m, cap, sc.Q, md)
    assert near >= 1 and seam_only >= 1, (near, seam_only)
    assert not np.array_equal(c, oracle_lib.gftt(img, m, cap, sc.Q, md))
    if cap:
        assert len(c) == cap  # the cap binds
    if m is not None:
        assert (m[c[:, 1].astype(int), c[:, 0].astype(int)] != 0).all()
    # accepted corners keep min_dist on the cylinder
    x, y = c[:, 0].astype(np.int64), c[:, 1].astype(np.int64)
    dx = np.abs(x[:, None] - x[None, :])
    dx = np.minimum(dx, W - dx)
    d2 = dx * dx + (y[:, None] - y[None, :]) ** 2
    np.fill_diagonal(d2, 1 << 40)
    assert d2.min() >= md * md


def test_pipeline_case_exercises_the_seam(vio):
    from test_tracker_gpu import pipeline_oracle
    W, H = sc.SIZES[0]
    prev, curr = sc.pair(W, H, sc.FLOWS[2])
    pts = sc.pipeline_points(W, H)
    prm = vio.default_tracker_params(max_corners=200, seed=21)
    klt = vio.default_klt_params()
    assert vio.seam_check(W, H, klt.win, klt.max_level, prm.min_dist) == OK
    nxt, st, kept, corners, crossing = so.pipeline_oracle(vio, prev, curr, pts, prm, klt)
    assert kept.sum() > 40 and crossing >= 1
    assert ((corners[:, 0] < prm.min_dist) | (corners[:, 0] >= W - prm.min_dist)).any()
    flat = pipeline_oracle(vio, prev, curr, pts, prm, klt)
    assert not np.array_equal(kept, flat[2]) and not np.array_equal(corners, flat[3])


def test_frontend_oracle_carries_ids_across_the_seam(vio):
    """six frames of the texture rolled by 9 px per frame (a pure yaw): with wrap some ids are seen right of the
    seam and later left of it with a growing track count; the flat front end never sees an id on both sides"""
    import frontend_oracle as fo
    W, H = sc.SIZES[0]
    base = sc.pair(W, H, sc.FLOWS[0])[0]
    prm = vio.default_frontend_params(seed=3)
    m = prm.boundary_margin
    for cls, expect in ((so.SeamFrontendOracle, True), (fo.FrontendOracle, False)):
        orc = cls(vio, W, H, prm)
        right, crossed = {}, set()
        for f in range(6):
            o = orc.track(np.roll(base, 9 * f, axis=1))
            for i, (x, _), tc in zip(o["ids"], o["xy"], o["track_count"]):
                if x > W - m:
                    right[int(i)] = int(tc)
                elif x < m and int(i) in right:
                    assert tc > right[int(i)]
                    crossed.add(int(i))
        assert bool(crossed) == expect, cls.__name__
