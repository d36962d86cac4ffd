"""IMU initialisation: Optimizer::OptimizeIMUInit (src/optimization/Optimizer.cpp:972-1257)
over InertialGravityScaleFactor (Factors.cpp:981-1293) and BiasPriorFactor (Factors.h:366-396).

CPU: the oracle (oracle_imu_init) on a known-answer case — a stationary, tilted IMU: every factor is
exact at gravity = the body-frame gravity, zero velocities and biases (the pose blocks enter the
factor as identity, Factors.cpp:1024-1042, so the answer lives in the body frame) — and its guards.
The reference's own tests do not cover this path and Ceres cannot be run beside it, so
the oracle is pinned by tests/imu_init_reference.py, a float64 restatement of the minimised cost
written from the reference source alone: on every case of tests/imu_init_cases.py the oracle's
initial and final cost equal the restated cost at the oracle's own parameters (1e-12 relative), a
derivative-free polish started at its answer finds nothing lower beyond the recorded drops (so the
oracle's Jacobians and LM loop end at a minimum of the right function), and frames that no factor
touches keep the velocity initialisation to the bit.
GPU: vio_imu_init_solve against the oracle on synthetic VIO windows and the KAT, batched; per case
of the table (up to the 64-frame bound: every `j += 64` loop over stage-2 columns takes 2 to 4
trips), in one mixed batch, after the 65-frame reject, and fed by the device preintegration."""
import numpy as np
import pytest

import imu_init_cases as cases
import imu_init_reference as ref
import oracle_lib

G = 9.81
FIELDS = ("gravity_dir", "gyro_bias", "accel_bias", "velocities", "gravity")


def rot(axis, deg):
    a = np.asarray(axis, float) / np.linalg.norm(axis)
    t = np.radians(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * K @ K


def stationary_frames(F=6, dt=0.1, tilt=(1.0, 0.5, 0.0), tilt_deg=4.0, seed=0):
    """A stationary IMU rotated by R_wb: specific force R_bw * (0, 0, +g), so the preintegrated
    dV = -g_b dt, dP = -g_b dt^2 / 2 with g_b = R_bw (0, 0, -g), dR = I."""
    rng = np.random.default_rng(seed)
    R_wb = rot(tilt, tilt_deg)
    g_b = R_wb.T @ np.array([0.0, 0.0, -G])
    T = np.tile(np.eye(4), (F, 1, 1))
    T[:, :3, :3] = R_wb
    pre = [None]
    for _ in range(1, F):
        pre.append({
            "delta_R": np.eye(3, dtype=np.float32), "delta_V": (-g_b * dt).astype(np.float32),
            "delta_P": (-0.5 * g_b * dt * dt).astype(np.float32),
            "J_Rg": (-dt * np.eye(3) + rng.normal(0, 1e-4, (3, 3))).astype(np.float32),
            "J_Vg": rng.normal(0, 1e-3, (3, 3)).astype(np.float32), "J_Va": (-dt * np.eye(3)).astype(np.float32),
            "J_Pg": rng.normal(0, 1e-4, (3, 3)).astype(np.float32),
            "J_Pa": (-0.5 * dt * dt * np.eye(3)).astype(np.float32),
            "cov": (np.eye(15) * 1e-4).astype(np.float32), "gyro_bias": np.zeros(3, np.float32),
            "accel_bias": np.zeros(3, np.float32), "dt_total": dt})
    return {"T_wb": T, "preint": pre}, g_b


def window_frames(synth, seed):
    w = synth.config3(seed)
    return {"T_wb": w["T_wb_init"], "preint": w["preint"]}


def test_oracle_stationary_kat(vio):
    fr, g_b = stationary_frames()
    r = oracle_lib.imu_init(vio, vio.abi.ImuInitProblem(fr))
    assert r["success"] == 1 and r["status"] == 0
    # gravity = R_wg (0, 0, -9.81) recovers the body-frame gravity (f32 inputs: ~1e-6)
    np.testing.assert_allclose(r["gravity"], g_b, rtol=0, atol=1e-4)
    # the quirky velocity initialisation R_wb_prev * dV = (0, 0, g dt) is matched in stage 1 by
    # scale -> 0; with scale ~ 0 the velocities are unobservable in stage 2: only s * v is pinned
    np.testing.assert_allclose(r["scale"] * r["velocities"], 0.0, atol=1e-6)
    np.testing.assert_allclose(r["gyro_bias"], 0.0, atol=1e-4)
    np.testing.assert_allclose(r["accel_bias"], 0.0, atol=1e-4)
    assert r["final_cost"] < 1e-8
    np.testing.assert_allclose(r["Rwg"] @ r["Rwg"].T, np.eye(3), atol=1e-12)


def test_oracle_guards(vio):
    fr, _ = stationary_frames(F=3)
    two = {"T_wb": fr["T_wb"][:2], "preint": fr["preint"][:2]}
    r = oracle_lib.imu_init(vio, vio.abi.ImuInitProblem(two))
    assert r["success"] == 0 and r["status"] == vio.abi.VIO_IMU_INIT_FEW_FRAMES
    assert r["scale"] == 1.0 and r["gravity"][2] == pytest.approx(-9.81, abs=1e-6)
    miss = {"T_wb": fr["T_wb"], "preint": [None, fr["preint"][1], None]}
    assert oracle_lib.imu_init(vio, vio.abi.ImuInitProblem(miss))["status"] == vio.abi.VIO_IMU_INIT_NO_PREINT
    long_dt = {"T_wb": fr["T_wb"], "preint": [None] + [dict(p, dt_total=2.5) for p in fr["preint"][1:]]}
    r = oracle_lib.imu_init(vio, vio.abi.ImuInitProblem(long_dt))
    assert r["status"] == vio.abi.VIO_IMU_INIT_NO_FACTORS and r["success"] == 0


def test_oracle_window_runs_both_stages(vio, synth):
    """A config-3 window's preintegrations: both stages run, the stage-2 cost does not exceed the
    stage-1 initial cost, the velocity initialisation R_wb_prev * delta_V feeds stage 2."""
    r = oracle_lib.imu_init(vio, vio.abi.ImuInitProblem(window_frames(synth, synth.SEED)))
    assert r["success"] == 1
    assert all(1 <= it <= 51 for it in r["iterations"])
    assert r["final_cost"] <= r["initial_cost"]
    assert abs(np.linalg.norm(r["gravity"]) - 9.81) < 1e-9


# ---------------------------------------------------------------------------------------------
# the oracle against the independent restatement (tests/imu_init_reference.py), per case
@pytest.fixture(scope="module")
def solved(vio, synth):
    """name -> (frames, kwargs, problem, the CPU oracle's result): built and solved once per
    module, shared read-only by the CPU and GPU tests."""
    cache = {}

    def get(name):
        if name not in cache:
            _, fr, kw = cases.build(synth, name)
            p = vio.abi.ImuInitProblem(fr, **kw)
            cache[name] = (fr, kw, p, oracle_lib.imu_init(vio, p))
        return cache[name]
    return get


def _ref_kw(kw):
    return {k: v for k, v in kw.items() if k != "max_iterations"}


def assert_cost_identity(fr, kw, res):
    """The reported costs are the restated cost at the reported parameters.  1e-12 relative is 200
    times the 5e-15 that summation order and libm leave between two float64 evaluations; the floor
    covers the stationary cases' costs of ~1e-16 (measured difference there: 1e-23)."""
    for what, got, want in (("initial", res["initial_cost"], ref.cost_initial(fr, **_ref_kw(kw))),
                            ("final", res["final_cost"], ref.cost_at(fr, res, 2, **_ref_kw(kw)))):
        print(f"{what}_cost {got!r} restated {want!r} diff {abs(got - want):.3e}")
        assert abs(got - want) <= 1e-12 * want + 1e-20, what


def assert_untouched_keep_vinit(fr, res):
    free = ref.touched(fr)
    np.testing.assert_array_equal(res["velocities"][~free], ref.vinit(fr)[~free])


def test_case_table_shapes(synth):
    """n2 / m2 as the table states them; every window case is past the wave (n2 > 64)."""
    for name in cases.NAMES:
        _, fr, _ = cases.build(synth, name)
        n2, m2 = 3 * int(ref.touched(fr).sum()) + 6, 9 * len(ref.kept(fr)) + 6
        assert (n2, m2) == cases.TABLE[name][:2], name
        assert n2 > 64
    assert sorted(cases.TABLE[n][0] // 64 for n in ("win20", "win43", "win64")) == [1, 2, 3]


@pytest.mark.parametrize("name", cases.NAMES)
def test_oracle_cost_identity(solved, name):
    fr, kw, _, o = solved(name)
    assert o["status"] == 0 and o["success"] == 1
    assert_cost_identity(fr, kw, o)


@pytest.mark.parametrize("name,stage", [(n, s) for n in cases.NAMES for s in (1, 2)
                                        if cases.TABLE[n][1 + s] is not None])
def test_oracle_answer_is_stationary(solved, name, stage):
    """A finite-difference least-squares polish over the stage's free parameters, started at the
    oracle's answer, lowers the restated cost by at most ten times the relative drop recorded in
    the case table (plus the cost identity's own resolution, below which a drop is rounding)."""
    fr, kw, _, o = solved(name)
    assert o["termination"][stage - 1] == 0
    c0, c1 = ref.polish(fr, o, stage, **_ref_kw(kw))
    print(f"stage {stage}: cost {c0!r} polished {c1!r} relative drop {(c0 - c1) / c0 if c0 else 0.0:.3e}")
    assert c1 <= c0  # the minimiser itself: never worse than where it started
    assert c0 - c1 <= 10.0 * cases.TABLE[name][1 + stage] * c0 + (1e-12 * c0 + 1e-20)


def test_oracle_skip_rules(solved):
    """Frames no kept factor touches stay out of stage 2 and keep vinit exactly; dt_total <= 0.001
    zeroes vinit but (0.0005 aside) does not by itself drop a frame."""
    seen = 0
    for name in cases.NAMES:
        fr, _, _, o = solved(name)
        assert_untouched_keep_vinit(fr, o)
        seen += int((~ref.touched(fr)).sum())
    assert seen == 3  # skip_mid: frame 7, skip_first: frame 0, skip_last: frame 23
    fr, _, _, o = solved("skip_mid")
    assert ref.kept(fr) == [i for i in range(23) if i not in (6, 7)]
    assert not ref.touched(fr)[7] and np.any(ref.vinit(fr)[7] != 0.0)
    np.testing.assert_array_equal(ref.vinit(fr)[8], 0.0)
    assert ref.touched(fr)[8] and np.any(o["velocities"][8] != 0.0)
    assert not ref.touched(solved("skip_first")[0])[0] and not ref.touched(solved("skip_last")[0])[23]


def test_oracle_iteration_caps(solved):
    o = solved("huber24_cap4")[3]
    assert o["iterations"] == [5, 5] and o["termination"] == [1, 1] and o["success"] == 1
    o = solved("win24_cap0")[3]
    assert o["iterations"] == [1, 1] and o["termination"] == [1, 1] and o["success"] == 1
    assert o["final_cost"] == pytest.approx(o["initial_cost"], rel=1e-12) and o["scale"] == 1.0
    # the Huber cases are long solves; the plain windows are not
    assert min(solved("huber24")[3]["iterations"]) >= 8 and min(solved("huber24_d05")[3]["iterations"]) >= 20
    assert solved("win64")[3]["iterations"] == [3, 2]


def assert_parity(g, o, tol=1e-9, field_tol=None):
    """field_tol: {field: tol} replacing tol for single fields (see cloud_tolerances)."""
    ft = field_tol or {}
    assert g["status"] == o["status"] and g["success"] == o["success"]
    if o["status"]:
        return
    assert g["iterations"] == o["iterations"] and g["termination"] == o["termination"]
    for k in FIELDS:
        np.testing.assert_allclose(g[k], o[k], rtol=ft.get(k, tol), atol=ft.get(k, tol) * 10, err_msg=k)
    assert g["scale"] == pytest.approx(o["scale"], rel=ft.get("scale", tol))
    assert g["initial_cost"] == pytest.approx(o["initial_cost"], rel=tol)
    assert g["final_cost"] == pytest.approx(o["final_cost"], rel=1e-7, abs=1e-12)


@pytest.mark.gpu
def test_gpu_matches_oracle_batched(vio, synth):
    ctx = vio.Context(0)
    try:
        frames = [window_frames(synth, synth.SEED + k) for k in range(4)]
        frames += [stationary_frames(F=3 + k, seed=k)[0] for k in range(4)]
        frames.append({"T_wb": frames[0]["T_wb"][:2], "preint": frames[0]["preint"][:2]})  # guard inside a batch
        probs = [vio.abi.ImuInitProblem(f) for f in frames]
        got = ctx.imu_init(probs)
        for k, p in enumerate(probs):
            assert_parity(got[k], oracle_lib.imu_init(vio, p))
    finally:
        ctx.close()


@pytest.mark.gpu
def test_gpu_stationary_kat(vio):
    ctx = vio.Context(0)
    try:
        fr, g_b = stationary_frames(F=10, tilt=(0.2, -1.0, 0.3), tilt_deg=7.0)
        r = ctx.imu_init([vio.abi.ImuInitProblem(fr)])[0]
        assert r["success"] == 1
        np.testing.assert_allclose(r["gravity"], g_b, rtol=0, atol=1e-4)
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------
# GPU: the case table, a mixed batch, the frame bound, the device preintegration chain
@pytest.fixture(scope="module")
def ctx(vio):
    c = vio.Context(0)
    yield c
    c.close()


def cloud_tolerances(vio, fr, kw, o, tol=1e-9):
    """Conditioning of the solve, CPU oracle only: gravity_magnitude and the T_wb rotations scaled by
    (1 +- 1e-15) and (1 +- 3e-15).  A field that this cloud moves by more than a tenth of its
    tolerance is not determined to that tolerance by the inputs, and gets ten times its cloud spread
    for this case (measured: only `scale` on the stationary cases, where scale -> 0); every other
    field keeps tol.  Nothing here looks at the GPU's output."""
    spread = dict.fromkeys(FIELDS + ("scale",), 0.0)
    for e in (1e-15, -1e-15, 3e-15, -3e-15):
        T = fr["T_wb"].copy()
        T[:, :3, :3] *= 1.0 + e
        gm = kw.get("gravity_magnitude", 9.81)
        for f2, kw2 in (({"T_wb": T, "preint": fr["preint"]}, kw), (fr, dict(kw, gravity_magnitude=gm * (1.0 + e)))):
            c = oracle_lib.imu_init(vio, vio.abi.ImuInitProblem(f2, **kw2))
            assert c["iterations"] == o["iterations"] and c["termination"] == o["termination"]
            for k in FIELDS:  # in units of assert_parity's rtol / atol pair at tol
                spread[k] = max(spread[k], float(np.max(np.abs(c[k] - o[k]) / (tol * 10 + tol * np.abs(o[k])))))
            spread["scale"] = max(spread["scale"], abs(c["scale"] - o["scale"]) / (tol * abs(o["scale"])))
    return {k: 10.0 * s * tol for k, s in spread.items() if s > 0.1}


def _case_parity(vio, ctx, solved, name):
    fr, kw, p, o = solved(name)
    g = ctx.imu_init([p])[0]
    ft = cloud_tolerances(vio, fr, kw, o)
    print(name, "iterations", g["iterations"], "termination", g["termination"], "widened", ft)
    assert_parity(g, o, field_tol=ft)
    assert_untouched_keep_vinit(fr, g)
    np.testing.assert_array_equal(g["velocities"][~ref.touched(fr)], o["velocities"][~ref.touched(fr)])
    assert_cost_identity(fr, kw, g)  # the GPU's costs at the GPU's parameters


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in cases.NAMES if n != "win64"])
def test_gpu_case_parity(vio, ctx, solved, name):
    _case_parity(vio, ctx, solved, name)


def assert_bitwise(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


def _mixed_batch(vio, synth, solved):
    few = cases.frames_of(synth, 20)
    none = stationary_frames(F=3)[0]
    none["preint"] = [None] + [dict(p, dt_total=2.5) for p in none["preint"][1:]]
    probs = [vio.abi.ImuInitProblem(stationary_frames(F=3, seed=1)[0]), solved("win64")[2], solved("win20")[2],
             vio.abi.ImuInitProblem({"T_wb": few["T_wb"][:2], "preint": few["preint"][:2]}), solved("win21")[2],
             vio.abi.ImuInitProblem(cases.frames_of(synth, 10)), vio.abi.ImuInitProblem(none), solved("win43")[2]]
    assert [p.F for p in probs] == [3, 64, 20, 2, 21, 10, 3, 43]
    return probs


@pytest.mark.gpu
def test_gpu_mixed_batch_bitwise(vio, synth, ctx, solved):
    """Problems of very different sizes (and two that the host answers) in one launch: per-problem
    scratch offsets and their rounding.  Each must equal the same problem solved alone, and the same
    batch again after a one-problem call has shrunk the arena's use — GPU against GPU, bitwise."""
    probs = _mixed_batch(vio, synth, solved)
    batch = ctx.imu_init(probs)
    st = [r["status"] for r in batch]
    assert st == [0, 0, 0, vio.abi.VIO_IMU_INIT_FEW_FRAMES, 0, 0, vio.abi.VIO_IMU_INIT_NO_FACTORS, 0]
    for k, p in enumerate(probs):
        assert_bitwise(batch[k], ctx.imu_init([p])[0])
    assert_bitwise(ctx.imu_init(probs[:1])[0], batch[0])
    again = ctx.imu_init(probs)
    for a, b in zip(again, batch):
        assert_bitwise(a, b)
    for k, name in ((1, "win64"), (2, "win20"), (4, "win21"), (7, "win43")):  # right, not only repeatable
        assert_parity(batch[k], solved(name)[3])


@pytest.mark.gpu
def test_gpu_frame_bound(vio, ctx, solved):
    """64 frames is the bound (the win64 case); 65 is rejected with VIO_EINVAL before anything is
    launched, alone or at the end of a batch, and the context goes on solving."""
    big = vio.abi.ImuInitProblem(stationary_frames(F=65)[0])
    for probs in ([big], [solved("win20")[2], big]):
        with pytest.raises(vio.VioError, match=r"\(-22\)"):
            ctx.imu_init(probs)
    assert_parity(ctx.imu_init([solved("win20")[2]])[0], solved("win20")[3])


@pytest.mark.gpu
def test_gpu_device_preintegration_chain(vio, synth, ctx):
    """vio_imu_preintegrate's factors of a 21-frame window fed to vio_imu_init_solve: the same as the
    CPU preintegration oracle's factors fed to the CPU oracle."""
    from test_imu_gpu import _as_dicts
    K = 21
    w = cases.window(synth, K)
    t0 = np.r_[-1.0, synth.KF_DT * np.arange(K - 1)]  # entry 0: empty range -> invalid, unused
    t1 = np.r_[-1.0, synth.KF_DT * np.arange(1, K)]
    res = []
    for pre in (ctx.imu_preintegrate, lambda *a: oracle_lib.imu_preintegrate(vio, *a)):
        rec, valid, _ = pre(w["imu_samples"], t0, t1)
        assert valid.tolist() == [0] + [1] * (K - 1)
        res.append(vio.abi.ImuInitProblem({"T_wb": w["T_wb"], "preint": _as_dicts(rec, K)}))
    o = oracle_lib.imu_init(vio, res[1])
    assert o["status"] == 0 and o["iterations"] == [3, 2]
    assert_parity(ctx.imu_init([res[0]])[0], o)


@pytest.mark.gpu
def test_gpu_win64_parity(vio, ctx, solved):
    """The 64-frame bound: n2 = 198 (fourth trip of the column loops), m2 = 573, five QR solves of a
    771 x 198 system by one wave.  Measured wall time of the one-problem call on an MI355X: 0.245 s
    (0.10 s at F = 43, 0.017 s at F = 20), so max_iterations stays at its default."""
    _case_parity(vio, ctx, solved, "win64")
