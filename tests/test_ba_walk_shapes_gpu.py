"""The phase route's walk kernels at the smallest (K, L) shapes where their lane geometry and offsets can go
wrong (tests/walk_shape_cases.py: one chunk exactly, one landmark over, ragged last chunks; K = 2 .. 16;
missing observations, outliers, constant landmarks, the constant first keyframe), forced onto the phase
kernels with vio_ctx_set_ba_route(VIO_BA_ROUTE_PHASES), in batches of 3, 2 and 1 windows of mixed shapes.

Each window is compared with the CPU oracle through test_ba_gpu.py's fixed-iteration parity checks and
tolerances, and a window's result inside its batch must be bitwise its result solved alone.  The oracle's
solutions are computed once for the module; a CPU test first confirms the oracle solves every case."""
import math

import numpy as np
import pytest

import oracle_lib
import walk_shape_cases as wsc
from test_ba_gpu import assert_parity

KEYS = ("T_wb", "lm_xyz", "obs_chi2", "obs_outlier", "vel", "bg", "ba")


@pytest.fixture(scope="module")
def shapes(vio, synth):
    cases, batches = wsc.build(vio, synth)
    probs = wsc.problems(vio, cases)
    ref = [oracle_lib.ba_solve(vio, p) for p in probs]
    for r in ref:  # shared by the tests below: read-only
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return cases, batches, probs, ref


def test_cases_cover_the_shapes_and_the_oracle_solves_them(vio, shapes):
    cases, batches, probs, ref = shapes
    got = sorted((p.K, p.L) for p in probs)
    assert got == [(2, 1), (3, 85), (3, 86), (7, 71), (10, 26), (16, 17)], got
    assert sorted(len(b) for b in batches) == [1, 2, 3] and sorted(sum(batches, [])) == list(range(len(cases)))
    variants = {var for _, _, var in cases}
    assert vio.VIO_BA_VI in variants and variants & {vio.VIO_BA_LOCAL, vio.VIO_BA_FULL}
    thinned = flagged = const_lm = 0
    for (name, w, var), p, o in zip(cases, probs, ref):
        assert o["success"] == 1, name
        assert math.isfinite(o["initial_cost"]) and math.isfinite(o["final_cost"]), name
        assert o["final_cost"] < o["initial_cost"], (name, o["initial_cost"], o["final_cost"])
        assert o["iterations"] == p.c.max_iterations + 1, name
        assert w["kf_const"][0] == 1 and not w["kf_const"][1:].any(), name   # the constant first keyframe
        if p.N > 2:
            thinned += 0.55 * p.K * p.L <= p.N <= 0.75 * p.K * p.L           # about a third missing
        flagged += bool(o["obs_outlier"][:p.N].any())
        const_lm += bool(np.asarray(w["lm_const"]).any())
    assert thinned >= 3 and flagged >= 3 and const_lm >= 2, (thinned, flagged, const_lm)


@pytest.mark.gpu
@pytest.mark.parametrize("bi", range(3))
def test_phase_route_matches_oracle_and_solo_bitwise(vio, gpu_ctx, shapes, bi):
    cases, batches, probs, ref = shapes
    idx = batches[bi]
    gpu_ctx.set_ba_route(gpu_ctx.ROUTE_PHASES)
    try:
        batch = gpu_ctx.ba_solve([probs[i] for i in idx])
        solo = [gpu_ctx.ba_solve([probs[i]])[0] for i in idx]
    finally:
        gpu_ctx.set_ba_route(gpu_ctx.ROUTE_AUTO)
    for i, g, s in zip(idx, batch, solo):
        name, p, o = cases[i][0], probs[i], ref[i]
        print(name, "oracle", o["final_cost"], "gpu", g["final_cost"], "steps", g["num_successful_steps"],
              g["num_unsuccessful_steps"], "|dlm|", np.abs(o["lm_xyz"] - g["lm_xyz"]).max())
        assert o["iterations"] == g["iterations"] == p.c.max_iterations + 1, name
        assert (o["num_successful_steps"], o["num_unsuccessful_steps"]) == \
            (g["num_successful_steps"], g["num_unsuccessful_steps"]), name
        assert_parity(o, g, p.c.chi2_threshold, iters_tol=0)
        for key in KEYS:
            assert np.array_equal(g[key], s[key]), (name, key)
        assert g["final_cost"] == s["final_cost"] and g["initial_cost"] == s["initial_cost"], name
