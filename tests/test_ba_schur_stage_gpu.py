"""The phase route's Schur kernel with a group's landmark values and rhs column kept in LDS (the staged
instance) and its fallback, at the smallest shapes where either can go wrong (tests/schur_stage_cases.py):
second chunks and second groups of one landmark, constant landmarks at the first and last slots of a chunk
and of a group, missing observations, outliers, T = 1 / 2 / 4 / 6, VI and visual-only windows, and mixed
batches of 8, 9 and 16 windows.  The route is forced with set_ba_route(ROUTE_PHASES), the group size with
VIO_BA_SCHUR_GS (read at every pack).

Each window is compared with the CPU oracle through test_ba_gpu.py's fixed-iteration parity checks and
tolerances, and a window's result inside its batch must be bitwise its result solved alone at the same
group size.  In the last run the batch takes the unstaged kernel and two of its windows alone the staged one,
so that comparison also pins the staged instance bitwise to the unstaged body.  The oracle's solutions are
computed once for the module; a CPU test first confirms the oracle solves every case."""
import math

import numpy as np
import pytest

import oracle_lib
import schur_stage_cases as ssc
from test_ba_gpu import assert_parity

KEYS = ("T_wb", "lm_xyz", "obs_chi2", "obs_outlier", "vel", "bg", "ba")


@pytest.fixture(scope="module")
def shapes(vio, synth):
    cases = ssc.build(vio, synth)
    probs = ssc.problems(vio, cases)
    ref = [oracle_lib.ba_solve(vio, p) for p in probs]
    for r in ref:  # shared by the tests below: read-only
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return cases, probs, ref


def test_cases_cover_the_shapes_and_the_oracle_solves_them(vio, shapes):
    cases, probs, ref = shapes
    assert [(p.K, p.L) for p in probs] == [(10, 26), (10, 26), (10, 51), (3, 86), (16, 17), (4, 65), (10, 500)]
    assert sorted(len(idx) for _, idx in ssc.RUNS)[-3:] == [8, 9, 16]
    assert {i for _, idx in ssc.RUNS for i in idx} == set(range(len(cases)))
    variants = {var for _, _, var, _ in cases}
    assert vio.VIO_BA_VI in variants and variants & {vio.VIO_BA_LOCAL, vio.VIO_BA_FULL}
    for (name, w, var, _), p, o in zip(cases, probs, ref):
        assert o["success"] == 1, name
        assert math.isfinite(o["initial_cost"]) and math.isfinite(o["final_cost"]), name
        assert o["final_cost"] < o["initial_cost"], (name, o["initial_cost"], o["final_cost"])
        assert o["iterations"] == p.c.max_iterations + 1, name
    name, w, _, _ = cases[2]
    p, o = probs[2], ref[2]
    assert list(np.nonzero(w["lm_const"])[0]) == [0, 24, 25, 49, 50], name
    assert 0.55 * p.K * p.L <= p.N <= 0.75 * p.K * p.L, (name, p.N)   # about a third missing
    assert o["obs_outlier"][:p.N].any(), name


@pytest.mark.gpu
@pytest.mark.parametrize("ri", range(len(ssc.RUNS)))
def test_phase_route_matches_oracle_and_solo_bitwise(vio, gpu_ctx, shapes, monkeypatch, ri):
    cases, probs, ref = shapes
    gs, idx = ssc.RUNS[ri]
    monkeypatch.setenv("VIO_BA_SCHUR_GS", str(gs))
    gpu_ctx.set_ba_route(gpu_ctx.ROUTE_PHASES)
    try:
        batch = gpu_ctx.ba_solve([probs[i] for i in idx])
        solo = {i: gpu_ctx.ba_solve([probs[i]])[0] for i in sorted(set(idx))}
    finally:
        gpu_ctx.set_ba_route(gpu_ctx.ROUTE_AUTO)
    for i, g in zip(idx, batch):
        name, p, o, s = cases[i][0], probs[i], ref[i], solo[i]
        print(name, "gs", gs, "oracle", o["final_cost"], "gpu", g["final_cost"], "steps", g["num_successful_steps"],
              g["num_unsuccessful_steps"], "|dlm|", np.abs(o["lm_xyz"] - g["lm_xyz"]).max())
        assert o["iterations"] == g["iterations"] == p.c.max_iterations + 1, name
        assert (o["num_successful_steps"], o["num_unsuccessful_steps"]) == \
            (g["num_successful_steps"], g["num_unsuccessful_steps"]), name
        assert_parity(o, g, p.c.chi2_threshold, iters_tol=0)
        for key in KEYS:
            assert np.array_equal(g[key], s[key]), (name, key)
        assert g["final_cost"] == s["final_cost"] and g["initial_cost"] == s["initial_cost"], name
