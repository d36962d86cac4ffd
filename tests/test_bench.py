"""bench.py's command line: a plain run prints the headline line alone, --dump-outputs writes what the
timed path computed in its last step, --full adds the other legs (CPU part: the helpers behind them)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "roofline")
FULL_LEGS = ("single_window", "sustained", "cpu_baseline", "config4_strong", "config4_shard32", "config2",
             "erp_klt", "global_ba", "imu_preint", "triangulation", "frame_resize")


def _same(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, list):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if a is None or b is None:
        return a is b
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and np.array_equal(a, b)


def test_shard_windows_are_the_serial_windows(synth):
    """the pool of host processes generates exactly synth.config3 of the shard's seeds, in order"""
    import bench
    ws = bench.shard_windows(synth, 1, 3)
    assert len(ws) == 3
    for w, seed in zip(ws, bench.shard_seeds(synth.SEED, 1, 3)):
        assert _same(w, synth.config3(seed))


def test_dump_outputs_layout(tmp_path):
    """one float64 file per result field, the windows stacked along axis 0; per-rank names in a multi-rank run"""
    import bench
    rng = np.random.default_rng(0)
    res = []
    for i in range(3):
        r = {"T_wb": rng.normal(size=(2, 4, 4)), "lm_xyz": rng.normal(size=(5, 3)), "vel": rng.normal(size=(2, 3)),
             "bg": rng.normal(size=3), "ba": rng.normal(size=3), "obs_chi2": rng.normal(size=7),
             "obs_outlier": rng.integers(0, 2, 7).astype(np.uint8), "lm_bad": rng.integers(0, 2, 5).astype(np.uint8)}
        r.update({k: i + j for j, k in enumerate(bench.DUMP_SCALARS)})
        res.append(r)
    bench.dump_outputs(str(tmp_path / "d"), res, 0, 1)
    names = sorted(os.listdir(tmp_path / "d"))
    assert names == sorted(f"{n}.npy" for n in bench.DUMP_ARRAYS + bench.DUMP_SCALARS)
    for n in bench.DUMP_ARRAYS + bench.DUMP_SCALARS:
        a = np.load(tmp_path / "d" / f"{n}.npy")
        assert a.dtype == np.float64 and a.shape[0] == 3
        for i in range(3):
            assert np.array_equal(a[i], np.asarray(res[i][n], np.float64))
    bench.dump_outputs(str(tmp_path / "e"), res, 1, 2)
    assert sorted(os.listdir(tmp_path / "e")) == sorted(f"{n}_rank1.npy" for n in bench.DUMP_ARRAYS + bench.DUMP_SCALARS)


@pytest.mark.gpu
def test_plain_run_headline_and_dump(vio, synth, gpu_ctx, tmp_path):
    """a plain run: the headline keys and none of the --full legs, --steps in the line, and the dump is
    bitwise what the same windows give through a BaBatch here (fixed-order reductions: run to run identical)"""
    import bench
    windows, lm_iters = 3, 4
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--windows", str(windows), "--lm-iters", str(lm_iters), "--dump-outputs", str(tmp_path / "d")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert all(k in d for k in HEADLINE) and not any(k in d for k in FULL_LEGS), sorted(d)
    assert d["steps"] == 2 and d["warmup"] == 1 and d["ms_per_step"] > 0
    assert d["value"] == pytest.approx(windows * lm_iters / (d["ms_per_step"] * 1e-3), rel=1e-9)
    probs = bench.make_shard(vio, [synth.config3(s) for s in bench.shard_seeds(synth.SEED, 0, windows)], lm_iters)
    b = vio.BaBatch(gpu_ctx, probs)
    b.run()
    b.sync()
    ref = b.download()
    b.close()
    for n in bench.DUMP_ARRAYS + bench.DUMP_SCALARS:
        a = np.load(tmp_path / "d" / f"{n}.npy")
        assert a.dtype == np.float64 and len(a) == windows
        for i in range(windows):
            assert np.array_equal(a[i], np.asarray(ref[i][n], np.float64)), (n, i)
