"""bench.py — sliding-window BA iterations/s on MI355X (+ CPU oracle baseline, roofline).

Workload (BASELINE.json metric "sliding-window BA iters/sec (10KF x 500pts)", configs 3/4):
each GPU holds a shard of independent VIO windows of config-3 shape (10 KF x 500 landmarks,
5,000 ERP observations, 9 IMU-preintegration factors; RunVIBA semantics) resident in HBM.
One step = one launch that runs exactly --lm-iters Levenberg-Marquardt iterations on every window
of the shard (benchmark mode: Ceres tolerances disabled, the same on the CPU baseline).
value = window-LM-iterations per second summed over all ranks (weak scaling: the per-GPU shard
is fixed; at 8 GPUs x 32 windows the job is config 4's 256 windows — the default shard of 256
windows per GPU fills the 256 CUs).

  python bench.py [--gpus N --steps K --warmup W --windows 256 --lm-iters 10]
  python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N   (one rank per GPU)

A plain run sets up, warms up, times the K steps and prints the headline line (value, ms_per_step, the
roofline of the timed steps).  --dump-outputs DIR writes what the last timed step computed for every
window as DIR/<name>.npy.  --full adds every other leg to the line: the sustained run, the single
window, the CPU oracle baselines, config 4 strong scaling and its 32-window shard, config 2, the
tracker, global BA, IMU, triangulation and resize legs (the --no-* options drop single legs of it).
"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

FP64_PEAK = 78.6e12  # MI355X FP64 vector (= FP64 matrix) peak, AMD spec


TRACKER_PREFIXES = ("pyr_down_kernel", "lk_kernel", "ransac_", "gftt_", "disc_mask_kernel", "rocprim")


def newest_profile(suffix):
    """The newest committed PMC summary profiles/r<round><letters>_<suffix>.json, ordered by its round
    number and session letters (not by file-name order), with its repo-relative path and the commit it
    was recorded at (the summary's "commit" field where the profiling script wrote one): (data, source)
    or (None, None).  The source goes into the bench line next to every traffic figure taken from it."""
    import glob
    import re
    best = None
    for f in glob.glob(os.path.join(ROOT, "profiles", f"r*_{suffix}.json")):
        m = re.match(r"r(\d+)([a-z]*)_", os.path.basename(f))
        if m:
            key = (int(m.group(1)), len(m.group(2)), m.group(2))
            if best is None or key > best[0]:
                best = (key, f)
    if best is None:
        return None, None
    with open(best[1]) as fh:
        d = json.load(fh)
    src = os.path.relpath(best[1], ROOT)
    if d.get("commit"):
        src += f"@{d['commit'][:12]}"
    return d, src


def traffic_fields(pair):
    """{"traffic": bytes, "traffic_source": profile@commit} of a (bytes, source) pair."""
    v, src = pair
    return {"traffic": v, "traffic_source": src}


def pmc_traffic():
    """PMC summary of the whole bench workload (profiles/r*_pmc_traffic.json): (kernels, source)."""
    d, src = newest_profile("pmc_traffic")
    return (d["kernels"], src) if d else (None, None)


def ba_traffic(args):
    """PMC HBM bytes of one 256-window x 10-iteration step of the phase route: every kernel of the
    step's graph, bytes per launch x launches per step (tools/gpu_pmc_ba.sh over tools/ba_batch_run.py
    -> profiles/r*_pmc_traffic_ba.json; a step = one ph_setup_kernel launch).  (bytes, source)."""
    d, src = newest_profile("pmc_traffic_ba")
    if not d or args.windows != 256 or args.lm_iters != 10:
        return None, None
    k = d["kernels"]
    if "ph_setup_kernel" not in k:
        return None, None
    steps = k["ph_setup_kernel"]["dispatches"]
    return sum(v["hbm_bytes_per_launch"] * v["dispatches"] for n, v in k.items() if n.startswith("ph_")) / steps, src


def cfg2_traffic():
    """PMC HBM bytes of one config-2 window solve (10 fixed LM iterations, one window, default route):
    every window-BA kernel's bytes per launch x launches, per solve (tools/gpu_pmc_cfg2.sh over
    tools/ba_batch_run.py -> profiles/r*_pmc_traffic_cfg2.json; a solve = one ph_cluster_kernel or
    ph_setup_kernel launch).  (bytes, source)."""
    d, src = newest_profile("pmc_traffic_cfg2")
    if not d:
        return None, None
    k = d["kernels"]
    head = "ph_cluster_kernel" if "ph_cluster_kernel" in k else "ph_setup_kernel" if "ph_setup_kernel" in k else None
    if head is None:
        return None, None
    return sum(v["hbm_bytes_per_launch"] * v["dispatches"] for n, v in k.items() if n.startswith("ph_")) / \
        k[head]["dispatches"], src


def klt_traffic():
    """PMC HBM bytes of one ERP-KLT pipeline run: per-launch bytes x launches per run (lk_kernel runs once).
    Source: the newest tracker-only summary (tools/gpu_trk_pmc.sh -> profiles/r*_pmc_traffic_klt.json),
    else the bench-wide one.  (bytes, source)."""
    d, src = newest_profile("pmc_traffic_klt")
    if d:
        k = d["kernels"]
    else:
        k, src = pmc_traffic()
    if not k or "lk_kernel" not in k:
        return None, None
    runs = k["lk_kernel"]["dispatches"]
    # every kernel the pipeline launches once or more per run (rocprim: the top-K key sort); the one-off
    # kernels of the standalone GFTT that picks the bench's start points run fewer times and are left out
    return sum(v["hbm_bytes_per_launch"] * v["dispatches"] for n, v in k.items()
               if n.startswith(TRACKER_PREFIXES) and v["dispatches"] >= runs) / runs, src


def sq_mix(route_leg="ph256"):
    """SQ-counter mix of the window-BA step kernels from the newest committed summary
    (tools/gpu_r5_prof.sh -> profiles/r*_pmc_mix.json): per kernel its MFMA-pipe busy share of the chip's
    SIMD cycles while it runs, VALU-issue share and dependency-wait share of its wave cycles.  The dominant
    kernel of the step by time is ph_back (no MFMA work); ph_schur holds the step's MFMA work.
    ({kernel: {...}}, source) or (None, None)."""
    d, src = newest_profile("pmc_mix")
    if not d:
        return None, None
    out = {}
    for k, v in d["kernels"].items():
        leg, _, name = k.partition(":")
        if leg != route_leg or not name.startswith("ph_"):
            continue
        out[name] = {"mfma_busy_frac": v.get("mfma_busy_frac_chip"), "valu_frac": v.get("valu_frac"),
                     "wait_frac": v.get("wait_frac"), "dispatches": v.get("dispatches")}
    return (out or None), src


def kernel_traffic(name):
    """PMC HBM bytes per launch of one kernel from the committed summary: (bytes, source) or (None, None)."""
    k, src = pmc_traffic()
    if not k or name not in k:
        return None, None
    return k[name]["hbm_bytes_per_launch"], src


def ba_flops_per_iter(prob):
    """SURVEY §8(d) counting convention for one LM iteration of one window."""
    K, L, N = prob.K, prob.L, prob.N
    k = np.bincount(prob.obs_lm, minlength=L)
    f = N * (216 + 250 + 100)
    f += int(np.sum(58 + 180 * k + 108 * k * (k + 1)))
    n_imu = int(prob.preint_valid.sum()) if prob.variant == 2 else 0
    f += n_imu * 7332
    n = 6 * int((prob.kf_const == 0).sum()) + (3 * K + 6 if n_imu else 0)
    f += n ** 3 / 3 + 2 * n ** 2
    return float(f)


def shard_seeds(seed0, rank, windows):
    """Window partition of the weak-scaling job: rank r owns windows [r*W, (r+1)*W) of the global
    sequence (seed = seed0 + global window index); no window is shared, no data crosses ranks."""
    return [seed0 + rank * windows + i for i in range(windows)]


def strong_shard(total, rank, world):
    """Config-4 strong scaling: windows [0, total) in contiguous blocks, rank r owning
    [r*total//world, (r+1)*total//world) (256 windows over 8 GPUs: 32 each)."""
    return list(range(rank * total // world, (rank + 1) * total // world))


def gather_records(local, dist, world, max_windows):
    """All-gather of the ranks' packed per-window result records (RCCL on GPU tensors, gloo on CPU
    ones): local is (n_local, record_bytes) uint8, padded here to max_windows rows (zero rows are
    not records); returns the (world * max_windows, record_bytes) gathered tensor."""
    import torch
    n, rb = local.shape
    if n < max_windows:
        local = torch.cat([local, torch.zeros((max_windows - n, rb), dtype=local.dtype, device=local.device)])
    if dist is None:
        return local
    parts = [torch.empty_like(local) for _ in range(world)]
    dist.all_gather(parts, local)
    return torch.cat(parts)


def reduce_max(x, dist, device):
    """Max of a per-rank scalar over all ranks (the slowest rank defines the job time)."""
    if dist is None:
        return x
    import torch
    t = torch.tensor([x], dtype=torch.float64, device=device)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


def _config3_window(seed):
    return importlib.import_module("360_visual_inertial_odometry_amd.synth").config3(seed)


def shard_windows(synth, rank, windows):
    """The shard's config-3 windows (synth.config3 of every seed of shard_seeds: each window is a function
    of its seed alone, ~0.1 s of numpy), generated over a pool of forked host processes.  Call it before
    this process opens the GPU."""
    import multiprocessing
    seeds = shard_seeds(synth.SEED, rank, windows)
    n = min(16, cpu_threads_available(), len(seeds))
    if n <= 1:
        return [synth.config3(s) for s in seeds]
    with multiprocessing.get_context("fork").Pool(n) as pool:
        return pool.map(_config3_window, seeds, chunksize=-(-len(seeds) // (4 * n)))


def make_shard(vio, shard, lm_iters):
    return [vio.BaProblem(w, variant=vio.VIO_BA_VI, max_iterations=lm_iters, fixed_iterations=1) for w in shard]


DUMP_ARRAYS = ("T_wb", "lm_xyz", "vel", "bg", "ba", "obs_chi2", "obs_outlier", "lm_bad")
DUMP_SCALARS = ("success", "termination", "iterations", "num_successful_steps", "num_unsuccessful_steps",
                "num_inliers", "num_outliers", "num_bad_lm", "initial_cost", "final_cost", "fixed_cost")


def dump_outputs(path, res, rank, world):
    """--dump-outputs: the shard's results of the last timed step (BaBatch.download(): what a caller of the
    timed path receives for every window) as <path>/<name>.npy, float64, the windows stacked along axis 0
    (<name>_rank<r>.npy for the shard of rank r in a multi-rank run).  ~60 kB per config-3 window."""
    os.makedirs(path, exist_ok=True)
    tail = "" if world == 1 else f"_rank{rank}"
    for name in DUMP_ARRAYS:
        np.save(os.path.join(path, f"{name}{tail}.npy"), np.stack([np.asarray(r[name], np.float64) for r in res]))
    for name in DUMP_SCALARS:
        np.save(os.path.join(path, f"{name}{tail}.npy"), np.array([r[name] for r in res], np.float64))


def config4_strong(vio, synth, ctx, dist, rank, world, steps, warmup, lm_iters, total=256):
    """Config 4 as SURVEY §8(e) specifies it: `total` windows in contiguous blocks per GPU (256 over 8:
    32 each); one step = the shard's solve (lm_iters LM iterations) + the device pack of its result
    records + ONE all-gather of the records over RCCL (xGMI); rank 0 decodes all `total` records.
    value = total * lm_iters window-iterations per step time (strong scaling: the job is fixed)."""
    import torch
    mine = strong_shard(total, rank, world)
    probs = [vio.BaProblem(synth.config3(synth.SEED + w), variant=vio.VIO_BA_VI, max_iterations=lm_iters,
                           fixed_iterations=1) for w in mine]
    b = vio.BaBatch(ctx, probs)
    rb = b.record_bytes()
    m = -(-total // world)
    dev = torch.device("cuda", torch.cuda.current_device())
    local = torch.zeros((m, rb), dtype=torch.uint8, device=dev)

    def step():
        b.run()
        b.pack(local.data_ptr())
        b.sync()
        return gather_records(local, dist, world, m)

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(steps):
        g = step()
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    el = reduce_max(time.perf_counter() - t0, dist, dev)
    ok = None
    if rank == 0:
        recs = g.cpu().numpy()
        rows = [vio.unpack_record(r) for r in recs if r[:4].view(np.int32)[0] > 0]
        ok = len(rows) == total and all(r["success"] == 1 and r["iterations"] == lm_iters + 1 for r in rows)
    b.close()
    return {"metric": f"config-4 strong scaling: {total} VIO windows over {world} GPU(s), window-LM-iterations/s",
            "value": total * lm_iters * steps / el, "unit": "window-LM-iterations/s", "ms_per_step": el / steps * 1e3,
            "windows_per_gpu": len(mine), "record_bytes": rb, "gathered_bytes": world * m * rb,
            "scaling": "strong", "records_verified": ok,
            "note": "step = shard solve + device pack of per-window result records + one all-gather (RCCL) of "
                    "the records; rank 0 decodes every record"}


def cpu_threads_available():
    """Host threads this process may use: the affinity mask, capped by OMP_NUM_THREADS (the GPU box
    exports its per-GPU CPU share there; os.cpu_count() is the whole machine)."""
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    env = os.environ.get("OMP_NUM_THREADS")
    if env and env.isdigit() and int(env) > 0:
        n = min(n, int(env))
    return max(1, n)


def cpu_model():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_host_info():
    return {"nproc": os.cpu_count(), "threads_available": cpu_threads_available(), "cpu_model": cpu_model()}


def cpu_baseline(vio, synth, lm_iters, seconds):
    """Oracle (C restatement of the reference path) on config-3 windows, fixed iterations, at 1 / 4 /
    all available host threads (Ceres runs num_threads = 4, Optimizer.cpp:79):
      - single window: the threads work inside one solve (oracle_set_threads: OpenMP over the
        observations, the Schur elimination chunks and the back-substitution), as Ceres does;
      - config 4: independent windows over a pool of threads (one window per thread at a time; the
        ctypes call releases the GIL), the CPU counterpart of the GPU's throughput metric.
    value = config-4 throughput at all available threads (the strongest CPU number)."""
    from concurrent.futures import ThreadPoolExecutor
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_lib
    L = oracle_lib.load()
    nthr = cpu_threads_available()
    pool = [vio.BaProblem(synth.config3(synth.SEED + i), variant=vio.VIO_BA_VI, max_iterations=lm_iters,
                          fixed_iterations=1) for i in range(max(8, min(nthr, 64)))]

    def solve(p):
        O = vio.BaOutput(p.K, p.L, p.N)
        rc = L.oracle_ba_solve(C.byref(p.c), C.byref(O.c))
        assert rc == 0

    single = {}
    for T in (1, 4):
        L.oracle_set_threads(T)
        n, t0 = 0, time.perf_counter()
        while n < 2 or time.perf_counter() - t0 < seconds / 4:
            solve(pool[n % len(pool)])
            n += 1
        single[T] = n * lm_iters / (time.perf_counter() - t0)
    L.oracle_set_threads(1)
    multi = {}
    for T in sorted({1, 4, nthr}):
        n, t0 = 0, time.perf_counter()
        with ThreadPoolExecutor(T) as ex:
            while n < 2 * T or time.perf_counter() - t0 < seconds / 6:
                list(ex.map(solve, [pool[(n + i) % len(pool)] for i in range(T)]))
                n += T
        multi[T] = n * lm_iters / (time.perf_counter() - t0)
    return {"value": multi[nthr], "unit": "window-LM-iterations/s", "cores": nthr, "kind": "port",
            **cpu_host_info(),
            "config4_windows_parallel": {str(t): v for t, v in multi.items()},
            "single_window_threads": {str(t): v for t, v in single.items()},
            "sample": f"config-3 VIO windows x {lm_iters} LM iterations through oracle/ba_oracle.c (-O3, OpenMP): "
                      f"single window at 1/4 threads inside the solve (~{seconds / 4:.0f} s each), independent "
                      f"windows over 1/4/{nthr} threads (~{seconds / 6:.0f} s each)"}


def time_batch(batch, reps, warmup=3):
    """Wall time per run of a resident BaBatch (inputs already in HBM) and the HIP-event kernel time."""
    for _ in range(warmup):
        batch.run()
    batch.sync()
    batch.kernel_ms()
    t0 = time.perf_counter()
    for _ in range(reps):
        batch.run()
    batch.sync()
    wall = (time.perf_counter() - t0) / reps
    kms, _ = batch.kernel_ms()
    return wall, kms


def time_solve_call(vio, ctx, probs, reps):
    """Wall time per vio_ba_solve_batched call on host problems (pack + one upload + solve + one download +
    scatter into the caller's buffers), the ctypes structs built once as a C++ host holds its windows; and
    per Python-level Context.ba_solve (which also marshals the structs and converts the results)."""
    call = ctx.ba_solve_call(probs)
    for _ in range(3):
        call()
    t0 = time.perf_counter()
    for _ in range(reps):
        call()
    c_call = (time.perf_counter() - t0) / reps
    ctx.ba_solve(probs)
    t0 = time.perf_counter()
    for _ in range(max(reps // 5, 3)):
        ctx.ba_solve(probs)
    py_call = (time.perf_counter() - t0) / max(reps // 5, 3)
    return c_call, py_call


def config2_bench(vio, synth, ctx, lm_iters, cpu_seconds, want_cpu, windows=256):
    """Config 2 (BASELINE.json configs[1]): visual-only sliding-window BA, 10 KF x 200 landmarks, 2,000
    ERP observations, RunLocalBA semantics (Optimizer.cpp:726-966; first keyframe constant).  Single
    window resident (value) and per vio_ba_solve call (host problem in, results out), a batch of
    `windows` independent windows for throughput, the oracle at 1 / 4 threads on the same window."""
    probs = [vio.BaProblem(synth.config2(synth.SEED + i), variant=vio.VIO_BA_LOCAL, max_iterations=lm_iters,
                           fixed_iterations=1) for i in range(windows)]
    flops = ba_flops_per_iter(probs[0])
    one = vio.BaBatch(ctx, probs[:1])
    wall1, kms1 = time_batch(one, 20)
    res = one.download()[0]
    one.close()
    xfer, _ = time_solve_call(vio, ctx, probs[:1], 50)
    many = vio.BaBatch(ctx, probs)
    wallm, kmsm = time_batch(many, 10)
    many.close()
    out = {
        "metric": "config 2: visual-only sliding-window BA LM iterations/s (10 KF x 200 landmarks, one window)",
        "value": lm_iters / wall1,
        "unit": "LM-iterations/s",
        "ms_per_solve_resident": wall1 * 1e3,
        "kernel_ms": kms1,
        "iters_per_s_with_transfer": lm_iters / xfer,
        "batched": {"windows": windows, "window_iters_per_s": windows * lm_iters / wallm, "ms_per_step": wallm * 1e3},
        "iterations": res["iterations"],
        "roofline": {"bound": "mfma", "achieved": flops * lm_iters / (kms1 * 1e-3) / 1e12, "peak": FP64_PEAK / 1e12,
                     "unit": "TFLOP/s", "frac": flops * lm_iters / (kms1 * 1e-3) / FP64_PEAK, **traffic_fields(cfg2_traffic()),
                     "flops_per_iteration": flops,
                     "note": "one window: latency-bound (the window's serial LM chain); SURVEY §8d flop convention; "
                             "traffic = PMC HBM bytes of one 10-iteration solve (committed profile)"},
        "cpu_baseline": None,
    }
    if want_cpu:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import oracle_lib
        L = oracle_lib.load()
        by_t = {}
        for T in (1, 4):
            L.oracle_set_threads(T)
            n, t0 = 0, time.perf_counter()
            while n < 3 or time.perf_counter() - t0 < cpu_seconds / 4:
                oracle_lib.ba_solve(vio, probs[n % len(probs)])
                n += 1
            by_t[str(T)] = n * lm_iters / (time.perf_counter() - t0)
        L.oracle_set_threads(1)
        out["cpu_baseline"] = {"value": by_t["4"], "unit": "LM-iterations/s", "cores": 4, "kind": "port",
                               **cpu_host_info(), "by_threads": by_t,
                               "sample": f"config-2 windows x {lm_iters} LM iterations through oracle/ba_oracle.c at "
                                         f"1 / 4 threads inside the solve (~{cpu_seconds / 4:.0f} s each; Ceres "
                                         f"num_threads = 4, Optimizer.cpp:79)"}
        out["vs_cpu_4t"] = out["value"] / by_t["4"]
    return out


def shard_bench(vio, synth, ctx, lm_iters, windows=32):
    """The per-rank shard of config 4 at 8 GPUs (256 windows / 8 = 32 windows) timed on
    this GPU: the step time that bounds the 8-GPU strong-scaling run (its all-gather is ~30 us)."""
    probs = [vio.BaProblem(synth.config3(synth.SEED + w), variant=vio.VIO_BA_VI, max_iterations=lm_iters,
                           fixed_iterations=1) for w in range(windows)]
    b = vio.BaBatch(ctx, probs)
    route, wg = b.route()
    wall, kms = time_batch(b, 100)
    b.close()
    return {"windows": windows, "ms_per_step": wall * 1e3, "kernel_ms": kms,
            "window_iters_per_s": windows * lm_iters / wall, "route": route, "workgroups_per_window": wg}


def global_cpu_baseline(vio, synth, w, threads=4):
    """Config 5 on the CPU: the oracle runs ONE LM iteration of the full problem (1000 KF x 50k
    landmarks; dense 5994^2 reduced system) at `threads` threads (Ceres num_threads = 4); the value is
    that iteration's wall time (oracle_iter_seconds: ComputeTrustRegionStep through the step's
    acceptance), without the solve's set-up and IterationZero.  The reduced-system LLT is single-
    threaded, as Eigen's SimplicialLDLT under SPARSE_SCHUR is (schur_complement_solver.cc:319-356)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_lib
    L = oracle_lib.load()
    L.oracle_iter_seconds.argtypes = [C.c_void_p, C.c_int]
    p = vio.BaProblem(w, variant=vio.VIO_BA_FULL, max_iterations=1, fixed_iterations=1)
    L.oracle_set_threads(threads)
    t0 = time.perf_counter()
    oracle_lib.ba_solve(vio, p)
    total = time.perf_counter() - t0
    L.oracle_set_threads(1)
    sec = (C.c_double * 4)()
    n = L.oracle_iter_seconds(sec, 4)
    it = sec[0] if n >= 1 else total
    return {"value": 1.0 / it, "unit": "LM-iterations/s", "cores": threads, "kind": "port", **cpu_host_info(),
            "seconds_per_iteration": it, "solve_seconds": total,
            "sample": f"one LM iteration of config 5 through oracle/ba_oracle.c at {threads} threads "
                      f"(whole 1-iteration solve incl. set-up: {total:.1f} s)"}


def klt_bench(vio, synth, ctx, steps, warmup, cpu_seconds, want_cpu):
    """Config 1: two-frame ERP KLT pair at 3840x1920, 300 corners.  One step = the
    device pipeline erp_tracker_run on frames resident in HBM: pyramids of both frames, LK of the
    300 points, status/polar/boundary filter + 1000-hypothesis rotation RANSAC, GFTT re-detection
    on frame 2 masked by the kept points."""
    W, H = 3840, 1920
    a, b, _ = synth.config1(W, H)
    mask = np.zeros((H, W), np.uint8)
    mask[int(np.float32(H) * np.float32(0.15)):int(np.float32(H) * np.float32(0.85)), 20:W - 20] = 255
    pts = ctx.gftt(a, mask, 300, float(np.float32(0.01)), 30.0)
    prm = vio.default_tracker_params(max_corners=300, seed=1)
    t = vio.Tracker(ctx, W, H, max_points=512, max_corners=512)
    t.upload(0, a)
    t.upload(1, b)
    t.set_points(pts)
    for _ in range(warmup):
        t.run(prm)
    t.sync()
    # timed steps record only the pipeline's start / end events (each extra stage marker costs the
    # stream a few microseconds); the stage breakdown comes from a separate set of runs with markers
    t.set_stage_timing(False)
    total = 0.0
    t0 = time.perf_counter()
    for _ in range(steps):
        t.run(prm)
        t.sync()
        total += t.stage_ms()["total"] / steps
    wall = (time.perf_counter() - t0) / steps
    t.set_stage_timing(True)
    stage = {k: 0.0 for k in ("pyramids", "lk", "ransac", "gftt", "total")}
    for _ in range(steps):
        t.run(prm)
        t.sync()
        for k, v in t.stage_ms().items():
            stage[k] += v / steps
    stage["total_with_stage_markers"] = stage.pop("total")
    stage["total"] = total
    res = t.download()
    fb = t.gftt_fallbacks()
    t.close()
    mpx = W * H / 1e6
    alg_bytes = 2.0 * W * H  # each u8 frame read once
    out = {
        "metric": "ERP-KLT Mpx/s (config 1: 3840x1920 pair, 300 corners)",
        "value": mpx / wall,
        "unit": "Mpx/s",
        "ms_per_step": wall * 1e3,
        "device_ms_per_step": stage["total"],
        "stage_ms": stage,
        "tracked": int(res["status"].sum()),
        "gftt_fallbacks": dict(zip(("exact_tail", "full_sort"), fb)),
        "kept": int(res["kept"].sum()),
        "new_corners": int(len(res["corners"])),
        "roofline": {
            "bound": "hbm",
            "achieved": alg_bytes / (stage["total"] * 1e-3) / 1e9,
            "peak": 8000.0,
            "unit": "GB/s",
            "frac": alg_bytes / (stage["total"] * 1e-3) / 8.0e12,
            **traffic_fields(klt_traffic()),
            "note": "algorithmic 2 B/px (both u8 frames read once) over the whole pipeline's device time; "
                    "traffic = PMC HBM bytes of one pipeline run (all tracker kernels, committed profile)",
        },
        "cpu_baseline": None,
    }
    if want_cpu:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import oracle_lib
        kp = vio.default_klt_params()
        L = oracle_lib.load()
        nthr = cpu_threads_available()
        by_t = {}
        for T in sorted({1, 4, nthr}):
            L.oracle_set_threads(T)
            n, busy = 0, 0.0
            while busy < cpu_seconds / 3 or n < 1:
                ts = time.perf_counter()
                nxt, st, _ = oracle_lib.klt_track(a, b, pts, kp)
                vr = nxt[:, 1] / np.float32(H)
                good = np.nonzero((st == 1) & (vr >= 0.15) & (vr <= 0.85) & (nxt[:, 0] >= 20) & (nxt[:, 0] <= W - 20))[0]
                s = vio.ransac_samples(1, len(good), 1000)
                km, _ = oracle_lib.rot_ransac(pts[good], nxt[good], W, H, s, vio.ransac_threshold())
                m2 = mask.copy()
                oracle_lib.gftt(b, m2, 300, float(np.float32(0.01)), 30.0)
                busy += time.perf_counter() - ts
                n += 1
            by_t[str(T)] = n * mpx / busy
        L.oracle_set_threads(1)
        out["cpu_baseline"] = {"value": by_t[str(nthr)], "unit": "Mpx/s", "cores": nthr, "kind": "port",
                               **cpu_host_info(), "by_threads": by_t,
                               "sample": f"config-1 frame pairs through oracle/tracker_oracle.c (pyramids+LK+RANSAC+GFTT; "
                                         f"OpenMP over rows / points at 1/4/{nthr} threads, ~{cpu_seconds / 3:.0f} s each)"}
    return out


def gba_traffic():
    """PMC HBM bytes of one config-5 LM iteration from the committed summary (tools/gpu_pmc_gba.sh ->
    profiles/r*_pmc_traffic_gba.json): every kernel's bytes per launch x launches per iteration.
    (bytes, source)."""
    d, src = newest_profile("pmc_traffic_gba")
    return (d.get("hbm_bytes_per_iteration"), src) if d else (None, None)


def global_ba_bench(vio, synth, ctx, lm_iters, want_cpu=False):
    """Config 5: global BA, 1000 KF x 50k landmarks, 500k observations, dense 5994^2 reduced camera
    system (RunBA semantics, fix first).  Timed: one solve of exactly lm_iters LM iterations with
    inputs uploaded once; value = LM iterations per second of that solve."""
    w = synth.make_global()
    p = vio.BaProblem(w, variant=vio.VIO_BA_FULL, max_iterations=lm_iters, fixed_iterations=1)
    p2 = vio.BaProblem(w, variant=vio.VIO_BA_FULL, max_iterations=2 * lm_iters, fixed_iterations=1)
    ctx.ba_solve([p])  # warm-up (allocations, code objects)

    def best_of(prob, reps=3):  # the minimum of a few calls: the host-side part of a call is noisy
        call = ctx.ba_solve_call([prob])  # one C-ABI call per solve on host buffers (structs built once)
        best = None
        for _ in range(reps):
            t0 = time.perf_counter()
            call()
            dt = time.perf_counter() - t0
            if best is None or dt < best:
                best = dt
        return best, call.results()[0]

    wall, r = best_of(p)
    wall2, _ = best_of(p2)
    # per-iteration time with the problem resident: the difference of a 2L- and an L-iteration solve
    # (the host-side assembly, allocation and upload of vio_ba_solve cancel)
    per_iter = max(wall2 - wall, 1e-9) / lm_iters
    flops = ba_flops_per_iter(p)
    return {
        "metric": "global BA LM iterations/s (config 5: 1000 KF x 50k landmarks)",
        "value": 1.0 / per_iter,
        "unit": "LM-iterations/s",
        "ms_per_iteration": per_iter * 1e3,
        "ms_per_solve_call": wall * 1e3,
        "iterations_per_s_whole_call": lm_iters / wall,
        "note": "value: LM iterations per second with the problem resident (time of a 2L-iteration solve "
                "minus an L-iteration solve, / L; each the fastest of 3 calls); whole_call: one vio_ba_solve "
                "C-ABI call on host buffers incl. host assembly, the upload, setup, the final chi2 pass and the "
                "download (the context's arena and captured Cholesky graph reused); fixed iterations",
        "final_cost_ratio": r["final_cost"] / r["initial_cost"],
        "roofline": {"bound": "mfma", "achieved": flops / per_iter / 1e12, "peak": FP64_PEAK / 1e12,
                     "unit": "TFLOP/s", "frac": flops / per_iter / FP64_PEAK, **traffic_fields(gba_traffic()),
                     "flops_per_iteration": flops},
        "cpu_baseline": global_cpu_baseline(vio, synth, w) if want_cpu else None,
    }


def imu_bench(vio, ctx, steps, cpu_seconds, want_cpu):
    """IMU preintegration (the producer of the VIBA factors) for config 4's 256 windows
    x 9 keyframe intervals = 2304 intervals of 50 samples (200 Hz IMU, 4 Hz keyframes) over one
    sorted 576 s stream (synthetic samples).  value = intervals per second of device kernel time."""
    rate, kf_dt, n_int = 200.0, 0.25, 256 * 9
    rng = np.random.default_rng(11)
    m = int(n_int * kf_dt * rate) + 1
    s = np.zeros((m, 7))
    s[:, 0] = np.arange(m) / rate
    tt = s[:, 0]
    s[:, 1:4] = np.stack([0.3 * np.sin(tt), 0.2 * np.cos(0.7 * tt), 9.81 + 0.1 * np.sin(2 * tt)], 1) + rng.normal(0, 1e-2, (m, 3))
    s[:, 4:7] = np.array([0.01, -0.02, 0.14]) + rng.normal(0, 1e-3, (m, 3))
    imu = vio.abi.imu_array(s)
    t0 = kf_dt * np.arange(n_int)
    t1 = t0 + kf_dt
    for _ in range(3):
        ctx.imu_preintegrate(imu, t0, t1)
    kms, t_start = [], time.perf_counter()
    for _ in range(steps):
        rec, valid, _ = ctx.imu_preintegrate(imu, t0, t1)
        kms.append(ctx.imu_kernel_ms())
    wall = (time.perf_counter() - t_start) / steps
    assert valid.all()
    k_ms = float(np.mean(kms))
    alg_bytes = m * 32 + n_int * (16 + 24 + C.sizeof(vio.abi.VioPreint) + 24 + 1)
    out = {
        "metric": "IMU preintegration intervals/s (256 windows x 9 KF intervals, 50 samples each)",
        "value": n_int / (k_ms * 1e-3),
        "unit": "intervals/s",
        "kernel_ms": k_ms,
        "wall_ms_per_call": wall * 1e3,
        "note": "value over the HIP-event kernel time; wall includes the 3.7 MB sample upload and result download",
        "roofline": {"bound": "latency", "achieved": alg_bytes / (k_ms * 1e-3) / 1e9, "peak": 8000.0, "unit": "GB/s",
                     "frac": alg_bytes / (k_ms * 1e-3) / 8.0e12, **traffic_fields(kernel_traffic("imu_preint_kernel")),
                     "note": "one lane per interval: a 50-step dependent f32 chain; 2304 lanes = 36 waves"},
        "cpu_baseline": None,
    }
    if want_cpu:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import oracle_lib
        reps, t_start = 0, time.perf_counter()
        while time.perf_counter() - t_start < cpu_seconds:
            oracle_lib.imu_preintegrate(vio, imu, t0, t1)
            reps += 1
        cpu_s = (time.perf_counter() - t_start) / reps
        out["cpu_baseline"] = {"value": n_int / cpu_s, "unit": "intervals/s", "cores": 1, "kind": "port", **cpu_host_info(),
                               "sample": f"{reps} x 2304 intervals through oracle/imu_oracle.c (1 thread)"}
    return out


def tri_bench(vio, ctx, steps, want_cpu):
    """two-view triangulation (Estimator::TriangulateSinglePoint) of 1 M candidates
    (64 keyframes, random pairs, exact bearings; synthetic) with inputs and outputs resident in HBM
    (vio_triangulate_device).  value = candidates per second of device kernel time."""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import tri_cases
    n = 1 << 20
    T, pairs, B, _ = tri_cases.make_case(n=n, n_poses=64, seed=5)
    dev = torch.device("cuda", torch.cuda.current_device())
    dT = torch.from_numpy(T.reshape(-1, 16)).to(dev)
    dP = torch.from_numpy(pairs).to(dev)
    dB = torch.from_numpy(B).to(dev)
    dX = torch.empty((n, 3), dtype=torch.float32, device=dev)
    dV = torch.empty(n, dtype=torch.uint8, device=dev)
    dE = torch.empty((n, 2), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    args = (dT.data_ptr(), len(T), dP.data_ptr(), dB.data_ptr(), n, 3840, dX.data_ptr(), dV.data_ptr(), dE.data_ptr())
    for _ in range(3):
        ctx.triangulate_device(*args)
        ctx.triangulate_kernel_ms()
    kms = []
    for _ in range(steps):
        ctx.triangulate_device(*args)
        kms.append(ctx.triangulate_kernel_ms())
    k_ms = float(np.mean(kms))
    assert int(dV.sum().item()) == n
    alg_bytes = n * (24 + 8 + 12 + 1 + 8)
    out = {
        "metric": "two-view triangulation candidates/s (1M candidates, 64 keyframes)",
        "value": n / (k_ms * 1e-3),
        "unit": "candidates/s",
        "kernel_ms": k_ms,
        "roofline": {"bound": "hbm", "achieved": alg_bytes / (k_ms * 1e-3) / 1e9, "peak": 8000.0, "unit": "GB/s",
                     "frac": alg_bytes / (k_ms * 1e-3) / 8.0e12, **traffic_fields(kernel_traffic("triangulate_kernel")),
                     "note": "53 B per candidate in/out (poses L2-resident); the f64 one-sided Jacobi "
                             "(~2 kFLOP per candidate) is the actual limiter"},
        "cpu_baseline": None,
    }
    if want_cpu:
        import importlib.util
        spec = importlib.util.spec_from_file_location("tri_oracle", os.path.join(ROOT, "oracle", "tri_oracle.py"))
        tri = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(tri)
        m = 1 << 17
        t_start = time.perf_counter()
        tri.triangulate(T, pairs[:m], B[:m], 3840)
        cpu_s = time.perf_counter() - t_start
        out["cpu_baseline"] = {"value": m / cpu_s, "unit": "candidates/s", "cores": 1, "kind": "port", **cpu_host_info(),
                               "sample": f"{m} candidates through oracle/tri_oracle.py (numpy / LAPACK batched SVD)"}
    return out


def resize_bench(vio, ctx, steps, want_cpu):
    """cv::resize INTER_AREA of the frames (app/main.cpp:203), 3840x1920 -> 960x480,
    64 device-resident frames per launch (synthetic noise frames).  HBM-bound: value = source Mpx/s."""
    import torch
    n, W, H, dW, dH = 64, 3840, 1920, 960, 480
    dev = torch.device("cuda", torch.cuda.current_device())
    src = torch.randint(0, 256, (n, H, W), dtype=torch.uint8, device=dev)
    dst = torch.empty((n, dH, dW), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    args = (src.data_ptr(), W, H, W, n, dst.data_ptr(), dW, dH, dW)
    for _ in range(3):
        ctx.resize_area_device(*args)
        ctx.resize_kernel_ms()
    kms = []
    for _ in range(steps):
        ctx.resize_area_device(*args)
        kms.append(ctx.resize_kernel_ms())
    k_ms = float(np.mean(kms))
    alg = n * (W * H + dW * dH)
    cpu = None
    if want_cpu:
        import importlib.util
        spec = importlib.util.spec_from_file_location("resize_oracle", os.path.join(ROOT, "oracle", "resize_oracle.py"))
        ro = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(ro)
        frame = src[0].cpu().numpy()
        reps, t_start = 0, time.perf_counter()
        while reps < 3 or time.perf_counter() - t_start < 2.0:
            ro.resize_area(frame, dW, dH)
            reps += 1
        cpu = {"value": reps * W * H / (time.perf_counter() - t_start) / 1e6, "unit": "Mpx/s", "cores": 1,
               "kind": "port", "sample": f"{reps} frames through oracle/resize_oracle.py (numpy)"}
    return {
        "metric": "INTER_AREA frame resize Mpx/s (3840x1920 -> 960x480, 64 frames per launch)",
        "value": n * W * H / (k_ms * 1e-3) / 1e6,
        "unit": "Mpx/s",
        "kernel_ms": k_ms,
        "roofline": {"bound": "hbm", "achieved": alg / (k_ms * 1e-3) / 1e9, "peak": 8000.0, "unit": "GB/s",
                     "frac": alg / (k_ms * 1e-3) / 8.0e12, **traffic_fields(kernel_traffic("resize_area4_kernel")),
                     "note": "1 + 1/16 B per source pixel (read once, written at 1/16)"},
        "cpu_baseline": cpu,
    }


def full_legs(vio, synth, ctx, args, world, probs, elapsed, sustained, c4):
    """--full, rank 0: every leg of the line beside the headline (the --no-* options drop single ones)."""
    want_cpu = not args.no_cpu_baseline and world == 1
    # single-window latency (config 3 exactly, one window per launch) for the >=50x CPU target
    one = vio.BaBatch(ctx, probs[:1])
    single_route, single_wg = one.route()
    for _ in range(3):
        one.run()
    one.sync()
    one.kernel_ms()
    t1 = time.perf_counter()
    n1 = 100
    for _ in range(n1):
        one.run()
    one.sync()
    single_wall = (time.perf_counter() - t1) / n1
    single_kms, _ = one.kernel_ms()
    one.close()
    # the same window through vio_ba_solve: host problem in, host result out (upload + solve +
    # download per call, SURVEY §8d's single-window definition)
    single_xfer_wall, single_py_wall = time_solve_call(vio, ctx, probs[:1], n1)
    cpu = cpu_baseline(vio, synth, args.lm_iters, args.cpu_seconds) if want_cpu else None
    gba = None if args.no_global else global_ba_bench(vio, synth, ctx, args.lm_iters, want_cpu)
    c2 = None if args.no_config2 else config2_bench(vio, synth, ctx, args.lm_iters, args.cpu_seconds, want_cpu)
    shard = shard_bench(vio, synth, ctx, args.lm_iters)
    klt = None if args.no_klt else klt_bench(vio, synth, ctx, args.klt_steps, 3, args.cpu_seconds, want_cpu)
    imu = None if args.no_imu else imu_bench(vio, ctx, 20, min(args.cpu_seconds, 3.0), want_cpu)
    tri = None if args.no_tri else tri_bench(vio, ctx, 20, want_cpu)
    rsz = None if args.no_resize else resize_bench(vio, ctx, 20, want_cpu)
    single_ips = args.lm_iters / single_wall
    return {
        "single_window": {
            "config": "config 3 (one window per launch)",
            "iters_per_s_wall": single_ips,
            "iters_per_s_with_transfer": args.lm_iters / single_xfer_wall,
            "ms_per_solve_call": single_xfer_wall * 1e3,
            "iters_per_s_python_call": args.lm_iters / single_py_wall,
            "kernel_ms": single_kms,
            "route": single_route,
            "workgroups": single_wg,
            "vs_cpu_1t": (single_ips / cpu["single_window_threads"]["1"]) if cpu else None,
            "vs_cpu_4t": (single_ips / cpu["single_window_threads"]["4"]) if cpu else None,
            "vs_cpu_4t_with_transfer": (args.lm_iters / single_xfer_wall / cpu["single_window_threads"]["4"])
            if cpu else None,
            "note": "resident = BaBatch re-run on device-resident inputs; with_transfer = one "
                    "vio_ba_solve_batched C-ABI call per solve on host buffers (pack + one pinned upload + solve "
                    "+ one pinned download + scatter; the call's structs built once, as a C++ host holds its "
                    "windows); python_call = Context.ba_solve (ctypes marshalling and result dicts included); "
                    "CPU = the oracle on one window at 1 / 4 threads inside the solve",
        },
        "sustained": sustained,
        "cpu_baseline": cpu,
        "config4_strong": c4,
        "config4_shard32": dict(shard, projected_8gpu_speedup=(elapsed / args.steps * 1e3) / shard["ms_per_step"]
                                if args.windows == 256 else None,
                                note="the 8-GPU strong-scaling shard (256 / 8 windows) on this GPU; projection = "
                                     "this run's 256-window step / the 32-window step (the all-gather is ~30 us)"),
        "config2": c2,
        "erp_klt": klt,
        "global_ba": gba,
        "imu_preint": imu,
        "triangulation": tri,
        "frame_resize": rsz,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--windows", type=int, default=256, help="windows per GPU")
    ap.add_argument("--lm-iters", type=int, default=10)
    ap.add_argument("--cpu-seconds", type=float, default=10.0)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-klt", action="store_true")
    ap.add_argument("--klt-steps", type=int, default=20)
    ap.add_argument("--no-global", action="store_true")
    ap.add_argument("--no-imu", action="store_true")
    ap.add_argument("--no-tri", action="store_true")
    ap.add_argument("--no-resize", action="store_true")
    ap.add_argument("--no-config4", action="store_true")
    ap.add_argument("--no-config2", action="store_true")
    ap.add_argument("--full", action="store_true",
                    help="also run every leg beside the headline (sustained run, single window, CPU baselines, "
                         "config 4 / 2, tracker, global BA, IMU, triangulation, resize)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write every window's results of the last timed step as DIR/<name>.npy")
    args = ap.parse_args()

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    synth = importlib.import_module("360_visual_inertial_odometry_amd.synth")
    shard = shard_windows(synth, rank, args.windows)  # host processes: before torch and the GPU runtime load
    import torch
    dist = None
    if world > 1:
        import torch.distributed as dist
        torch.cuda.set_device(local_rank)
        dist.init_process_group("nccl")
    vio = importlib.import_module("360_visual_inertial_odometry_amd")

    ctx = vio.Context(local_rank)
    probs = make_shard(vio, shard, args.lm_iters)
    flops_iter = sum(ba_flops_per_iter(p) for p in probs)
    batch = vio.BaBatch(ctx, probs)
    for _ in range(args.warmup):
        batch.run()
    batch.sync()
    batch.kernel_ms()  # reset the kernel-time accumulator

    def barrier():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        batch.run()
    batch.sync()
    barrier()
    elapsed = time.perf_counter() - t0
    kms, kcount = batch.kernel_ms()
    elapsed = reduce_max(elapsed, dist, f"cuda:{local_rank}")
    head_route, _ = batch.route()
    # sanity: every window actually ran its iterations (every run solves from the resident inputs again, so
    # this is what the last timed step computed)
    res = batch.download()
    assert all(r["iterations"] == args.lm_iters + 1 and r["final_cost"] < r["initial_cost"] for r in res)
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, res, rank, world)
    # --full: a sustained run of >= 200 steps beside the K timed steps (clock ramp / launch jitter check of a
    # short timed region); reported, never the value
    sustained = None
    if args.full and args.steps < 200:
        barrier()
        t0 = time.perf_counter()
        for _ in range(200):
            batch.run()
        batch.sync()
        barrier()
        s_el = reduce_max(time.perf_counter() - t0, dist, f"cuda:{local_rank}")
        batch.kernel_ms()
        sustained = {"steps": 200, "ms_per_step": s_el / 200 * 1e3,
                     "value": world * args.windows * args.lm_iters * 200 / s_el}
    batch.close()

    total_iters = world * args.windows * args.lm_iters * args.steps
    value = total_iters / elapsed
    achieved = flops_iter * args.lm_iters / (kms * 1e-3)

    c4 = None
    if args.full and not args.no_config4:
        c4 = config4_strong(vio, synth, ctx, dist, rank, world, args.steps, args.warmup, args.lm_iters)
    mix, mix_src = sq_mix()
    mix_note = ""
    if mix:
        def _busy(name):
            v = next((m for k, m in mix.items() if k.startswith(name)), None)
            return v["mfma_busy_frac"] if v and v.get("mfma_busy_frac") is not None else float("nan")
        mix_note = (f"; MFMA pipe busy (rocprofv3 SQ_VALU_MFMA_BUSY_CYCLES over the chip's SIMD cycles, {mix_src}): "
                    f"dominant kernel ph_back {_busy('ph_back_kernel'):.3f} (no MFMA work: the walk is VALU / memory "
                    f"bound), ph_schur {_busy('ph_schur_kernel'):.3f}, ph_solve {_busy('ph_solve_kernel'):.3f}")
    out = None
    if rank == 0:
        out = {
            "metric": "sliding-window BA iters/sec (10KF x 500pts)",
            "value": value,
            "unit": "window-LM-iterations/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1e3,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "f64",
            "data": "synthetic (SURVEY §8d config-3 generator, seeds 20251205+w; random-perturbed init)",
            "config": {
                "workload": f"config-4 shard: {args.windows} independent config-3 VIO windows per GPU "
                            f"(10 KF x 500 LM, 5000 ERP obs, 9 IMU factors), {args.lm_iters} LM iterations per step",
                "windows_per_gpu": args.windows,
                "lm_iterations": args.lm_iters,
                "parallelism": f"windows sharded over {world} GPU(s), no data-path collective",
            },
            "roofline": {
                "bound": "mfma",
                "achieved": achieved / 1e12,
                "peak": FP64_PEAK / 1e12,
                "unit": "TFLOP/s",
                "frac": achieved / FP64_PEAK,
                **traffic_fields(ba_traffic(args)),
                "kernel": f"{head_route}-route step graph (ph_setup, ph_lin, 10 x [ph_prep, ph_schur, ph_solve, "
                          "ph_back], ph_prep, ph_post)",
                "kernel_avg_ms": kms,
                "kernel_launches": kcount,
                "flops_per_launch": flops_iter * args.lm_iters,
                "note": "FP64 (vector = matrix peak on MI355X); flops by the SURVEY §8d convention; achieved = "
                        "flops of one step / HIP-event time of the step's graph on the batch stream; traffic = "
                        "PMC HBM bytes of all the step's kernels" + mix_note,
                "sq_mix": mix,
                "sq_mix_source": mix_src,
            },
        }
        if args.full:
            out.update(full_legs(vio, synth, ctx, args, world, probs, elapsed, sustained, c4))
        print(json.dumps(out), flush=True)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    ctx.close()
    return out


if __name__ == "__main__":
    main()
