"""Diagnostic: device time of the contrast equalisation (erp_equalize_device), GRAY8 3840x1920 and 960x480, CLAHE 8x8 /
3.0 and HIST, on a noise frame and on a constant frame (every lane of the histogram kernel on one bin), device events,
median of `steps`.  Per case, ms per frame of
  batch      32 frames per launch: the three stages' total, and each stage from a second series with the markers
             between the stages on (erp_equalize_set_stage_timing; a marker costs the stream a few microseconds, so
             the stages sum to more than the total)
  single     one frame per launch, total (three launches: what erp_tracker_equalize costs the stream)
  1:1 pass   the yardstick: the grey 1:1 area kernel over the same frames (erp_ingest_device at dW = W, dH = H)
and the algorithmic bytes, 3 per pixel (the histogram's read, the apply's read and write), over the batch time as a
share of 8.0 TB/s.
Usage: equalize_time.py [steps]"""
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

vio = importlib.import_module("360_visual_inertial_odometry_amd")
steps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
FRAMES, PEAK = 32, 8.0e12
ctx = vio.Context(0)


def median(call, read):
    for _ in range(3):
        call()
        read()
    out = []
    for _ in range(steps):
        call()
        out.append(read())
    if isinstance(out[0], dict):
        return {k: sorted(o[k] for o in out)[len(out) // 2] for k in out[0]}
    return sorted(out)[len(out) // 2]


MODES = [("CLAHE 8x8/3.0", vio.equalize_params(vio.VIO_EQ_CLAHE, 8, 8, 3.0)), ("HIST", vio.equalize_params(vio.VIO_EQ_HIST))]
for W, H in [(3840, 1920), (960, 480)]:
    gen = torch.Generator(device="cuda:0").manual_seed(W)
    frames = {"noise": torch.randint(0, 256, (FRAMES, H, W), dtype=torch.uint8, device="cuda:0", generator=gen),
              "constant": torch.full((FRAMES, H, W), 93, dtype=torch.uint8, device="cuda:0")}
    dst = torch.zeros((FRAMES, H, W), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    for kind, src in frames.items():
        yard = median(lambda: ctx.ingest_device(src.data_ptr(), vio.VIO_PIX_GRAY8, vio.VIO_LUMA_CVTCOLOR, W, H, W, FRAMES,
                                                dst.data_ptr(), W, H, W), ctx.resize_kernel_ms) / FRAMES
        for name, p in MODES:
            def run(n):
                ctx.equalize_device(src.data_ptr(), W, H, W, n, p, dst.data_ptr(), W)

            ctx.set_equalize_stage_timing(False)
            batch = median(lambda: run(FRAMES), ctx.equalize_kernel_ms) / FRAMES
            single = median(lambda: run(1), ctx.equalize_kernel_ms)
            ctx.set_equalize_stage_timing(True)
            st = median(lambda: run(FRAMES), ctx.equalize_stage_ms)
            ctx.set_equalize_stage_timing(False)
            alg = 3 * W * H
            print(f"GRAY8 {W}x{H} {name} {kind}  ms/frame: batch {batch:.4f} (hist {st['hist'] / FRAMES:.4f}  lut "
                  f"{st['lut'] / FRAMES:.4f}  apply {st['apply'] / FRAMES:.4f})  single {single:.4f}  1:1 pass {yard:.4f}"
                  f"  | batch / 1:1 pass {batch / yard:.2f}, {alg / 1e6:.2f} MB/frame: "
                  f"{alg / (batch * 1e-3) / 1e12:.2f} TB/s = {100 * alg / (batch * 1e-3) / PEAK:.1f} % of 8.0 TB/s "
                  f"(median of {steps})", flush=True)
    del frames, dst
ctx.close()
