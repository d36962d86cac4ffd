"""Diagnostic: device time of the INTER_AREA resize kernels, 64 frames per launch as bench.py's frame_resize
leg: the general kernel (4096x2048 and 5376x2688 -> 960x480) next to the generic integer kernel
(5120x2560 -> 1024x512, factor 5) and the factor-4 fast kernel (3840x1920 -> 960x480).  Prints ms per frame,
source Mpx/s and the algorithmic bytes (W*H + dW*dH per frame) over time as a share of the 8.0 TB/s HBM peak.
Usage: resize_time.py [steps]"""
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

vio = importlib.import_module("360_visual_inertial_odometry_amd")
steps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
FRAMES, PEAK = 64, 8.0e12
CASES = [("resize_area_general_kernel", 4096, 2048, 960, 480),
         ("resize_area_general_kernel", 5376, 2688, 960, 480),
         ("resize_area_kernel (factor 5)", 5120, 2560, 1024, 512),
         ("resize_area4_kernel", 3840, 1920, 960, 480)]
ctx = vio.Context(0)
for name, W, H, dW, dH in CASES:
    gen = torch.Generator(device="cuda:0").manual_seed(W)
    src = torch.randint(0, 256, (FRAMES, H, W), dtype=torch.uint8, device="cuda:0", generator=gen)
    dst = torch.zeros((FRAMES, dH, dW), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    args = (src.data_ptr(), W, H, W, FRAMES, dst.data_ptr(), dW, dH, dW)
    for _ in range(3):
        ctx.resize_area_any_device(*args)
        ctx.resize_kernel_ms()
    ms = []
    for _ in range(steps):
        ctx.resize_area_any_device(*args)
        ms.append(ctx.resize_kernel_ms())
    ms.sort()
    k_ms = ms[len(ms) // 2] / FRAMES
    alg = W * H + dW * dH
    print(f"{name}: {W}x{H} -> {dW}x{dH}  {k_ms:.4f} ms/frame  {W * H / (k_ms * 1e-3) / 1e6:.0f} src Mpx/s  "
          f"{alg / (k_ms * 1e-3) / 1e12:.2f} TB/s = {100 * alg / (k_ms * 1e-3) / PEAK:.1f} % of 8.0 TB/s "
          f"(median of {steps}, min {ms[0] / FRAMES:.4f})", flush=True)
    del src, dst
ctx.close()
