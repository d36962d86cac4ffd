"""Diagnostic: device time of the colour ingest (erp_ingest_device), 64 frames per launch, device events, median
of `steps`: BGR8, BGRA8, YUYV, and BGRA8 at an address 1 byte off alignment (no dword loads), at 3840x1920,
4096x2048 and 5376x2688 -> 960x480.  Per case, ms per frame of
  fused        the one-pass kernels as AUTO's variant choice runs them (dword / run loads where they apply)
  fused bytes  the one-pass kernels' byte-load variants
  two-pass     convert to a grey plane, then the grey resize (both launches inside the timed interval)
  grey         the grey resize alone on a grey frame of the same size (the kernels before the colour ingest)
  auto         what the library dispatches by default
and the fused kernel's algorithmic bytes (bpp*W*H + dW*dH per frame) over its time as a share of 8.0 TB/s.
Usage: ingest_time.py [steps]"""
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

vio = importlib.import_module("360_visual_inertial_odometry_amd")
steps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
FRAMES, PEAK, DW, DH = 64, 8.0e12, 960, 480
SIZES = [(3840, 1920), (4096, 2048), (5376, 2688)]
FORMATS = [("BGR8", vio.VIO_PIX_BGR8, 0), ("BGRA8", vio.VIO_PIX_BGRA8, 0), ("YUYV", vio.VIO_PIX_YUYV, 0),
           ("BGRA8 at +1 byte", vio.VIO_PIX_BGRA8, 1)]
ROUTES = [("fused", vio.VIO_INGEST_ROUTE_FUSED), ("fused bytes", vio.VIO_INGEST_ROUTE_FUSED_BYTES),
          ("two-pass", vio.VIO_INGEST_ROUTE_TWO_PASS), ("auto", vio.VIO_INGEST_ROUTE_AUTO)]
ctx = vio.Context(0)


def median_ms(call):
    for _ in range(3):
        call()
        ctx.resize_kernel_ms()
    ms = []
    for _ in range(steps):
        call()
        ms.append(ctx.resize_kernel_ms())
    ms.sort()
    return ms[len(ms) // 2] / FRAMES


for W, H in SIZES:
    dst = torch.zeros((FRAMES, DH, DW), dtype=torch.uint8, device="cuda:0")
    gen = torch.Generator(device="cuda:0").manual_seed(W)
    grey = torch.randint(0, 256, (FRAMES, H, W), dtype=torch.uint8, device="cuda:0", generator=gen)
    torch.cuda.synchronize()
    g_ms = median_ms(lambda: ctx.resize_area_any_device(grey.data_ptr(), W, H, W, FRAMES, dst.data_ptr(), DW, DH, DW))
    del grey
    for name, fmt, off in FORMATS:
        bpp = vio.Context.pixel_bytes(fmt)
        src = torch.randint(0, 256, (FRAMES * H * W * bpp + 16,), dtype=torch.uint8, device="cuda:0", generator=gen)
        torch.cuda.synchronize()
        t = {}
        for rname, route in ROUTES:
            ctx.set_ingest_route(route)
            t[rname] = median_ms(lambda: ctx.ingest_device(src.data_ptr() + off, fmt, vio.VIO_LUMA_CVTCOLOR, W, H, W * bpp,
                                                           FRAMES, dst.data_ptr(), DW, DH, DW))
        ctx.set_ingest_route(vio.VIO_INGEST_ROUTE_AUTO)
        alg = bpp * W * H + DW * DH
        print(f"{name} {W}x{H} -> {DW}x{DH}  ms/frame: " + "  ".join(f"{k} {v:.4f}" for k, v in t.items()) +
              f"  grey {g_ms:.4f}  | fused: {alg / (t['fused'] * 1e-3) / 1e12:.2f} TB/s = "
              f"{100 * alg / (t['fused'] * 1e-3) / PEAK:.1f} % of 8.0 TB/s (median of {steps})", flush=True)
        del src
    del dst
ctx.close()
