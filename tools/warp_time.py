"""Diagnostic: device time of the lens-to-ERP warp (erp_warp_apply_device), 64 frames per launch, device events,
median of `steps`: GRAY8 and BGR8, for a 5760x2880 dual-fisheye source -> 3840x1920 and -> 960x480, and for a
3840x1920 ERP rotation.  Per case, ms per frame of
  warp       the kernel as the library runs it (VIO_WARP_ROUTE_AUTO: the two taps of a row as one pixel pair)
  single     one load per tap (VIO_WARP_ROUTE_SINGLE; three byte loads per tap for BGR8)
  1:1 pass   the one-lane-per-pixel pass over the same source as a yardstick: erp_ingest_device at dW = W, dH = H
             (ingest_convert_kernel for BGR8, the grey 1:1 area kernel for GRAY8)
and the warp's algorithmic bytes per frame, map bytes / frames + bpp * (source pixels that a tap touches) + dW * dH,
over its time as a share of 8.0 TB/s.
Usage: warp_time.py [steps]"""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

vio = importlib.import_module("360_visual_inertial_odometry_amd")
steps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
FRAMES, PEAK = 64, 8.0e12
FORMATS = [("GRAY8", vio.VIO_PIX_GRAY8), ("BGR8", vio.VIO_PIX_BGR8)]
ctx = vio.Context(0)


def rot(axis, a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]] if axis == "y" else [[1, 0, 0], [0, c, -s], [0, s, c]])


def dual_fisheye(circle):
    """two back-to-back 190-degree lenses, image circles side by side in a (2 circle) x circle frame"""
    f, c, t = (circle / 2.0) / np.deg2rad(95.0), (circle - 1) / 2.0, np.deg2rad(95.0)
    return [{"R": np.eye(3), "cx": c, "cy": c, "f": f, "theta_max": t},
            {"R": rot("y", np.pi), "cx": circle + c, "cy": c, "f": f, "theta_max": t}]


def touched_pixels(mx, my, sW, sH, bx, by):
    """how many source pixels some tap of the quantised map reads"""
    qx, vx = vio.warp_quantize(mx, sW, bx)
    qy, vy = vio.warp_quantize(my, sH, by)
    ok = (vx & vy).astype(bool)
    ix, iy = qx[ok] >> 5, qy[ok] >> 5
    seen = np.zeros((sH, sW), bool)
    for dx in (0, 1):
        for dy in (0, 1):
            x = (ix + dx) % sW if bx == vio.VIO_WARP_X_WRAP else ix + dx
            y = iy + dy
            inside = (x >= 0) & (x < sW) & ((y >= 0) & (y < sH) if by == vio.VIO_WARP_Y_CONSTANT else True)
            seen[np.clip(y, 0, sH - 1)[inside], x[inside]] = True
    return int(seen.sum())


def median_ms(call, read):
    for _ in range(3):
        call()
        read()
    ms = []
    for _ in range(steps):
        call()
        ms.append(read())
    ms.sort()
    return ms[len(ms) // 2] / FRAMES


R = rot("y", 0.1234) @ rot("x", 0.0567)
CASES = [("dual-fisheye 5760x2880 -> 3840x1920", 5760, 2880, 3840, 1920, "fisheye"),
         ("dual-fisheye 5760x2880 -> 960x480", 5760, 2880, 960, 480, "fisheye"),
         ("ERP rotation 3840x1920 -> 3840x1920", 3840, 1920, 3840, 1920, "erp")]
for name, sW, sH, dW, dH, kind in CASES:
    if kind == "fisheye":
        mx, my = vio.warp_map_fisheye(dual_fisheye(sH), dW, dH, R)
        bx, by = vio.VIO_WARP_X_CONSTANT, vio.VIO_WARP_Y_CONSTANT
    else:
        mx, my = vio.warp_map_erp(sW, sH, dW, dH, R)
        bx, by = vio.VIO_WARP_X_WRAP, vio.VIO_WARP_Y_REPLICATE
    touched = touched_pixels(mx, my, sW, sH, bx, by)
    w = ctx.warp_create(mx, my, sW, sH, bx, by)
    dst = torch.zeros((FRAMES, dH, dW), dtype=torch.uint8, device="cuda:0")
    gen = torch.Generator(device="cuda:0").manual_seed(sW + dW)
    for fname, fmt in FORMATS:
        bpp = vio.Context.pixel_bytes(fmt)
        src = torch.randint(0, 256, (FRAMES * sH * sW * bpp,), dtype=torch.uint8, device="cuda:0", generator=gen)
        full = torch.zeros((FRAMES, sH, sW), dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()

        def warp():
            w.apply_device(src.data_ptr(), fmt, vio.VIO_LUMA_CVTCOLOR, sW * bpp, FRAMES, dst.data_ptr(), dW)

        t = {}
        for label, route in (("warp", vio.VIO_WARP_ROUTE_AUTO), ("single", vio.VIO_WARP_ROUTE_SINGLE)):
            w.set_route(route)
            t[label] = median_ms(warp, w.kernel_ms)
        w.set_route(vio.VIO_WARP_ROUTE_AUTO)
        t["1:1 pass"] = median_ms(lambda: ctx.ingest_device(src.data_ptr(), fmt, vio.VIO_LUMA_CVTCOLOR, sW, sH, sW * bpp,
                                                            FRAMES, full.data_ptr(), sW, sH, sW), ctx.resize_kernel_ms)
        alg = 8 * dW * dH / FRAMES + bpp * touched + dW * dH
        print(f"{fname} {name}  ms/frame: " + "  ".join(f"{k} {v:.4f}" for k, v in t.items()) +
              f"  | touched {touched} of {sW * sH} source pixels, {alg / 1e6:.2f} MB/frame: "
              f"{alg / (t['warp'] * 1e-3) / 1e12:.2f} TB/s = {100 * alg / (t['warp'] * 1e-3) / PEAK:.1f} % of 8.0 TB/s "
              f"(median of {steps})", flush=True)
        del src, full
    del dst
    w.close()
ctx.close()
