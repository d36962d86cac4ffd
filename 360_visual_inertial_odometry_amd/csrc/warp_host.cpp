// warp_host.cpp — host side of the lens-to-ERP warp (erp_warp_*, include/vio360.h): the quantisation of a float
// map, the map generators of the three source geometries (rotated ERP, equidistant fisheye lenses, cubemap / EAC
// faces) and the launches of warp.hip's kernel.  Everything here that decides a byte of the result is integer
// arithmetic or IEEE double in the written order (the file is built without FMA contraction); the generators'
// transcendentals come from libm, and tests/warp_oracle.py restates them in float64 (tests/test_warp.py gives the
// tolerance).  OpenCV is not available to this project: parity with cv::remap is unpinned.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <string>
#include <vector>

#include "frame_io.h"
#include "resize.h"
#include "warp.h"

using namespace vio360;

namespace {

constexpr int kMaxSize = 1 << 25;  // 32 * size and the row index fit an int32 with room to spare

bool border_mode_ok(int m) { return m == VIO_WARP_X_CONSTANT || m == VIO_WARP_X_WRAP || m == VIO_WARP_Y_REPLICATE; }

// q of one coordinate (include/vio360.h); false for a non-finite one
bool quantize(float s, int S, int border_mode, int32_t* q) {
    if (!std::isfinite(s)) {
        *q = 0;
        return false;
    }
    double d = std::nearbyint((double)s * 32.0);  // lrint: the default rounding mode, half to even
    const double M = 32.0 * S;
    if (border_mode == VIO_WARP_X_WRAP) {
        d = std::fmod(d, M);  // exact
        if (d < 0) d += M;
    } else {
        d = std::min(std::max(d, -32.0), M);
    }
    *q = (int32_t)d;
    return true;
}

// the kernel variant and pixel source of a format at this address and stride
//   pair route (sW >= 2): two neighbouring pixels per run of loads at any alignment, px in bit shifts
//   single route: one load per tap; 4-byte pixels take one aligned dword when src and stride are multiples of 4
//   (then every frame of a batch is aligned), else three byte loads
int pixel_mode(int format, int luma, const uint8_t* src, int stride, bool pair, PixSrc* px) {
    *px = pix_source(format, luma);
    if (format == VIO_PIX_GRAY8) return kPixGray;
    int mode = pix_is_422(format) ? kPixByte : kPixBytes3;
    if (px->bpp == 4 && (pair || pix_dword_ok(src, stride))) mode = kPixDword;
    if (pair || mode == kPixDword) pix_to_bit_shifts(px);
    return mode;
}

int warp_check(const erp_warp* w, int format, int luma, int stride, int dst_stride, int n_frames) {
    vio_ctx* ctx = w->ctx;
    const char* why;
    if (!pix_check(format, luma, w->sW, &why) &&
        ((long long)stride < (long long)w->sW * erp_pixel_bytes(format) || dst_stride < w->dW || n_frames < 0))
        why = "bad sizes";
    if (why) set_error(ctx, std::string("erp_warp: ") + why);
    return why ? VIO_EINVAL : VIO_OK;
}

struct Vec3 {
    double x, y, z;
};

Vec3 rotate(const double* R, const Vec3& b) {
    if (!R) return b;
    return {R[0] * b.x + R[1] * b.y + R[2] * b.z, R[3] * b.x + R[4] * b.y + R[5] * b.z,
            R[6] * b.x + R[7] * b.y + R[8] * b.z};
}

// Camera::PixelToBearing (Camera.cpp:22-47) at (u, v) = (x, y) in double (the reference's final normalize() is
// left out: the vector is a unit vector to 1 ulp), rotated by R_dst
Vec3 dst_bearing(int x, int y, int dW, int dH, const double* R_dst) {
    const double lon = ((double)x / dW - 0.5) * 2.0 * M_PI;
    const double lat = -((double)y / dH - 0.5) * M_PI;
    const double cl = std::cos(lat);
    return rotate(R_dst, {cl * std::sin(lon), -std::sin(lat), cl * std::cos(lon)});
}

bool map_args_ok(int dW, int dH, const float* map_x, const float* map_y) {
    return dW > 0 && dH > 0 && dW <= kMaxSize && dH <= kMaxSize && map_x && map_y;
}

}  // namespace

extern "C" {

int erp_warp_quantize(const float* s, int n, int S, int border_mode, int32_t* q, uint8_t* valid) {
    if (n < 0 || S <= 0 || S > kMaxSize || !border_mode_ok(border_mode) || (n > 0 && (!s || !q || !valid)))
        return VIO_EINVAL;
    for (int i = 0; i < n; ++i) valid[i] = quantize(s[i], S, border_mode, &q[i]) ? 1 : 0;
    return VIO_OK;
}

int erp_warp_create(vio_ctx* ctx, const float* map_x, const float* map_y, int dW, int dH, int map_stride, int sW,
                    int sH, int border_x, int border_y, int border_value, erp_warp** out) {
    if (out) *out = nullptr;
    if (!map_x || !map_y || !out || dW <= 0 || dH <= 0 || map_stride < dW || sW <= 0 || sH <= 0 || sW > kMaxSize ||
        sH > kMaxSize || dH > 65535 ||
        (border_x != VIO_WARP_X_CONSTANT && border_x != VIO_WARP_X_WRAP) ||
        (border_y != VIO_WARP_Y_CONSTANT && border_y != VIO_WARP_Y_REPLICATE) || border_value < 0 || border_value > 255) {
        if (ctx) set_error(ctx, "erp_warp_create: bad sizes, border mode or border value");
        return VIO_EINVAL;
    }
    if (!ctx) {  // a host-only object: what erp_warp_check needs, on a machine without a device
        erp_warp* w = new erp_warp();
        w->dW = dW; w->dH = dH; w->sW = sW; w->sH = sH;
        w->border_x = border_x; w->border_y = border_y; w->border_value = border_value;
        *out = w;
        return VIO_OK;
    }
    std::vector<WarpEntry> q((size_t)dW * dH);
    for (int y = 0; y < dH; ++y)
        for (int x = 0; x < dW; ++x) {
            const size_t i = (size_t)y * map_stride + x;
            WarpEntry& e = q[(size_t)y * dW + x];
            const bool okx = quantize(map_x[i], sW, border_x, &e.qx), oky = quantize(map_y[i], sH, border_y, &e.qy);
            if (!okx || !oky) e = {0, kWarpInvalid};
        }
    VIO_DEVICE(ctx);
    erp_warp* w = new erp_warp();
    w->ctx = ctx;
    w->dW = dW; w->dH = dH; w->sW = sW; w->sH = sH;
    w->border_x = border_x; w->border_y = border_y; w->border_value = border_value;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&w->d_map), sizeof(WarpEntry) * q.size());
    if (e != hipSuccess) {
        delete w;
        set_error(ctx, "erp_warp_create: device allocation failed");
        return VIO_ENOMEM;
    }
    for (hipEvent_t& ev : w->ev)
        if (e == hipSuccess) e = hipEventCreate(&ev);
    // on the context stream and blocking: the host table dies with this scope
    if (e == hipSuccess) e = hipMemcpyAsync(w->d_map, q.data(), sizeof(WarpEntry) * q.size(), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        erp_warp_destroy(w);
        return hip_fail(ctx, e, "erp_warp_create");
    }
    *out = w;
    return VIO_OK;
}

void erp_warp_destroy(erp_warp* w) {
    if (!w) return;
    if (!w->ctx) {
        delete w;
        return;
    }
    DeviceScope _vio_dev_scope(w->ctx->device);
    (void)hipStreamSynchronize(w->ctx->stream);
    for (hipEvent_t ev : w->ev)
        if (ev) (void)hipEventDestroy(ev);
    if (w->d_map) (void)hipFree(w->d_map);
    delete w;
}

int erp_warp_check(const erp_warp* w, int format, int luma, int stride, int dst_stride) {
    if (!w) return VIO_EINVAL;
    return warp_check(w, format, luma, stride, dst_stride, 1);
}

int erp_warp_set_route(erp_warp* w, int route) {
    if (!w || (route != VIO_WARP_ROUTE_AUTO && route != VIO_WARP_ROUTE_SINGLE)) return VIO_EINVAL;
    w->route = route;
    return VIO_OK;
}

int erp_warp_apply_device(erp_warp* w, const uint8_t* src, int format, int luma, int stride, int n_frames,
                          uint8_t* dst, int dst_stride) {
    if (!w || !w->ctx || !src || !dst) return VIO_EINVAL;
    vio_ctx* ctx = w->ctx;
    int rc = warp_check(w, format, luma, stride, dst_stride, n_frames);
    if (rc) return rc;
    if (n_frames == 0) return VIO_OK;
    WarpArgs a;
    const bool pair = w->route == VIO_WARP_ROUTE_AUTO && w->sW >= 2;
    const int mode = pixel_mode(format, luma, src, stride, pair, &a.px);
    a.src = src;
    a.sW = w->sW; a.sH = w->sH; a.stride = stride;
    a.frame_bytes_src = (long long)stride * w->sH;
    a.dst = dst;
    a.dW = w->dW; a.dH = w->dH; a.dstride = dst_stride;
    a.frame_bytes_dst = (long long)dst_stride * w->dH;
    a.map = w->d_map;
    a.n_frames = n_frames;
    a.wrap_x = w->border_x == VIO_WARP_X_WRAP;
    a.replicate_y = w->border_y == VIO_WARP_Y_REPLICATE;
    a.border_value = w->border_value;
    VIO_DEVICE(ctx);
    VIO_HIP(ctx, hipEventRecord(w->ev[0], ctx->stream));
    VIO_HIP(ctx, launch_warp(a, mode, pair, ctx->stream));
    VIO_HIP(ctx, hipEventRecord(w->ev[1], ctx->stream));
    return VIO_OK;
}

int erp_warp_apply(erp_warp* w, const uint8_t* src, int format, int luma, int stride, uint8_t* dst, int dst_stride) {
    if (!w || !w->ctx || !src || !dst) return VIO_EINVAL;
    vio_ctx* ctx = w->ctx;
    int rc = warp_check(w, format, luma, stride, dst_stride, 1);
    if (rc) return rc;
    // source rows padded to 16 bytes (dword loads for 4-byte pixels)
    uint8_t *d_src = nullptr, *d_dst = nullptr;
    int sp = 0, dp = 0;
    if ((rc = stage_rows(ctx, kSlotResizeSrc, src, stride, (long long)w->sW * erp_pixel_bytes(format), w->sH, 16,
                         "erp_warp", &d_src, &sp)))
        return rc;
    if ((rc = scratch_rows(ctx, kSlotResizeDst, w->dW, w->dH, 4, "erp_warp", &d_dst, &dp))) return rc;
    if ((rc = erp_warp_apply_device(w, d_src, format, luma, sp, 1, d_dst, dp))) return rc;
    return fetch_rows(ctx, d_dst, dp, dst, dst_stride, w->dW, w->dH);
}

int erp_warp_kernel_ms(erp_warp* w, double* ms) {
    return w && w->ctx ? events_ms(w->ctx, w->ev[0], w->ev[1], ms) : VIO_EINVAL;
}

// ---- map generators ----

int erp_warp_map_erp(int sW, int sH, const double* R_dst, int dW, int dH, float* map_x, float* map_y) {
    if (sW <= 0 || sH <= 0 || sW > kMaxSize || sH > kMaxSize || !map_args_ok(dW, dH, map_x, map_y)) return VIO_EINVAL;
    for (int y = 0; y < dH; ++y)
        for (int x = 0; x < dW; ++x) {
            const Vec3 b = dst_bearing(x, y, dW, dH, R_dst);
            // Camera::BearingToPixel (Camera.cpp:49-67)
            const double theta = std::atan2(b.x, b.z);
            const double norm = std::sqrt(b.x * b.x + b.y * b.y + b.z * b.z);
            const double phi = -std::asin(std::min(std::max(b.y / norm, -1.0), 1.0));
            const size_t i = (size_t)y * dW + x;
            map_x[i] = (float)(sW * (0.5 + theta / (2.0 * M_PI)));
            map_y[i] = (float)(sH * (0.5 - phi / M_PI));
        }
    return VIO_OK;
}

int erp_warp_map_fisheye(const erp_fisheye_lens* lenses, int n, const double* R_dst, int dW, int dH, float* map_x,
                         float* map_y) {
    if (!lenses || n <= 0 || !map_args_ok(dW, dH, map_x, map_y)) return VIO_EINVAL;
    for (int k = 0; k < n; ++k) {
        const erp_fisheye_lens& l = lenses[k];
        if (!std::isfinite(l.cx) || !std::isfinite(l.cy) || !std::isfinite(l.f) || !(l.f > 0) || !(l.theta_max > 0))
            return VIO_EINVAL;
    }
    const float nan = std::numeric_limits<float>::quiet_NaN();
    for (int y = 0; y < dH; ++y)
        for (int x = 0; x < dW; ++x) {
            const Vec3 b = dst_bearing(x, y, dW, dH, R_dst);
            int best = -1;
            double best_theta = 0, best_h = 0;
            Vec3 best_bl{0, 0, 0};
            for (int k = 0; k < n; ++k) {
                const Vec3 bl = rotate(lenses[k].R, b);
                const double h = std::hypot(bl.x, bl.y);
                const double theta = std::atan2(h, bl.z);
                if (theta <= lenses[k].theta_max && (best < 0 || theta < best_theta)) {
                    best = k;
                    best_theta = theta;
                    best_h = h;
                    best_bl = bl;
                }
            }
            const size_t i = (size_t)y * dW + x;
            if (best < 0) {
                map_x[i] = map_y[i] = nan;
            } else if (best_h == 0) {
                map_x[i] = (float)lenses[best].cx;
                map_y[i] = (float)lenses[best].cy;
            } else {
                const erp_fisheye_lens& l = lenses[best];
                map_x[i] = (float)(l.cx + l.f * best_theta * best_bl.x / best_h);
                map_y[i] = (float)(l.cy + l.f * best_theta * best_bl.y / best_h);
            }
        }
    return VIO_OK;
}

int erp_warp_map_cubemap(const erp_cube_face* faces, int n, int eac, int sW, int sH, const double* R_dst, int dW,
                         int dH, float* map_x, float* map_y) {
    if (!faces || n <= 0 || sW <= 0 || sH <= 0 || sW > kMaxSize || sH > kMaxSize || !map_args_ok(dW, dH, map_x, map_y))
        return VIO_EINVAL;
    for (int k = 0; k < n; ++k) {
        const erp_cube_face& f = faces[k];
        if (f.w <= 0 || f.h <= 0 || f.x0 < 0 || f.y0 < 0 || (long long)f.x0 + f.w > sW || (long long)f.y0 + f.h > sH)
            return VIO_EINVAL;  // a face outside the source
    }
    const float nan = std::numeric_limits<float>::quiet_NaN();
    for (int y = 0; y < dH; ++y)
        for (int x = 0; x < dW; ++x) {
            const Vec3 b = dst_bearing(x, y, dW, dH, R_dst);
            int best = -1;
            Vec3 bf{0, 0, 0};
            for (int k = 0; k < n; ++k) {
                const Vec3 c = rotate(faces[k].R, b);
                if (c.z > 0 && (best < 0 || c.z > bf.z)) {
                    best = k;
                    bf = c;
                }
            }
            const size_t i = (size_t)y * dW + x;
            if (best < 0) {
                map_x[i] = map_y[i] = nan;
                continue;
            }
            double u = bf.x / bf.z, v = bf.y / bf.z;
            if (eac) {
                u = (4.0 / M_PI) * std::atan(u);
                v = (4.0 / M_PI) * std::atan(v);
            }
            const erp_cube_face& f = faces[best];
            const double sx = f.x0 + (u + 1.0) * f.w / 2.0 - 0.5, sy = f.y0 + (v + 1.0) * f.h / 2.0 - 0.5;
            map_x[i] = (float)std::min(std::max(sx, (double)f.x0), (double)(f.x0 + f.w - 1));
            map_y[i] = (float)std::min(std::max(sy, (double)f.y0), (double)(f.y0 + f.h - 1));
        }
    return VIO_OK;
}

}  // extern "C"
