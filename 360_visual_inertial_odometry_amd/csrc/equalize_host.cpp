// equalize_host.cpp — host side of the contrast equalisation (erp_equalize*, include/vio360.h): the argument check,
// the LUT rule of one histogram restated on the host (erp_equalize_lut, what eq_lut_kernel computes per tile), the
// tiling and the launches of equalize.hip's three kernels.  Built without FMA contraction, like the kernels.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "equalize.h"
#include "frame_io.h"

using namespace vio360;

namespace {

constexpr long long kMaxPixels = 1LL << 30;
constexpr long long kMaxGrid = 1LL << 21;  // workgroups of a launch's x axis: with 1024 lanes each, below 2^32 lanes

uint8_t saturate_u8(float f) { return (uint8_t)(int)std::fmin(std::fmax(std::nearbyintf(f), 0.f), 255.f); }

// CLAHE's bin limit c of a tile of `area` pixels; 0 = no clipping
int clip_bins(double clip_limit, int area) {
    if (!(clip_limit > 0)) return 0;
    const double v = clip_limit * area / 256.0;
    return v >= (double)area ? area : std::max((int)v, 1);  // no bin exceeds area: a larger limit changes nothing
}

int check(const erp_equalize_params* p, int W, int H, int stride, int dst_stride) {
    if (!p || W < 2 || H < 2 || (long long)W * H > kMaxPixels || stride < W || dst_stride < W) return VIO_EINVAL;
    if (p->mode == VIO_EQ_NONE || p->mode == VIO_EQ_HIST) return VIO_OK;
    if (p->mode != VIO_EQ_CLAHE) return VIO_EINVAL;
    if (p->tiles_x < 1 || p->tiles_y < 1 || p->tiles_x > W / 2 || p->tiles_y > H / 2) return VIO_EINVAL;
    if (!std::isfinite(p->clip_limit) || p->clip_limit < 0) return VIO_EINVAL;
    if (p->border_x != VIO_EQ_X_CLAMP && p->border_x != VIO_EQ_X_WRAP) return VIO_EINVAL;
    if (p->border_x == VIO_EQ_X_WRAP && (W % p->tiles_x || H % p->tiles_y)) return VIO_EINVAL;
    return VIO_OK;
}

int ceil_div(long long a, long long b) { return (int)((a + b - 1) / b); }

}  // namespace

extern "C" {

int erp_equalize_check(const erp_equalize_params* p, int W, int H, int stride, int dst_stride) {
    return check(p, W, H, stride, dst_stride);
}

int erp_equalize_lut(int mode, const uint32_t* hist, int area, double clip_limit, uint8_t* lut) {
    if (!hist || !lut || area < 1 || (mode != VIO_EQ_HIST && mode != VIO_EQ_CLAHE)) return VIO_EINVAL;
    if (mode == VIO_EQ_CLAHE) {
        if (!std::isfinite(clip_limit) || clip_limit < 0) return VIO_EINVAL;
        uint32_t h[256];
        std::copy(hist, hist + 256, h);
        const uint32_t c = (uint32_t)clip_bins(clip_limit, area);
        if (c > 0) {
            uint32_t excess = 0;
            for (uint32_t& v : h)
                if (v > c) {
                    excess += v - c;
                    v = c;
                }
            const uint32_t batch = excess / 256;
            uint32_t resid = excess - 256 * batch;
            for (uint32_t& v : h) v += batch;
            if (resid > 0) {
                const uint32_t step = std::max(256u / resid, 1u);
                for (uint32_t i = 0; i < 256 && resid > 0; i += step, --resid) ++h[i];
            }
        }
        const float scale = 255.f / (float)area;
        uint32_t sum = 0;
        for (int i = 0; i < 256; ++i) {
            sum += h[i];
            lut[i] = saturate_u8((float)sum * scale);
        }
        return VIO_OK;
    }
    int i0 = 0;
    while (i0 < 255 && !hist[i0]) ++i0;
    if (hist[i0] == (uint32_t)area) {
        std::fill(lut, lut + 256, (uint8_t)i0);
        return VIO_OK;
    }
    const float scale = 255.f / (float)((uint32_t)area - hist[i0]);
    uint32_t sum = 0;
    for (int i = 0; i < 256; ++i) {
        if (i <= i0) {
            lut[i] = 0;
            continue;
        }
        sum += hist[i];
        lut[i] = saturate_u8((float)sum * scale);
    }
    return VIO_OK;
}

int erp_equalize_device(vio_ctx* ctx, const uint8_t* src, int W, int H, int stride, int n_frames,
                        const erp_equalize_params* p, uint8_t* dst, int dst_stride) {
    if (!ctx || !src || !dst || n_frames < 0 || n_frames > 65535) return VIO_EINVAL;
    if (check(p, W, H, stride, dst_stride) || (dst == src && dst_stride != stride)) {
        set_error(ctx, "erp_equalize: bad sizes, mode, tiles, clip limit or border mode");
        return VIO_EINVAL;
    }
    if (n_frames == 0) return VIO_OK;
    VIO_DEVICE(ctx);
    if (p->mode == VIO_EQ_NONE) {  // a copy; the frames of a batch follow each other at the row stride
        if (dst != src)
            VIO_HIP(ctx, hipMemcpy2DAsync(dst, dst_stride, src, stride, W, (size_t)H * n_frames, hipMemcpyDeviceToDevice,
                                          ctx->stream));
        return VIO_OK;
    }
    EqArgs a{};
    a.src = src; a.dst = dst;
    a.W = W; a.H = H; a.stride = stride; a.dstride = dst_stride;
    a.frame_bytes_src = (long long)stride * H;
    a.frame_bytes_dst = (long long)dst_stride * H;
    a.n_frames = n_frames;
    a.mode = p->mode;
    const long long pixels = (long long)W * H * n_frames;
    if (p->mode == VIO_EQ_HIST) {
        a.tiles_x = a.tiles_y = 1;
        a.tw = W; a.th = H;
        a.area = W * H;
    } else {
        a.tiles_x = p->tiles_x; a.tiles_y = p->tiles_y;
        const bool fits = W % a.tiles_x == 0 && H % a.tiles_y == 0;
        // both axes are extended as soon as one is not divisible (a divisible one by a whole tiles count)
        a.tw = (fits ? W : W + a.tiles_x - W % a.tiles_x) / a.tiles_x;
        a.th = (fits ? H : H + a.tiles_y - H % a.tiles_y) / a.tiles_y;
        a.area = a.tw * a.th;  // tiles 1 x 1 is not extended, more tiles make it smaller: at most 2^30
        a.wrap_x = p->border_x == VIO_EQ_X_WRAP;
        a.clip = clip_bins(p->clip_limit, a.area);
        a.lut_scale = 255.f / (float)a.area;
    }
    a.inv_tw = 1.f / (float)a.tw;
    a.inv_th = 1.f / (float)a.th;
    const long long tiles = (long long)a.tiles_x * a.tiles_y;
    // pixels per workgroup of (a) and (c): about a thousand workgroups per launch, each with 2 to 8 Kpixels
    const long long target = std::min(std::max(pixels / 1024, 2048LL), 8192LL);
    a.chunk_rows = std::max(ceil_div(target, a.tw), ceil_div(a.th, kEqMaxChunks));
    a.chunks = ceil_div(a.th, a.chunk_rows);
    a.rw = std::min(a.tw, 2048);
    a.rh = (int)std::min<long long>(std::max<long long>(target / a.rw, 1), a.th);
    a.nrx = ceil_div(W, a.rw);
    a.nry = ceil_div(H, a.rh);
    if (tiles * a.chunks > kMaxGrid || (long long)a.nrx * a.nry > kMaxGrid) {
        set_error(ctx, "erp_equalize: too many tiles for one launch");
        return VIO_ENOSYS;
    }
    a.part = static_cast<uint32_t*>(ctx_buffer(ctx, kSlotEqHist, sizeof(uint32_t) * 256 * tiles * a.chunks * n_frames));
    a.lut = static_cast<uint8_t*>(ctx_buffer(ctx, kSlotEqLut, (size_t)256 * tiles * n_frames));
    if (!a.part || !a.lut) {
        set_error(ctx, "erp_equalize: device allocation failed");
        return VIO_ENOMEM;
    }
    hipEvent_t* ev = ctx->ev + kEvEq;
    int rc;
    if ((rc = events_ready(ctx, ev, 4))) return rc;
    const bool staged = ctx->eq_stage_timing;
    VIO_HIP(ctx, hipEventRecord(ev[0], ctx->stream));
    VIO_HIP(ctx, launch_eq_hist(a, ctx->stream));
    if (staged) VIO_HIP(ctx, hipEventRecord(ev[1], ctx->stream));
    VIO_HIP(ctx, launch_eq_lut(a, ctx->stream));
    if (staged) VIO_HIP(ctx, hipEventRecord(ev[2], ctx->stream));
    VIO_HIP(ctx, launch_eq_apply(a, ctx->stream));
    VIO_HIP(ctx, hipEventRecord(ev[3], ctx->stream));
    ctx->eq_staged = staged;
    return VIO_OK;
}

int erp_equalize(vio_ctx* ctx, const uint8_t* src, int W, int H, int stride, const erp_equalize_params* p, uint8_t* dst,
                 int dst_stride) {
    if (!ctx || !src || !dst) return VIO_EINVAL;
    if (check(p, W, H, stride, dst_stride)) {
        set_error(ctx, "erp_equalize: bad sizes, mode, tiles, clip limit or border mode");
        return VIO_EINVAL;
    }
    uint8_t *d_src = nullptr, *d_dst = nullptr;
    int sp = 0, dp = 0, rc;
    if ((rc = stage_rows(ctx, kSlotEqSrc, src, stride, W, H, 16, "erp_equalize", &d_src, &sp))) return rc;
    if ((rc = scratch_rows(ctx, kSlotEqDst, W, H, 16, "erp_equalize", &d_dst, &dp))) return rc;
    if ((rc = erp_equalize_device(ctx, d_src, W, H, sp, 1, p, d_dst, dp))) return rc;
    return fetch_rows(ctx, d_dst, dp, dst, dst_stride, W, H);
}

int erp_equalize_kernel_ms(vio_ctx* ctx, double* ms) {
    return ctx ? events_ms(ctx, ctx->ev[kEvEq], ctx->ev[kEvEq + 3], ms) : VIO_EINVAL;
}

int erp_equalize_set_stage_timing(vio_ctx* ctx, int on) {
    if (!ctx) return VIO_EINVAL;
    ctx->eq_stage_timing = on != 0;
    return VIO_OK;
}

int erp_equalize_stage_ms(vio_ctx* ctx, double* hist_ms, double* lut_ms, double* apply_ms) {
    if (!ctx || !hist_ms || !lut_ms || !apply_ms || !ctx->eq_staged) return VIO_EINVAL;
    const hipEvent_t* ev = ctx->ev + kEvEq;
    double* out[3] = {hist_ms, lut_ms, apply_ms};
    int rc = VIO_OK;
    for (int i = 0; i < 3 && !rc; ++i) rc = events_ms(ctx, ev[i], ev[i + 1], out[i]);
    return rc;
}

}  // extern "C"
