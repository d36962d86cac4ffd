// resize.hip — cv::resize(..., INTER_AREA) of the grayscale ERP frames before tracking.
//
// Reference: app/main.cpp:199-204 resizes every frame to (camera_width, camera_height) with
// INTER_AREA when the image size differs (3840x1920 -> 960x480 in the demo configuration).
// OpenCV 4.x takes its integer-factor "area fast" path there (modules/imgproc/src/resize.cpp,
// resizeAreaFast_ for uchar): dst = saturate_cast<uchar>(Σ block · (1.f / (fx·fy))), i.e. the block
// sum times the f32 reciprocal, rounded half-to-even — except 2x2 blocks, which OpenCV's
// ResizeAreaFastVec handles as (a + b + c + d + 2) >> 2 (round half up).  erp_resize_area[_device] take
// integer factors only (fx = W / dW, fy = H / dH exact; other sizes return VIO_ENOSYS).  OpenCV is not in
// /root/reference nor in this image, so parity with it is unpinned; the oracle restates that formula
// (oracle/resize_oracle.py) and the GPU matches it bitwise.
//
// erp_resize_area_any[_device] add every other downscale (4096x2048 or 5376x2688 -> 960x480, ...): OpenCV's
// general area path, computeResizeAreaTab + ResizeArea_Invoker<uchar, float>.  Per axis a tap table
// (source index, f32 weight) is built on the host in double, in OpenCV's expression order; an output pixel is
// sum_y beta * (sum_x src * alpha) in f32 with separate multiply and add roundings, taps in ascending source
// order, then saturate_cast<uchar> (half to even).  The taps of one output index are contiguous source
// indices, and only the first and the last weight differ from 1/cell, so the device table holds one 20-byte
// AreaTaps record per output column / row.  tests/resize_general_oracle.py restates this in numpy; the GPU
// matches it bitwise.
//
// Roofline: HBM-bound streaming, 1 + 1/(fx·fy) bytes per source pixel.  The factor-4 fast path gives
// each lane 4 output pixels on two output rows: eight 16-byte non-temporal row loads (two 16x4
// source blocks), no LDS; the grid covers (output row pair, 4-pixel group, frame).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "ctx.h"

namespace vio360 {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

struct ResizeArgs {
    const uint8_t* src;
    int W, H, stride;
    long long frame_bytes_src;
    uint8_t* dst;
    int dW, dH, dstride;
    long long frame_bytes_dst;
    int fx, fy;
    float scale;  // 1.f / (fx * fy)
};

__device__ __forceinline__ uint8_t area_round(int sum, float scale) {
    const float v = rintf((float)sum * scale);  // cvRound: half to even
    return (uint8_t)fminf(fmaxf(v, 0.f), 255.f);
}

__device__ __forceinline__ int sum_bytes4(uint32_t w) {
    return (int)(w & 0xff) + (int)((w >> 8) & 0xff) + (int)((w >> 16) & 0xff) + (int)(w >> 24);
}

// fx = fy = 4, dst width a multiple of 4, dst height even and 16-byte aligned source rows: lane ->
// 4 output pixels on each of two output rows (eight 16-byte streaming loads in flight per lane)
__global__ __launch_bounds__(256) void resize_area4_kernel(ResizeArgs a) {
    const int groups = a.dW >> 2;
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    const int y0 = 2 * blockIdx.y;
    const int f = blockIdx.z;
    if (g >= groups) return;
    const uint8_t* s = a.src + f * a.frame_bytes_src + (long long)(4 * y0) * a.stride + 16 * g;
    u32x4 r[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) r[k] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(s + (long long)k * a.stride));
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        uint32_t out = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            int sum = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const u32x4 v = r[4 * h + k];
                const uint32_t w = c == 0 ? v.x : (c == 1 ? v.y : (c == 2 ? v.z : v.w));
                sum += sum_bytes4(w);
            }
            out |= (uint32_t)area_round(sum, a.scale) << (8 * c);
        }
        *reinterpret_cast<uint32_t*>(a.dst + f * a.frame_bytes_dst + (long long)(y0 + h) * a.dstride + 4 * g) = out;
    }
}

// any integer factors: lane -> 1 output pixel
__global__ __launch_bounds__(256) void resize_area_kernel(ResizeArgs a) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y;
    const int f = blockIdx.z;
    if (x >= a.dW) return;
    const uint8_t* s = a.src + f * a.frame_bytes_src + (long long)(a.fy * y) * a.stride + a.fx * x;
    int sum = 0;
    for (int k = 0; k < a.fy; ++k)
        for (int j = 0; j < a.fx; ++j) sum += s[(long long)k * a.stride + j];
    // 2x2: ResizeAreaFastVec's (sum + 2) >> 2; every other factor: sum * (1.f / (fx fy)), cvRound
    a.dst[f * a.frame_bytes_dst + (long long)y * a.dstride + x] =
        (a.fx == 2 && a.fy == 2) ? (uint8_t)((sum + 2) >> 2) : area_round(sum, a.scale);
}

// the taps of one output column / row of the general path: source indices first .. first + count - 1, weight
// w_first for the first of them, w_last for the last (when count > 1), w_mid for the others
struct AreaTaps {
    int32_t first, count;
    float w_first, w_mid, w_last;
};

struct ResizeAnyArgs {
    const uint8_t* src;
    int stride;
    long long frame_bytes_src;
    uint8_t* dst;
    int dW, dstride;
    long long frame_bytes_dst;
    const AreaTaps* tx;  // dW records
    const AreaTaps* ty;  // dH records
};

__device__ __forceinline__ float tap_weight(int k, int count, float w_first, float w_mid, float w_last) {
    return k == 0 ? w_first : (k == count - 1 ? w_last : w_mid);
}

// any downscale: lane -> 1 output pixel; the host has checked every table record against [0, W) / [0, H).
// MAXT > 0 (no column has more than MAXT taps): a row's MAXT byte loads are issued together, a lane with fewer
// taps repeating its last address, and every lane adds MAXT products with weight 0.f past its last tap
// (buf + 0.f * v = buf exactly: buf is finite and never -0).  MAXT == 0: any tap count, one load per
// iteration.
template <int MAXT>
__global__ __launch_bounds__(256) void resize_area_general_kernel(ResizeAnyArgs a) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y;
    const int f = blockIdx.z;
    if (x >= a.dW) return;
    const int x0 = a.tx[x].first, nx = a.tx[x].count;
    const float ax_first = a.tx[x].w_first, ax_mid = a.tx[x].w_mid, ax_last = a.tx[x].w_last;
    const int y0 = a.ty[y].first, ny = a.ty[y].count;
    const float by_first = a.ty[y].w_first, by_mid = a.ty[y].w_mid, by_last = a.ty[y].w_last;
    const uint8_t* s = a.src + f * a.frame_bytes_src + (long long)y0 * a.stride + x0;
    float sum = 0.f;
    if constexpr (MAXT > 0) {
        float w[MAXT];
#pragma unroll
        for (int k = 0; k < MAXT; ++k) w[k] = k < nx ? tap_weight(k, nx, ax_first, ax_mid, ax_last) : 0.f;
        for (int j = 0; j < ny; ++j) {
            uint8_t v[MAXT];
#pragma unroll
            for (int k = 0; k < MAXT; ++k) v[k] = s[min(k, nx - 1)];
            float buf = (float)v[0] * w[0];  // = 0.f + it, exactly
#pragma unroll
            for (int k = 1; k < MAXT; ++k) buf = buf + (float)v[k] * w[k];
            sum = sum + tap_weight(j, ny, by_first, by_mid, by_last) * buf;
            s += a.stride;
        }
    } else {
        for (int j = 0; j < ny; ++j) {
            float buf = (float)s[0] * ax_first;
            for (int k = 1; k < nx - 1; ++k) buf = buf + (float)s[k] * ax_mid;
            if (nx > 1) buf = buf + (float)s[nx - 1] * ax_last;
            sum = sum + tap_weight(j, ny, by_first, by_mid, by_last) * buf;
            s += a.stride;
        }
    }
    const float v = rintf(sum);  // saturate_cast<uchar>: cvRound (half to even), then clamp
    a.dst[f * a.frame_bytes_dst + (long long)y * a.dstride + x] = (uint8_t)fminf(fmaxf(v, 0.f), 255.f);
}

}  // namespace vio360

using namespace vio360;

namespace {

struct AreaTap {
    int32_t di, si;
    float alpha;
};

// computeResizeAreaTab (OpenCV 4.x modules/imgproc/src/resize.cpp) for one axis, scale = ssize / dsize >= 1:
// IEEE double in this expression order (the file is built without FMA contraction)
void area_tab(int ssize, int dsize, std::vector<AreaTap>& tab) {
    const double scale = (double)ssize / dsize;
    tab.clear();
    for (int d = 0; d < dsize; ++d) {
        const double fsx1 = d * scale;
        const double fsx2 = fsx1 + scale;
        const double cell = std::min(scale, ssize - fsx1);
        int sx1 = (int)std::ceil(fsx1), sx2 = (int)std::floor(fsx2);
        sx2 = std::min(sx2, ssize - 1);
        sx1 = std::min(sx1, sx2);
        if (sx1 - fsx1 > 1e-3) tab.push_back({d, sx1 - 1, (float)((sx1 - fsx1) / cell)});
        for (int sx = sx1; sx < sx2; ++sx) tab.push_back({d, sx, (float)(1.0 / cell)});
        if (fsx2 - sx2 > 1e-3) tab.push_back({d, sx2, (float)(std::min(std::min(fsx2 - sx2, 1.0), cell) / cell)});
    }
}

// the tap list as one AreaTaps record per output index; false if the list is not of that shape (every output
// index present, contiguous ascending source indices within [0, ssize), equal inner weights)
bool area_tab_compact(const std::vector<AreaTap>& tab, int ssize, int dsize, std::vector<AreaTaps>& out) {
    out.assign(dsize, AreaTaps{0, 0, 0.f, 0.f, 0.f});
    size_t i = 0;
    for (int d = 0; d < dsize; ++d) {
        size_t e = i;
        while (e < tab.size() && tab[e].di == d) ++e;
        const int n = (int)(e - i);
        if (n < 1) return false;
        AreaTaps& r = out[d];
        r.first = tab[i].si;
        r.count = n;
        r.w_first = tab[i].alpha;
        r.w_last = tab[e - 1].alpha;
        r.w_mid = n > 2 ? tab[i + 1].alpha : 0.f;
        if (r.first < 0 || (long long)r.first + n > ssize) return false;
        for (int k = 0; k < n; ++k) {
            const float w = k == 0 ? r.w_first : (k == n - 1 ? r.w_last : r.w_mid);
            if (tab[i + k].si != r.first + k || std::memcmp(&w, &tab[i + k].alpha, sizeof(float))) return false;
        }
        i = e;
    }
    return i == tab.size();
}

// device tap tables of (W -> dW, H -> dH) in the context's two table slots, rebuilt when the sizes change
int general_tables(vio_ctx* ctx, int W, int dW, int H, int dH, const AreaTaps** d_tx, const AreaTaps** d_ty,
                   int* max_x_taps) {
    const int key[4] = {W, dW, H, dH};
    const bool hit = !std::memcmp(key, ctx->rsz_tab_key, sizeof(key)) && (int)ctx->bufs.size() > kSlotResizeTabY &&
                     ctx->bufs[kSlotResizeTabX] && ctx->bufs[kSlotResizeTabY];
    if (!hit) {
        std::memset(ctx->rsz_tab_key, 0, sizeof(key));
        std::vector<AreaTap> tab;
        std::vector<AreaTaps> hx, hy;
        area_tab(W, dW, tab);
        const bool okx = area_tab_compact(tab, W, dW, hx);
        area_tab(H, dH, tab);
        if (!okx || !area_tab_compact(tab, H, dH, hy)) {
            set_error(ctx, "erp_resize_area_any: tap table outside the source frame");
            return VIO_EINVAL;
        }
        void* bx = ctx_buffer(ctx, kSlotResizeTabX, sizeof(AreaTaps) * hx.size());
        void* by = ctx_buffer(ctx, kSlotResizeTabY, sizeof(AreaTaps) * hy.size());
        if (!bx || !by) {
            set_error(ctx, "erp_resize_area_any: device allocation failed");
            return VIO_ENOMEM;
        }
        // on the context stream, so after any kernel that still reads the previous tables; blocking, since the
        // host tables die with this scope
        VIO_HIP(ctx, hipMemcpyAsync(bx, hx.data(), sizeof(AreaTaps) * hx.size(), hipMemcpyHostToDevice, ctx->stream));
        VIO_HIP(ctx, hipMemcpyAsync(by, hy.data(), sizeof(AreaTaps) * hy.size(), hipMemcpyHostToDevice, ctx->stream));
        VIO_HIP(ctx, hipStreamSynchronize(ctx->stream));
        std::memcpy(ctx->rsz_tab_key, key, sizeof(key));
        ctx->rsz_max_x_taps = 0;
        for (const AreaTaps& r : hx) ctx->rsz_max_x_taps = std::max(ctx->rsz_max_x_taps, (int)r.count);
    }
    *max_x_taps = ctx->rsz_max_x_taps;
    *d_tx = static_cast<const AreaTaps*>(ctx->bufs[kSlotResizeTabX]);
    *d_ty = static_cast<const AreaTaps*>(ctx->bufs[kSlotResizeTabY]);
    return VIO_OK;
}

}  // namespace

static int resize_check(int W, int H, int stride, int dW, int dH, int dstride, int n_frames) {
    if (W <= 0 || H <= 0 || dW <= 0 || dH <= 0 || stride < W || dstride < dW || n_frames < 0) return VIO_EINVAL;
    if (W % dW || H % dH) return VIO_ENOSYS;
    if ((long long)(W / dW) * (H / dH) > (1 << 23)) return VIO_ENOSYS;  // int block sums
    return VIO_OK;
}

extern "C" int erp_resize_area_device(vio_ctx* ctx, const uint8_t* src, int W, int H, int stride, int n_frames,
                                      uint8_t* dst, int dW, int dH, int dst_stride) {
    if (!ctx || !src || !dst) return VIO_EINVAL;
    int rc = resize_check(W, H, stride, dW, dH, dst_stride, n_frames);
    if (rc) {
        set_error(ctx, rc == VIO_ENOSYS ? "erp_resize_area: only integer downscale factors are supported"
                                        : "erp_resize_area: bad sizes");
        return rc;
    }
    if (n_frames == 0) return VIO_OK;
    ResizeArgs a;
    a.src = src;
    a.W = W;
    a.H = H;
    a.stride = stride;
    a.frame_bytes_src = (long long)stride * H;
    a.dst = dst;
    a.dW = dW;
    a.dH = dH;
    a.dstride = dst_stride;
    a.frame_bytes_dst = (long long)dst_stride * dH;
    a.fx = W / dW;
    a.fy = H / dH;
    a.scale = 1.f / (float)(a.fx * a.fy);
    VIO_DEVICE(ctx);
    for (hipEvent_t& ev : ctx->rsz_ev)
        if (!ev) VIO_HIP(ctx, hipEventCreate(&ev));
    VIO_HIP(ctx, hipEventRecord(ctx->rsz_ev[0], ctx->stream));
    const bool fast = a.fx == 4 && a.fy == 4 && dW % 4 == 0 && dH % 2 == 0 && stride % 16 == 0 && dst_stride % 4 == 0 &&
                      (reinterpret_cast<uintptr_t>(src) & 15) == 0 && (reinterpret_cast<uintptr_t>(dst) & 3) == 0;
    if (fast) {
        const int groups = dW / 4;
        hipLaunchKernelGGL(resize_area4_kernel, dim3((groups + 255) / 256, dH / 2, n_frames), dim3(256), 0, ctx->stream,
                           a);
    } else {
        hipLaunchKernelGGL(resize_area_kernel, dim3((dW + 255) / 256, dH, n_frames), dim3(256), 0, ctx->stream, a);
    }
    VIO_HIP(ctx, hipGetLastError());
    VIO_HIP(ctx, hipEventRecord(ctx->rsz_ev[1], ctx->stream));
    return VIO_OK;
}

extern "C" int erp_resize_area(vio_ctx* ctx, const uint8_t* src, int W, int H, int stride, uint8_t* dst, int dW,
                               int dH, int dst_stride) {
    if (!ctx || !src || !dst) return VIO_EINVAL;
    int rc = resize_check(W, H, stride, dW, dH, dst_stride, 1);
    if (rc) {
        set_error(ctx, rc == VIO_ENOSYS ? "erp_resize_area: only integer downscale factors are supported"
                                        : "erp_resize_area: bad sizes");
        return rc;
    }
    // device copies with 16-byte-aligned pitches (fast path)
    const int sp = (W + 15) & ~15, dp = (dW + 3) & ~3;
    uint8_t* d_src = static_cast<uint8_t*>(ctx_buffer(ctx, kSlotResizeSrc, (size_t)sp * H));
    uint8_t* d_dst = static_cast<uint8_t*>(ctx_buffer(ctx, kSlotResizeDst, (size_t)dp * dH));
    if (!d_src || !d_dst) {
        set_error(ctx, "erp_resize_area: device allocation failed");
        return VIO_ENOMEM;
    }
    VIO_DEVICE(ctx);
    VIO_HIP(ctx, hipMemcpy2DAsync(d_src, sp, src, stride, W, H, hipMemcpyHostToDevice, ctx->stream));
    if ((rc = erp_resize_area_device(ctx, d_src, W, H, sp, 1, d_dst, dW, dH, dp))) return rc;
    VIO_HIP(ctx, hipMemcpy2DAsync(dst, dst_stride, d_dst, dp, dW, dH, hipMemcpyDeviceToHost, ctx->stream));
    VIO_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return VIO_OK;
}

// 0: integer factors (the area-fast kernels), 1: the general path, < 0: error (set on ctx)
static int resize_any_check(vio_ctx* ctx, int W, int H, int stride, int dW, int dH, int dstride, int n_frames) {
    if (W <= 0 || H <= 0 || dW <= 0 || dH <= 0 || stride < W || dstride < dW || n_frames < 0) {
        set_error(ctx, "erp_resize_area_any: bad sizes");
        return VIO_EINVAL;
    }
    if (dW > W || dH > H) {
        set_error(ctx, "erp_resize_area_any: enlarging is not supported");
        return VIO_ENOSYS;
    }
    return (W % dW || H % dH) ? 1 : 0;
}

extern "C" int erp_resize_area_any_device(vio_ctx* ctx, const uint8_t* src, int W, int H, int stride, int n_frames,
                                          uint8_t* dst, int dW, int dH, int dst_stride) {
    if (!ctx || !src || !dst) return VIO_EINVAL;
    const int path = resize_any_check(ctx, W, H, stride, dW, dH, dst_stride, n_frames);
    if (path < 0) return path;
    if (path == 0) return erp_resize_area_device(ctx, src, W, H, stride, n_frames, dst, dW, dH, dst_stride);
    if (n_frames == 0) return VIO_OK;
    VIO_DEVICE(ctx);
    ResizeAnyArgs a;
    int max_x_taps = 0;
    int rc = general_tables(ctx, W, dW, H, dH, &a.tx, &a.ty, &max_x_taps);
    if (rc) return rc;
    a.src = src;
    a.stride = stride;
    a.frame_bytes_src = (long long)stride * H;
    a.dst = dst;
    a.dW = dW;
    a.dstride = dst_stride;
    a.frame_bytes_dst = (long long)dst_stride * dH;
    for (hipEvent_t& ev : ctx->rsz_ev)
        if (!ev) VIO_HIP(ctx, hipEventCreate(&ev));
    VIO_HIP(ctx, hipEventRecord(ctx->rsz_ev[0], ctx->stream));
    const dim3 grid((dW + 255) / 256, dH, n_frames);
    if (max_x_taps <= 4) hipLaunchKernelGGL(resize_area_general_kernel<4>, grid, dim3(256), 0, ctx->stream, a);
    else if (max_x_taps <= 8) hipLaunchKernelGGL(resize_area_general_kernel<8>, grid, dim3(256), 0, ctx->stream, a);
    else hipLaunchKernelGGL(resize_area_general_kernel<0>, grid, dim3(256), 0, ctx->stream, a);
    VIO_HIP(ctx, hipGetLastError());
    VIO_HIP(ctx, hipEventRecord(ctx->rsz_ev[1], ctx->stream));
    return VIO_OK;
}

extern "C" int erp_resize_area_any(vio_ctx* ctx, const uint8_t* src, int W, int H, int stride, uint8_t* dst, int dW,
                                   int dH, int dst_stride) {
    if (!ctx || !src || !dst) return VIO_EINVAL;
    const int path = resize_any_check(ctx, W, H, stride, dW, dH, dst_stride, 1);
    if (path < 0) return path;
    if (path == 0) return erp_resize_area(ctx, src, W, H, stride, dst, dW, dH, dst_stride);
    const int sp = (W + 15) & ~15, dp = (dW + 3) & ~3;  // the pitches of erp_resize_area's device copies
    uint8_t* d_src = static_cast<uint8_t*>(ctx_buffer(ctx, kSlotResizeSrc, (size_t)sp * H));
    uint8_t* d_dst = static_cast<uint8_t*>(ctx_buffer(ctx, kSlotResizeDst, (size_t)dp * dH));
    if (!d_src || !d_dst) {
        set_error(ctx, "erp_resize_area_any: device allocation failed");
        return VIO_ENOMEM;
    }
    VIO_DEVICE(ctx);
    int rc;
    VIO_HIP(ctx, hipMemcpy2DAsync(d_src, sp, src, stride, W, H, hipMemcpyHostToDevice, ctx->stream));
    if ((rc = erp_resize_area_any_device(ctx, d_src, W, H, sp, 1, d_dst, dW, dH, dp))) return rc;
    VIO_HIP(ctx, hipMemcpy2DAsync(dst, dst_stride, d_dst, dp, dW, dH, hipMemcpyDeviceToHost, ctx->stream));
    VIO_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return VIO_OK;
}

extern "C" int erp_resize_area_tab(int ssize, int dsize, int32_t* di, int32_t* si, float* alpha, int cap, int* n) {
    if (ssize <= 0 || dsize <= 0 || cap < 0 || !n || (cap > 0 && (!di || !si || !alpha))) return VIO_EINVAL;
    if (dsize > ssize) return VIO_ENOSYS;
    std::vector<AreaTap> tab;
    area_tab(ssize, dsize, tab);
    const int m = std::min(cap, (int)tab.size());
    for (int i = 0; i < m; ++i) {
        di[i] = tab[i].di;
        si[i] = tab[i].si;
        alpha[i] = tab[i].alpha;
    }
    *n = (int)tab.size();
    return VIO_OK;
}

extern "C" int erp_resize_area_kernel_ms(vio_ctx* ctx, double* ms) {
    if (!ctx || !ms || !ctx->rsz_ev[1]) return VIO_EINVAL;
    float f = 0.f;
    VIO_HIP(ctx, hipEventSynchronize(ctx->rsz_ev[1]));
    VIO_HIP(ctx, hipEventElapsedTime(&f, ctx->rsz_ev[0], ctx->rsz_ev[1]));
    *ms = f;
    return VIO_OK;
}
