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
// erp_ingest[_device] take packed colour (BGR / RGB / BGRA / RGBA) and packed 4:2:2 (YUYV / UYVY) frames: the
// one-lane-per-pixel kernels are templates on where the u8 value of a source pixel comes from (PixSrc, pix_dev.h), and
// for those formats it is the integer luma of luma_dev.h, computed in registers.  The result is bit for bit
// erp_resize_area_any of the grey image, which is never stored (tests/ingest_oracle.py).
//
// Roofline: HBM-bound streaming, 1 + 1/(fx·fy) bytes per source pixel.  The factor-4 fast path gives
// each lane 4 output pixels on two output rows: eight 16-byte non-temporal row loads (two 16x4
// source blocks), no LDS; the grid covers (output row pair, 4-pixel group, frame).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "luma_dev.h"
#include "resize.h"

namespace vio360 {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// Where the one-lane-per-pixel kernels take the u8 value of a source pixel from: PixSrc / pix_value of pix_dev.h.

// the 3 N bytes at s (any alignment) into r[0 .. 3 N / 4]: whole dwords first, the last 3 N % 4 bytes one by one,
// so exactly [s, s + 3 N) is read
template <int N>
__device__ __forceinline__ void load_run3(const uint8_t* s, uint32_t (&r)[3 * N / 4 + 1]) {
    constexpr int kFull = 3 * N / 4;
#pragma unroll
    for (int d = 0; d < kFull; ++d) __builtin_memcpy(&r[d], s + 4 * d, 4);
    r[kFull] = 0;
#pragma unroll
    for (int b = 0; b < 3 * N % 4; ++b) r[kFull] |= (uint32_t)s[4 * kFull + b] << (8 * b);
}

// pixel k of such a run: its three bytes in the low 24 bits
template <int N>
__device__ __forceinline__ uint32_t run3_pixel(const uint32_t (&r)[3 * N / 4 + 1], int k) {
    const int i = 3 * k, d = i >> 2, b = i & 3;  // constants once the caller's loop is unrolled
    return b <= 1 ? r[d] >> (8 * b) : __builtin_amdgcn_alignbyte(r[d + 1], r[d], b);
}

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

// packed -> pitched u8 plane (erp_ingest* with dW == W and dH == H): lane -> 1 pixel
template <int MODE>
__global__ __launch_bounds__(256) void ingest_convert_kernel(ResizeArgs a) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y;
    const int f = blockIdx.z;
    if (x >= a.dW) return;
    const uint8_t* s = a.src + f * a.frame_bytes_src + (long long)y * a.stride + (long long)x * pix_step<MODE>(a.px);
    a.dst[f * a.frame_bytes_dst + (long long)y * a.dstride + x] = pix_value<MODE>(s, a.px);
}

// any integer factors: lane -> 1 output pixel
template <int MODE>
__global__ __launch_bounds__(256) void resize_area_kernel(ResizeArgs a) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y;
    const int f = blockIdx.z;
    if (x >= a.dW) return;
    const int step = pix_step<MODE>(a.px);
    const uint8_t* s = a.src + f * a.frame_bytes_src + (long long)(a.fy * y) * a.stride + (long long)(a.fx * x) * step;
    int sum = 0;
    for (int k = 0; k < a.fy; ++k)
        for (int j = 0; j < a.fx; ++j) sum += pix_value<MODE>(s + (long long)k * a.stride + j * step, a.px);
    // 2x2: ResizeAreaFastVec's (sum + 2) >> 2; every other factor: sum * (1.f / (fx fy)), cvRound
    a.dst[f * a.frame_bytes_dst + (long long)y * a.dstride + x] =
        (a.fx == 2 && a.fy == 2) ? (uint8_t)((sum + 2) >> 2) : area_round(sum, a.scale);
}

// the same for BGR / RGB with fx = FX: a block row is one run of FX pixels (kPixRun3)
template <int FX>
__global__ __launch_bounds__(256) void resize_area_run3_kernel(ResizeArgs a) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y;
    const int f = blockIdx.z;
    if (x >= a.dW) return;
    const uint8_t* s = a.src + f * a.frame_bytes_src + (long long)(a.fy * y) * a.stride + (long long)(FX * x) * 3;
    int sum = 0;
    for (int k = 0; k < a.fy; ++k) {
        uint32_t r[3 * FX / 4 + 1];
        load_run3<FX>(s + (long long)k * a.stride, r);
#pragma unroll
        for (int j = 0; j < FX; ++j) sum += word_luma(run3_pixel<FX>(r, j), a.px);
    }
    a.dst[f * a.frame_bytes_dst + (long long)y * a.dstride + x] =
        (FX == 2 && a.fy == 2) ? (uint8_t)((sum + 2) >> 2) : area_round(sum, a.scale);
}

__device__ __forceinline__ float tap_weight(int k, int count, float w_first, float w_mid, float w_last) {
    return k == 0 ? w_first : (k == count - 1 ? w_last : w_mid);
}

// any downscale: lane -> 1 output pixel; the host has checked every table record against [0, W) / [0, H).
// MAXT > 0 (no column has more than MAXT taps): a row's MAXT byte loads are issued together, a lane with fewer
// taps repeating its last address, and every lane adds MAXT products with weight 0.f past its last tap
// (buf + 0.f * v = buf exactly: buf is finite and never -0).  MAXT == 0: any tap count, one load per
// iteration.  kPixRun3 (MAXT > 0, W >= MAXT): every lane loads a run of MAXT pixels, the one that starts at its
// first tap or, where that would pass the end of the row, the last MAXT pixels of the row; its taps then sit `sh`
// pixels into the run and the weights before them are 0.f as well (0.f + x = x exactly).
template <int MAXT, int MODE>
__global__ __launch_bounds__(256) void resize_area_general_kernel(ResizeAnyArgs a) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y;
    const int f = blockIdx.z;
    if (x >= a.dW) return;
    const int x0 = a.tx[x].first, nx = a.tx[x].count;
    const float ax_first = a.tx[x].w_first, ax_mid = a.tx[x].w_mid, ax_last = a.tx[x].w_last;
    const int y0 = a.ty[y].first, ny = a.ty[y].count;
    const float by_first = a.ty[y].w_first, by_mid = a.ty[y].w_mid, by_last = a.ty[y].w_last;
    const int step = pix_step<MODE>(a.px);
    const uint8_t* s = a.src + f * a.frame_bytes_src + (long long)y0 * a.stride + (long long)x0 * step;
    float sum = 0.f;
    if constexpr (MAXT > 0) {
        float w[MAXT];
        if constexpr (MODE == kPixRun3) {
            const int sh = x0 - min(x0, a.W - MAXT);
            s -= sh * 3;
#pragma unroll
            for (int k = 0; k < MAXT; ++k)
                w[k] = (k >= sh && k - sh < nx) ? tap_weight(k - sh, nx, ax_first, ax_mid, ax_last) : 0.f;
        } else {
#pragma unroll
            for (int k = 0; k < MAXT; ++k) w[k] = k < nx ? tap_weight(k, nx, ax_first, ax_mid, ax_last) : 0.f;
        }
        for (int j = 0; j < ny; ++j) {
            uint8_t v[MAXT];
            if constexpr (MODE == kPixRun3) {
                uint32_t r[3 * MAXT / 4 + 1];
                load_run3<MAXT>(s, r);
#pragma unroll
                for (int k = 0; k < MAXT; ++k) v[k] = word_luma(run3_pixel<MAXT>(r, k), a.px);
            } else {
#pragma unroll
                for (int k = 0; k < MAXT; ++k) v[k] = pix_value<MODE>(s + min(k, nx - 1) * step, a.px);
            }
            float buf = (float)v[0] * w[0];  // = 0.f + it, exactly
#pragma unroll
            for (int k = 1; k < MAXT; ++k) buf = buf + (float)v[k] * w[k];
            sum = sum + tap_weight(j, ny, by_first, by_mid, by_last) * buf;
            s += a.stride;
        }
    } else if constexpr (MODE != kPixRun3) {
        for (int j = 0; j < ny; ++j) {
            float buf = (float)pix_value<MODE>(s, a.px) * ax_first;
            for (int k = 1; k < nx - 1; ++k) buf = buf + (float)pix_value<MODE>(s + k * step, a.px) * ax_mid;
            if (nx > 1) buf = buf + (float)pix_value<MODE>(s + (nx - 1) * step, a.px) * ax_last;
            sum = sum + tap_weight(j, ny, by_first, by_mid, by_last) * buf;
            s += a.stride;
        }
    }
    const float v = rintf(sum);  // saturate_cast<uchar>: cvRound (half to even), then clamp
    a.dst[f * a.frame_bytes_dst + (long long)y * a.dstride + x] = (uint8_t)fminf(fmaxf(v, 0.f), 255.f);
}

// the integer-factor kernel of a pixel source (grey: the factor-4 kernel where it applies)
hipError_t launch_area_integer(const ResizeArgs& a, int mode, int n_frames, hipStream_t stream) {
    const dim3 grid((a.dW + 255) / 256, a.dH, n_frames);
    const bool fast = mode == kPixGray && a.fx == 4 && a.fy == 4 && a.dW % 4 == 0 && a.dH % 2 == 0 &&
                      a.stride % 16 == 0 && a.dstride % 4 == 0 && (reinterpret_cast<uintptr_t>(a.src) & 15) == 0 &&
                      (reinterpret_cast<uintptr_t>(a.dst) & 3) == 0;
    if (fast) {
        const int groups = a.dW / 4;
        hipLaunchKernelGGL(resize_area4_kernel, dim3((groups + 255) / 256, a.dH / 2, n_frames), dim3(256), 0, stream, a);
    } else if (mode == kPixGray) {
        hipLaunchKernelGGL(resize_area_kernel<kPixGray>, grid, dim3(256), 0, stream, a);
    } else if (mode == kPixByte) {
        hipLaunchKernelGGL(resize_area_kernel<kPixByte>, grid, dim3(256), 0, stream, a);
    } else if (mode == kPixBytes3) {
        hipLaunchKernelGGL(resize_area_kernel<kPixBytes3>, grid, dim3(256), 0, stream, a);
    } else if (mode == kPixDword) {
        hipLaunchKernelGGL(resize_area_kernel<kPixDword>, grid, dim3(256), 0, stream, a);
    } else if (a.fx == 2) {
        hipLaunchKernelGGL(resize_area_run3_kernel<2>, grid, dim3(256), 0, stream, a);
    } else {  // kPixRun3 is chosen for fx 2 and 4 only
        hipLaunchKernelGGL(resize_area_run3_kernel<4>, grid, dim3(256), 0, stream, a);
    }
    return hipGetLastError();
}

template <int MODE>
static void launch_general_mode(const ResizeAnyArgs& a, const dim3& grid, int max_x_taps, hipStream_t stream) {
    if (max_x_taps <= 4) hipLaunchKernelGGL((resize_area_general_kernel<4, MODE>), grid, dim3(256), 0, stream, a);
    else if (max_x_taps <= 8) hipLaunchKernelGGL((resize_area_general_kernel<8, MODE>), grid, dim3(256), 0, stream, a);
    else hipLaunchKernelGGL((resize_area_general_kernel<0, MODE>), grid, dim3(256), 0, stream, a);
}

hipError_t launch_area_general(const ResizeAnyArgs& a, int mode, int dH, int n_frames, int max_x_taps,
                               hipStream_t stream) {
    const dim3 grid((a.dW + 255) / 256, dH, n_frames);
    if (mode == kPixGray) launch_general_mode<kPixGray>(a, grid, max_x_taps, stream);
    else if (mode == kPixByte) launch_general_mode<kPixByte>(a, grid, max_x_taps, stream);
    else if (mode == kPixBytes3) launch_general_mode<kPixBytes3>(a, grid, max_x_taps, stream);
    else if (mode == kPixDword) launch_general_mode<kPixDword>(a, grid, max_x_taps, stream);
    else if (max_x_taps <= 4) hipLaunchKernelGGL((resize_area_general_kernel<4, kPixRun3>), grid, dim3(256), 0, stream, a);
    else hipLaunchKernelGGL((resize_area_general_kernel<8, kPixRun3>), grid, dim3(256), 0, stream, a);  // <= 8
    return hipGetLastError();
}

hipError_t launch_ingest_convert(const ResizeArgs& a, int mode, int n_frames, hipStream_t stream) {
    const dim3 grid((a.dW + 255) / 256, a.dH, n_frames);
    if (mode == kPixByte) hipLaunchKernelGGL(ingest_convert_kernel<kPixByte>, grid, dim3(256), 0, stream, a);
    else if (mode == kPixBytes3) hipLaunchKernelGGL(ingest_convert_kernel<kPixBytes3>, grid, dim3(256), 0, stream, a);
    else hipLaunchKernelGGL(ingest_convert_kernel<kPixDword>, grid, dim3(256), 0, stream, a);
    return hipGetLastError();
}

}  // namespace vio360
