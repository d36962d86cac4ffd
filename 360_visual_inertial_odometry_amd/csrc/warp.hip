// warp.hip — the lens-to-ERP warp kernel: cv::remap(..., INTER_LINEAR) in exact integer arithmetic, fused with the
// luma rules (erp_warp_*, include/vio360.h; host side in warp_host.cpp).
//
// No 360 camera delivers an equirectangular frame: the sensors give two fisheye circles, an equi-angular cubemap
// or a cubemap, and an ERP source often needs a fixed rotation.  The reference leaves that to whoever produces its
// input images (app/main.cpp:199-204 only resizes); here it is one map-driven pass on the device.  OpenCV is not
// available to this project, so parity with cv::remap is unpinned: the contract is the arithmetic below, restated
// in numpy by tests/warp_oracle.py, which this kernel matches bitwise.
//
// One lane per destination pixel; the grid is (256-column tile, row) in launch order (giving each XCD a contiguous
// range of blocks, as trk_lk.hip and trk_gftt.hip do, measured 5 to 30 % slower: DESIGN 4.7).  A lane's map entry
// (quantised on the host, WarpEntry) is one aligned 8-byte load and stays in registers while the lane loops over the frames of
// the launch, so the map is read once per launch.  The taps are loaded from addresses clamped into the source
// frame, whatever the border modes, and a tap that the modes put outside the frame is replaced by border_value
// afterwards: nothing outside [0, sW bpp) of a source row or outside rows [0, sH) is ever read.  No LDS, no scratch.
#include <hip/hip_runtime.h>

#include "warp.h"

namespace vio360 {

// The u8 values of source pixels c and c + 1 of a row, both inside it, from one run of loads at s = row + c * step
// (the route VIO_WARP_ROUTE_AUTO): 2 bytes for grey, one dword for 4:2:2, a dword and a ushort for 3-byte pixels,
// 8 bytes for 4-byte pixels, at any alignment; exactly the bytes of the two pixels are read.  p holds bit shifts
// (kPixByte: o0 of the luma byte).
template <int MODE>
__device__ __forceinline__ void pix_pair(const uint8_t* s, const PixSrc& p, int& lo, int& hi) {
    if constexpr (MODE == kPixGray) {
        uint16_t w;
        __builtin_memcpy(&w, s, 2);
        lo = w & 0xff;
        hi = w >> 8;
    } else if constexpr (MODE == kPixByte) {
        uint32_t w;
        __builtin_memcpy(&w, s, 4);
        lo = (w >> p.o0) & 0xff;
        hi = (w >> (16 + p.o0)) & 0xff;
    } else if constexpr (MODE == kPixBytes3) {
        uint32_t w0;
        uint16_t w1;
        __builtin_memcpy(&w0, s, 4);
        __builtin_memcpy(&w1, s + 4, 2);
        lo = word_luma(w0, p);
        hi = word_luma((w0 >> 24) | ((uint32_t)w1 << 8), p);
    } else {
        static_assert(MODE == kPixDword, "4-byte pixels");
        uint32_t w[2];
        __builtin_memcpy(w, s, 8);
        lo = word_luma(w[0], p);
        hi = word_luma(w[1], p);
    }
}

// one pixel of the same source, bytewise (the wrap seam of the pair route)
template <int MODE>
__device__ __forceinline__ int pix_single(const uint8_t* s, const PixSrc& p) {
    if constexpr (MODE == kPixGray) return s[0];
    else if constexpr (MODE == kPixByte) return s[p.o0 >> 3];
    else return luma_u8(s[p.o0 >> 3], s[p.o1 >> 3], s[p.o2 >> 3], p.rule);
}

// PAIR = false: one load (three byte loads for kPixBytes3) per tap, the pixel sources of pix_dev.h.
// PAIR = true (sW >= 2): the taps of a row are two neighbouring pixels except at the wrap seam, so a lane loads the
// pixel pair (c, c + 1) with c = clamp(x0, 0, sW - 2), which lies inside the row and holds both clamped tap columns,
// and picks its taps from it; only a lane on the wrap seam (x0 = sW - 1, x1 = 0) loads column 0 on its own.
template <int MODE, bool PAIR>
__global__ __launch_bounds__(256) void warp_kernel(WarpArgs a) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    const int y = blockIdx.y;
    if (x >= a.dW) return;
    const WarpEntry e = a.map[(long long)y * a.dW + x];
    const bool valid = e.qy != kWarpInvalid;
    const int fa = e.qx & 31, fb = e.qy & 31;
    const int x0 = e.qx >> 5, y0 = e.qy >> 5;  // floor
    int x1 = x0 + 1;
    const int y1 = y0 + 1;
    if (a.wrap_x && x1 >= a.sW) x1 -= a.sW;  // the host keeps x0 in [0, sW) under wrap
    const bool in_x0 = a.wrap_x || (unsigned)x0 < (unsigned)a.sW, in_x1 = a.wrap_x || (unsigned)x1 < (unsigned)a.sW;
    const bool in_y0 = a.replicate_y || (unsigned)y0 < (unsigned)a.sH, in_y1 = a.replicate_y || (unsigned)y1 < (unsigned)a.sH;
    // the columns and rows that are loaded: always inside the frame (this is also the row clamp of Y_REPLICATE)
    const int step = PAIR ? (MODE == kPixGray ? 1 : (MODE == kPixByte ? 2 : (MODE == kPixBytes3 ? 3 : 4))) : pix_step<MODE>(a.px);
    const int xc0 = min(max(x0, 0), a.sW - 1), xc1 = min(max(x1, 0), a.sW - 1);
    const long long r0 = (long long)min(max(y0, 0), a.sH - 1) * a.stride, r1 = (long long)min(max(y1, 0), a.sH - 1) * a.stride;
    const int w00 = (32 - fa) * (32 - fb), w01 = fa * (32 - fb), w10 = (32 - fa) * fb, w11 = fa * fb;  // sum 1024
    const int bv = a.border_value;
    const int cp = min(xc0, a.sW - 2);           // PAIR: the pair's first column
    const bool hi0 = xc0 != cp, hi1 = xc1 != cp;  // PAIR: the tap is the pair's second pixel ...
    const bool seam = (unsigned)(xc1 - cp) > 1u;  // ... or, for x1 on the wrap seam, not in the pair
    const long long c0 = (long long)(PAIR ? cp : xc0) * step, c1 = (long long)xc1 * step;
    const uint8_t* s = a.src;
    uint8_t* d = a.dst + (long long)y * a.dstride + x;
    for (int f = 0; f < a.n_frames; ++f) {
        int p00, p01, p10, p11;
        if constexpr (PAIR) {
            int lo0, up0, lo1, up1;
            pix_pair<MODE>(s + r0 + c0, a.px, lo0, up0);
            pix_pair<MODE>(s + r1 + c0, a.px, lo1, up1);
            p00 = hi0 ? up0 : lo0;
            p01 = hi1 ? up0 : lo0;
            p10 = hi0 ? up1 : lo1;
            p11 = hi1 ? up1 : lo1;
            if (seam) {
                p01 = pix_single<MODE>(s + r0 + c1, a.px);
                p11 = pix_single<MODE>(s + r1 + c1, a.px);
            }
        } else {
            p00 = pix_value<MODE>(s + r0 + c0, a.px), p01 = pix_value<MODE>(s + r0 + c1, a.px);
            p10 = pix_value<MODE>(s + r1 + c0, a.px), p11 = pix_value<MODE>(s + r1 + c1, a.px);
        }
        const int v = w00 * (in_x0 && in_y0 ? p00 : bv) + w01 * (in_x1 && in_y0 ? p01 : bv) +
                      w10 * (in_x0 && in_y1 ? p10 : bv) + w11 * (in_x1 && in_y1 ? p11 : bv);
        *d = (uint8_t)(valid ? (v + 512) >> 10 : bv);
        s += a.frame_bytes_src;
        d += a.frame_bytes_dst;
    }
}

template <bool PAIR>
static void launch_mode(const WarpArgs& a, int mode, hipStream_t stream) {
    const dim3 grid((a.dW + 255) >> 8, a.dH), block(256);
    if (mode == kPixGray) hipLaunchKernelGGL((warp_kernel<kPixGray, PAIR>), grid, block, 0, stream, a);
    else if (mode == kPixByte) hipLaunchKernelGGL((warp_kernel<kPixByte, PAIR>), grid, block, 0, stream, a);
    else if (mode == kPixBytes3) hipLaunchKernelGGL((warp_kernel<kPixBytes3, PAIR>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((warp_kernel<kPixDword, PAIR>), grid, block, 0, stream, a);
}

hipError_t launch_warp(const WarpArgs& a, int mode, bool pair, hipStream_t stream) {
    if (mode < kPixGray || mode > kPixDword || (pair && a.sW < 2)) return hipErrorInvalidValue;
    if (pair) launch_mode<true>(a, mode, stream);
    else launch_mode<false>(a, mode, stream);
    return hipGetLastError();
}

}  // namespace vio360
