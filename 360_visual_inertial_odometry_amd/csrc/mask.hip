// mask.hip — region masks of the ERP tracker on MI355X (gfx950): erp_mask_* (include/vio360.h; host side in
// mask_host.cpp).
//
// A usable-region mask (u8, nonzero = usable) is painted on the camera frame, the lens image or the tracker frame.
// The tracker holds it as an exclusion bit-plane in the layout of its disc plane (mask.h), so every kernel here
// ends in, or works on, 32-pixel words:
//
//   mask_reduce_kernel    one lane per destination pixel: the AND over the pixel's INTER_AREA footprint (the taps
//                         of erp_resize_area_tab per axis, a rectangle of the source), 8 source bytes per load and a
//                         zero-byte test on the word; a wave's ballot is two words of the plane.  The source is read
//                         once (neighbouring footprints of a non-integer scale share their edge pixel).
//   mask_warp_kernel      one lane per pixel of a warp's destination: the map entry is valid and its four taps are
//                         inside the source (under the warp's border modes) and usable; packed by the same ballot.
//   mask_erode_h_kernel   one workgroup per row, the row in LDS extended by r bits on both sides (zeros, or the
//                         row's own bits modulo W under X_WRAP: funnel shifts across the words, the wrap carried
//                         through the last, partial word); the OR over 2r + 1 shifts by span doubling,
//                         D(k + d)(x) = D(k)(x) | D(k)(x + d) with d <= k: about log2(2r + 1) passes over the words.
//   mask_erode_v_kernel   one lane per word: the OR over the rows y - r .. y + r inside the image.
//   mask_unpack_kernel    plane -> 0 / 255 bytes;  mask_gather_kernel: the bit under each tracked point.
// All of it is integer: tests/mask_oracle.py restates the rules and these kernels match it bit for bit.
#include <hip/hip_runtime.h>

#include "mask.h"

namespace vio360 {

namespace {

// bits [p, p + n) of a row of `words` words as the low n bits, 1 <= n <= 32, p + n <= 32 words
__device__ __forceinline__ uint32_t take_bits(const uint32_t* row, int words, int p, int n) {
    const int w = p >> 5, s = p & 31;
    const uint32_t lo = row[w], hi = (s && w + 1 < words) ? row[w + 1] : 0u;
    const uint32_t v = (uint32_t)((((uint64_t)hi << 32) | lo) >> s);
    return n == 32 ? v : v & ((1u << n) - 1u);
}

// some byte of row[lo .. hi] is zero; every load lies inside row[0, sW)
__device__ __forceinline__ bool bytes_have_zero(const uint8_t* row, int sW, int lo, int hi) {
    if (sW < 8) {
        bool z = false;
        for (int c = lo; c <= hi; ++c) z |= row[c] == 0;
        return z;
    }
    bool z = false;
    for (int c = lo; c <= hi;) {
        const int start = min(c, sW - 8), off = c - start, n = min(hi - c + 1, 8 - off);
        uint64_t v;
        __builtin_memcpy(&v, row + start, 8);
        v >>= 8 * off;  // the bytes below the footprint leave: a borrow out of them cannot flag a byte of it
        const uint64_t zero = (v - 0x0101010101010101ull) & ~v & 0x8080808080808080ull;
        const uint64_t m = n == 8 ? ~0ull : ((1ull << (8 * n)) - 1ull);
        z |= (zero & m) != 0ull;  // (a flag above a zero byte may be false, the lowest flag never is)
        c += n;
    }
    return z;
}

// some bit of row[lo .. hi] is set
__device__ __forceinline__ bool bits_have_one(const uint32_t* row, int lo, int hi) {
    bool one = false;
    for (int w = lo >> 5; w <= hi >> 5; ++w) {
        const int b0 = max(lo - 32 * w, 0), b1 = min(hi - 32 * w, 31);
        const uint32_t m = (b1 - b0 == 31) ? 0xffffffffu : (((1u << (b1 - b0 + 1)) - 1u) << b0);
        one |= (row[w] & m) != 0u;
    }
    return one;
}

// the wave's 64 pixels (x0 = a multiple of 64) as two words of the plane's row
__device__ __forceinline__ void store_ballot(bool excluded, uint32_t* row, int words, int x0) {
    const unsigned long long bal = __ballot(excluded);
    if ((threadIdx.x & 63) == 0) {
        const int w = x0 >> 5;
        if (w < words) row[w] = (uint32_t)bal;
        if (w + 1 < words) row[w + 1] = (uint32_t)(bal >> 32);
    }
}

template <bool BITS>
__global__ void __launch_bounds__(256) mask_reduce_kernel(MaskReduceArgs a) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    bool excluded = false;
    if (x < a.dW) {
        const int xlo = a.fx[2 * x], xhi = a.fx[2 * x + 1];
        const int ylo = a.fy[2 * y], yhi = a.fy[2 * y + 1];
        for (int sy = ylo; sy <= yhi; ++sy) {
            if constexpr (BITS) excluded |= bits_have_one(a.sbits + (size_t)sy * a.swords, xlo, xhi);
            else excluded |= bytes_have_zero(a.src + (long long)sy * a.stride, a.sW, xlo, xhi);
        }
    }
    store_ballot(excluded, a.out + (size_t)y * a.words, a.words, x & ~63);
}

__global__ void __launch_bounds__(256) mask_warp_kernel(MaskWarpArgs a) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    bool excluded = false;
    if (x < a.wW) {
        const WarpEntry e = a.map[(long long)y * a.wW + x];
        // the taps of warp_kernel (warp.hip): columns modulo sW under wrap, rows clamped under replicate
        const int x0 = e.qx >> 5, y0 = e.qy >> 5, y1 = y0 + 1;
        int x1 = x0 + 1;
        if (a.wrap_x && x1 >= a.sW) x1 -= a.sW;
        const bool in = (a.wrap_x || ((unsigned)x0 < (unsigned)a.sW && (unsigned)x1 < (unsigned)a.sW)) &&
                        (a.replicate_y || ((unsigned)y0 < (unsigned)a.sH && (unsigned)y1 < (unsigned)a.sH));
        bool usable = e.qy != kWarpInvalid && in;
        if (usable && a.mask) {
            const int xc0 = min(max(x0, 0), a.sW - 1), xc1 = min(max(x1, 0), a.sW - 1);
            const long long r0 = (long long)min(max(y0, 0), a.sH - 1) * a.stride;
            const long long r1 = (long long)min(max(y1, 0), a.sH - 1) * a.stride;
            usable = a.mask[r0 + xc0] && a.mask[r0 + xc1] && a.mask[r1 + xc0] && a.mask[r1 + xc1];
        }
        excluded = !usable;
    }
    store_ballot(excluded, a.out + (size_t)y * a.words, a.words, x & ~63);
}

__global__ void __launch_bounds__(256) mask_erode_h_kernel(const uint32_t* in, uint32_t* out, int W, int words, int r,
                                                           int wrap) {
    __shared__ uint32_t A[2][kMaskRowWords];
    const uint32_t* row = in + (size_t)blockIdx.x * words;
    const int nP = (W + 2 * r + 31) >> 5;  // the extended row: bit j is source column j - r
    for (int i = threadIdx.x; i < nP; i += 256) {
        const int j0 = 32 * i - r;
        uint32_t v = 0;
        if (wrap) {
            int p = j0 % W;
            if (p < 0) p += W;
            for (int filled = 0; filled < 32;) {  // runs up to the end of the row, then on from column 0
                const int n = min(32 - filled, W - p);
                v |= take_bits(row, words, p, n) << filled;
                filled += n;
                p += n;
                if (p == W) p = 0;
            }
        } else {
            const int b0 = max(-j0, 0), b1 = min(W - j0, 32);  // columns outside the row are usable
            if (b0 < b1) v = take_bits(row, words, j0 + b0, b1 - b0) << b0;
        }
        A[0][i] = v;
    }
    __syncthreads();
    int cur = 0;
    for (int k = 1, K = 2 * r + 1; k < K;) {
        const int d = min(k, K - k), dw = d >> 5, ds = d & 31;
        for (int i = threadIdx.x; i < nP; i += 256) {
            const uint32_t lo = i + dw < nP ? A[cur][i + dw] : 0u, hi = (ds && i + dw + 1 < nP) ? A[cur][i + dw + 1] : 0u;
            A[cur ^ 1][i] = A[cur][i] | (uint32_t)((((uint64_t)hi << 32) | lo) >> ds);
        }
        __syncthreads();
        cur ^= 1;
        k += d;
    }
    for (int i = threadIdx.x; i < words; i += 256) {
        uint32_t v = A[cur][i];
        if (i == words - 1 && (W & 31)) v &= (1u << (W & 31)) - 1u;
        out[(size_t)blockIdx.x * words + i] = v;
    }
}

__global__ void __launch_bounds__(256) mask_erode_v_kernel(const uint32_t* in, uint32_t* out, int words, int H, int r) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)words * H) return;
    const int y = (int)(i / words), w = (int)(i % words);
    uint32_t v = 0;
    for (int yy = max(y - r, 0); yy <= min(y + r, H - 1); ++yy) v |= in[(size_t)yy * words + w];  // rows outside: usable
    out[i] = v;
}

__global__ void __launch_bounds__(256) mask_unpack_kernel(const uint32_t* bits, int W, int words, uint8_t* dst,
                                                          long long dstride) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= W) return;
    dst[(long long)y * dstride + x] = ((bits[(size_t)y * words + (x >> 5)] >> (x & 31)) & 1u) ? 0 : 255;
}

__global__ void __launch_bounds__(256) mask_gather_kernel(const float* pts, int n, const uint32_t* bits, int W, int H,
                                                          int words, uint8_t* usable, int x_wrap) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int xi = (int)rintf(pts[2 * i]);
    const int yi = (int)rintf(pts[2 * i + 1]);
    if (x_wrap && xi == W) xi = 0;  // seam wrap mode: a column within half a pixel of the seam rounds across it
    bool u = (unsigned)xi < (unsigned)W && (unsigned)yi < (unsigned)H;
    if (u) u = !((bits[(size_t)yi * words + (xi >> 5)] >> (xi & 31)) & 1u);
    usable[i] = u ? 1 : 0;
}

}  // namespace

hipError_t launch_mask_reduce(const MaskReduceArgs& a, hipStream_t st) {
    const dim3 grid((a.dW + 255) >> 8, a.dH), block(256);
    if (a.src) hipLaunchKernelGGL(mask_reduce_kernel<false>, grid, block, 0, st, a);
    else hipLaunchKernelGGL(mask_reduce_kernel<true>, grid, block, 0, st, a);
    return hipGetLastError();
}

hipError_t launch_mask_warp(const MaskWarpArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(mask_warp_kernel, dim3((a.wW + 255) >> 8, a.wH), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_mask_erode_h(const uint32_t* in, uint32_t* out, int W, int H, int r, int wrap, hipStream_t st) {
    if (W > kMaskMaxSize || r > kMaskMaxRadius) return hipErrorInvalidValue;  // the LDS row
    hipLaunchKernelGGL(mask_erode_h_kernel, dim3(H), dim3(256), 0, st, in, out, W, mask_words(W), r, wrap);
    return hipGetLastError();
}

hipError_t launch_mask_erode_v(const uint32_t* in, uint32_t* out, int W, int H, int r, hipStream_t st) {
    const size_t n = (size_t)mask_words(W) * H;
    hipLaunchKernelGGL(mask_erode_v_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, in, out, mask_words(W),
                       H, r);
    return hipGetLastError();
}

hipError_t launch_mask_unpack(const uint32_t* bits, int W, int H, uint8_t* dst, long long dstride, hipStream_t st) {
    hipLaunchKernelGGL(mask_unpack_kernel, dim3((W + 255) >> 8, H), dim3(256), 0, st, bits, W, mask_words(W), dst,
                       dstride);
    return hipGetLastError();
}

hipError_t launch_mask_gather(const float* pts, int n, const uint32_t* bits, int W, int H, uint8_t* usable,
                              hipStream_t st, int x_wrap) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(mask_gather_kernel, dim3((n + 255) >> 8), dim3(256), 0, st, pts, n, bits, W, H, mask_words(W),
                       usable, x_wrap);
    return hipGetLastError();
}

}  // namespace vio360
