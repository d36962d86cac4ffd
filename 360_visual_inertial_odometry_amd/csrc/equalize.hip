// equalize.hip — contrast equalisation of a u8 frame on the device: cv::equalizeHist and cv::CLAHE::apply restated
// (erp_equalize*, include/vio360.h; host side in equalize_host.cpp).
//
// KLT front ends equalise the frame before tracking (VINS-style trackers: createCLAHE(3.0, Size(8, 8))); the reference
// does not (app/main.cpp:199-204), so this is off unless asked for.  OpenCV is not available to this project: parity
// with it is unpinned, the contract is the arithmetic of include/vio360.h, restated in numpy by
// tests/equalize_oracle.py, which these kernels match bitwise.  Everything up to the LUTs is integer arithmetic
// except one float32 multiply and round per LUT entry; the apply is a handful of float32 operations per pixel, each
// rounded on its own (the file is built without FMA contraction).
//
// Three launches on the context stream:
//   (a) eq_hist_kernel   one workgroup per run of rows of a tile: 256 bins in LDS, kept as 16 copies in 16 different
//                        banks (lane & 15 picks the copy) so that a constant or low-contrast frame, which sends every
//                        lane to the same few bins, serialises 4 lanes per address and not 64; a lane takes 4
//                        neighbouring pixels as one dword and adds 4 once when they are equal.  The workgroup writes
//                        its 256 sums with plain stores: no global atomics, no clearing pass, any grid gives the same
//                        counts.  The BORDER_REFLECT_101 extension of a frame that the tiles do not divide is index
//                        arithmetic here; no padded copy exists.
//   (b) eq_lut_kernel    one workgroup per tile: sums the partial histograms (16-byte loads, 16 groups of lanes over
//                        the chunks), clips and redistributes (CLAHE), scans, writes 256 bytes.
//   (c) eq_apply_kernel  one workgroup per pixel rectangle no larger than a tile: the at most 3 x 3 LUTs it can touch
//                        in LDS (2.25 KB), 4 pixels per lane as one dword load and one dword store at any alignment.
//                        A pixel depends on itself and the LUTs only, so dst may be src.
// Nothing outside [0, W) of a row or outside rows [0, H) is read or written; no scratch.
#include <hip/hip_runtime.h>

#include "equalize.h"

namespace vio360 {

namespace {

constexpr int kCopies = 16;

// column / row of the frame that index p of the extended frame reads (BORDER_REFLECT_101; the host keeps the
// extension below half the size, so one reflection suffices; the clamp only guards the address)
__device__ __forceinline__ int reflect(int p, int n) { return p < n ? p : max(2 * n - 2 - p, 0); }

__global__ __launch_bounds__(256) void eq_hist_kernel(EqArgs a) {
    __shared__ uint32_t sh[256 * kCopies];  // [bin][copy]
    const int tid = threadIdx.x;
    for (int i = tid; i < 256 * kCopies; i += 256) sh[i] = 0;
    __syncthreads();
    const int chunk = blockIdx.x % a.chunks, tile = blockIdx.x / a.chunks;
    const int tx = tile % a.tiles_x, ty = tile / a.tiles_x;
    const uint8_t* s = a.src + (long long)blockIdx.y * a.frame_bytes_src;
    const int r0 = chunk * a.chunk_rows, r1 = min(r0 + a.chunk_rows, a.th);
    const int upr = (a.tw + 3) >> 2;  // 4-pixel units per tile row
    const int units = (r1 - r0) * upr;
    const int copy = tid & (kCopies - 1);
    for (int u = tid; u < units; u += 256) {
        const int r = u / upr, c = (u - r * upr) * 4;
        const int px = tx * a.tw + c;
        const uint8_t* row = s + (long long)reflect(ty * a.th + r0 + r, a.H) * a.stride;
        const int n = min(4, a.tw - c);
        if (n == 4 && px + 3 < a.W) {
            uint32_t w;
            __builtin_memcpy(&w, row + px, 4);
            if (w == (w & 0xffu) * 0x01010101u) {
                atomicAdd(&sh[(w & 0xffu) * kCopies + copy], 4u);
            } else {
                atomicAdd(&sh[(w & 0xffu) * kCopies + copy], 1u);
                atomicAdd(&sh[((w >> 8) & 0xffu) * kCopies + copy], 1u);
                atomicAdd(&sh[((w >> 16) & 0xffu) * kCopies + copy], 1u);
                atomicAdd(&sh[(w >> 24) * kCopies + copy], 1u);
            }
        } else {
            for (int k = 0; k < n; ++k) atomicAdd(&sh[row[reflect(px + k, a.W)] * kCopies + copy], 1u);
        }
    }
    __syncthreads();
    uint32_t sum = 0;
    for (int k = 0; k < kCopies; ++k) sum += sh[tid * kCopies + k];
    a.part[(((size_t)blockIdx.y * (a.tiles_x * a.tiles_y) + tile) * a.chunks + chunk) * 256 + tid] = sum;
}

// inclusive scan of the 256 values of lanes 0..255 (every lane of the workgroup calls); *total = the sum
__device__ uint32_t scan256(uint32_t v, uint32_t* buf, int tid, uint32_t* total) {
    if (tid < 256) buf[tid] = v;
    __syncthreads();
    int cur = 0;
    for (int off = 1; off < 256; off <<= 1) {
        if (tid < 256) {
            uint32_t x = buf[cur * 256 + tid];
            if (tid >= off) x += buf[cur * 256 + tid - off];
            buf[(cur ^ 1) * 256 + tid] = x;
        }
        cur ^= 1;
        __syncthreads();
    }
    const uint32_t r = buf[cur * 256 + (tid & 255)];
    *total = buf[cur * 256 + 255];
    __syncthreads();
    return r;
}

__device__ __forceinline__ uint8_t saturate_u8(float f) { return (uint8_t)(int)fminf(fmaxf(rintf(f), 0.f), 255.f); }

__global__ __launch_bounds__(1024) void eq_lut_kernel(EqArgs a) {
    __shared__ uint32_t part[16 * 256];
    __shared__ uint32_t buf[2 * 256];
    __shared__ int first;
    const int tid = threadIdx.x;
    const int tile = blockIdx.x;
    const size_t tix = (size_t)blockIdx.y * (a.tiles_x * a.tiles_y) + tile;
    {   // the tile's histogram: lane group g sums chunks g, g + 16, ...; lane q of a group holds bins 4q .. 4q + 3
        const int q = tid & 63, g = tid >> 6;
        const uint4* p = reinterpret_cast<const uint4*>(a.part + tix * a.chunks * 256);
        uint4 acc = make_uint4(0, 0, 0, 0);
        for (int c = g; c < a.chunks; c += 16) {
            const uint4 v = p[(size_t)c * 64 + q];
            acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
        }
        uint32_t* o = part + g * 256 + 4 * q;
        o[0] = acc.x; o[1] = acc.y; o[2] = acc.z; o[3] = acc.w;
        if (tid == 0) first = 256;
    }
    __syncthreads();
    const int b = tid & 255;
    uint32_t h = 0;
    for (int g = 0; g < 16; ++g) h += part[g * 256 + b];
    uint32_t total;
    uint8_t out;
    if (a.mode == VIO_EQ_CLAHE) {
        if (a.clip > 0) {
            const uint32_t c = (uint32_t)a.clip;
            uint32_t excess;
            (void)scan256(h > c ? h - c : 0u, buf, tid, &excess);
            h = min(h, c) + (excess >> 8);
            const uint32_t resid = excess & 255u;
            if (resid) {
                const uint32_t step = max(256u / resid, 1u);
                if (b % step == 0 && b / step < resid) ++h;
            }
        }
        const uint32_t cs = scan256(h, buf, tid, &total);
        out = saturate_u8((float)cs * a.lut_scale);
    } else {
        if (tid < 256 && h) atomicMin(&first, b);
        const uint32_t cs = scan256(h, buf, tid, &total);  // its barriers also publish `first`
        const int i0 = min(first, 255);
        // the count of bin i0 = its inclusive sum, every bin below being empty
        const uint32_t h0 = i0 == b ? cs : 0u;
        if (tid == i0) buf[0] = h0;
        __syncthreads();
        const uint32_t n0 = buf[0];
        if (n0 == (uint32_t)a.area) {
            out = (uint8_t)i0;
        } else {
            const float scale = 255.f / (float)((uint32_t)a.area - n0);
            out = b <= i0 ? (uint8_t)0 : saturate_u8((float)(cs - n0) * scale);
        }
    }
    if (tid < 256) a.lut[tix * 256 + tid] = out;
}

template <bool INTERP>
__global__ __launch_bounds__(256) void eq_apply_kernel(EqArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t sl[(INTERP ? 9 : 1) * 256];  // [slot y][slot x][value]
    const int tid = threadIdx.x;
    const int rx = blockIdx.x % a.nrx, ry = blockIdx.x / a.nrx;
    const int x0 = rx * a.rw, x1 = min(x0 + a.rw, a.W);
    const int y0 = ry * a.rh, y1 = min(y0 + a.rh, a.H);
    const uint8_t* luts = a.lut + (size_t)blockIdx.y * (a.tiles_x * a.tiles_y) * 256;
    // slot (j, i) holds the LUT of tile (by + j, bx + i) after the border rule, (bx, by) the unclamped (tx1, ty1) of
    // the rectangle's first pixel: the rectangle is no larger than a tile, so its pixels' tx1 is bx or bx + 1
    int bx = 0, by = 0;
    if constexpr (INTERP) {
        bx = (int)floorf((float)x0 * a.inv_tw - 0.5f);
        by = (int)floorf((float)y0 * a.inv_th - 0.5f);
        for (int i = tid; i < 9 * 64; i += 256) {
            const int slot = i >> 6;
            int t_x = bx + slot % 3, t_y = by + slot / 3;
            if (a.wrap_x) t_x = t_x < 0 ? t_x + a.tiles_x : (t_x >= a.tiles_x ? t_x - a.tiles_x : t_x);
            t_x = min(max(t_x, 0), a.tiles_x - 1);
            t_y = min(max(t_y, 0), a.tiles_y - 1);
            reinterpret_cast<uint32_t*>(sl)[i] =
                reinterpret_cast<const uint32_t*>(luts + (size_t)(t_y * a.tiles_x + t_x) * 256)[i & 63];
        }
    } else {
        if (tid < 64) reinterpret_cast<uint32_t*>(sl)[tid] = reinterpret_cast<const uint32_t*>(luts)[tid];
    }
    __syncthreads();
    const uint8_t* s = a.src + (long long)blockIdx.y * a.frame_bytes_src;
    uint8_t* d = a.dst + (long long)blockIdx.y * a.frame_bytes_dst;
    const int upr = (x1 - x0 + 3) >> 2;
    const int units = (y1 - y0) * upr;
    for (int u = tid; u < units; u += 256) {
        const int r = u / upr, x = x0 + (u - r * upr) * 4, y = y0 + r;
        const int n = min(4, x1 - x);
        const uint8_t* sp = s + (long long)y * a.stride + x;
        uint8_t* dp = d + (long long)y * a.dstride + x;
        uint32_t w = 0;
        if (n == 4) {
            __builtin_memcpy(&w, sp, 4);
        } else {
            for (int k = 0; k < n; ++k) w |= (uint32_t)sp[k] << (8 * k);
        }
        uint32_t o = 0;
        if constexpr (INTERP) {
            const float tyf = (float)y * a.inv_th - 0.5f;
            const float ty1f = floorf(tyf);
            const float ya = tyf - ty1f, ya1 = 1.f - ya;
            const int j1 = min(max((int)ty1f - by, 0), 1);
            const uint8_t* l1 = sl + j1 * 768;
            const uint8_t* l2 = l1 + 768;
            for (int k = 0; k < 4; ++k) {
                const int v = (w >> (8 * k)) & 0xff;
                const float txf = (float)(x + k) * a.inv_tw - 0.5f;
                const float tx1f = floorf(txf);
                const float xa = txf - tx1f, xa1 = 1.f - xa;
                const int i1 = min(max((int)tx1f - bx, 0), 1);
                const float p11 = (float)l1[i1 * 256 + v], p12 = (float)l1[i1 * 256 + 256 + v];
                const float p21 = (float)l2[i1 * 256 + v], p22 = (float)l2[i1 * 256 + 256 + v];
                const float res = (p11 * xa1 + p12 * xa) * ya1 + (p21 * xa1 + p22 * xa) * ya;
                o |= (uint32_t)saturate_u8(res) << (8 * k);
            }
        } else {
            for (int k = 0; k < 4; ++k) o |= (uint32_t)sl[(w >> (8 * k)) & 0xff] << (8 * k);
        }
        if (n == 4) {
            __builtin_memcpy(dp, &o, 4);
        } else {
            for (int k = 0; k < n; ++k) dp[k] = (uint8_t)(o >> (8 * k));
        }
    }
}

}  // namespace

hipError_t launch_eq_hist(const EqArgs& a, hipStream_t stream) {
    hipLaunchKernelGGL(eq_hist_kernel, dim3(a.tiles_x * a.tiles_y * a.chunks, a.n_frames), dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_eq_lut(const EqArgs& a, hipStream_t stream) {
    hipLaunchKernelGGL(eq_lut_kernel, dim3(a.tiles_x * a.tiles_y, a.n_frames), dim3(1024), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_eq_apply(const EqArgs& a, hipStream_t stream) {
    const dim3 grid(a.nrx * a.nry, a.n_frames), block(256);
    if (a.mode == VIO_EQ_CLAHE) hipLaunchKernelGGL(eq_apply_kernel<true>, grid, block, 0, stream, a);
    else hipLaunchKernelGGL(eq_apply_kernel<false>, grid, block, 0, stream, a);
    return hipGetLastError();
}

}  // namespace vio360
