// trk_dev.h — device helpers shared by the tracker's translation units (trk_lk.hip, trk_ransac.hip,
// trk_gftt.hip): border handling, the XCD tile placement, the bearing of a pixel, ordered-int floats and the
// bit tests of GFTT's static region and disc plane.  Every function is inline or static: each unit compiles
// its own copy (no relocatable device code).
#pragma once
#include <hip/hip_runtime.h>

#include "tracker_types.h"

namespace vio360 {

// LDS writes of this wave visible to its own later reads (no workgroup barrier)
__device__ __forceinline__ void wave_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Tile of linear block b of an n-block grid such that each XCD works on one contiguous range of tiles:
// blocks b and b + 8 share an XCD (round-robin dispatch, MI355X_MICROARCH.md "Workgroup dispatch"), so
// neighbouring tiles read their shared halo lines through one L2 instead of fetching them once per XCD
// (speed only: any placement gives the same results)
__device__ __forceinline__ int xcd_tile(int b, int n) {
    const int x = b & 7, s = b >> 3, q = n >> 3, r = n & 7;
    return x < r ? x * (q + 1) + s : r * (q + 1) + (x - r) * q + s;
}

__device__ __forceinline__ int reflect101(int p, int n) {
    if (n == 1) return 0;
    while (p < 0 || p >= n) p = p < 0 ? -p : 2 * n - 2 - p;
    return p;
}

// Seam wrap mode: column p of the frame continued periodically, for p in [-n, 2n) -- one conditional add or
// subtract, no division.  Columns further right are never part of a result (they lie beyond the last output
// of a partial tile); the min only keeps their address inside the row.
__device__ __forceinline__ int wrap_x(int p, int n) {
    return p < 0 ? p + n : (p >= n ? min(p - n, n - 1) : p);
}
// the column border of an edge path: REFLECT_101, or the periodic continuation in wrap mode (wave-uniform flag)
__device__ __forceinline__ int border_x(int p, int n, int x_wrap) { return x_wrap ? wrap_x(p, n) : reflect101(p, n); }

// MASKED: G.static_bits (a region mask's exclusion plane) is part of the static region (pass 1 with a mask set; the
// maskless instance is the code it was before masks existed)
template <bool MASKED = false>
__device__ __forceinline__ bool lm_static_in(const GfArgs& G, int x, int y) {
    const bool in = y >= G.top_rows && y < G.bottom_start && x >= G.margin && x < G.W - G.margin;
    if constexpr (MASKED) return in && !((G.static_bits[(size_t)y * G.disc_words + (x >> 5)] >> (x & 31)) & 1u);
    else return in;
}
__device__ __forceinline__ bool lm_disc(const GfArgs& G, int x, int y) {
    return G.disc_bits && ((G.disc_bits[(size_t)y * G.disc_words + (x >> 5)] >> (x & 31)) & 1u);
}
// per-run reset of the GFTT scalars (one thread of gftt_reset_kernel, or of lk_aux in the pipeline)
__device__ __forceinline__ void gftt_reset_scalars(int* scal) {
    scal[TS_MAX_ORD] = scal[TS_N_CAND] = scal[TS_N_OUT] = 0;
    scal[TS_N_TOP] = scal[TS_CUT] = scal[TS_CUT + 1] = scal[TS_INCOMPLETE] = 0;
    scal[TS_LMAX_OVER] = scal[TS_N_FLAT] = 0;
}

// Camera::PixelToBearing in f32 with the oracle's f64 trigonometry (LK's bearings and guess, RANSAC's input)
static __device__ void pixel_to_bearing(float u, float v, int W, int H, float* b) {
    float un = u / (float)W, vn = v / (float)H;
    float lon = (float)((double)((un - 0.5f) * 2.0f) * M_PI);
    float lat = (float)((double)(-(vn - 0.5f)) * M_PI);
    float cl = (float)cos((double)lat), sl = (float)sin((double)lat);
    float so = (float)sin((double)lon), co = (float)cos((double)lon);
    float x = cl * so, y = -sl, z = cl * co;
    float sq = (x * x + y * y) + z * z;
    if (sq > 0.f) {
        float nr = sqrtf(sq);
        x /= nr; y /= nr; z /= nr;
    }
    b[0] = x; b[1] = y; b[2] = z;
}

// order-preserving map of an f32 onto unsigned integers (atomicMax of responses), and back
__device__ __forceinline__ uint32_t ord_f32(float v) {
    uint32_t u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float unord_f32(uint32_t u) {
    return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}

}  // namespace vio360
