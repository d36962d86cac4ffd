// trk_lk.hip — ERP feature tracking on MI355X (gfx950), the image pyramid and the LK search: the first stage
// of FeatureTracker::TrackFeatures (src/processing/FeatureTracker.cpp:61-379).  The other stages are
// trk_ransac.hip (rotation RANSAC, discs) and trk_gftt.hip (detection); trk_dev.h holds the device helpers
// the three share.
//
//   pyr_down_kernel      cv::pyrDown inside buildOpticalFlowPyramid: 5x5 [1 4 6 4 1]^2/256,
//                        BORDER_REFLECT_101; both frames of a pair in one launch (blockIdx.z).
//   lk_kernel            cv::calcOpticalFlowPyrLK's LKTrackerInvoker, one wavefront per point,
//                        all pyramid levels in one launch; the Scharr derivatives of the previous
//                        frame are computed on the fly from an LDS-staged 24x24 tile (never
//                        materialised for the whole image), the 21x21 patch, its derivatives and
//                        every 22x22 next-frame tile live in LDS; gradient/mismatch sums are exact
//                        int64 wave reductions.
// Seam wrap mode (VIO_SEAM_WRAP, the x_wrap flag of the argument blocks): every stage on the horizontally periodic
// continuation of the frame -- wrapped border columns, no sideways exit and no side margins, discs and the
// min-distance test on the cylinder, detection through the map path.  Off by default; on the pipeline's critical
// path the flag selects a template instance, so the default kernels are the code they were.
// Float expressions follow tracker_oracle.c literally and every tracker unit is built with
// -ffp-contract=off, so results are bitwise those of the oracle.
#include <float.h>
#include <hip/hip_runtime.h>

#include <cstring>

#include "tracker_types.h"
#include "trk_dev.h"
#include "trk_ransac_dev.h"

namespace vio360 {

// ------------------------------------------------------------------------------------------
// pyrDown.  Block = 64 x BY outputs; LDS tile of the (2*BY+4) REFLECT_101 source rows, columns
// [2 ox - 16, 2 ox + 144), staged with 16-B loads (all of a thread's loads issued before its LDS stores; the
// few reflected columns at the left / right image edge are patched bytewise); each thread makes two adjacent
// outputs in BY / 8 rows.  BY = 8 (BY = 32 for the large levels -- a quarter of the blocks and of the halo
// rows, the 3840 x 1920 level-1 launch in one round of resident workgroups -- measured 15.0 against 13.2 us,
// profiles/r6c_ab_pyr.log).
constexpr int PD_BX = 64;
constexpr int PD_TW = 160;
// WRAP (seam wrap mode, src.x_wrap): the edge columns are patched from the opposite side of the level instead of
// reflected; the default instance is the code as it was
template <int BY, bool WRAP = false>
__global__ void __launch_bounds__(256) pyr_down_kernel(PyrLevelPair src, PyrLevelPair dst) {
    constexpr int PD_BY = BY, PD_TH = 2 * PD_BY + 4;
    __shared__ uint8_t tile[PD_TH][PD_TW];
    const int gxy = gridDim.x * gridDim.y;
    const int t = xcd_tile(blockIdx.x + gridDim.x * blockIdx.y + gxy * blockIdx.z, gxy * gridDim.z);
    const int f = t / gxy, bxy = t - f * gxy, bx = bxy % gridDim.x, by = bxy / gridDim.x;
    const uint8_t* s = f == 0 ? src.p0 : src.p1;
    uint8_t* d = f == 0 ? dst.p0 : dst.p1;
    const int sw = src.w, sh = src.h, sp = src.pitch;
    const int dw = dst.w, dh = dst.h, dp = dst.pitch;
    const int ox = bx * PD_BX, oy = by * PD_BY;
    const int cx0 = 2 * ox - 16, sy0 = 2 * oy - 2;  // tile column 0 = source x cx0
    {  // 16-B chunks of the REFLECT_101 rows; chunks beyond the pitch are skipped
        constexpr int NCH = PD_TH * (PD_TW / 16);
        uint4 v[(NCH + 255) / 256];
#pragma unroll
        for (int it = 0; it < (NCH + 255) / 256; ++it) {
            const int e = threadIdx.x + 256 * it;
            const int x0 = cx0 + 16 * (e % (PD_TW / 16));
            v[it] = make_uint4(0u, 0u, 0u, 0u);
            if (e < NCH && x0 >= 0 && x0 + 16 <= sp)
                v[it] = *reinterpret_cast<const uint4*>(s + (size_t)reflect101(sy0 + e / (PD_TW / 16), sh) * sp + x0);
        }
#pragma unroll
        for (int it = 0; it < (NCH + 255) / 256; ++it) {
            const int e = threadIdx.x + 256 * it;
            const int x0 = cx0 + 16 * (e % (PD_TW / 16));
            if (e < NCH && x0 >= 0 && x0 + 16 <= sp)
                *reinterpret_cast<uint4*>(&tile[e / (PD_TW / 16)][16 * (e % (PD_TW / 16))]) = v[it];
        }
    }
    if (2 * ox - 2 < 0 || 2 * ox + 2 * PD_BX + 2 > sw) {  // left / right image edge: reflected columns
        __syncthreads();
        for (int e = threadIdx.x; e < PD_TH * (2 * PD_BX + 4); e += 256) {
            const int ty = e / (2 * PD_BX + 4), x = 2 * ox - 2 + e % (2 * PD_BX + 4);
            if (x < 0 || x >= sw)
                tile[ty][x - cx0] = s[(size_t)reflect101(sy0 + ty, sh) * sp + (WRAP ? wrap_x(x, sw) : reflect101(x, sw))];
        }
    }
    __syncthreads();
    const int q = threadIdx.x % (PD_BX / 2);  // outputs 2q, 2q+1 of rows ty0 + 8 r
#pragma unroll
    for (int rr = 0; rr < PD_BY / 8; ++rr) {
        const int ty = threadIdx.x / (PD_BX / 2) + 8 * rr;
        const int y = oy + ty;
        if (y >= dh) break;
        uint32_t packed = 0;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int tx = 2 * q + j;
            int tot = 0;
#pragma unroll
            for (int ky = 0; ky < 5; ++ky) {
                const uint8_t* r = &tile[2 * ty + ky][2 * tx + 14];
                const int rs = r[0] + 4 * r[1] + 6 * r[2] + 4 * r[3] + r[4];
                tot += (ky == 0 || ky == 4 ? 1 : (ky == 2 ? 6 : 4)) * rs;
            }
            packed |= (uint32_t)((tot + 128) >> 8) << (8 * j);
        }
        const int x = ox + 2 * q;
        if (x + 1 < dw && ((dp & 1) == 0)) {
            *reinterpret_cast<uint16_t*>(d + (size_t)y * dp + x) = (uint16_t)packed;
        } else {
            for (int j = 0; j < 2; ++j)
                if (x + j < dw) d[(size_t)y * dp + x + j] = (uint8_t)(packed >> (8 * j));
        }
    }
}

// ------------------------------------------------------------------------------------------
// LK.  One workgroup per point.
constexpr int LK_WAVES = 4;  // one point per workgroup of LK_WAVES waves
constexpr int LK_THREADS = 64 * LK_WAVES;
constexpr int LK_NIT = (LK_WIN_MAX * LK_WIN_MAX + LK_THREADS - 1) / LK_THREADS;  // patch pixels per lane
// (LK_T, LK_D, LK_MARGIN, LK_R: the staging tiles' sizes, tracker_types.h)

struct LkShared {
    uint8_t Jr[LK_R * LK_R];                 // next-frame region (reflect-101 values), origin (rx0, ry0)
    uint8_t It[LK_T * LK_T];
    int16_t dx[LK_D * LK_D], dy[LK_D * LK_D];
};

// Wave sum of integer partials, exact while |sum| < 2^53: the partials are summed as doubles
// (integer-valued, so every order gives the same exact value) with DPP row reductions (xor 1, xor 2,
// half-row mirror, row mirror: VALU lane moves, no LDS crossbar) and the four row totals read out.
template <int CTRL>
__device__ __forceinline__ double dpp_d(double v) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xF, 0xF, false);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double lane_d(double v, int l) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), l);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
}

#define DESCALE(x, n) (((x) + (1 << ((n)-1))) >> (n))

__device__ __forceinline__ void lk_weights(float a, float b, int& w00, int& w01, int& w10, int& w11) {
    w00 = (int)rintf((1.f - a) * (1.f - b) * 16384.f);
    w01 = (int)rintf(a * (1.f - b) * 16384.f);
    w10 = (int)rintf((1.f - a) * b * 16384.f);
    w11 = 16384 - w00 - w01 - w10;
}

// workgroup sum of integer partials (exact: each wave's partials summed as doubles with DPP row
// reductions and the four row totals read out, then the LK_WAVES wave totals
// added in wave order through LDS); every thread gets the total.  red: LK_WAVES doubles of LDS.
__device__ __forceinline__ long long wg_sum_i64(long long v, double* red) {
    double d = (double)v;
    d += dpp_d<0xB1>(d);
    d += dpp_d<0x4E>(d);
    d += dpp_d<0x141>(d);
    d += dpp_d<0x140>(d);
    const double ws = ((lane_d(d, 0) + lane_d(d, 16)) + lane_d(d, 32)) + lane_d(d, 48);
    const int wid = threadIdx.x >> 6;
    __syncthreads();  // red is free (the previous sum's readers are done)
    if ((threadIdx.x & 63) == 0) red[wid] = ws;
    __syncthreads();
    double t = 0.0;
#pragma unroll
    for (int q = 0; q < LK_WAVES; ++q) t += red[q];
    return (long long)t;
}

// Seam wrap mode: the column of the frame under the unwrapped column x0 of a staged tile's origin.  The iteration
// may carry x0 any distance from the frame, so this is a true remainder -- once per staged tile, workgroup-uniform,
// never per pixel.
__device__ __forceinline__ int lk_fold_origin(int x0, int w) {
    const int m = x0 % w;
    return m < 0 ? m + w : m;
}

// make the staged region cover the (win+1)^2 window at (ix, iy); restage around it when it does
// not (one global round trip per level instead of one per iteration).  Values are the
// REFLECT_101-padded pixels, exactly what a per-window load would read.  Workgroup-uniform.
// WRAP (seam wrap mode): rx0 stays in the iteration's unwrapped coordinates; the columns are those of the
// periodic continuation (lk_fold_origin, then one conditional subtract per pixel: w >= LK_R).
template <bool WRAP>
__device__ __forceinline__ void lk_region(uint8_t* Jr, int& rx0, int& ry0, const uint8_t* J, int w, int h, int pitch,
                                          int ix, int iy, int win) {
    const int D = win + 1;
    if (ix >= rx0 && iy >= ry0 && ix + D <= rx0 + LK_R && iy + D <= ry0 + LK_R) return;
    rx0 = ix - LK_MARGIN;
    ry0 = iy - LK_MARGIN;
    __syncthreads();  // the previous region's readers are done
    // every global load of the region is issued before the first LDS store
    constexpr int NR = (LK_R * LK_R + LK_THREADS - 1) / LK_THREADS;
    uint32_t v[NR];
    const int fx0 = WRAP ? lk_fold_origin(rx0, w) : 0;
#pragma unroll
    for (int it = 0; it < NR; ++it) {
        const int e = threadIdx.x + LK_THREADS * it;
        const int ty = e / LK_R, tx = e - ty * LK_R;
        v[it] = e < LK_R * LK_R ? J[(size_t)reflect101(ry0 + ty, h) * pitch +
                                    (WRAP ? wrap_x(fx0 + tx, w) : reflect101(rx0 + tx, w))] : 0u;
    }
#pragma unroll
    for (int it = 0; it < NR; ++it) {
        const int e = threadIdx.x + LK_THREADS * it;
        if (e < LK_R * LK_R) Jr[e] = (uint8_t)v[it];
    }
    __syncthreads();
}

// calcOpticalFlowPyrLK for one point per workgroup (LK_WAVES waves): the patch pixels are spread over
// all lanes (<= LK_NIT each), the window sums are exact integer workgroup sums, so every order gives
// the sequential values; the per-iteration update is computed by every thread from the same totals.
constexpr int LK_AUX_BLOCKS = 17;  // LkAux: one workgroup for the raw draws, 16 for the reset and the bitmap clear
__device__ void lk_aux(const LkAux& X, int b) {
    if (b == 0) {
        __shared__ uint32_t mt[624];
        if (X.raw) ransac_raw_body<LK_THREADS>(X.seed, X.raw, mt);
        if (X.cmin && threadIdx.x == 0) *X.cmin = ransac_cos_bound(X.thresh);
        return;
    }
    const size_t t = (size_t)(b - 1) * LK_THREADS + threadIdx.x, stride = (size_t)(LK_AUX_BLOCKS - 1) * LK_THREADS;
    if (X.hist) {  // gftt_reset_kernel's work
        if (t == 0) gftt_reset_scalars(X.scal);
        for (size_t i = t; i < (size_t)GF_BUCKETS; i += stride) X.hist[i] = 0u;
        for (size_t i = t; i < X.topk_cap; i += stride) X.topk[i] = 0ull;
    }
    if (X.bear0)
        for (size_t i = t; i < (size_t)X.n; i += stride)
            pixel_to_bearing(X.pts[2 * i], X.pts[2 * i + 1], X.W, X.H, X.bear0 + 3 * i);
    if (X.disc) {
        const size_t n4 = X.disc_words / 4;
        uint4* d4p = reinterpret_cast<uint4*>(X.disc);
        if (X.disc_src) {  // a region mask is set: the discs are stamped onto its exclusion plane
            const uint4* s4p = reinterpret_cast<const uint4*>(X.disc_src);
            for (size_t i = t; i < n4; i += stride) d4p[i] = s4p[i];
            for (size_t i = 4 * n4 + t; i < X.disc_words; i += stride) X.disc[i] = X.disc_src[i];
        } else {
            for (size_t i = t; i < n4; i += stride) d4p[i] = make_uint4(0u, 0u, 0u, 0u);
            for (size_t i = 4 * n4 + t; i < X.disc_words; i += stride) X.disc[i] = 0u;
        }
    }
}

// Guided search: the start position (gx, gy) of point pt at the top level, in level-0 pixels; on entry the point's
// previous position (px, py), which stays when the point has no usable guess.  Workgroup-uniform.
//   LK_GUESS_PTS  A.guess[pt]
//   LK_GUESS_ROT  Camera::BearingToPixel(R * PixelToBearing(prev)) (Camera.cpp:22-67) in f32, operations in this
//                 order: r_i = ((R_i0 b0 + R_i1 b1) + R_i2 b2), theta = atan2f(r0, r2), phi = -asinf(r1 / |r|),
//                 u = W (0.5 + theta / 2pi), v = H (0.5 - phi / pi)
// A guess that is not finite or lies outside [-W, 2W) x [-H, 2H) counts as absent (OpenCV would index with it).
// WRAP: x folded into [0, W) by one f32 +-W, as the final fold of the tracked column.
template <bool WRAP>
__device__ __forceinline__ void lk_guess(const LkArgs& A, int pt, float px, float py, float& gx, float& gy) {
    const int W = A.lv[0].w, H = A.lv[0].h;
    const float Wf = (float)W, Hf = (float)H;
    float u, v;
    if (A.guided == LK_GUESS_ROT) {
        float b[3];
        pixel_to_bearing(px, py, W, H, b);
        const float r0 = (A.rot[0] * b[0] + A.rot[1] * b[1]) + A.rot[2] * b[2];
        const float r1 = (A.rot[3] * b[0] + A.rot[4] * b[1]) + A.rot[5] * b[2];
        const float r2 = (A.rot[6] * b[0] + A.rot[7] * b[1]) + A.rot[8] * b[2];
        const float nr = sqrtf((r0 * r0 + r1 * r1) + r2 * r2);
        const float theta = atan2f(r0, r2);
        const float phi = -asinf(fminf(fmaxf(r1 / nr, -1.f), 1.f));
        u = Wf * (0.5f + theta / 6.2831855f);
        v = Hf * (0.5f - phi / 3.1415927f);
    } else {
        u = A.guess[2 * pt];
        v = A.guess[2 * pt + 1];
    }
    if (!(u >= -Wf && u < 2.f * Wf && v >= -Hf && v < 2.f * Hf)) return;  // (a NaN fails every comparison)
    if (WRAP) {
        if (u < 0.f) u += Wf;
        else if (u >= Wf) u -= Wf;
        if (u == Wf) u = 0.f;  // (a tiny negative column rounds up to W)
    }
    gx = u;
    gy = v;
}

// WRAP (seam wrap mode, A.x_wrap): every level is the periodic continuation of the frame in x -- tile columns
// modulo the level width, no "left the frame" test in x, the iteration in unwrapped coordinates; only the final
// next.x is folded into [0, W) by one f32 +-W.  The default instance is the code it was before the mode existed.
// GUIDED (OPTFLOW_USE_INITIAL_FLOW, A.guided): the top level starts at the point's guess (lk_guess) instead of its
// previous position; nothing else differs, and a guess equal to the previous position gives the unguided bits.  The
// two unguided instances are the code they were before the guided ones existed.
// FB (round-trip check, A.fb): after the forward search and its fold the workgroup of a found point runs the level
// loop once more with the frames' roles swapped -- the point its own next, the top level started at the previous
// position (always "guided") -- then tests where it lands against the previous position.  next, err, guess_out and
// bear1 are the forward search's; status is stored once, as forward AND pass.  The LDS tiles and red are reused;
// every branch on status is workgroup-uniform.  The four instances without FB are the code they were.
// The rules a guess passes, for the backward direction of the round-trip check (lk_guess applies the same to its
// own): (u, v) replaces (gx, gy) unless it is not finite or lies outside [-W, 2W) x [-H, 2H); WRAP folds x into [0, W).
template <bool WRAP>
__device__ __forceinline__ void lk_guess_at(float Wf, float Hf, float u, float v, float& gx, float& gy) {
    if (!(u >= -Wf && u < 2.f * Wf && v >= -Hf && v < 2.f * Hf)) return;  // (a NaN fails every comparison)
    if (WRAP) {
        if (u < 0.f) u += Wf;
        else if (u >= Wf) u -= Wf;
        if (u == Wf) u = 0.f;  // (a tiny negative column rounds up to W)
    }
    gx = u;
    gy = v;
}

template <bool WRAP, bool GUIDED = false, bool FB = false>
__global__ void __launch_bounds__(LK_THREADS) lk_kernel(LkArgs A, LkAux X) {
    __shared__ LkShared S;
    __shared__ double red[LK_WAVES];
    const int tid = threadIdx.x;
    const int pt = blockIdx.x;
    if (pt >= A.n) {  // whole workgroup
        lk_aux(X, pt - A.n);
        return;
    }
    const int win = A.win;
    const float hw = (win - 1) * 0.5f;
    const float FLT_SCALE = 1.f / (1 << 20);
    const int np = win * win;
    float prev_x = A.pts[2 * pt], prev_y = A.pts[2 * pt + 1];
    float nxt_x = 0.f, nxt_y = 0.f;
    int status = 1;
    float err = 0.f;
    float gs_x = prev_x, gs_y = prev_y;  // GUIDED: the top level's start position in level-0 pixels
    if constexpr (GUIDED) {
        lk_guess<WRAP>(A, pt, prev_x, prev_y, gs_x, gs_y);
        if (A.guess_out && tid == 128) {
            A.guess_out[2 * pt] = gs_x;
            A.guess_out[2 * pt + 1] = gs_y;
        }
    }
    // FB: the forward result while the backward direction runs, and the check's outputs.  The second direction is
    // a jump back to `direction`, not a loop around the level loop: without FB the label is no branch target, and
    // the compiler emits the instructions it emitted before the check existed.
    float fw_x = 0.f, fw_y = 0.f, fw_err = 0.f, bk_x = 0.f, bk_y = 0.f, fb_d2 = 0.f;
    int fb_state = LK_FB_NOT_RUN, dir = 0;
direction:
    for (int level = A.levels; level >= 0; --level) {
        const LkLevel& Lv = A.lv[level];
        const int w = Lv.w, h = Lv.h;
        const uint8_t* I = FB && dir ? Lv.curr : Lv.prev;  // (the backward direction: the frames swap roles)
        const uint8_t* J = FB && dir ? Lv.prev : Lv.curr;
        const float sc = (float)(1. / (1 << level));
        float px = prev_x * sc, py = prev_y * sc;
        float nx, ny;
        if (level == A.levels) {
            if constexpr (GUIDED || FB) { nx = gs_x * sc; ny = gs_y * sc; }
            else { nx = px; ny = py; }
        } else { nx = nxt_x * 2.f; ny = nxt_y * 2.f; }
        nxt_x = nx; nxt_y = ny;
        px -= hw; py -= hw;
        const int ipx = (int)floorf(px), ipy = (int)floorf(py);
        if ((!WRAP && (ipx < -win || ipx >= w)) || ipy < -win || ipy >= h) {
            if (level == 0) { status = 0; err = 0.f; }
            continue;
        }
        // stage the prev tile: rows ipy-1 .. ipy+win+1, cols ipx-1 .. ipx+win+1
        const int T = win + 3;
        __syncthreads();  // the previous level's readers of It / dx / dy are done
        {
            constexpr int NT = (LK_T * LK_T + LK_THREADS - 1) / LK_THREADS;  // loads first, then the LDS stores
            uint32_t v[NT];
            const int fx0 = WRAP ? lk_fold_origin(ipx - 1, w) : 0;
#pragma unroll
            for (int it = 0; it < NT; ++it) {
                const int e = tid + LK_THREADS * it;
                const int ty = e / T, tx = e - (e / T) * T;
                v[it] = e < T * T ? I[(size_t)reflect101(ipy - 1 + ty, h) * Lv.pitch +
                                      (WRAP ? wrap_x(fx0 + tx, w) : reflect101(ipx - 1 + tx, w))] : 0u;
            }
#pragma unroll
            for (int it = 0; it < NT; ++it) {
                const int e = tid + LK_THREADS * it;
                if (e < T * T) S.It[e] = (uint8_t)v[it];
            }
        }
        __syncthreads();
        // Scharr derivatives at (ipx+tx, ipy+ty), tx,ty in [0, win]; zero outside the image
        const int D = win + 1;
        for (int e = tid; e < D * D; e += LK_THREADS) {
            int ty = e / D, tx = e % D;
            int X = ipx + tx, Y = ipy + ty;
            int gx = 0, gy = 0;
            if ((WRAP || X >= 0) && Y >= 0 && (WRAP || X < w) && Y < h) {
                const uint8_t* r0 = &S.It[ty * T + tx];      // (X-1, Y-1)
                const uint8_t* r1 = r0 + T;
                const uint8_t* r2 = r1 + T;
                int t0m = (r0[0] + r2[0]) * 3 + r1[0] * 10, t0p = (r0[2] + r2[2]) * 3 + r1[2] * 10;
                int t1m = r2[0] - r0[0], t1c = r2[1] - r0[1], t1p = r2[2] - r0[2];
                gx = (int16_t)(t0p - t0m);
                gy = (int16_t)((t1p + t1m) * 3 + t1c * 10);
            }
            S.dx[e] = (int16_t)gx;
            S.dy[e] = (int16_t)gy;
        }
        __syncthreads();
        float a = px - ipx, b = py - ipy;
        int w00, w01, w10, w11;
        lk_weights(a, b, w00, w01, w10, w11);
        // the lane's patch pixels e = tid + LK_THREADS it: interpolated I and derivatives stay in registers
        // for all iterations of the level; joff = offset of the pixel in the next-frame window (-1: none)
        int joff[LK_NIT], iwv[LK_NIT], ixr[LK_NIT], iyr[LK_NIT];
        int sA11 = 0, sA12 = 0, sA22 = 0;
#pragma unroll
        for (int it = 0; it < LK_NIT; ++it) {
            const int e = tid + LK_THREADS * it;
            joff[it] = -1;
            iwv[it] = ixr[it] = iyr[it] = 0;
            if (e < np) {
                const int y = e / win, x = e - (e / win) * win;
                const uint8_t* t = &S.It[(y + 1) * T + x + 1];
                const int ival = DESCALE(t[0] * w00 + t[1] * w01 + t[T] * w10 + t[T + 1] * w11, 9);
                const int q = y * D + x;
                const int ixv =
                    DESCALE(S.dx[q] * w00 + S.dx[q + 1] * w01 + S.dx[q + D] * w10 + S.dx[q + D + 1] * w11, 14);
                const int iyv =
                    DESCALE(S.dy[q] * w00 + S.dy[q + 1] * w01 + S.dy[q + D] * w10 + S.dy[q + D + 1] * w11, 14);
                iwv[it] = (int16_t)ival;
                ixr[it] = (int16_t)ixv;
                iyr[it] = (int16_t)iyv;
                joff[it] = y * LK_R + x;
                sA11 += ixv * ixv;
                sA12 += ixv * iyv;
                sA22 += iyv * iyv;
            }
        }
        const long long tA11 = wg_sum_i64(sA11, red), tA12 = wg_sum_i64(sA12, red), tA22 = wg_sum_i64(sA22, red);
        const float A11 = (float)tA11 * FLT_SCALE, A12 = (float)tA12 * FLT_SCALE, A22 = (float)tA22 * FLT_SCALE;
        float Dt = A11 * A22 - A12 * A12;
        const float minEig = (A22 + A11 - sqrtf((A11 - A22) * (A11 - A22) + 4.f * A12 * A12)) / (float)(2 * win * win);
        if (minEig < A.min_eig || Dt < FLT_EPSILON) {
            if (level == 0) status = 0;
            continue;
        }
        Dt = 1.f / Dt;
        nx -= hw; ny -= hw;
        float pdx = 0.f, pdy = 0.f;
        int rx0 = -(1 << 29), ry0 = -(1 << 29);  // no region staged for this level yet
        for (int j = 0; j < A.max_iters; ++j) {
            const int inx = (int)floorf(nx), iny = (int)floorf(ny);
            if ((!WRAP && (inx < -win || inx >= w)) || iny < -win || iny >= h) {
                if (level == 0) status = 0;
                break;
            }
            a = nx - inx; b = ny - iny;
            lk_weights(a, b, w00, w01, w10, w11);
            lk_region<WRAP>(S.Jr, rx0, ry0, J, w, h, Lv.pitch, inx, iny, win);
            const uint8_t* Jw = S.Jr + (iny - ry0) * LK_R + (inx - rx0);
            int ib1 = 0, ib2 = 0;
#pragma unroll
            for (int it = 0; it < LK_NIT; ++it) {
                if (joff[it] >= 0) {
                    const uint8_t* t = Jw + joff[it];
                    const int diff = DESCALE(t[0] * w00 + t[1] * w01 + t[LK_R] * w10 + t[LK_R + 1] * w11, 9) - iwv[it];
                    ib1 += diff * ixr[it];
                    ib2 += diff * iyr[it];
                }
            }
            const float b1 = (float)wg_sum_i64(ib1, red) * FLT_SCALE, b2 = (float)wg_sum_i64(ib2, red) * FLT_SCALE;
            const float ddx = (A12 * b2 - A22 * b1) * Dt;
            const float ddy = (A12 * b1 - A11 * b2) * Dt;
            nx += ddx; ny += ddy;
            nxt_x = nx + hw; nxt_y = ny + hw;
            if ((double)ddx * ddx + (double)ddy * ddy <= A.eps2) break;
            if (j > 0 && fabs((double)(ddx + pdx)) < 0.01 && fabs((double)(ddy + pdy)) < 0.01) {
                nxt_x -= ddx * 0.5f;
                nxt_y -= ddy * 0.5f;
                break;
            }
            pdx = ddx; pdy = ddy;
        }
        if (status && level == 0) {
            const float fx = nxt_x - hw, fy = nxt_y - hw;
            const int ix = (int)floorf(fx), iy = (int)floorf(fy);
            if ((!WRAP && (ix < -win || ix >= w)) || iy < -win || iy >= h) {
                status = 0;
            } else {
                lk_weights(fx - ix, fy - iy, w00, w01, w10, w11);
                lk_region<WRAP>(S.Jr, rx0, ry0, J, w, h, Lv.pitch, ix, iy, win);
                const uint8_t* Jw = S.Jr + (iy - ry0) * LK_R + (ix - rx0);
                long long es = 0;
#pragma unroll
                for (int it = 0; it < LK_NIT; ++it) {
                    if (joff[it] >= 0) {
                        const uint8_t* t = Jw + joff[it];
                        const int diff =
                            DESCALE(t[0] * w00 + t[1] * w01 + t[LK_R] * w10 + t[LK_R + 1] * w11, 9) - iwv[it];
                        es += diff < 0 ? -diff : diff;
                    }
                }
                es = wg_sum_i64(es, red);
                err = (float)es * (1.f / (32 * win * win));
            }
        }
    }
    if (WRAP) {  // fold the tracked column into [0, W): one +-W (exact for a point within one turn of the frame)
        const float Wf = (float)A.lv[0].w;
        if (nxt_x < 0.f) nxt_x += Wf;
        else if (nxt_x >= Wf) nxt_x -= Wf;
        if (nxt_x == Wf) nxt_x = 0.f;  // (a tiny negative column rounds up to W)
        if (!(nxt_x >= 0.f && nxt_x < Wf)) {  // more than a turn away, or not a number: the point is lost
            nxt_x = 0.f;
            status = 0;
            err = 0.f;
        }
    }
    if constexpr (FB) {
        const float Wf = (float)A.lv[0].w, Hf = (float)A.lv[0].h;
        if (dir == 0) {
            fw_x = nxt_x; fw_y = nxt_y; fw_err = err;
            if (status) {  // found (workgroup-uniform): track it back
                // the point is its own next, the guess its previous position under lk_guess's rules.  The level
                // loop's first LDS access follows a barrier, so the tiles and red are free as at a level change.
                prev_x = gs_x = nxt_x;
                prev_y = gs_y = nxt_y;
                lk_guess_at<WRAP>(Wf, Hf, A.pts[2 * pt], A.pts[2 * pt + 1], gs_x, gs_y);
                err = 0.f;
                dir = 1;
                goto direction;
            }
        } else {
            bk_x = nxt_x; bk_y = nxt_y;
            float dx = bk_x - A.pts[2 * pt];
            const float dy = bk_y - A.pts[2 * pt + 1];
            if (WRAP) {  // the short way round
                const float half = Wf * 0.5f;
                if (dx > half) dx -= Wf;
                else if (dx < -half) dx += Wf;
            }
            const float d2 = dx * dx + dy * dy;
            const bool pass = status && d2 <= A.fb_max_dist * A.fb_max_dist;  // (a NaN fails)
            fb_state = !status ? LK_FB_BACK_LOST : pass ? LK_FB_PASS : LK_FB_TOO_FAR;
            fb_d2 = status ? d2 : 0.f;
            nxt_x = fw_x; nxt_y = fw_y; err = fw_err;
            status = pass;
        }
    }
    if (tid == 0) {
        A.next[2 * pt] = nxt_x;
        A.next[2 * pt + 1] = nxt_y;
        A.status[pt] = (uint8_t)status;
        A.err[pt] = err;
    }
    // the tracked point's bearing (RANSAC's input, FeatureTracker.cpp:262-271) by another wave, beside the stores
    if (A.bear1 && tid == 64) pixel_to_bearing(nxt_x, nxt_y, A.lv[0].w, A.lv[0].h, A.bear1 + 3 * pt);
    if constexpr (FB) {
        if (tid == 192) {
            A.back[2 * pt] = bk_x;
            A.back[2 * pt + 1] = bk_y;
            A.fb_state[pt] = (uint8_t)fb_state;
            A.fb_d2[pt] = fb_d2;
        }
    }
}

// ------------------------------------------------------------------------------------------
// launchers
hipError_t launch_pyr_down(const PyrLevelPair& s, const PyrLevelPair& d, int frames, hipStream_t st) {
    constexpr int by = 8;
    dim3 g((d.w + PD_BX - 1) / PD_BX, (d.h + by - 1) / by, frames);
    const auto k = s.x_wrap ? pyr_down_kernel<by, true> : pyr_down_kernel<by, false>;
    hipLaunchKernelGGL(k, g, dim3(256), 0, st, s, d);
    return hipGetLastError();
}
// every instance of lk_kernel, [x_wrap][guided][fb]
using LkKernel = void (*)(LkArgs, LkAux);
static const LkKernel lk_kernels[2][2][2] = {
    {{lk_kernel<false, false, false>, lk_kernel<false, false, true>},
     {lk_kernel<false, true, false>, lk_kernel<false, true, true>}},
    {{lk_kernel<true, false, false>, lk_kernel<true, false, true>},
     {lk_kernel<true, true, false>, lk_kernel<true, true, true>}}};
hipError_t launch_lk(const LkArgs& a, hipStream_t st, const LkAux* aux) {
    LkAux x;
    std::memset(&x, 0, sizeof x);
    if (aux) x = *aux;
    const int n = a.n > 0 ? a.n : 0, blocks = n + (aux ? LK_AUX_BLOCKS : 0);
    if (blocks == 0) return hipSuccess;
    const LkKernel k = lk_kernels[a.x_wrap != 0][a.guided != LK_GUESS_NONE][a.fb != 0];
    hipLaunchKernelGGL(k, dim3(blocks), dim3(LK_THREADS), 0, st, a, x);
    return hipGetLastError();
}

}  // namespace vio360
