// trk_ransac.hip — ERP feature tracking on MI355X (gfx950), outlier rejection and the feature mask's discs
// (FeatureTracker.cpp:253-379); the stage between trk_lk.hip and trk_gftt.hip.
//
//   ransac_*             RejectOutliersRotationRANSAC: one wavefront per hypothesis.
//   disc_mask_kernel     CreateFeatureMask's discs as a 1-bit plane; fused with RANSAC's selection in the pipeline
//                        (ransac_select_disc_kernel).
// The sampler's mt19937 stream and the inlier test's cosine bound are in trk_ransac_dev.h: the pipeline forms the
// raw draws and the bound in extra workgroups of the LK launch (trk_lk.hip, lk_aux).
// Float expressions follow tracker_oracle.c literally and every tracker unit is built with
// -ffp-contract=off, so results are bitwise those of the oracle.
#include <hip/hip_runtime.h>

#include "tracker_types.h"
#include "trk_dev.h"
#include "trk_ransac_dev.h"

namespace vio360 {

// ------------------------------------------------------------------------------------------
// filter / RANSAC

// order-preserving compaction of the RANSAC input (single workgroup of RP_THREADS: four waves get a CU
// sooner than sixteen while GFTT pass 1 occupies the chip from the side stream):
//   mode 0: all n points (erp_rot_ransac); mode 1: status ∧ !polar ∧ !boundary (pipeline)
constexpr int RP_THREADS = 256;
// WRAP: seam wrap mode (R.x_wrap); the default instance is the code as it was
template <int NT, bool WRAP = false>
__device__ int ransac_prep_body(const RansacArgs& R, int* wsum, int& base) {
    if (threadIdx.x == 0) base = 0;
    __syncthreads();
    const int n = R.n;
    for (int c0 = 0; c0 < n; c0 += NT) {
        int i = c0 + threadIdx.x;
        int good = 0;
        if (i < n) {
            if (R.mode == 0) good = 1;
            else {
                float x = R.p1[2 * i], y = R.p1[2 * i + 1];
                float vr = y / (float)R.H;
                bool polar = (vr < R.polar_ratio) || (vr > (1.0f - R.polar_ratio));
                float m = (float)R.margin;
                // (seam wrap mode: no left / right margin, x is already folded into [0, W))
                bool nearb = WRAP ? (y < m) || (y > (float)R.H - m)
                                  : (x < m) || (x > (float)R.W - m) || (y < m) || (y > (float)R.H - m);
                good = R.status[i] && !polar && !nearb;
                if (R.excl_bits && good) {  // region mask: the pixel the point rounds to (as the disc centres)
                    int xi = (int)rintf(x);
                    const int yi = (int)rintf(y);
                    if (WRAP && xi == R.W) xi = 0;  // a column within half a pixel of the seam rounds across it
                    good = (unsigned)xi < (unsigned)R.W && (unsigned)yi < (unsigned)R.H &&
                           !((R.excl_bits[(size_t)yi * R.excl_words + (xi >> 5)] >> (xi & 31)) & 1u);
                }
            }
            R.kept[i] = 0;
        }
        unsigned long long bal = __ballot(good);
        int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
        int pre = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) wsum[wid] = __popcll(bal);
        __syncthreads();
        int off = base;
        for (int k = 0; k < wid; ++k) off += wsum[k];
        if (good) {
            int j = off + pre;
            R.gidx[j] = i;
            if (R.bear0) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    R.b0[3 * j + c] = R.bear0[3 * i + c];
                    R.b1[3 * j + c] = R.bear1[3 * i + c];
                }
            } else {
                pixel_to_bearing(R.p0[2 * i], R.p0[2 * i + 1], R.W, R.H, R.b0 + 3 * j);
                pixel_to_bearing(R.p1[2 * i], R.p1[2 * i + 1], R.W, R.H, R.b1 + 3 * j);
            }
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            int t = 0;
            for (int k = 0; k < NT / 64; ++k) t += wsum[k];
            base += t;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) *R.n_good = base;
    return base;
}

__global__ void __launch_bounds__(RP_THREADS) ransac_prep_kernel(RansacArgs R) {
    __shared__ int wsum[RP_THREADS / 64];
    __shared__ int base;
    ransac_prep_body<RP_THREADS>(R, wsum, base);
    if (threadIdx.x == 0) *R.cmin = ransac_cos_bound(R.thresh);
}

// the sequential sampler (trk_ransac_dev.h): what the parallel form below falls back to when its stream runs out
__device__ void ransac_sample_seq(const RansacArgs& R, Mt19937& g, int n) {
    g.seed(R.seed);
    for (int it = 0; it < R.iters; ++it) {
        int got[3];
        int k = 0;
        while (k < 3) {
            int idx = (int)uniform_below(g, (uint32_t)n);
            bool dup = false;
            for (int q = 0; q < k; ++q) dup |= got[q] == idx;
            if (!dup) got[k++] = idx;
        }
        R.samples[3 * it] = got[0];
        R.samples[3 * it + 1] = got[1];
        R.samples[3 * it + 2] = got[2];
    }
}

// The input compaction (ransac_prep_body) first, in the same workgroup (one launch fewer on the
// tracker's critical path); the sampler then reads the count from LDS.  Four waves (a sixteen-wave
// workgroup waits longer for a CU while GFTT pass 1 fills the chip from the side stream): thread t
// tests the RS_CHUNK contiguous stream words [t RS_CHUNK, (t+1) RS_CHUNK), one block scan of the
// per-thread accept counts places its accepted draws in stream order.
constexpr int RS_SAMPLE_THREADS = 256;
constexpr int RS_CHUNK = 20;
static_assert(RS_CHUNK % 4 == 0 && RS_RAW % 4 == 0 && RS_SAMPLE_THREADS * RS_CHUNK >= RS_RAW, "sampler chunks");
template <bool WRAP = false>
__global__ void __launch_bounds__(RS_SAMPLE_THREADS) ransac_sample_kernel(RansacArgs R) {
    __shared__ uint32_t acc[RS_RAW];    // accepted draws (compacted), in stream order
    __shared__ uint8_t len3[RS_RAW];    // 1: a hypothesis starting at draw p consumes exactly 3 draws
    __shared__ int wsum[RS_SAMPLE_THREADS / 64];
    __shared__ int s_fallback, s_base;
#ifdef TRK_STAMPS
    const unsigned long long ts0 = __builtin_amdgcn_s_memtime();
#endif
    const int n = ransac_prep_body<RS_SAMPLE_THREADS, WRAP>(R, wsum, s_base);
#ifdef TRK_STAMPS
    const unsigned long long ts1 = __builtin_amdgcn_s_memtime();
#endif
    __syncthreads();  // wsum is reused below
    if (n < 3 || R.iters <= 0) return;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int w0 = tid * RS_CHUNK;
    uint32_t yw[RS_CHUNK];  // the thread's tempered words (raw: a 256-B aligned allocation)
#pragma unroll
    for (int q = 0; q < RS_CHUNK / 4; ++q) {
        const int w = w0 + 4 * q;
        const uint4 v = w < RS_RAW ? *reinterpret_cast<const uint4*>(R.raw + w) : make_uint4(0u, 0u, 0u, 0u);
        yw[4 * q] = v.x;
        yw[4 * q + 1] = v.y;
        yw[4 * q + 2] = v.z;
        yw[4 * q + 3] = v.w;
    }
    const uint32_t range = (uint32_t)n;
    const uint32_t thr = (uint32_t)(-range) % range;
    auto accepted = [&](int u) {  // uniform_int_distribution's rejection test of word u
        const uint32_t low = (uint32_t)((uint64_t)yw[u] * range);
        return w0 + u < RS_RAW && !(low < range && low < thr);
    };
    int cnt = 0;
#pragma unroll
    for (int u = 0; u < RS_CHUNK; ++u) cnt += accepted(u) ? 1 : 0;
    int incl = cnt;  // inclusive scan over the wave
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int v = __shfl_up(incl, off, 64);
        if (lane >= off) incl += v;
    }
    if (lane == 63) wsum[wid] = incl;
    __syncthreads();
    int pos = incl - cnt;
    for (int q = 0; q < wid; ++q) pos += wsum[q];
#pragma unroll
    for (int u = 0; u < RS_CHUNK; ++u)
        if (accepted(u)) acc[pos++] = (uint32_t)(((uint64_t)yw[u] * range) >> 32);
    const int M = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    __syncthreads();
    for (int p = tid; p < M; p += RS_SAMPLE_THREADS)
        len3[p] = (p + 2 < M && acc[p] != acc[p + 1] && acc[p] != acc[p + 2] && acc[p + 1] != acc[p + 2]) ? 1 : 0;
    __syncthreads();
#ifdef TRK_STAMPS
    const unsigned long long ts2 = __builtin_amdgcn_s_memtime();
#endif
    if (wid == 0) {
        int s = 0, h = 0;
        bool fb = false;
        while (h < R.iters && !fb) {
            const int p = s + 3 * lane;
            const bool ok = h + lane < R.iters && p + 2 < M && len3[p];
            const unsigned long long bad = __ballot(!ok);
            const int f = bad ? __ffsll((long long)bad) - 1 : 64;
            if (lane < f) {
                R.samples[3 * (h + lane)] = (int)acc[p];
                R.samples[3 * (h + lane) + 1] = (int)acc[p + 1];
                R.samples[3 * (h + lane) + 2] = (int)acc[p + 2];
            }
            s += 3 * f;
            h += f;
            if (h >= R.iters) break;
            if (f < 64) {  // hypothesis h consumes more than 3 draws (a duplicate) or the stream ends
                int got[3], k = 0, q = s;
                while (k < 3 && q < M) {
                    const int idx = (int)acc[q++];
                    bool dup = false;
                    for (int u = 0; u < k; ++u) dup |= got[u] == idx;
                    if (!dup) got[k++] = idx;
                }
                if (k < 3) { fb = true; break; }
                if (lane == 0) {
                    R.samples[3 * h] = got[0];
                    R.samples[3 * h + 1] = got[1];
                    R.samples[3 * h + 2] = got[2];
                }
                s = q;
                ++h;
            }
        }
        if (lane == 0) s_fallback = fb ? 1 : 0;
    }
    __syncthreads();
#ifdef TRK_STAMPS
    if (tid == 0)
        printf("ransac_sample: prep %llu draws %llu chain %llu (n %d, M %d)\n", ts1 - ts0, ts2 - ts1,
               __builtin_amdgcn_s_memtime() - ts2, n, M);
#endif
    if (s_fallback && tid == 0) {
        __shared__ Mt19937 g;  // stream exhausted: the sequential sampler from the seed
        ransac_sample_seq(R, g, n);
    }
}

__device__ void jacobi3(double* A, double* V) {
    for (int i = 0; i < 9; ++i) V[i] = (i % 4 == 0) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 12; ++sweep) {
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                double apq = A[3 * p + q];
                if (apq == 0.0) continue;
                double app = A[3 * p + p], aqq = A[3 * q + q];
                double theta = (aqq - app) / (2.0 * apq);
                double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < 3; ++k) {
                    double akp = A[3 * k + p], akq = A[3 * k + q];
                    A[3 * k + p] = c * akp - s * akq;
                    A[3 * k + q] = s * akp + c * akq;
                }
                for (int k = 0; k < 3; ++k) {
                    double apk = A[3 * p + k], aqk = A[3 * q + k];
                    A[3 * p + k] = c * apk - s * aqk;
                    A[3 * q + k] = s * apk + c * aqk;
                }
                for (int k = 0; k < 3; ++k) {
                    double vkp = V[3 * k + p], vkq = V[3 * k + q];
                    V[3 * k + p] = c * vkp - s * vkq;
                    V[3 * k + q] = s * vkp + c * vkq;
                }
            }
    }
}

// EstimateRotation (FeatureTracker.cpp:330-355): nearest proper rotation of H (see oracle)
__device__ void kabsch_rotation(const float* Hf, float* Rf) {
    double H[9], HtH[9], V[9];
    for (int i = 0; i < 9; ++i) H[i] = Hf[i];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) HtH[3 * i + j] = H[i] * H[j] + H[3 + i] * H[3 + j] + H[6 + i] * H[6 + j];
    jacobi3(HtH, V);
    double w[3] = {HtH[0], HtH[4], HtH[8]};
    int idx[3] = {0, 1, 2};
    for (int i = 0; i < 3; ++i)
        for (int j = i + 1; j < 3; ++j)
            if (w[idx[j]] > w[idx[i]]) { int t = idx[i]; idx[i] = idx[j]; idx[j] = t; }
    double v[3][3], u[3][3];
    for (int c = 0; c < 3; ++c)
        for (int r = 0; r < 3; ++r) v[c][r] = V[3 * r + idx[c]];
    for (int c = 0; c < 2; ++c) {
        for (int r = 0; r < 3; ++r) u[c][r] = H[3 * r] * v[c][0] + H[3 * r + 1] * v[c][1] + H[3 * r + 2] * v[c][2];
        double nn = sqrt(u[c][0] * u[c][0] + u[c][1] * u[c][1] + u[c][2] * u[c][2]);
        if (nn > 0) { u[c][0] /= nn; u[c][1] /= nn; u[c][2] /= nn; }
    }
    double d01 = u[0][0] * u[1][0] + u[0][1] * u[1][1] + u[0][2] * u[1][2];
    for (int r = 0; r < 3; ++r) u[1][r] -= d01 * u[0][r];
    double n1 = sqrt(u[1][0] * u[1][0] + u[1][1] * u[1][1] + u[1][2] * u[1][2]);
    if (n1 > 0) { u[1][0] /= n1; u[1][1] /= n1; u[1][2] /= n1; }
    u[2][0] = u[0][1] * u[1][2] - u[0][2] * u[1][1];
    u[2][1] = u[0][2] * u[1][0] - u[0][0] * u[1][2];
    u[2][2] = u[0][0] * u[1][1] - u[0][1] * u[1][0];
    double dV = v[0][0] * (v[1][1] * v[2][2] - v[1][2] * v[2][1]) - v[1][0] * (v[0][1] * v[2][2] - v[0][2] * v[2][1]) +
                v[2][0] * (v[0][1] * v[1][2] - v[0][2] * v[1][1]);
    double d = dV < 0 ? -1.0 : 1.0;
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) Rf[3 * r + c] = (float)(u[0][r] * v[0][c] + u[1][r] * v[1][c] + d * u[2][r] * v[2][c]);
}

__device__ __forceinline__ float det3f(const float* m) {
    return m[0] * (m[4] * m[8] - m[7] * m[5]) - m[3] * (m[1] * m[8] - m[7] * m[2]) + m[6] * (m[1] * m[5] - m[4] * m[2]);
}

__device__ __forceinline__ bool rot_inlier(const float* R, const float* a, const float* q, float cmin) {
    float r0 = (R[0] * a[0] + R[1] * a[1]) + R[2] * a[2];
    float r1 = (R[3] * a[0] + R[4] * a[1]) + R[5] * a[2];
    float r2 = (R[6] * a[0] + R[7] * a[1]) + R[8] * a[2];
    float c = (r0 * q[0] + r1 * q[1]) + r2 * q[2];
    c = c < -1.f ? -1.f : (c > 1.f ? 1.f : c);
    return c >= cmin;  // (float)acos((double)c) < thr (ransac_cos_bound)
}

// one wavefront per hypothesis: count[it] = inliers, or -1 when |det R - 1| > 0.1 (skipped)
__global__ void __launch_bounds__(256) ransac_hyp_kernel(RansacArgs R) {
    const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int it = blockIdx.x * 4 + wid;
    if (it >= R.iters) return;
    const int n = *R.n_good;
    if (n < 3) return;
#ifdef TRK_STAMPS
    const unsigned long long ts0 = __builtin_amdgcn_s_memtime();
#endif
    float Hm[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int s = 0; s < 3; ++s) {
        int k = R.samples[3 * it + s];
        const float* q = R.b1 + 3 * k;
        const float* a = R.b0 + 3 * k;
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) Hm[3 * r + c] += q[r] * a[c];
    }
    float Rm[9];
#ifdef TRK_STAMPS
    const unsigned long long ts1 = __builtin_amdgcn_s_memtime();
#endif
    kabsch_rotation(Hm, Rm);
#ifdef TRK_STAMPS
    const unsigned long long ts2 = __builtin_amdgcn_s_memtime();
#endif
#pragma unroll
    for (int i = 0; i < 9; ++i)  // ransac_select reads the best one back
        if (lane == i) R.rot[9 * it + i] = Rm[i];
    if (fabsf(det3f(Rm) - 1.0f) > 0.1f) {
        if (lane == 0) R.count[it] = -1;
        return;
    }
    int cnt = 0;
    const float cmin = *R.cmin;
    for (int i = lane; i < n; i += 64) cnt += rot_inlier(Rm, R.b0 + 3 * i, R.b1 + 3 * i, cmin) ? 1 : 0;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
    if (lane == 0) R.count[it] = cnt;
#ifdef TRK_STAMPS
    if (it == 0 && lane == 0)
        printf("ransac_hyp: loads %llu kabsch %llu count %llu\n", ts1 - ts0, ts2 - ts1, __builtin_amdgcn_s_memtime() - ts2);
#endif
}

// first strictly-best hypothesis (256 threads; its rotation into Rs): returns its index, -1 when none
__device__ int ransac_best(const RansacArgs& R, int n, int* sbest, int* sidx, float* Rs) {
    int best = 0, bi = -1;
    if (n >= 3)
        for (int it = threadIdx.x; it < R.iters; it += 256) {
            int c = R.count[it];
            if (c > best) { best = c; bi = it; }  // strictly greater keeps the earliest of this thread
        }
    sbest[threadIdx.x] = best;
    sidx[threadIdx.x] = bi;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) {
            int b2 = sbest[threadIdx.x + s], i2 = sidx[threadIdx.x + s];
            if (b2 > sbest[threadIdx.x] || (b2 == sbest[threadIdx.x] && b2 > 0 && i2 < sidx[threadIdx.x])) {
                sbest[threadIdx.x] = b2;
                sidx[threadIdx.x] = i2;
            }
        }
        __syncthreads();
    }
    const int bit = sidx[0];
    if (threadIdx.x == 0 && blockIdx.x == 0) *R.n_in = n < 3 ? n : sbest[0];
    if (bit >= 0 && threadIdx.x < 9) Rs[threadIdx.x] = R.rot[9 * bit + threadIdx.x];  // ransac_hyp's rotation
    __syncthreads();
    return bit;
}
// -> mask over the good points, scattered to the input order
__global__ void __launch_bounds__(256) ransac_select_kernel(RansacArgs R) {
    __shared__ int sbest[256], sidx[256];
    __shared__ float Rs[9];
    const int n = *R.n_good;
    const int bit = ransac_best(R, n, sbest, sidx, Rs);
    for (int j = threadIdx.x; j < n; j += 256) {
        uint8_t m = 1;
        if (n >= 3 && bit >= 0) m = rot_inlier(Rs, R.b0 + 3 * j, R.b1 + 3 * j, *R.cmin) ? 1 : 0;
        R.kept[R.gidx[j]] = m;
    }
}

// rasterise the discs of CreateFeatureMask (cv::circle filled, LINE_8; half-widths precomputed
// on the host from OpenCV's midpoint Circle()) into a 1-bit-per-pixel exclusion mask
// the bits of columns [x0, x1] (inside the frame) of row y
__device__ __forceinline__ void disc_span(const DiscArgs& D, int y, int x0, int x1) {
    for (int x = x0; x <= x1;) {
        int wi = x >> 5;
        int b0 = x & 31;
        int b1 = min(31, x1 - (wi << 5));
        uint32_t m = (b1 - b0 == 31) ? 0xffffffffu : (((1u << (b1 - b0 + 1)) - 1u) << b0);
        atomicOr(&D.bits[(size_t)y * D.words + wi], m);
        x = (wi + 1) << 5;
    }
}
template <bool WRAP>
__device__ __forceinline__ void disc_raster(const DiscArgs& D, int i, int nthreads) {
    const float fx = D.pts[2 * i], fy = D.pts[2 * i + 1];
    const int cx = (int)rintf(fx), cy = (int)rintf(fy);  // Point2f -> Point (cvRound)
    const int r = D.radius;
    // seam wrap mode: the columns are taken modulo W -- a span that leaves the frame on one side continues on the
    // other (radius < W / 2: the two parts never meet); a centre further than W outside draws nothing
    if (WRAP && (cx < -D.W || cx >= 2 * D.W)) return;
    for (int dy = -r + (int)threadIdx.x; dy <= r; dy += nthreads) {
        int y = cy + dy;
        if (y < 0 || y >= D.H) continue;
        int hwd = D.halfw[dy < 0 ? -dy : dy];
        if (WRAP) {
            const int c = cx < 0 ? cx + D.W : (cx >= D.W ? cx - D.W : cx);
            const int a = c - hwd, b = c + hwd;
            disc_span(D, y, max(a, 0), min(b, D.W - 1));
            if (a < 0) disc_span(D, y, max(a + D.W, 0), D.W - 1);
            if (b >= D.W) disc_span(D, y, 0, min(b - D.W, D.W - 1));
            continue;
        }
        disc_span(D, y, max(cx - hwd, 0), min(cx + hwd, D.W - 1));
    }
}
template <bool WRAP>
__global__ void __launch_bounds__(128) disc_mask_kernel(DiscArgs D) {
    const int k = blockIdx.x;
    if (D.n_pts_dev && k >= *D.n_pts_dev) return;  // null: the grid is exactly the point count
    if (D.kept && !D.kept[D.src_index ? D.src_index[k] : k]) return;
    disc_raster<WRAP>(D, D.src_index ? D.src_index[k] : k, 128);
}

// tracker pipeline: RANSAC's selection and CreateFeatureMask's discs in one launch (one launch fewer on the
// critical path).  Workgroup j (compacted point j < n_good; the grid covers every input point) finds the best
// hypothesis itself -- the same reduction in every workgroup -- tests its point, scatters the kept flag and,
// when kept, rasterises the point's disc (disc_mask_kernel's rows; D.radius <= 0: no discs)
template <bool WRAP>
__global__ void __launch_bounds__(256) ransac_select_disc_kernel(RansacArgs R, DiscArgs D) {
    __shared__ int sbest[256], sidx[256];
    __shared__ float Rs[9];
    __shared__ int s_m;
    const int n = *R.n_good;
    if ((int)blockIdx.x >= max(n, 1)) return;  // (workgroup 0 always runs: it writes n_in)
    const int bit = ransac_best(R, n, sbest, sidx, Rs);
    const int j = blockIdx.x;
    if (j >= n) return;
    if (threadIdx.x == 0) {
        uint8_t m = 1;
        if (n >= 3 && bit >= 0) m = rot_inlier(Rs, R.b0 + 3 * j, R.b1 + 3 * j, *R.cmin) ? 1 : 0;
        R.kept[R.gidx[j]] = m;
        s_m = m;
    }
    __syncthreads();
    if (s_m && D.radius > 0) disc_raster<WRAP>(D, R.gidx[j], 256);
}

// ------------------------------------------------------------------------------------------
// launchers
size_t ransac_raw_words() { return RS_RAW; }
// the head of both sequences: the input compaction -- with the sampler behind it in one workgroup when the draws
// come from r.raw (`stream`), else alone and without wrap (the samples were uploaded) -- then, with `hyp`, one
// wavefront per hypothesis
static void ransac_head(const RansacArgs& r, bool stream, bool hyp, hipStream_t st) {
    if (stream) {
        const auto k = r.x_wrap ? ransac_sample_kernel<true> : ransac_sample_kernel<false>;
        hipLaunchKernelGGL(k, dim3(1), dim3(RS_SAMPLE_THREADS), 0, st, r);
    } else {
        hipLaunchKernelGGL(ransac_prep_kernel, dim3(1), dim3(RP_THREADS), 0, st, r);
    }
    if (hyp && r.iters > 0) hipLaunchKernelGGL(ransac_hyp_kernel, dim3((r.iters + 3) / 4), dim3(256), 0, st, r);
}
hipError_t launch_ransac_parts(const RansacArgs& r, bool stream, bool rot, hipStream_t st) {
    ransac_head(r, stream, rot, st);
    if (rot) hipLaunchKernelGGL(ransac_select_kernel, dim3(1), dim3(256), 0, st, r);
    return hipGetLastError();
}
hipError_t launch_ransac_pipeline(const RansacArgs& r, const DiscArgs& d, hipStream_t st) {
    ransac_head(r, true, true, st);
    const auto k = d.x_wrap ? ransac_select_disc_kernel<true> : ransac_select_disc_kernel<false>;
    hipLaunchKernelGGL(k, dim3(r.n > 0 ? r.n : 1), dim3(256), 0, st, r, d);
    return hipGetLastError();
}
hipError_t launch_disc_mask(const DiscArgs& d, int max_pts, hipStream_t st) {
    if (max_pts <= 0) return hipSuccess;
    const auto k = d.x_wrap ? disc_mask_kernel<true> : disc_mask_kernel<false>;
    hipLaunchKernelGGL(k, dim3(max_pts), dim3(128), 0, st, d);
    return hipGetLastError();
}

}  // namespace vio360
