// epipolar.hip — known-rotation epipolar RANSAC for gfx950 (the rule: include/vio360.h, erp_epi_params).
//
//   epi_prep_kernel    one thread per compacted point: a = R b0, nrm = a x b1, nn, the flags rin / par_ok, packed
//                      as two float4 per point (32 B: every wave of the hypothesis kernel reads all of them, they
//                      stay in L2 / the vector L1).  R is the given rotation or the rotation RANSAC's best, which
//                      every workgroup picks from the hypotheses' counts itself (no extra launch, no hand-off).
//   epi_hyp_kernel     one wavefront per hypothesis, four per workgroup (as ransac_hyp_kernel): lanes stride over the
//                      points, pos / neg / rin reduced with __shfl_xor, lane 0 writes count and rescued / sigma.
//   epi_select_kernel  one workgroup: first strictly-best hypothesis, the support test, the mask scattered through
//                      gidx into kept, n_in, t_dir and the counters.
// Compiled with -ffp-contract=off: every f32 expression is the oracle's (tests/epipolar_oracle.py), bit for bit.
#include "epipolar.h"

namespace vio360 {

namespace {

constexpr uint32_t EF_RIN = 1u, EF_PAR = 2u;

struct V3 {
    float x, y, z;
};
__device__ __forceinline__ V3 cross3(const V3& a, const V3& q) {
    return V3{a.y * q.z - a.z * q.y, a.z * q.x - a.x * q.z, a.x * q.y - a.y * q.x};
}
__device__ __forceinline__ float dot3(const V3& a, const V3& q) { return (a.x * q.x + a.y * q.y) + a.z * q.z; }

// the vote of point k under t: 0 off the plane (or s == 0), +1 / -1 the sign of s
__device__ __forceinline__ int epi_vote(const V3& t, float tt, const float4& pa, const float4& pn, float s2_epi) {
    const V3 a{pa.x, pa.y, pa.z}, nrm{pn.x, pn.y, pn.z};
    const V3 m = cross3(t, a);
    const float mm = dot3(m, m);
    const float e = dot3(t, nrm);
    const bool on_plane = mm > 1e-6f * tt && e * e < s2_epi * mm;
    const float s = -dot3(nrm, m);
    return !on_plane ? 0 : s > 0.f ? 1 : s < 0.f ? -1 : 0;
}

// t of hypothesis `it` and tt; false when the hypothesis is skipped
__device__ __forceinline__ bool epi_model(const EpiArgs& E, int it, int n, V3& t, float& tt) {
    const int i = E.samples[3 * it], j = E.samples[3 * it + 1];
    if ((unsigned)i >= (unsigned)n || (unsigned)j >= (unsigned)n) return false;  // (never for a valid sample row)
    const float4 ai = E.pa[i], aj = E.pa[j];
    if ((__float_as_uint(ai.w) | __float_as_uint(aj.w)) & EF_RIN) return false;
    const float4 ni = E.pn[i], nj = E.pn[j];
    t = cross3(V3{ni.x, ni.y, ni.z}, V3{nj.x, nj.y, nj.z});
    tt = dot3(t, t);
    return tt >= E.s2_plane * (ni.w * nj.w);
}

// first strictly-best entry of count[0, iters) above `floor` over the 256 threads: its index, -1 when none
__device__ int first_best(const int* count, int iters, int floor, int* sbest, int* sidx) {
    int best = floor, bi = -1;
    for (int it = threadIdx.x; it < iters; it += 256) {
        const int c = count[it];
        if (c > best) { best = c; bi = it; }  // strictly greater keeps the earliest of this thread
    }
    sbest[threadIdx.x] = best;
    sidx[threadIdx.x] = bi;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) {
            const int b2 = sbest[threadIdx.x + s], i2 = sidx[threadIdx.x + s];
            if (b2 > sbest[threadIdx.x] || (b2 == sbest[threadIdx.x] && i2 >= 0 && i2 < sidx[threadIdx.x])) {
                sbest[threadIdx.x] = b2;
                sidx[threadIdx.x] = i2;
            }
        }
        __syncthreads();
    }
    return sidx[0];
}

}  // namespace

__global__ void __launch_bounds__(256) epi_prep_kernel(EpiArgs E) {
    __shared__ int sbest[256], sidx[256];
    __shared__ float Rs[9];
    const int n = *E.n_good;
    bool have = true;
    if (E.given) {
        if (threadIdx.x == 0) {
#pragma unroll
            for (int i = 0; i < 9; ++i) Rs[i] = E.rot[i];
        }
    } else {
        // ransac_best's choice: the first hypothesis with the strictly greatest inlier count > 0 (n >= 3)
        const int bit = n >= 3 ? first_best(E.rot_count, E.rot_iters, 0, sbest, sidx) : -1;
        have = bit >= 0;
        if (have && threadIdx.x < 9) Rs[threadIdx.x] = E.rot_all[9 * bit + threadIdx.x];
    }
    __syncthreads();
    if (blockIdx.x == 0 && threadIdx.x == 0) E.scal[ES_HAVE_R] = have ? 1 : 0;
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (!have || k >= n) return;
    const float* p = E.b0 + 3 * k;
    const V3 q{E.b1[3 * k], E.b1[3 * k + 1], E.b1[3 * k + 2]};
    const V3 a{(Rs[0] * p[0] + Rs[1] * p[1]) + Rs[2] * p[2], (Rs[3] * p[0] + Rs[4] * p[1]) + Rs[5] * p[2],
               (Rs[6] * p[0] + Rs[7] * p[1]) + Rs[8] * p[2]};
    const float c = dot3(a, q);
    const V3 nrm = cross3(a, q);
    const float nn = dot3(nrm, nrm);
    const float cc = c < -1.f ? -1.f : (c > 1.f ? 1.f : c);  // rot_inlier's clamp
    const uint32_t flags = (cc >= *E.cmin ? EF_RIN : 0u) | (c >= E.cmax ? EF_PAR : 0u);
    E.pa[k] = make_float4(a.x, a.y, a.z, __uint_as_float(flags));
    E.pn[k] = make_float4(nrm.x, nrm.y, nrm.z, nn);
}

__global__ void __launch_bounds__(256) epi_hyp_kernel(EpiArgs E) {
    const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int it = blockIdx.x * 4 + wid;
    if (it >= E.iters || !E.scal[ES_HAVE_R]) return;
    const int n = *E.n_good;
    if (n < E.min_n) return;
    V3 t;
    float tt;
    if (!epi_model(E, it, n, t, tt)) {  // (wave-uniform)
        if (lane == 0) E.count[it] = -1;
        return;
    }
    int pos = 0, neg = 0, rin = 0;
    for (int k = lane; k < n; k += 64) {
        const float4 pa = E.pa[k];
        const uint32_t f = __float_as_uint(pa.w);
        if (f & EF_RIN) { ++rin; continue; }
        if (!(f & EF_PAR)) continue;
        const int v = epi_vote(t, tt, pa, E.pn[k], E.s2_epi);
        pos += v > 0 ? 1 : 0;
        neg += v < 0 ? 1 : 0;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        pos += __shfl_xor(pos, off, 64);
        neg += __shfl_xor(neg, off, 64);
        rin += __shfl_xor(rin, off, 64);
    }
    if (lane == 0) {
        const int rescued = pos > neg ? pos : neg;
        E.count[it] = rin + rescued;
        E.resc[it] = (rescued << 1) | (pos >= neg ? 1 : 0);
    }
}

__global__ void __launch_bounds__(256) epi_select_kernel(EpiArgs E) {
    __shared__ int sbest[256], sidx[256];
    __shared__ int wsum[4];
    int* info = E.scal + ES_INFO;
    if (!E.scal[ES_HAVE_R]) {  // the rotation RANSAC found nothing: its result (everything kept) stands
        if (threadIdx.x == 0) {
            info[0] = *E.n_in;
            info[1] = 0;
            info[2] = -1;
            info[3] = 0;
            info[4] = info[5] = info[6] = 0;
        }
        return;
    }
    const int n = *E.n_good;
    const int bi = (n >= E.min_n && E.iters > 0) ? first_best(E.count, E.iters, -1, sbest, sidx) : -1;
    int rescued = 0, sigma = 1;
    V3 t{0.f, 0.f, 0.f};
    float tt = 0.f;
    bool valid = false;
    if (bi >= 0) {
        const int r = E.resc[bi];
        rescued = r >> 1;
        sigma = (r & 1) ? 1 : -1;
        valid = rescued >= E.min_support && epi_model(E, bi, n, t, tt);
    }
    int n_rot = 0;
    for (int j = threadIdx.x; j < n; j += 256) {
        const float4 pa = E.pa[j];
        const uint32_t f = __float_as_uint(pa.w);
        const bool rin = f & EF_RIN;
        n_rot += rin ? 1 : 0;
        bool m = rin;
        if (valid && !rin && (f & EF_PAR)) m = epi_vote(t, tt, pa, E.pn[j], E.s2_epi) == sigma;
        E.kept[E.gidx[j]] = m ? 1 : 0;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) n_rot += __shfl_xor(n_rot, off, 64);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = n_rot;
    __syncthreads();
    if (threadIdx.x == 0) {
        n_rot = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
        info[0] = n_rot;
        info[1] = valid ? rescued : 0;
        info[2] = bi;
        info[3] = valid ? 1 : 0;
        float d[3] = {0.f, 0.f, 0.f};
        if (valid) {
            const float nr = sqrtf(tt);
            const float sx = sigma > 0 ? -t.x : t.x, sy = sigma > 0 ? -t.y : t.y, sz = sigma > 0 ? -t.z : t.z;
            d[0] = sx / nr;
            d[1] = sy / nr;
            d[2] = sz / nr;
        }
        info[4] = __float_as_int(d[0]);
        info[5] = __float_as_int(d[1]);
        info[6] = __float_as_int(d[2]);
        *E.n_in = n_rot + (valid ? rescued : 0);
    }
}

hipError_t launch_epipolar(const EpiArgs& e, hipStream_t st) {
    const int nb = ((e.n_max > 0 ? e.n_max : 1) + 255) / 256;
    hipLaunchKernelGGL(epi_prep_kernel, dim3(nb), dim3(256), 0, st, e);
    if (e.iters > 0) hipLaunchKernelGGL(epi_hyp_kernel, dim3((e.iters + 3) / 4), dim3(256), 0, st, e);
    hipLaunchKernelGGL(epi_select_kernel, dim3(1), dim3(256), 0, st, e);
    return hipGetLastError();
}

}  // namespace vio360
