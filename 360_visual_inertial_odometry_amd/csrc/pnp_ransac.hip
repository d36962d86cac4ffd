// pnp_ransac.hip — absolute-pose RANSAC on map points and spherical bearings (beyond the reference,
// whose Optimizer::SolvePnP only refines a predicted pose).  The rule is stated in include/vio360.h.
//
// Kernels (one call = three launches on the context stream, no host synchronisation between them):
//   pnp_hyp_kernel     one lane per sample row: the skip predicates, then P3P (mode A: up to four poses) or the
//                      known-rotation two-point solve (mode B: one pose), f64 in registers (pnp_dev.h);
//   pnp_count_kernel   one 256-thread workgroup per row: every point is read once and tested against each of the
//                      row's poses, integer LDS atomics (exact), the row's best count and solution;
//   pnp_finish_kernel  one workgroup: the first strictly best row, its mask, refit_iters Gauss-Newton steps on its
//                      inliers (normal equations as fixed-order f64 sums: lane l of kFitLanes sums points
//                      i = l mod kFitLanes in increasing i, the partials are summed in lane order; 6x6 Cholesky in
//                      one lane), the recount, the final mask, the RMS angle and the result record.
#include <hip/hip_runtime.h>

#include <cmath>

#include "pnp_ransac.h"

namespace vio360 {

__global__ __launch_bounds__(kPnpHypLanes) void pnp_hyp_kernel(PnpArgs a) {
    const int h = blockIdx.x * kPnpHypLanes + threadIdx.x;
    if (h >= a.iters) return;
    a.nsol[h] = pnp_row_poses(a.points, a.bearings, a.samples[3 * h], a.samples[3 * h + 1],
                              a.known ? -1 : a.samples[3 * h + 2], a.known != 0, a.Rk, a.cp2,
                              a.poses + (size_t)h * (4 * 12));
}

__global__ __launch_bounds__(kPnpThreads) void pnp_count_kernel(PnpArgs a) {
    __shared__ int cnt[4];
    const int h = blockIdx.x;
    const int nsol = a.nsol[h];
    if (nsol == 0) {
        if (threadIdx.x == 0) {
            a.count[h] = -1;
            a.best_sol[h] = -1;
        }
        return;
    }
    if (threadIdx.x < 4) cnt[threadIdx.x] = 0;
    double P[4][12];
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int q = 0; q < 12; ++q) P[s][q] = s < nsol ? a.poses[(size_t)h * 48 + 12 * s + q] : 0.0;
    __syncthreads();
    int mine[4] = {0, 0, 0, 0};
    for (int i = threadIdx.x; i < a.n; i += kPnpThreads) {
        const PnpV3 p = pnp_load3(a.points, i), b = pnp_load3(a.bearings, i);
#pragma unroll
        for (int s = 0; s < 4; ++s)
            if (s < nsol) mine[s] += pnp_inlier(pnp_transform(P[s], P[s] + 9, p), b, a.c2) ? 1 : 0;
    }
#pragma unroll
    for (int s = 0; s < 4; ++s)
        if (mine[s]) atomicAdd(&cnt[s], mine[s]);
    __syncthreads();
    if (threadIdx.x == 0) {
        int best = 0, bc = cnt[0];
        for (int s = 1; s < nsol; ++s)
            if (cnt[s] > bc) {
                bc = cnt[s];
                best = s;
            }
        a.count[h] = bc;
        a.best_sol[h] = best;
    }
}

struct PnpFinShared {
    double part[kPnpSums][kPnpFitLanes];
    double H[36], g[6], dx[6];
    double R0[9], t0[3], R[9], t[3];
    double rms;
    uint8_t mask[kPnpMaxPoints];
    int bc[kPnpThreads], bh[kPnpThreads];
    int best, cnt, ok;
};

// the inliers of (R, t) into sh.mask, their number into sh.cnt
__device__ __forceinline__ void fin_mask(const PnpArgs& a, PnpFinShared& sh, const double* R, const double* t, bool any) {
    const int tid = threadIdx.x;
    if (tid == 0) sh.cnt = 0;
    __syncthreads();
    int mine = 0;
    for (int i = tid; i < a.n; i += kPnpThreads) {
        const bool in = any && pnp_inlier(pnp_transform(R, t, pnp_load3(a.points, i)), pnp_load3(a.bearings, i), a.c2);
        sh.mask[i] = in ? 1 : 0;
        mine += in ? 1 : 0;
    }
    if (mine) atomicAdd(&sh.cnt, mine);
    __syncthreads();
}

// sh.part[0 .. m) summed over lanes in lane order into dst
__device__ __forceinline__ void fin_reduce(PnpFinShared& sh, int m, double* dst) {
    const int tid = threadIdx.x;
    if (tid < m) {
        double s = 0.0;
        for (int l = 0; l < kPnpFitLanes; ++l) s += sh.part[tid][l];
        dst[tid] = s;
    }
    __syncthreads();
}

__global__ __launch_bounds__(kPnpThreads) void pnp_finish_kernel(PnpArgs a) {
    __shared__ PnpFinShared sh;
    const int tid = threadIdx.x;
    const int n = a.n;
    vio_pnp_ransac_result* res = a.res;
    // the first row with the strictly greatest count >= 0: each thread over its strided rows, then thread 0
    {
        int bc = -1, bh = -1;
        for (int h = tid; h < a.iters; h += kPnpThreads) {
            const int c = a.count[h];
            if (c > bc) {
                bc = c;
                bh = h;
            }
        }
        sh.bc[tid] = bc;
        sh.bh[tid] = bh;
    }
    __syncthreads();
    if (tid == 0) {
        int bc = -1, bh = -1;
        for (int l = 0; l < kPnpThreads; ++l)
            if (sh.bc[l] > bc || (sh.bc[l] == bc && bc >= 0 && sh.bh[l] < bh)) {
                bc = sh.bc[l];
                bh = sh.bh[l];
            }
        sh.best = bh;
        const int bs = bh >= 0 ? a.best_sol[bh] : -1;
        for (int q = 0; q < 9; ++q) sh.R0[q] = sh.R[q] = bh >= 0 ? a.poses[(size_t)bh * 48 + 12 * bs + q] : 0.0;
        for (int q = 0; q < 3; ++q) sh.t0[q] = sh.t[q] = bh >= 0 ? a.poses[(size_t)bh * 48 + 12 * bs + 9 + q] : 0.0;
        res->best_hypothesis = bh;
        res->best_solution = bs;
        res->num_inliers_sample = bh >= 0 ? bc : 0;
        res->num_inliers = 0;
        res->refit_kept = 0;
        res->rms_angle_rad = 0.0;
        res->status = bh < 0 ? VIO_PNPR_NO_MODEL : (bc < a.p.min_inliers ? VIO_PNPR_FEW_INLIERS : VIO_PNPR_OK);
        sh.ok = 1;
    }
    __syncthreads();
    const bool any = sh.best >= 0;
    fin_mask(a, sh, sh.R0, sh.t0, any);
    const int count0 = sh.cnt;
    int kept = 0;
    if (any && a.p.refit_iters > 0 && count0 >= 3) {
        for (int it = 0; it < a.p.refit_iters; ++it) {
            // normal equations of r = unit(x) - b under x <- x + w x x + v: J = (I - u u^T) / |x| * [-[x]x  I]
            if (tid < kPnpFitLanes) {
                double acc[kPnpSums];
#pragma unroll
                for (int q = 0; q < kPnpSums; ++q) acc[q] = 0.0;
                for (int i = tid; i < n; i += kPnpFitLanes) {
                    if (!sh.mask[i]) continue;
                    const PnpV3 x = pnp_transform(sh.R, sh.t, pnp_load3(a.points, i));
                    const PnpV3 b = pnp_load3(a.bearings, i);
                    const double inv = 1.0 / sqrt(pdot(x, x));
                    const PnpV3 u = pscale(inv, x);
                    const PnpV3 r = psub(u, b);
                    // rows of M = (I - u u^T) * inv
                    const PnpV3 m0 = pv((1.0 - u.x * u.x) * inv, -(u.x * u.y) * inv, -(u.x * u.z) * inv);
                    const PnpV3 m1 = pv(-(u.y * u.x) * inv, (1.0 - u.y * u.y) * inv, -(u.y * u.z) * inv);
                    const PnpV3 m2 = pv(-(u.z * u.x) * inv, -(u.z * u.y) * inv, (1.0 - u.z * u.z) * inv);
                    // J_w = -M [x]x: its row k is x x m_k
                    const PnpV3 w0 = pcross(x, m0), w1 = pcross(x, m1), w2 = pcross(x, m2);
                    const double J[3][6] = {{w0.x, w0.y, w0.z, m0.x, m0.y, m0.z},
                                            {w1.x, w1.y, w1.z, m1.x, m1.y, m1.z},
                                            {w2.x, w2.y, w2.z, m2.x, m2.y, m2.z}};
                    const double rr[3] = {r.x, r.y, r.z};
                    int q = 0;
#pragma unroll
                    for (int c = 0; c < 6; ++c) {
#pragma unroll
                        for (int d = c; d < 6; ++d) {
                            acc[q] += (J[0][c] * J[0][d] + J[1][c] * J[1][d]) + J[2][c] * J[2][d];
                            ++q;
                        }
                    }
#pragma unroll
                    for (int c = 0; c < 6; ++c) acc[21 + c] += (J[0][c] * rr[0] + J[1][c] * rr[1]) + J[2][c] * rr[2];
                }
#pragma unroll
                for (int q = 0; q < kPnpSums; ++q) sh.part[q][tid] = acc[q];
            }
            __syncthreads();
            if (tid < kPnpSums) {
                double s = 0.0;
                for (int l = 0; l < kPnpFitLanes; ++l) s += sh.part[tid][l];
                if (tid < 21) {
                    // upper triangle in row order -> (c, d)
                    int c = 0, q = tid;
                    while (q >= 6 - c) {
                        q -= 6 - c;
                        ++c;
                    }
                    const int d = c + q;
                    sh.H[6 * c + d] = s;
                    sh.H[6 * d + c] = s;
                } else {
                    sh.g[tid - 21] = s;
                }
            }
            __syncthreads();
            if (tid == 0) {
                // Cholesky H = L L^T in place (lower), then L L^T dx = -g
                bool good = true;
                for (int c = 0; c < 6 && good; ++c) {
                    double d = sh.H[6 * c + c];
                    for (int q = 0; q < c; ++q) d -= sh.H[6 * c + q] * sh.H[6 * c + q];
                    if (!(d > 0.0) || !pfinite(d)) {
                        good = false;
                        break;
                    }
                    d = sqrt(d);
                    sh.H[6 * c + c] = d;
                    for (int r = c + 1; r < 6; ++r) {
                        double s = sh.H[6 * r + c];
                        for (int q = 0; q < c; ++q) s -= sh.H[6 * r + q] * sh.H[6 * c + q];
                        sh.H[6 * r + c] = s / d;
                    }
                }
                if (good) {
                    for (int r = 0; r < 6; ++r) {
                        double s = -sh.g[r];
                        for (int q = 0; q < r; ++q) s -= sh.H[6 * r + q] * sh.dx[q];
                        sh.dx[r] = s / sh.H[6 * r + r];
                    }
                    for (int r = 5; r >= 0; --r) {
                        double s = sh.dx[r];
                        for (int q = r + 1; q < 6; ++q) s -= sh.H[6 * q + r] * sh.dx[q];
                        sh.dx[r] = s / sh.H[6 * r + r];
                    }
                    for (int q = 0; q < 6; ++q) good = good && pfinite(sh.dx[q]);
                }
                if (good) {
                    // R <- Q R, t <- Q t + v with Q the rotation of the unit quaternion (1, w / 2) / |.|
                    const double hx = 0.5 * sh.dx[0], hy = 0.5 * sh.dx[1], hz = 0.5 * sh.dx[2];
                    const double qn = 1.0 / sqrt(((1.0 + hx * hx) + hy * hy) + hz * hz);
                    const double qw = qn, qx = hx * qn, qy = hy * qn, qz = hz * qn;
                    const double Q[9] = {1.0 - 2.0 * (qy * qy + qz * qz), 2.0 * (qx * qy - qw * qz), 2.0 * (qx * qz + qw * qy),
                                         2.0 * (qx * qy + qw * qz), 1.0 - 2.0 * (qx * qx + qz * qz), 2.0 * (qy * qz - qw * qx),
                                         2.0 * (qx * qz - qw * qy), 2.0 * (qy * qz + qw * qx), 1.0 - 2.0 * (qx * qx + qy * qy)};
                    double Rn[9], tn[3];
                    for (int r = 0; r < 3; ++r) {
                        for (int c = 0; c < 3; ++c)
                            Rn[3 * r + c] = (Q[3 * r] * sh.R[c] + Q[3 * r + 1] * sh.R[3 + c]) + Q[3 * r + 2] * sh.R[6 + c];
                        tn[r] = ((Q[3 * r] * sh.t[0] + Q[3 * r + 1] * sh.t[1]) + Q[3 * r + 2] * sh.t[2]) + sh.dx[3 + r];
                    }
                    for (int q = 0; q < 9; ++q) sh.R[q] = Rn[q];
                    for (int q = 0; q < 3; ++q) sh.t[q] = tn[q];
                } else {
                    sh.ok = 0;
                }
            }
            __syncthreads();
            if (!sh.ok) break;
        }
        // the recount: the refit is kept when it counts at least as many inliers as the minimal pose
        fin_mask(a, sh, sh.R, sh.t, true);
        kept = sh.cnt >= count0 ? 1 : 0;
        if (!kept) fin_mask(a, sh, sh.R0, sh.t0, true);
    }
    const double* Rf = kept ? sh.R : sh.R0;
    const double* tf = kept ? sh.t : sh.t0;
    // the RMS angle over the returned pose's inliers, the same fixed-order sum
    if (tid < kPnpFitLanes) {
        double s = 0.0;
        for (int i = tid; i < n; i += kPnpFitLanes) {
            if (!sh.mask[i]) continue;
            const PnpV3 x = pnp_transform(Rf, tf, pnp_load3(a.points, i));
            const PnpV3 b = pnp_load3(a.bearings, i), c = pcross(b, x);
            const double ang = atan2(sqrt(pdot(c, c)), pdot(b, x));
            s += ang * ang;
        }
        sh.part[0][tid] = s;
    }
    __syncthreads();
    fin_reduce(sh, 1, &sh.rms);
    for (int i = tid; i < n; i += kPnpThreads) a.mask[i] = sh.mask[i];
    if (tid == 0) {
        res->num_inliers = any ? sh.cnt : 0;
        res->refit_kept = kept;
        res->rms_angle_rad = sh.cnt > 0 ? sqrt(sh.rms / (double)sh.cnt) : 0.0;
        for (int q = 0; q < 9; ++q) {
            res->R_cw[q] = Rf[q];
            res->R0_cw[q] = sh.R0[q];
        }
        for (int q = 0; q < 3; ++q) {
            res->t_cw[q] = tf[q];
            res->t0_cw[q] = sh.t0[q];
        }
    }
}

int pnp_launch(hipStream_t st, const PnpArgs& a) {
    hipLaunchKernelGGL(pnp_hyp_kernel, dim3((a.iters + kPnpHypLanes - 1) / kPnpHypLanes), dim3(kPnpHypLanes), 0, st, a);
    if (hipGetLastError() != hipSuccess) return 1;
    hipLaunchKernelGGL(pnp_count_kernel, dim3(a.iters), dim3(kPnpThreads), 0, st, a);
    if (hipGetLastError() != hipSuccess) return 2;
    hipLaunchKernelGGL(pnp_finish_kernel, dim3(1), dim3(kPnpThreads), 0, st, a);
    if (hipGetLastError() != hipSuccess) return 3;
    return 0;
}

}  // namespace vio360
