// pnp_ransac.h — what pnp_ransac.hip and pnp_host.cpp share: the kernels' argument record and the launcher.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "pnp_dev.h"
#include "vio360.h"

namespace vio360 {

constexpr int kPnpMaxPoints = 4096;  // the cap of vio_pnp_ransac_check, on points and on rows
constexpr int kPnpHypLanes = 64;     // sample rows per workgroup of pnp_hyp_kernel
constexpr int kPnpThreads = 256;     // pnp_count_kernel / pnp_finish_kernel
constexpr int kPnpFitLanes = 128;    // lanes of the refit's fixed-order sums
constexpr int kPnpSums = 27;         // 21 upper entries of J^T J + 6 of J^T r

struct PnpArgs {
    const float* points;     // n x 3 world
    const float* bearings;   // n x 3
    int n;
    const int32_t* samples;  // iters x 3
    int iters;
    int known;               // mode B
    double Rk[9];            // the known rotation (mode B)
    double c2, cp2;          // cos^2 of the inlier threshold / of the minimum pair angle
    vio_pnp_ransac_params p;
    double* poses;           // iters x 4 x (R 9, t 3)
    int32_t* nsol;           // iters
    int32_t* count;          // iters: the row's best count, -1 skipped
    int32_t* best_sol;       // iters
    vio_pnp_ransac_result* res;
    uint8_t* mask;           // n
};

// the three launches on `st`; 0, or the 1-based index of the launch that failed
int pnp_launch(hipStream_t st, const PnpArgs& a);

}  // namespace vio360
