// epipolar.h — argument block and launch of the known-rotation epipolar RANSAC (epipolar.hip), shared with the
// host side (tracker_host.cpp, frontend_host.cpp).  The rule is stated in include/vio360.h (erp_epi_params).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vio360 {

// words of the stage's device scalars (erp_tracker::d_epi_scal)
enum EpiScal {
    ES_HAVE_R = 0,  // a rotation is known: given, or the rotation RANSAC found one
    ES_INFO = 1,    // erp_epi_info: n_rot, n_rescued, best, model_valid, t_dir[3] (7 words)
    ES_COUNT = 8
};

struct EpiArgs {
    const float* b0;         // [n][3] bearings of the compacted points (ransac_prep_body)
    const float* b1;
    const int* gidx;         // [n] compacted -> input index
    const int* n_good;       // device scalar: n
    int n_max;               // upper bound of n (the input point count): epi_prep's grid
    const int32_t* samples;  // [iters][3]: a hypothesis is the first two indices of its row
    int iters;
    int min_n;               // hypotheses are evaluated from this n on (2: one-shot, 3: the sample stream's minimum)
    const float* cmin;       // device scalar: the rotation test's cosine bound (ransac_cos_bound)
    int given;               // 1: rot below; 0: the rotation RANSAC's best (rot_count / rot_all)
    float rot[9];
    const int* rot_count;    // [rot_iters] the rotation hypotheses' inlier counts (ransac_hyp_kernel)
    const float* rot_all;    // [rot_iters][9] their rotations
    int rot_iters;
    float s2_epi, s2_plane, cmax;
    int min_support;
    float4* pa;              // [n] (a0, a1, a2, flags as bits: 1 rin, 2 par_ok)
    float4* pn;              // [n] (nrm0, nrm1, nrm2, nn)
    int* count;              // [iters] count, -1: skipped
    int* resc;               // [iters] rescued << 1 | (sigma > 0)
    int* scal;               // [ES_COUNT]
    uint8_t* kept;           // [n_max] the mask in input order (written for every compacted point)
    int* n_in;               // device scalar: inliers
};

// prep (per-point terms), hypotheses, selection: three launches on st
hipError_t launch_epipolar(const EpiArgs& e, hipStream_t st);

}  // namespace vio360
