// resize.h — what resize.hip (kernels) and resize_host.cpp (erp_resize_area*, erp_ingest*) share.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "ctx.h"
#include "pix_dev.h"

namespace vio360 {

struct ResizeArgs {
    PixSrc px;
    const uint8_t* src;
    int W, H, stride;
    long long frame_bytes_src;
    uint8_t* dst;
    int dW, dH, dstride;
    long long frame_bytes_dst;
    int fx, fy;
    float scale;  // 1.f / (fx * fy)
};

// the taps of one output column / row of the general path: source indices first .. first + count - 1, weight
// w_first for the first of them, w_last for the last (when count > 1), w_mid for the others
struct AreaTaps {
    int32_t first, count;
    float w_first, w_mid, w_last;
};

struct ResizeAnyArgs {
    PixSrc px;
    const uint8_t* src;
    int W, stride;
    long long frame_bytes_src;
    uint8_t* dst;
    int dW, dstride;
    long long frame_bytes_dst;
    const AreaTaps* tx;  // dW records
    const AreaTaps* ty;  // dH records
};

// the integer-factor kernel of a pixel source (grey: the factor-4 kernel where sizes, pitches and pointers allow
// it; kPixRun3 with fx 2 or 4 only)
hipError_t launch_area_integer(const ResizeArgs& a, int mode, int n_frames, hipStream_t stream);
// the general kernel of a pixel source: the <4>, <8> or any-count variant by max_x_taps, the widest column of a.tx
// (kPixRun3 with max_x_taps <= 8 only)
hipError_t launch_area_general(const ResizeAnyArgs& a, int mode, int dH, int n_frames, int max_x_taps,
                               hipStream_t stream);
// packed -> pitched u8 plane of the same size (mode: kPixByte, kPixBytes3 or kPixDword)
hipError_t launch_ingest_convert(const ResizeArgs& a, int mode, int n_frames, hipStream_t stream);

}  // namespace vio360
