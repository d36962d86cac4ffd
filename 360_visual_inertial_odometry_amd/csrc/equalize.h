// equalize.h — what equalize.hip (kernels) and equalize_host.cpp (erp_equalize*) share.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "ctx.h"

namespace vio360 {

constexpr int kEqMaxChunks = 256;  // workgroups that share one tile's histogram, at most

// One launch of the three stages over n_frames frames.  HIST runs as one tile: tiles 1 x 1, tw = W, th = H.
struct EqArgs {
    const uint8_t* src;
    uint8_t* dst;
    int W, H, stride, dstride;
    long long frame_bytes_src, frame_bytes_dst;
    int n_frames;
    int mode;  // VIO_EQ_HIST or VIO_EQ_CLAHE
    int tiles_x, tiles_y, tw, th;
    int wrap_x;
    int clip;         // CLAHE: the bin limit c, 0 = no clipping
    int area;         // CLAHE: tw * th; HIST: W * H
    float lut_scale;  // CLAHE: 255.f / (float)area
    float inv_tw, inv_th;  // 1.f / (float)tw, 1.f / (float)th
    // (a): a tile's rows are split into `chunks` runs of chunk_rows rows, one workgroup each
    int chunk_rows, chunks;
    uint32_t* part;  // [frame][tile][chunk][256]
    // (b)
    uint8_t* lut;  // [frame][tile][256]
    // (c): one workgroup per rw x rh pixel rectangle, rw <= tw and rh <= th
    int rw, rh, nrx, nry;
};

// grids: (tiles * chunks, n_frames), (tiles, n_frames), (nrx * nry, n_frames)
hipError_t launch_eq_hist(const EqArgs& a, hipStream_t stream);
hipError_t launch_eq_lut(const EqArgs& a, hipStream_t stream);
hipError_t launch_eq_apply(const EqArgs& a, hipStream_t stream);

}  // namespace vio360
