// mask.h — what mask.hip (kernels), mask_host.cpp (erp_mask_*) and tracker_host.cpp (erp_*_set_mask*) share.
//
// A region mask lives on the device as an exclusion bit-plane in the layout of the tracker's disc plane: one bit
// per pixel, (W + 31) / 32 words per row, bit x & 31 of word x >> 5, set = excluded; the bits of a row's last word
// beyond W are zero.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "ctx.h"
#include "warp.h"

namespace vio360 {

constexpr int kMaskMaxSize = 65535;                                  // per axis, as erp_tracker_create
constexpr int kMaskMaxRadius = 255;
constexpr int kMaskRowWords = (kMaskMaxSize + 2 * kMaskMaxRadius + 31) / 32 + 2;  // LDS row of mask_erode_h_kernel

inline int mask_words(int W) { return (W + 31) / 32; }

// reduce + pack: the sW x sH source (u8, nonzero = usable; or an exclusion bit-plane) to the dW x dH plane; the
// footprint of destination column d is the source columns [fx[2d], fx[2d+1]], of row d the rows [fy[2d], fy[2d+1]]
struct MaskReduceArgs {
    const uint8_t* src;      // u8 source, or null
    long long stride;
    const uint32_t* sbits;   // bit-plane source (src == null)
    int swords;
    int sW, sH;
    const int32_t* fx;
    const int32_t* fy;
    uint32_t* out;
    int dW, dH, words;
};
hipError_t launch_mask_reduce(const MaskReduceArgs& a, hipStream_t st);

// the usable pixels of a warp's destination (erp_mask_build_warped's rule) as an exclusion plane of wW x wH
struct MaskWarpArgs {
    const WarpEntry* map;
    int wW, wH, sW, sH;
    int wrap_x, replicate_y;
    const uint8_t* mask;  // sW x sH u8 or null (every source pixel usable)
    long long stride;
    uint32_t* out;
    int words;
};
hipError_t launch_mask_warp(const MaskWarpArgs& a, hipStream_t st);

// erosion of the usable region = dilation of the excluded bits by r: columns (wrap: modulo W), then rows
hipError_t launch_mask_erode_h(const uint32_t* in, uint32_t* out, int W, int H, int r, int wrap, hipStream_t st);
hipError_t launch_mask_erode_v(const uint32_t* in, uint32_t* out, int W, int H, int r, hipStream_t st);
// plane -> 0 / 255 bytes (any alignment of dst and its stride)
hipError_t launch_mask_unpack(const uint32_t* bits, int W, int H, uint8_t* dst, long long dstride, hipStream_t st);
// usable[i] = 1 iff (rintf(x_i), rintf(y_i)) is inside the frame and not excluded (x_wrap, the tracker's seam wrap
// mode: a column that rounds to W is column 0)
hipError_t launch_mask_gather(const float* pts, int n, const uint32_t* bits, int W, int H, uint8_t* usable,
                              hipStream_t st, int x_wrap = 0);

// Enqueues on the context stream the build of the dW x dH exclusion plane `out` (device, mask_words(dW) * dH
// words) from a DEVICE source: without a warp an sW x sH u8 mask, with one the warp's source-space mask (or null).
// Arguments are checked before anything is enqueued (erp_mask_check's codes); records the context's mask events.
int mask_enqueue(vio_ctx* ctx, const uint8_t* d_src, int sW, int sH, long long stride, erp_warp* w, int dW, int dH,
                 const erp_mask_params* p, uint32_t* out);
// the argument rules of a build through a warp (no stride of a null mask is looked at)
int mask_warp_check(const erp_warp* w, const uint8_t* src_mask, int stride, int dW, int dH, const erp_mask_params* p);

// a host mask (W x H u8) into the context's device copy, rows padded to 16 bytes; errors carry `who`
int mask_stage(vio_ctx* ctx, const uint8_t* mask, int W, int H, int stride, const char* who, uint8_t** d, int* pitch);

}  // namespace vio360
