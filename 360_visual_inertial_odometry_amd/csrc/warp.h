// warp.h — what warp.hip (kernel), warp_host.cpp (erp_warp_*) and tracker_host.cpp (erp_*_warped) share.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "ctx.h"
#include "pix_dev.h"

// One destination pixel of the quantised map: qx = 32 ix + a, qy = 32 iy + b (include/vio360.h), one aligned
// 8-byte load per lane.  An invalid pixel is qy = kWarpInvalid (qx = 0).
struct WarpEntry {
    int32_t qx, qy;
};
static_assert(sizeof(WarpEntry) == 8, "one 8-byte load per lane");
enum : int32_t { kWarpInvalid = INT32_MIN };

struct erp_warp {
    vio_ctx* ctx = nullptr;
    int dW = 0, dH = 0, sW = 0, sH = 0;
    int border_x = 0, border_y = 0, border_value = 0;
    int route = VIO_WARP_ROUTE_AUTO;  // erp_warp_set_route
    WarpEntry* d_map = nullptr;    // dW * dH entries, row-major
    hipEvent_t ev[2] = {nullptr, nullptr};
};

namespace vio360 {

struct WarpArgs {
    PixSrc px;
    const uint8_t* src;
    int sW, sH, stride;
    long long frame_bytes_src;
    uint8_t* dst;
    int dW, dH, dstride;
    long long frame_bytes_dst;
    const WarpEntry* map;
    int n_frames;
    int wrap_x, replicate_y, border_value;
};

// warp_kernel<mode, pair> (mode: kPixGray, kPixByte, kPixBytes3 or kPixDword) on `stream`.  pair (sW >= 2): a.px
// holds bit shifts, kPixDword stands for 4-byte pixels at any alignment and kPixBytes3 for 3-byte pixels.
hipError_t launch_warp(const WarpArgs& a, int mode, bool pair, hipStream_t stream);

}  // namespace vio360
