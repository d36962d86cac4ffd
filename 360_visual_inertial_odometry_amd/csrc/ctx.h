// ctx.h — vio_ctx: device + stream + grow-only device scratch (host side of the C-ABI).
#pragma once
#include <hip/hip_runtime.h>

#include <memory>
#include <string>

#include "vio360.h"

// first event of each module's timing in vio_ctx::ev: start / end of its last launch (equalisation: start /
// histograms done / LUTs done / end)
enum { kEvImu = 0, kEvTri = 2, kEvResize = 4, kEvInit = 6, kEvEq = 8, kEvMask = 12, kEvPnp = 14, kEvCount = 16 };

// Device scratch slots of vio_ctx::bufs (ctx_buffer), one owner each.
enum {
    // vio_imu_preintegrate
    kSlotImuData, kSlotImuIntervals, kSlotImuOut,
    // vio_triangulate
    kSlotTriIn, kSlotTriOut,
    // the frame resize and ingest (resize_host.cpp): the host entry points' source and result (every
    // preprocessing stage stages its source in kSlotResizeSrc), the general path's per-output-column /
    // per-output-row tap tables, and the two-pass ingest route's grey camera-resolution plane between the
    // convert and the resize
    kSlotResizeSrc, kSlotResizeDst, kSlotResizeTabX, kSlotResizeTabY, kSlotIngestPlane,
    // erp_tracker_upload_warped: the warped frame of the supersampled route, before the resize
    kSlotWarpDst,
    // staging of vio_ba_batch_pack to host memory
    kSlotRecords,
    // vio_imu_init_solve inputs, outputs and per-problem scratch
    kSlotImuInit,
    // vio_mono_init_solve inputs, outputs and scratch
    kSlotMonoInit,
    // vio_lie_eval / vio_imu_factor_eval inputs and outputs
    kSlotLie,
    // the one-shot window solves' arena (vio_ba_solve[_batched]: inputs, outputs, workspace)
    kSlotBaSolve,
    // the global BA solves' arena (inputs, outputs, the dense reduced system and the rest of the state)
    kSlotGbaSolve,
    // erp_equalize*: per-workgroup partial histograms, the tiles' LUTs, and the host entry point's frame
    kSlotEqHist, kSlotEqLut, kSlotEqSrc, kSlotEqDst,
    // the region-mask builds (mask_host.cpp): the uploaded host mask, the two intermediate planes, the
    // footprint tables, the 0 / 255 image of the host entry points
    kSlotMaskSrc, kSlotMaskTmp0, kSlotMaskTmp1, kSlotMaskTab, kSlotMaskDst,
    // vio_pnp_ransac's arena: inputs, the rows' poses and counts, the result record and the mask
    kSlotPnpRansac,
    kSlotCount
};
// Pinned host slots of vio_ctx::hbufs (ctx_host_buffer): the one-shot window solves' input image, every BA
// download's outputs image, the global BA solves' staging
enum { kHostSlotBaIn, kHostSlotBaOut, kHostSlotGba, kHostSlotCount };

struct vio_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string last_error;
    // grow-only device buffers keyed by slot
    void* bufs[kSlotCount] = {};
    size_t caps[kSlotCount] = {};
    // grow-only pinned host staging buffers keyed by slot
    void* hbufs[kHostSlotCount] = {};
    size_t hcaps[kHostSlotCount] = {};
    // kernel timing of every module: the events of kEv* (created on first use, frame_io.h events_ready)
    hipEvent_t ev[kEvCount] = {};
    float imu_ms = -1.f;  // < 0: no IMU preintegration has run on this context
    // (W, dW, H, dH) of the general INTER_AREA tap tables now in kSlotResizeTabX / kSlotResizeTabY
    int rsz_tab_key[4] = {0, 0, 0, 0};
    int rsz_max_x_taps = 0;  // the largest tap count of a column of those tables
    // colour ingest execution route (erp_ingest_set_route)
    int ingest_route = VIO_INGEST_ROUTE_AUTO;
    // window-BA execution route (vio_ctx_set_ba_route)
    int ba_route = VIO_BA_ROUTE_AUTO;
    // global-BA state kept between solves (ba_global_host.cpp GbaCache: look-ahead stream, captured graph)
    std::shared_ptr<void> gba_cache;
    // equalisation: the two inner events of kEvEq are recorded only under erp_equalize_set_stage_timing
    bool eq_stage_timing = false;
    bool eq_staged = false;  // the last launch recorded the inner events
    // region masks: the (sW, dW, sH, dH) of the footprint tables now in kSlotMaskTab
    int mask_tab_key[4] = {0, 0, 0, 0};
};

namespace vio360 {

void set_error(vio_ctx* ctx, const std::string& msg);
int hip_fail(vio_ctx* ctx, hipError_t e, const char* what);
// device buffer of at least `bytes` for slot `slot` (contents undefined); nullptr on failure
void* ctx_buffer(vio_ctx* ctx, int slot, size_t bytes);
// pinned host buffer of at least `bytes` for slot `slot` (contents undefined); nullptr on failure
void* ctx_host_buffer(vio_ctx* ctx, int slot, size_t bytes);
// Selects a device for the rest of the enclosing scope and restores the calling thread's current
// device on exit, so a C-ABI call never leaves the caller's thread on the context's device (a process
// that also drives other GPUs, e.g. through torch, keeps its own current device).
struct DeviceScope {
    int prev = -1;
    hipError_t err = hipSuccess;
    explicit DeviceScope(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) err = hipSetDevice(dev);
        else prev = -1;  // nothing to restore
    }
    ~DeviceScope() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
    DeviceScope(const DeviceScope&) = delete;
    DeviceScope& operator=(const DeviceScope&) = delete;
};
#define VIO_DEVICE(ctx)                     \
    DeviceScope _vio_dev_scope((ctx)->device); \
    VIO_HIP(ctx, _vio_dev_scope.err)

#define VIO_HIP(ctx, expr)                                  \
    do {                                                    \
        hipError_t _e = (expr);                             \
        if (_e != hipSuccess) return hip_fail(ctx, _e, #expr); \
    } while (0)

}  // namespace vio360
