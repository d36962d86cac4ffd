// ctx.h — vio_ctx: device + stream + grow-only device scratch (host side of the C-ABI).
#pragma once
#include <hip/hip_runtime.h>

#include <memory>
#include <string>
#include <vector>

#include "vio360.h"

// first event of each module's timing in vio_ctx::ev: start / end of its last launch (equalisation: start /
// histograms done / LUTs done / end)
enum { kEvImu = 0, kEvTri = 2, kEvResize = 4, kEvInit = 6, kEvEq = 8, kEvMask = 12, kEvCount = 14 };

struct vio_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string last_error;
    // grow-only device buffers keyed by slot
    std::vector<void*> bufs;
    std::vector<size_t> caps;
    // grow-only pinned host staging buffers keyed by slot
    std::vector<void*> hbufs;
    std::vector<size_t> hcaps;
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
// scratch slots owned by vio_imu_preintegrate
enum { kSlotImuData = 8, kSlotImuIntervals = 9, kSlotImuOut = 10 };
// scratch slots owned by vio_triangulate
enum { kSlotTriIn = 11, kSlotTriOut = 12 };
// (slots 13, 14 and 21 to 23: the frame resize and ingest, resize.h)
// staging of vio_ba_batch_pack to host memory
enum { kSlotRecords = 15 };
// vio_imu_init_solve inputs, outputs and per-problem scratch
enum { kSlotImuInit = 16 };
// vio_mono_init_solve inputs, outputs and scratch
enum { kSlotMonoInit = 17 };
// vio_lie_eval inputs and outputs
enum { kSlotLie = 18 };
// the one-shot window solves' arena (vio_ba_solve[_batched]: inputs, outputs, workspace)
enum { kSlotBaSolve = 19 };
// the global BA solves' arena (inputs, outputs, the dense reduced system and the rest of the state)
enum { kSlotGbaSolve = 20 };
// erp_equalize*: per-workgroup partial histograms, the tiles' LUTs, and the host entry point's frame
enum { kSlotEqHist = 25, kSlotEqLut = 26, kSlotEqSrc = 27, kSlotEqDst = 28 };
// (slots 29 to 33: the region-mask builds, mask.h)
// pinned host slots: the one-shot solves' input image and every BA download's outputs image
enum { kHostSlotBaIn = 0, kHostSlotBaOut = 1, kHostSlotGba = 2 };

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
