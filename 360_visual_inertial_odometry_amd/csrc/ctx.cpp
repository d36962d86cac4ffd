// ctx.cpp — the context every module works on (ctx.h): creation and teardown, the last-error string and the
// grow-only device / pinned host scratch buffers.
#include "ctx.h"

#include <algorithm>

namespace vio360 {

void set_error(vio_ctx* ctx, const std::string& msg) {
    if (ctx) ctx->last_error = msg;
}
int hip_fail(vio_ctx* ctx, hipError_t e, const char* what) {
    set_error(ctx, std::string("HIP error in ") + what + ": " + hipGetErrorString(e));
    return e == hipErrorOutOfMemory ? VIO_ENOMEM : VIO_EDEVICE;
}
void* ctx_buffer(vio_ctx* ctx, int slot, size_t bytes) {
    // the buffer must live on the context's device whatever device the calling thread has current
    DeviceScope dev_scope(ctx->device);
    if (dev_scope.err != hipSuccess) return nullptr;
    if (ctx->caps[slot] >= bytes && ctx->bufs[slot]) return ctx->bufs[slot];
    if (ctx->bufs[slot]) (void)hipFree(ctx->bufs[slot]);
    ctx->bufs[slot] = nullptr;
    ctx->caps[slot] = 0;
    // 25 % headroom: per-keyframe solves grow and shrink by a few landmarks from call to call
    size_t cap = std::max<size_t>(bytes + bytes / 4, 256);
    if (hipMalloc(&ctx->bufs[slot], cap) != hipSuccess) return nullptr;
    ctx->caps[slot] = cap;
    return ctx->bufs[slot];
}
void* ctx_host_buffer(vio_ctx* ctx, int slot, size_t bytes) {
    if (ctx->hcaps[slot] >= bytes && ctx->hbufs[slot]) return ctx->hbufs[slot];
    DeviceScope dev_scope(ctx->device);
    if (dev_scope.err != hipSuccess) return nullptr;
    if (ctx->hbufs[slot]) {
        (void)hipStreamSynchronize(ctx->stream);  // no copy from / into the old buffer is in flight
        (void)hipHostFree(ctx->hbufs[slot]);
    }
    ctx->hbufs[slot] = nullptr;
    ctx->hcaps[slot] = 0;
    size_t cap = std::max<size_t>(bytes + bytes / 4, 4096);
    if (hipHostMalloc(&ctx->hbufs[slot], cap, hipHostMallocDefault) != hipSuccess) return nullptr;
    ctx->hcaps[slot] = cap;
    return ctx->hbufs[slot];
}

}  // namespace vio360

using namespace vio360;

extern "C" {

static std::string g_create_error;

int vio_abi_version(void) { return VIO360_ABI_VERSION; }

int vio_ctx_create(int device, vio_ctx** out) {
    if (!out) return VIO_EINVAL;
    *out = nullptr;
    if (vio_layout_check() != VIO_OK) {
        g_create_error = "translation units disagree on the BaWin/BaPools/GbaArgs layout (stale object: rebuild)";
        return VIO_EDEVICE;
    }
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        g_create_error = "no HIP device available";
        return VIO_EDEVICE;
    }
    if (device < 0 || device >= n) {
        g_create_error = "device index out of range";
        return VIO_EINVAL;
    }
    DeviceScope dev_scope(device);
    if (dev_scope.err != hipSuccess) {
        g_create_error = "hipSetDevice failed";
        return VIO_EDEVICE;
    }
    vio_ctx* c = new vio_ctx();
    c->device = device;
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
        delete c;
        g_create_error = "hipStreamCreate failed";
        return VIO_EDEVICE;
    }
    *out = c;
    return VIO_OK;
}

void vio_ctx_destroy(vio_ctx* ctx) {
    if (!ctx) return;
    DeviceScope _vio_dev_scope(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    ctx->gba_cache.reset();  // its graph / side stream before the buffers and the stream
    for (void* p : ctx->bufs)
        if (p) (void)hipFree(p);
    for (void* p : ctx->hbufs)
        if (p) (void)hipHostFree(p);
    for (hipEvent_t e : ctx->ev)
        if (e) (void)hipEventDestroy(e);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

const char* vio_ctx_last_error(const vio_ctx* ctx) {
    return ctx ? ctx->last_error.c_str() : g_create_error.c_str();
}

int vio_ctx_set_ba_route(vio_ctx* ctx, int route) {
    if (!ctx || route < VIO_BA_ROUTE_AUTO || route > VIO_BA_ROUTE_CLUSTER) return VIO_EINVAL;
    ctx->ba_route = route;
    return VIO_OK;
}

}  // extern "C"
