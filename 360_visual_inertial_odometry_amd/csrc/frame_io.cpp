// frame_io.cpp — see frame_io.h.
#include "frame_io.h"

#include <string>

namespace vio360 {

int scratch_rows(vio_ctx* ctx, int slot, long long row_bytes, int rows, int pitch_align, const char* who, uint8_t** d,
                 int* pitch) {
    const long long p = (row_bytes + pitch_align - 1) / pitch_align * pitch_align;
    if (row_bytes <= 0 || rows <= 0 || p > INT32_MAX) {
        set_error(ctx, std::string(who) + ": bad sizes");
        return VIO_EINVAL;
    }
    *d = static_cast<uint8_t*>(ctx_buffer(ctx, slot, (size_t)p * rows));
    if (!*d) {
        set_error(ctx, std::string(who) + ": device allocation failed");
        return VIO_ENOMEM;
    }
    *pitch = (int)p;
    return VIO_OK;
}

int upload_rows(vio_ctx* ctx, uint8_t* d_dst, long long pitch, const uint8_t* host_src, long long src_stride,
                long long row_bytes, int rows) {
    VIO_DEVICE(ctx);
    VIO_HIP(ctx, hipMemcpy2DAsync(d_dst, pitch, host_src, src_stride, row_bytes, rows, hipMemcpyHostToDevice, ctx->stream));
    return VIO_OK;
}

int stage_rows(vio_ctx* ctx, int slot, const uint8_t* host_src, long long src_stride, long long row_bytes, int rows,
               int pitch_align, const char* who, uint8_t** d, int* pitch) {
    const int rc = scratch_rows(ctx, slot, row_bytes, rows, pitch_align, who, d, pitch);
    return rc ? rc : upload_rows(ctx, *d, *pitch, host_src, src_stride, row_bytes, rows);
}

int fetch_rows(vio_ctx* ctx, const uint8_t* d_src, long long pitch, uint8_t* host_dst, long long dst_stride,
               long long row_bytes, int rows) {
    VIO_DEVICE(ctx);
    VIO_HIP(ctx, hipMemcpy2DAsync(host_dst, dst_stride, d_src, pitch, row_bytes, rows, hipMemcpyDeviceToHost, ctx->stream));
    VIO_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return VIO_OK;
}

int events_ready(vio_ctx* ctx, hipEvent_t* ev, int n) {
    VIO_DEVICE(ctx);
    for (int i = 0; i < n; ++i)
        if (!ev[i]) VIO_HIP(ctx, hipEventCreate(&ev[i]));
    return VIO_OK;
}

int events_ms(vio_ctx* ctx, hipEvent_t first, hipEvent_t last, double* ms) {
    if (!ctx || !ms || !last) return VIO_EINVAL;
    float f = 0.f;
    VIO_DEVICE(ctx);
    VIO_HIP(ctx, hipEventSynchronize(last));
    VIO_HIP(ctx, hipEventElapsedTime(&f, first, last));
    *ms = f;
    return VIO_OK;
}

}  // namespace vio360
