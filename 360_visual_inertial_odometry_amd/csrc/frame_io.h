// frame_io.h — the host plumbing every frame-preprocessing stage shares: a host image into a pitched device slot,
// a pitched device image back to the host, and the timing events of a module's last launch.  Nothing here decides
// a byte of a result.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "ctx.h"

namespace vio360 {

// `rows` rows of row_bytes in slot `slot`, the pitch padded to a multiple of pitch_align (contents undefined).
// "<who>: bad sizes" / VIO_EINVAL for a pitch beyond INT32_MAX, "<who>: device allocation failed" / VIO_ENOMEM.
int scratch_rows(vio_ctx* ctx, int slot, long long row_bytes, int rows, int pitch_align, const char* who, uint8_t** d,
                 int* pitch);
// rows of a host image to the device at `pitch`, asynchronously on the context stream
int upload_rows(vio_ctx* ctx, uint8_t* d_dst, long long pitch, const uint8_t* host_src, long long src_stride,
                long long row_bytes, int rows);
// scratch_rows, then upload_rows into it
int stage_rows(vio_ctx* ctx, int slot, const uint8_t* host_src, long long src_stride, long long row_bytes, int rows,
               int pitch_align, const char* who, uint8_t** d, int* pitch);
// rows of a device image to the host; returns once they have arrived (the context stream is drained)
int fetch_rows(vio_ctx* ctx, const uint8_t* d_src, long long pitch, uint8_t* host_dst, long long dst_stride,
               long long row_bytes, int rows);

// creates those of ev[0 .. n) that do not exist yet, on the context's device
int events_ready(vio_ctx* ctx, hipEvent_t* ev, int n);
// the time from `first` to `last` once `last` has completed; VIO_EINVAL while `last` was never created
int events_ms(vio_ctx* ctx, hipEvent_t first, hipEvent_t last, double* ms);

}  // namespace vio360
