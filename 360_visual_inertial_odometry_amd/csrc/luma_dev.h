// luma_dev.h — the two integer luma rules of the colour ingest (erp_luma_u8, erp_ingest*): one function for
// the host entry point and every kernel.  Restatements of OpenCV 4.x (not available here, parity unpinned):
//   VIO_LUMA_CVTCOLOR  cvtColor(BGR2GRAY) for u8:                    (3735 B + 19235 G + 9798 R + 16384) >> 15
//   VIO_LUMA_IMREAD    imread(IMREAD_GRAYSCALE) of a colour PNG:     (1868 B +  9617 G + 4899 R +  8192) >> 14
// The coefficients sum to 2^shift: (v, v, v) -> v, and the result stays in [0, 255].
#pragma once
#include <stdint.h>

#include "vio360.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define VIO_LUMA_HD __host__ __device__
#else
#define VIO_LUMA_HD
#endif

namespace vio360 {

VIO_LUMA_HD inline uint8_t luma_u8(int b, int g, int r, int rule) {
    return rule == VIO_LUMA_IMREAD ? (uint8_t)((1868 * b + 9617 * g + 4899 * r + 8192) >> 14)
                                   : (uint8_t)((3735 * b + 19235 * g + 9798 * r + 16384) >> 15);
}

}  // namespace vio360
