// pix_dev.h — where a kernel takes the u8 value of a source pixel from (erp_ingest*, erp_warp*): the grey byte
// itself, or the luma of a packed pixel (luma_dev.h), computed in registers.  Everything after that value is the
// same code for every format, so a fused result equals the same operation on luma(frame) bit for bit.
//   kPixGray    s[x]                                            (the grey kernels: bpp and offsets unused)
//   kPixByte    s[bpp x + o0]                                   YUYV / UYVY
//   kPixBytes3  luma(s[bpp x + o0], .. + o1, .. + o2)           BGR / RGB, and BGRA / RGBA at any alignment
//   kPixDword   one aligned dword at s + 4 x, B G R at bit shifts o0 o1 o2: BGRA / RGBA with src and stride
//               multiples of 4 (checked on the host)
//   kPixRun3    BGR / RGB: a lane's run of N consecutive pixels of a row (resize.hip load_run3)
// No variant reads a byte outside [0, W bpp) of a row.
#pragma once
#include <stdint.h>

#include "luma_dev.h"

namespace vio360 {

enum { kPixGray = 0, kPixByte = 1, kPixBytes3 = 2, kPixDword = 3, kPixRun3 = 4 };

struct PixSrc {
    int bpp, o0, o1, o2;  // o*: byte offsets of B, G, R in a pixel (kPixByte: o0 of the luma byte); kPixDword, kPixRun3: bit shifts
    int rule;             // VIO_LUMA_*
};

inline bool pix_is_colour(int format) { return format >= VIO_PIX_BGR8 && format <= VIO_PIX_RGBA8; }
inline bool pix_is_422(int format) { return format == VIO_PIX_YUYV || format == VIO_PIX_UYVY; }

// the byte-variant pixel source of a format (kPixByte / kPixBytes3; GRAY8 is kPixByte at offset 0)
inline PixSrc pix_source(int format, int luma) {
    PixSrc p = {erp_pixel_bytes(format), 0, 1, 2, luma};
    if (format == VIO_PIX_RGB8 || format == VIO_PIX_RGBA8) {
        p.o0 = 2;
        p.o2 = 0;
    } else if (format == VIO_PIX_UYVY) {
        p.o0 = 1;
    }
    return p;
}

// the rules of every entry point that takes a pixel format: a known format, for colour a known luma rule, an even
// width W for 4:2:2; *why names the broken one
inline int pix_check(int format, int luma, int W, const char** why) {
    *why = erp_pixel_bytes(format) < 0 ? "unknown pixel format"
           : pix_is_colour(format) && luma != VIO_LUMA_CVTCOLOR && luma != VIO_LUMA_IMREAD ? "unknown luma rule"
           : pix_is_422(format) && W % 2 ? "a 4:2:2 frame has an even width"
                                         : nullptr;
    return *why ? VIO_EINVAL : VIO_OK;
}

// can a kernel take each 4-byte pixel of the rows at src as one aligned dword (kPixDword)?
inline bool pix_dword_ok(const uint8_t* src, int stride) {
    return (reinterpret_cast<uintptr_t>(src) & 3) == 0 && stride % 4 == 0;
}

// byte offsets -> bit shifts: what kPixDword and kPixRun3 (and the warp's pair route) read
inline void pix_to_bit_shifts(PixSrc* p) {
    p->o0 *= 8;
    p->o1 *= 8;
    p->o2 *= 8;
}

#if defined(__HIPCC__)

template <int MODE>
__device__ __forceinline__ int pix_step(const PixSrc& p) {
    return MODE == kPixGray ? 1 : (MODE == kPixDword ? 4 : (MODE == kPixRun3 ? 3 : p.bpp));
}

// the luma of a pixel held in a word, B G R at bit shifts o0 o1 o2
__device__ __forceinline__ uint8_t word_luma(uint32_t w, const PixSrc& p) {
    return luma_u8((int)((w >> p.o0) & 0xff), (int)((w >> p.o1) & 0xff), (int)((w >> p.o2) & 0xff), p.rule);
}

// the u8 value of the pixel whose first byte is at s
template <int MODE>
__device__ __forceinline__ uint8_t pix_value(const uint8_t* s, const PixSrc& p) {
    if constexpr (MODE == kPixGray) {
        return s[0];
    } else if constexpr (MODE == kPixByte) {
        return s[p.o0];
    } else if constexpr (MODE == kPixBytes3) {
        return luma_u8(s[p.o0], s[p.o1], s[p.o2], p.rule);
    } else {
        static_assert(MODE == kPixDword, "kPixRun3 loads runs, not pixels");
        return word_luma(*reinterpret_cast<const uint32_t*>(s), p);
    }
}

#endif  // __HIPCC__

}  // namespace vio360
