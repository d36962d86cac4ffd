// mask_host.cpp — host side of the region masks (erp_mask_*, include/vio360.h): the argument check, the per-axis
// footprints of the conservative reduce (the taps of erp_resize_area_tab, what the frame's INTER_AREA resize reads)
// and the launches of mask.hip's kernels.  The tracker's entry points are in tracker_host.cpp, the front end's forwards in frontend_host.cpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "frame_io.h"
#include "mask.h"

using namespace vio360;

namespace {

int params_check(const erp_mask_params* p) {
    if (!p || p->erode_radius < 0 || p->erode_radius > kMaskMaxRadius) return VIO_EINVAL;
    if (p->border_x != VIO_MASK_X_CLAMP && p->border_x != VIO_MASK_X_WRAP) return VIO_EINVAL;
    return VIO_OK;
}

int check(int sW, int sH, long long stride, int dW, int dH, long long dst_stride, const erp_mask_params* p) {
    if (params_check(p)) return VIO_EINVAL;
    if (sW <= 0 || sH <= 0 || dW <= 0 || dH <= 0 || sW > kMaskMaxSize || sH > kMaskMaxSize || stride < sW ||
        dst_stride < dW)
        return VIO_EINVAL;
    if (dW > sW || dH > sH) return VIO_ENOSYS;  // a mask is never enlarged
    return VIO_OK;
}

// [lo, hi] per destination index: the source indices with a tap in erp_resize_area_tab(ssize, dsize)
bool footprints(int ssize, int dsize, int32_t* out) {
    int n = 0;
    if (erp_resize_area_tab(ssize, dsize, nullptr, nullptr, nullptr, 0, &n) != VIO_OK || n <= 0) return false;
    std::vector<int32_t> di(n), si(n);
    std::vector<float> al(n);
    if (erp_resize_area_tab(ssize, dsize, di.data(), si.data(), al.data(), n, &n) != VIO_OK) return false;
    for (int d = 0; d < dsize; ++d) {
        out[2 * d] = INT32_MAX;
        out[2 * d + 1] = -1;
    }
    for (int i = 0; i < n; ++i) {
        if (di[i] < 0 || di[i] >= dsize || si[i] < 0 || si[i] >= ssize) return false;
        out[2 * di[i]] = std::min(out[2 * di[i]], si[i]);
        out[2 * di[i] + 1] = std::max(out[2 * di[i] + 1], si[i]);
    }
    for (int d = 0; d < dsize; ++d)
        if (out[2 * d] > out[2 * d + 1]) return false;
    return true;
}

// the footprint tables of (sW -> dW, sH -> dH) on the device, x then y; they stay until another geometry is asked
// for (then: a blocking upload after the stream has drained, the tables may still be in use)
int footprint_tables(vio_ctx* ctx, int sW, int dW, int sH, int dH, const int32_t** fx, const int32_t** fy) {
    const int key[4] = {sW, dW, sH, dH};
    const size_t bytes = sizeof(int32_t) * 2 * ((size_t)dW + dH);
    const bool hit = !std::memcmp(key, ctx->mask_tab_key, sizeof key) && ctx->bufs[kSlotMaskTab];
    if (!hit) {
        std::vector<int32_t> tab(2 * ((size_t)dW + dH));
        if (!footprints(sW, dW, tab.data()) || !footprints(sH, dH, tab.data() + 2 * (size_t)dW)) {
            set_error(ctx, "erp_mask: no footprint table for these sizes");
            return VIO_ENOSYS;
        }
        VIO_HIP(ctx, hipStreamSynchronize(ctx->stream));
        std::memset(ctx->mask_tab_key, 0, sizeof ctx->mask_tab_key);
        void* d = ctx_buffer(ctx, kSlotMaskTab, bytes);
        if (!d) {
            set_error(ctx, "erp_mask: device allocation failed");
            return VIO_ENOMEM;
        }
        VIO_HIP(ctx, hipMemcpy(d, tab.data(), bytes, hipMemcpyHostToDevice));
        std::memcpy(ctx->mask_tab_key, key, sizeof key);
    }
    *fx = static_cast<const int32_t*>(ctx->bufs[kSlotMaskTab]);
    *fy = *fx + 2 * (size_t)dW;
    return VIO_OK;
}

// the plane of mask_enqueue as a 0 / 255 image: to a device image, or through the context's to a host one
int build_image(vio_ctx* ctx, const uint8_t* d_src, int sW, int sH, long long stride, erp_warp* w, int dW, int dH,
                const erp_mask_params* p, uint8_t* dst, int dst_stride, bool dst_on_host) {
    uint32_t* plane = static_cast<uint32_t*>(ctx_buffer(ctx, kSlotMaskDst, sizeof(uint32_t) * mask_words(dW) * dH +
                                                                               (dst_on_host ? (size_t)dW * dH : 0)));
    if (!plane) {
        set_error(ctx, "erp_mask: device allocation failed");
        return VIO_ENOMEM;
    }
    int rc;
    if ((rc = mask_enqueue(ctx, d_src, sW, sH, stride, w, dW, dH, p, plane))) return rc;
    uint8_t* d_img = dst_on_host ? reinterpret_cast<uint8_t*>(plane + (size_t)mask_words(dW) * dH) : dst;
    VIO_HIP(ctx, launch_mask_unpack(plane, dW, dH, d_img, dst_on_host ? dW : dst_stride, ctx->stream));
    VIO_HIP(ctx, hipEventRecord(ctx->ev[kEvMask + 1], ctx->stream));
    return dst_on_host ? fetch_rows(ctx, d_img, dW, dst, dst_stride, dW, dH) : VIO_OK;
}

}  // namespace

namespace vio360 {

int mask_warp_check(const erp_warp* w, const uint8_t* src_mask, int stride, int dW, int dH, const erp_mask_params* p) {
    if (!w || !w->ctx || params_check(p) || dW <= 0 || dH <= 0 || (src_mask && stride < w->sW)) return VIO_EINVAL;
    if (dW > w->dW || dH > w->dH) return VIO_ENOSYS;  // a warp smaller than the plane asked for
    return VIO_OK;
}

int mask_stage(vio_ctx* ctx, const uint8_t* mask, int W, int H, int stride, const char* who, uint8_t** d, int* pitch) {
    return stage_rows(ctx, kSlotMaskSrc, mask, stride, W, H, 16, who, d, pitch);
}

int mask_enqueue(vio_ctx* ctx, const uint8_t* d_src, int sW, int sH, long long stride, erp_warp* w, int dW, int dH,
                 const erp_mask_params* p, uint32_t* out) {
    if (!ctx || !out) return VIO_EINVAL;
    int rc = w ? mask_warp_check(w, d_src, (int)std::min<long long>(stride, INT32_MAX), dW, dH, p)
               : (d_src ? check(sW, sH, stride, dW, dH, dW, p) : VIO_EINVAL);
    if (!rc && w && w->ctx != ctx) rc = VIO_EINVAL;
    if (rc) {
        set_error(ctx, rc == VIO_ENOSYS ? "erp_mask: a mask is reduced, never enlarged"
                                        : "erp_mask: bad sizes, stride, radius or border mode");
        return rc;
    }
    VIO_DEVICE(ctx);
    const int r = p->erode_radius, words = mask_words(dW);
    const int pW = w ? w->dW : sW, pH = w ? w->dH : sH;  // the plane (or image) that is reduced
    const bool reduce = !w || pW != dW || pH != dH;
    const int n_stages = (w ? 1 : 0) + (reduce ? 1 : 0) + (r > 0 ? 2 : 0);
    const size_t plane = sizeof(uint32_t) * std::max((size_t)words * dH, w ? (size_t)mask_words(pW) * pH : 0);
    uint32_t* tmp[2] = {nullptr, nullptr};
    if (n_stages > 1) {
        tmp[0] = static_cast<uint32_t*>(ctx_buffer(ctx, kSlotMaskTmp0, plane));
        tmp[1] = static_cast<uint32_t*>(ctx_buffer(ctx, kSlotMaskTmp1, plane));
        if (!tmp[0] || !tmp[1]) {
            set_error(ctx, "erp_mask: device allocation failed");
            return VIO_ENOMEM;
        }
    }
    const int32_t *fx = nullptr, *fy = nullptr;
    if (reduce && (rc = footprint_tables(ctx, pW, dW, pH, dH, &fx, &fy))) return rc;
    hipEvent_t* ev = ctx->ev + kEvMask;
    if ((rc = events_ready(ctx, ev, 2))) return rc;
    hipStream_t st = ctx->stream;
    VIO_HIP(ctx, hipEventRecord(ev[0], st));
    int stage = 0;
    const uint32_t* cur = nullptr;
    auto next_out = [&]() { return stage + 1 == n_stages ? out : tmp[stage & 1]; };
    if (w) {
        MaskWarpArgs a{};
        a.map = w->d_map;
        a.wW = w->dW; a.wH = w->dH; a.sW = w->sW; a.sH = w->sH;
        a.wrap_x = w->border_x == VIO_WARP_X_WRAP;
        a.replicate_y = w->border_y == VIO_WARP_Y_REPLICATE;
        a.mask = d_src; a.stride = stride;
        a.out = next_out(); a.words = mask_words(w->dW);
        VIO_HIP(ctx, launch_mask_warp(a, st));
        cur = a.out;
        ++stage;
    }
    if (reduce) {
        MaskReduceArgs a{};
        if (w) { a.sbits = cur; a.swords = mask_words(pW); }
        else { a.src = d_src; a.stride = stride; }
        a.sW = pW; a.sH = pH;
        a.fx = fx; a.fy = fy;
        a.out = next_out(); a.dW = dW; a.dH = dH; a.words = words;
        VIO_HIP(ctx, launch_mask_reduce(a, st));
        cur = a.out;
        ++stage;
    }
    if (r > 0) {
        uint32_t* o = next_out();
        VIO_HIP(ctx, launch_mask_erode_h(cur, o, dW, dH, r, p->border_x == VIO_MASK_X_WRAP, st));
        cur = o;
        ++stage;
        o = next_out();
        VIO_HIP(ctx, launch_mask_erode_v(cur, o, dW, dH, r, st));
        ++stage;
    }
    VIO_HIP(ctx, hipEventRecord(ev[1], st));
    return VIO_OK;
}

}  // namespace vio360

extern "C" {

int erp_mask_check(int sW, int sH, int stride, int dW, int dH, int dst_stride, const erp_mask_params* p) {
    return check(sW, sH, stride, dW, dH, dst_stride, p);
}

int erp_mask_build_device(vio_ctx* ctx, const uint8_t* mask, int sW, int sH, int stride, int dW, int dH,
                          const erp_mask_params* p, uint8_t* dst, int dst_stride) {
    if (!ctx || !mask || !dst) return VIO_EINVAL;
    const int rc = check(sW, sH, stride, dW, dH, dst_stride, p);
    if (rc) {
        set_error(ctx, "erp_mask_build: bad sizes, stride, radius or border mode, or a mask to enlarge");
        return rc;
    }
    VIO_DEVICE(ctx);
    return build_image(ctx, mask, sW, sH, stride, nullptr, dW, dH, p, dst, dst_stride, false);
}

int erp_mask_build(vio_ctx* ctx, const uint8_t* mask, int sW, int sH, int stride, int dW, int dH,
                   const erp_mask_params* p, uint8_t* dst, int dst_stride) {
    if (!ctx || !mask || !dst) return VIO_EINVAL;
    int rc = check(sW, sH, stride, dW, dH, dst_stride, p);
    if (rc) {
        set_error(ctx, "erp_mask_build: bad sizes, stride, radius or border mode, or a mask to enlarge");
        return rc;
    }
    VIO_DEVICE(ctx);
    uint8_t* d_src = nullptr;
    int sp = 0;
    if ((rc = mask_stage(ctx, mask, sW, sH, stride, "erp_mask", &d_src, &sp))) return rc;
    return build_image(ctx, d_src, sW, sH, sp, nullptr, dW, dH, p, dst, dst_stride, true);
}

int erp_mask_build_warped(erp_warp* w, const uint8_t* src_mask, int stride, int dW, int dH, const erp_mask_params* p,
                          uint8_t* dst, int dst_stride) {
    if (!w || !w->ctx || !dst) return VIO_EINVAL;
    vio_ctx* ctx = w->ctx;
    int rc = mask_warp_check(w, src_mask, stride, dW, dH, p);
    if (!rc && dst_stride < dW) rc = VIO_EINVAL;
    if (rc) {
        set_error(ctx, "erp_mask_build_warped: bad sizes, stride, radius or border mode, or a warp smaller than the mask");
        return rc;
    }
    VIO_DEVICE(ctx);
    uint8_t* d_src = nullptr;
    int sp = 0;
    if (src_mask && (rc = mask_stage(ctx, src_mask, w->sW, w->sH, stride, "erp_mask", &d_src, &sp))) return rc;
    return build_image(ctx, d_src, w->sW, w->sH, sp, w, dW, dH, p, dst, dst_stride, true);
}

int erp_mask_kernel_ms(vio_ctx* ctx, double* ms) {
    return ctx ? events_ms(ctx, ctx->ev[kEvMask], ctx->ev[kEvMask + 1], ms) : VIO_EINVAL;
}

}  // extern "C"
