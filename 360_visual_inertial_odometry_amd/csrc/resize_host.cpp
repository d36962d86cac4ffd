// resize_host.cpp — host side of the frame resize and ingest (erp_resize_area*, erp_ingest*, include/vio360.h): the
// argument checks, the general path's tap tables, the choice of route and kernel variant, and the launches of
// resize.hip's kernels.  The tap tables are IEEE double in OpenCV's expression order and compared bitwise with
// tests/resize_general_oracle.py: the file is built without FMA contraction.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "frame_io.h"
#include "luma_dev.h"
#include "resize.h"

using namespace vio360;

namespace {

struct AreaTap {
    int32_t di, si;
    float alpha;
};

// computeResizeAreaTab (OpenCV 4.x modules/imgproc/src/resize.cpp) for one axis, scale = ssize / dsize >= 1:
// IEEE double in this expression order (the file is built without FMA contraction)
void area_tab(int ssize, int dsize, std::vector<AreaTap>& tab) {
    const double scale = (double)ssize / dsize;
    tab.clear();
    for (int d = 0; d < dsize; ++d) {
        const double fsx1 = d * scale;
        const double fsx2 = fsx1 + scale;
        const double cell = std::min(scale, ssize - fsx1);
        int sx1 = (int)std::ceil(fsx1), sx2 = (int)std::floor(fsx2);
        sx2 = std::min(sx2, ssize - 1);
        sx1 = std::min(sx1, sx2);
        if (sx1 - fsx1 > 1e-3) tab.push_back({d, sx1 - 1, (float)((sx1 - fsx1) / cell)});
        for (int sx = sx1; sx < sx2; ++sx) tab.push_back({d, sx, (float)(1.0 / cell)});
        if (fsx2 - sx2 > 1e-3) tab.push_back({d, sx2, (float)(std::min(std::min(fsx2 - sx2, 1.0), cell) / cell)});
    }
}

// the tap list as one AreaTaps record per output index; false if the list is not of that shape (every output
// index present, contiguous ascending source indices within [0, ssize), equal inner weights)
bool area_tab_compact(const std::vector<AreaTap>& tab, int ssize, int dsize, std::vector<AreaTaps>& out) {
    out.assign(dsize, AreaTaps{0, 0, 0.f, 0.f, 0.f});
    size_t i = 0;
    for (int d = 0; d < dsize; ++d) {
        size_t e = i;
        while (e < tab.size() && tab[e].di == d) ++e;
        const int n = (int)(e - i);
        if (n < 1) return false;
        AreaTaps& r = out[d];
        r.first = tab[i].si;
        r.count = n;
        r.w_first = tab[i].alpha;
        r.w_last = tab[e - 1].alpha;
        r.w_mid = n > 2 ? tab[i + 1].alpha : 0.f;
        if (r.first < 0 || (long long)r.first + n > ssize) return false;
        for (int k = 0; k < n; ++k) {
            const float w = k == 0 ? r.w_first : (k == n - 1 ? r.w_last : r.w_mid);
            if (tab[i + k].si != r.first + k || std::memcmp(&w, &tab[i + k].alpha, sizeof(float))) return false;
        }
        i = e;
    }
    return i == tab.size();
}

// device tap tables of (W -> dW, H -> dH) in the context's two table slots, rebuilt when the sizes change
int general_tables(vio_ctx* ctx, int W, int dW, int H, int dH, const AreaTaps** d_tx, const AreaTaps** d_ty,
                   int* max_x_taps) {
    const int key[4] = {W, dW, H, dH};
    const bool hit = !std::memcmp(key, ctx->rsz_tab_key, sizeof(key)) && ctx->bufs[kSlotResizeTabX] &&
                     ctx->bufs[kSlotResizeTabY];
    if (!hit) {
        std::memset(ctx->rsz_tab_key, 0, sizeof(key));
        std::vector<AreaTap> tab;
        std::vector<AreaTaps> hx, hy;
        area_tab(W, dW, tab);
        const bool okx = area_tab_compact(tab, W, dW, hx);
        area_tab(H, dH, tab);
        if (!okx || !area_tab_compact(tab, H, dH, hy)) {
            set_error(ctx, "erp_resize_area_any: tap table outside the source frame");
            return VIO_EINVAL;
        }
        void* bx = ctx_buffer(ctx, kSlotResizeTabX, sizeof(AreaTaps) * hx.size());
        void* by = ctx_buffer(ctx, kSlotResizeTabY, sizeof(AreaTaps) * hy.size());
        if (!bx || !by) {
            set_error(ctx, "erp_resize_area_any: device allocation failed");
            return VIO_ENOMEM;
        }
        // on the context stream, so after any kernel that still reads the previous tables; blocking, since the
        // host tables die with this scope
        VIO_HIP(ctx, hipMemcpyAsync(bx, hx.data(), sizeof(AreaTaps) * hx.size(), hipMemcpyHostToDevice, ctx->stream));
        VIO_HIP(ctx, hipMemcpyAsync(by, hy.data(), sizeof(AreaTaps) * hy.size(), hipMemcpyHostToDevice, ctx->stream));
        VIO_HIP(ctx, hipStreamSynchronize(ctx->stream));
        std::memcpy(ctx->rsz_tab_key, key, sizeof(key));
        ctx->rsz_max_x_taps = 0;
        for (const AreaTaps& r : hx) ctx->rsz_max_x_taps = std::max(ctx->rsz_max_x_taps, (int)r.count);
    }
    *max_x_taps = ctx->rsz_max_x_taps;
    *d_tx = static_cast<const AreaTaps*>(ctx->bufs[kSlotResizeTabX]);
    *d_ty = static_cast<const AreaTaps*>(ctx->bufs[kSlotResizeTabY]);
    return VIO_OK;
}

enum { kPathInteger = 0, kPathGeneral = 1 };

const PixSrc kGrayPix = {1, 0, 0, 0, 0};

// format, luma rule and sizes of a call: kPathInteger, kPathGeneral, or < 0 with "<who>: ..." set on ctx.
// integer_only (erp_resize_area*): every other size pair is VIO_ENOSYS, not the general path.
int area_check(vio_ctx* ctx, const char* who, bool integer_only, int format, int luma, int W, int H, int stride, int dW,
               int dH, int dstride, int n_frames) {
    const auto fail = [&](int rc, const char* why) {
        set_error(ctx, std::string(who) + ": " + why);
        return rc;
    };
    const char* why;
    if (pix_check(format, luma, W, &why)) return fail(VIO_EINVAL, why);
    if (W <= 0 || H <= 0 || dW <= 0 || dH <= 0 || (long long)stride < (long long)W * erp_pixel_bytes(format) ||
        dstride < dW || n_frames < 0)
        return fail(VIO_EINVAL, "bad sizes");
    const bool general = W % dW || H % dH;
    if (integer_only && general) return fail(VIO_ENOSYS, "only integer downscale factors are supported");
    if (dW > W || dH > H) return fail(VIO_ENOSYS, "enlarging is not supported");
    if (general) return kPathGeneral;
    if ((long long)(W / dW) * (H / dH) > (1 << 23)) return fail(VIO_ENOSYS, "integer factors too large");  // int block sums
    return kPathInteger;
}

// the one place each argument struct is filled
ResizeArgs integer_args(const PixSrc& px, const uint8_t* src, int W, int H, int stride, uint8_t* dst, int dW, int dH,
                        int dst_stride) {
    ResizeArgs a;
    a.px = px;
    a.src = src;
    a.W = W;
    a.H = H;
    a.stride = stride;
    a.frame_bytes_src = (long long)stride * H;
    a.dst = dst;
    a.dW = dW;
    a.dH = dH;
    a.dstride = dst_stride;
    a.frame_bytes_dst = (long long)dst_stride * dH;
    a.fx = W / dW;
    a.fy = H / dH;
    a.scale = 1.f / (float)(a.fx * a.fy);
    return a;
}

ResizeAnyArgs general_args(const PixSrc& px, const uint8_t* src, int W, int H, int stride, uint8_t* dst, int dW, int dH,
                           int dst_stride, const AreaTaps* tx, const AreaTaps* ty) {
    ResizeAnyArgs a;
    a.px = px;
    a.src = src;
    a.W = W;
    a.stride = stride;
    a.frame_bytes_src = (long long)stride * H;
    a.dst = dst;
    a.dW = dW;
    a.dstride = dst_stride;
    a.frame_bytes_dst = (long long)dst_stride * dH;
    a.tx = tx;
    a.ty = ty;
    return a;
}

// VIO_INGEST_ROUTE_AUTO: does the one-pass kernel of this pixel source and path run, or convert + grey resize?
// What measured faster (tools/ingest_time.py) at 3840x1920, 4096x2048 and 5376x2688 -> 960x480: the
// one-pass kernel by 2.1x to 4.4x, except for 4-byte pixels that cannot take dword loads (src or stride no
// multiple of 4), where three byte loads per tap lose to two-pass by 5 % at factor 4 and at 4096 (columns of up to
// 6 taps in the 8-tap variant) and win by 11 % at 5376 (up to 7 taps).
bool ingest_fused_by_default(int mode, int bpp, int path, int max_x_taps) {
    if (mode == kPixBytes3 && bpp == 4) return path == kPathGeneral && max_x_taps > 6;
    return true;
}

// The wider-load variant of a byte pixel source, where one applies (else `mode` itself); *px gets its bit shifts.
// fx: the integer x factor (0: the general path, max_x_taps its widest column; 1: the convert pass).
//   4-byte pixels: one aligned dword per pixel when src and stride are multiples of 4
//   3-byte pixels: runs of fx = 2 or 4 pixels, or of the general <4> / <8> kernels' 4 / 8 taps (W no smaller)
int ingest_wide_mode(int mode, const uint8_t* src, int stride, int W, int fx, int max_x_taps, PixSrc* px) {
    if (mode != kPixBytes3) return mode;
    int wide = mode;
    if (px->bpp == 4 && pix_dword_ok(src, stride)) wide = kPixDword;
    if (px->bpp == 3 && (fx == 2 || fx == 4)) wide = kPixRun3;
    if (px->bpp == 3 && fx == 0 && max_x_taps <= 8 && W >= (max_x_taps <= 4 ? 4 : 8)) wide = kPixRun3;
    if (wide != mode) pix_to_bit_shifts(px);
    return wide;
}

// One INTER_AREA downscale of n_frames DEVICE frames on the context stream, after area_check (`path` is its
// answer): the tap tables, the route (one fused kernel, or convert to a grey plane and resize that), the kernel
// variants, the launches and the resize events around them.  px / mode: kGrayPix / kPixGray for grey frames, else
// the byte-variant source of the format (pix_source).
int enqueue_area(vio_ctx* ctx, const PixSrc& px, int mode, const uint8_t* src, int W, int H, int stride, int n_frames,
                 uint8_t* dst, int dW, int dH, int dst_stride, int path) {
    if (n_frames == 0) return VIO_OK;
    VIO_DEVICE(ctx);
    int rc, max_x_taps = 0;
    const AreaTaps *tx = nullptr, *ty = nullptr;
    if (path == kPathGeneral && (rc = general_tables(ctx, W, dW, H, dH, &tx, &ty, &max_x_taps))) return rc;
    const bool grey = mode == kPixGray;
    const bool convert_only = !grey && dW == W && dH == H;
    const bool bytes_only = ctx->ingest_route == VIO_INGEST_ROUTE_FUSED_BYTES;
    // the pixel source of the convert pass (one pixel per lane) and of the fused resize kernel
    PixSrc cpx = px, fpx = px;
    const int cmode = bytes_only ? mode : ingest_wide_mode(mode, src, stride, W, 1, 0, &cpx);
    const int fmode = bytes_only || convert_only
                          ? mode
                          : ingest_wide_mode(mode, src, stride, W, path == kPathInteger ? W / dW : 0, max_x_taps, &fpx);
    const bool fused = grey || (ctx->ingest_route == VIO_INGEST_ROUTE_AUTO
                                    ? ingest_fused_by_default(fmode, px.bpp, path, max_x_taps)
                                    : ctx->ingest_route != VIO_INGEST_ROUTE_TWO_PASS);
    // two-pass route: the grey plane of every frame, rows padded to 16 bytes (the factor-4 grey kernel's layout)
    const int pp = (W + 15) & ~15;
    uint8_t* plane = nullptr;
    if (!convert_only && !fused) {
        plane = static_cast<uint8_t*>(ctx_buffer(ctx, kSlotIngestPlane, (size_t)pp * H * n_frames));
        if (!plane) {
            set_error(ctx, "erp_ingest: device allocation failed");
            return VIO_ENOMEM;
        }
    }
    // every argument before the first event: on an idle stream the events also time the host between the launches
    const bool convert = convert_only || !fused;
    const ResizeArgs c = integer_args(cpx, src, W, H, stride, convert_only ? dst : plane, W, H,
                                      convert_only ? dst_stride : pp);
    // what the resize kernel reads: the frames as they came, or the convert pass's grey plane
    const uint8_t* rsrc = convert ? plane : src;
    const int rstride = convert ? pp : stride, rmode = convert ? kPixGray : fmode;
    const PixSrc& rpx = convert ? kGrayPix : fpx;
    ResizeArgs ia{};
    ResizeAnyArgs ga{};
    if (path == kPathInteger) ia = integer_args(rpx, rsrc, W, H, rstride, dst, dW, dH, dst_stride);
    else ga = general_args(rpx, rsrc, W, H, rstride, dst, dW, dH, dst_stride, tx, ty);
    hipEvent_t* ev = ctx->ev + kEvResize;
    if ((rc = events_ready(ctx, ev, 2))) return rc;
    VIO_HIP(ctx, hipEventRecord(ev[0], ctx->stream));
    if (convert) VIO_HIP(ctx, launch_ingest_convert(c, cmode, n_frames, ctx->stream));
    if (!convert_only)
        VIO_HIP(ctx, path == kPathInteger ? launch_area_integer(ia, rmode, n_frames, ctx->stream)
                                          : launch_area_general(ga, rmode, dH, n_frames, max_x_taps, ctx->stream));
    VIO_HIP(ctx, hipEventRecord(ev[1], ctx->stream));
    return VIO_OK;
}

// One entry point: the checks, then the enqueue on DEVICE frames, or for a host frame (on_host; n_frames 1) the
// round trip through the context's resize slots.
int area_call(vio_ctx* ctx, const char* who, bool integer_only, bool on_host, const uint8_t* src, int format, int luma,
              int W, int H, int stride, int n_frames, uint8_t* dst, int dW, int dH, int dst_stride) {
    if (!ctx || !src || !dst) return VIO_EINVAL;
    const int path = area_check(ctx, who, integer_only, format, luma, W, H, stride, dW, dH, dst_stride, n_frames);
    if (path < 0) return path;
    const bool grey = format == VIO_PIX_GRAY8;
    const PixSrc px = grey ? kGrayPix : pix_source(format, luma);
    const int mode = grey ? kPixGray : (pix_is_colour(format) ? kPixBytes3 : kPixByte);
    if (!on_host) return enqueue_area(ctx, px, mode, src, W, H, stride, n_frames, dst, dW, dH, dst_stride, path);
    // device copies: source rows padded to 16 bytes, result rows to 4 (the factor-4 kernel's layout)
    uint8_t *d_src = nullptr, *d_dst = nullptr;
    int sp = 0, dp = 0, rc;
    if ((rc = stage_rows(ctx, kSlotResizeSrc, src, stride, (long long)W * px.bpp, H, 16, who, &d_src, &sp))) return rc;
    if ((rc = scratch_rows(ctx, kSlotResizeDst, dW, dH, 4, who, &d_dst, &dp))) return rc;
    if ((rc = enqueue_area(ctx, px, mode, d_src, W, H, sp, 1, d_dst, dW, dH, dp, path))) return rc;
    return fetch_rows(ctx, d_dst, dp, dst, dst_stride, dW, dH);
}

}  // namespace

extern "C" {

int erp_resize_area_device(vio_ctx* ctx, const uint8_t* src, int W, int H, int stride, int n_frames, uint8_t* dst,
                           int dW, int dH, int dst_stride) {
    return area_call(ctx, "erp_resize_area", true, false, src, VIO_PIX_GRAY8, 0, W, H, stride, n_frames, dst, dW, dH,
                     dst_stride);
}

int erp_resize_area(vio_ctx* ctx, const uint8_t* src, int W, int H, int stride, uint8_t* dst, int dW, int dH,
                    int dst_stride) {
    return area_call(ctx, "erp_resize_area", true, true, src, VIO_PIX_GRAY8, 0, W, H, stride, 1, dst, dW, dH, dst_stride);
}

int erp_resize_area_any_device(vio_ctx* ctx, const uint8_t* src, int W, int H, int stride, int n_frames, uint8_t* dst,
                               int dW, int dH, int dst_stride) {
    return area_call(ctx, "erp_resize_area_any", false, false, src, VIO_PIX_GRAY8, 0, W, H, stride, n_frames, dst, dW,
                     dH, dst_stride);
}

int erp_resize_area_any(vio_ctx* ctx, const uint8_t* src, int W, int H, int stride, uint8_t* dst, int dW, int dH,
                        int dst_stride) {
    return area_call(ctx, "erp_resize_area_any", false, true, src, VIO_PIX_GRAY8, 0, W, H, stride, 1, dst, dW, dH,
                     dst_stride);
}

int erp_ingest_device(vio_ctx* ctx, const uint8_t* src, int format, int luma, int W, int H, int stride, int n_frames,
                      uint8_t* dst, int dW, int dH, int dst_stride) {
    return area_call(ctx, "erp_ingest", false, false, src, format, luma, W, H, stride, n_frames, dst, dW, dH, dst_stride);
}

int erp_ingest(vio_ctx* ctx, const uint8_t* src, int format, int luma, int W, int H, int stride, uint8_t* dst, int dW,
               int dH, int dst_stride) {
    return area_call(ctx, "erp_ingest", false, true, src, format, luma, W, H, stride, 1, dst, dW, dH, dst_stride);
}

int erp_ingest_check(int format, int luma, int W, int H, int stride, int dW, int dH, int dst_stride) {
    const int path = area_check(nullptr, "erp_ingest", false, format, luma, W, H, stride, dW, dH, dst_stride, 1);
    return path < 0 ? path : VIO_OK;
}

int erp_ingest_set_route(vio_ctx* ctx, int route) {
    if (!ctx || route < VIO_INGEST_ROUTE_AUTO || route > VIO_INGEST_ROUTE_FUSED_BYTES) return VIO_EINVAL;
    ctx->ingest_route = route;
    return VIO_OK;
}

int erp_resize_area_kernel_ms(vio_ctx* ctx, double* ms) {
    return ctx ? events_ms(ctx, ctx->ev[kEvResize], ctx->ev[kEvResize + 1], ms) : VIO_EINVAL;
}

int erp_resize_area_tab(int ssize, int dsize, int32_t* di, int32_t* si, float* alpha, int cap, int* n) {
    if (ssize <= 0 || dsize <= 0 || cap < 0 || !n || (cap > 0 && (!di || !si || !alpha))) return VIO_EINVAL;
    if (dsize > ssize) return VIO_ENOSYS;
    std::vector<AreaTap> tab;
    area_tab(ssize, dsize, tab);
    const int m = std::min(cap, (int)tab.size());
    for (int i = 0; i < m; ++i) {
        di[i] = tab[i].di;
        si[i] = tab[i].si;
        alpha[i] = tab[i].alpha;
    }
    *n = (int)tab.size();
    return VIO_OK;
}

int erp_pixel_bytes(int format) {
    switch (format) {
        case VIO_PIX_GRAY8: return 1;
        case VIO_PIX_BGR8:
        case VIO_PIX_RGB8: return 3;
        case VIO_PIX_BGRA8:
        case VIO_PIX_RGBA8: return 4;
        case VIO_PIX_YUYV:
        case VIO_PIX_UYVY: return 2;
        default: return VIO_EINVAL;
    }
}

int erp_luma_u8(int format, int luma, const uint8_t* px, int n, uint8_t* out) {
    const char* why;
    if (pix_check(format, luma, n, &why) || n < 0 || (n > 0 && (!px || !out))) return VIO_EINVAL;
    const PixSrc p = pix_source(format, luma);
    for (int i = 0; i < n; ++i) {
        const uint8_t* s = px + (size_t)i * p.bpp;
        out[i] = pix_is_colour(format) ? luma_u8(s[p.o0], s[p.o1], s[p.o2], p.rule) : s[p.o0];
    }
    return VIO_OK;
}

}  // extern "C"
