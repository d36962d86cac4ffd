// pnp_host.cpp — host side of the absolute-pose RANSAC: the parameter check, the call that stages
// the inputs, enqueues pnp_ransac.hip's three launches and downloads once, and the two host helpers that connect
// the stage to vio_ba_gather(VIO_PNP) and to the VIO_PNP solve's initial pose.
#include <cmath>
#include <cstring>

#include "ctx.h"
#include "frame_io.h"
#include "pnp_ransac.h"
#include "tracker_host.h"

using namespace vio360;

namespace {

bool angle_ok(float a) { return std::isfinite(a) && a > 0.f && (double)a < M_PI / 2; }

void empty_result(vio_pnp_ransac_result* res, int status) {
    std::memset(res, 0, sizeof *res);
    res->status = status;
    res->best_hypothesis = res->best_solution = -1;
}

}  // namespace

extern "C" int vio_pnp_ransac_check(const vio_pnp_ransac_params* p, int n, int iters) {
    if (!p || n < 0 || n > kPnpMaxPoints || iters < 0 || iters > kPnpMaxPoints) return VIO_EINVAL;
    if (!angle_ok(p->inlier_thresh_rad) || !angle_ok(p->min_pair_angle_rad)) return VIO_EINVAL;
    if (p->min_inliers < 0 || p->refit_iters < 0 || p->refit_iters > 10) return VIO_EINVAL;
    return VIO_OK;
}

extern "C" int vio_pnp_ransac(vio_ctx* ctx, const float* points, const float* bearings, int n, const float* R_known,
                              const int32_t* samples, int iters, const vio_pnp_ransac_params* p,
                              vio_pnp_ransac_result* res, uint8_t* mask, int32_t* counts) {
    if (!ctx) return VIO_EINVAL;
    if (vio_pnp_ransac_check(p, n, iters) != VIO_OK || !res || (n > 0 && (!points || !bearings))) {
        set_error(ctx, "vio_pnp_ransac: bad parameters, sizes or null pointers");
        return VIO_EINVAL;
    }
    if (R_known && !is_rotation(R_known)) {
        set_error(ctx, "vio_pnp_ransac: R_cw_known is not a rotation");
        return VIO_EINVAL;
    }
    const int used = R_known ? 2 : 3;
    if (n < used + 1 || iters == 0) {
        empty_result(res, VIO_PNPR_TOO_FEW);
        if (mask) std::memset(mask, 0, (size_t)n);
        if (counts)
            for (int h = 0; h < iters; ++h) counts[h] = -1;
        return VIO_OK;
    }
    if (!samples) {
        set_error(ctx, "vio_pnp_ransac: null samples");
        return VIO_EINVAL;
    }
    for (int h = 0; h < iters; ++h)
        for (int q = 0; q < used; ++q)
            if (samples[3 * h + q] < 0 || samples[3 * h + q] >= n) {
                set_error(ctx, "vio_pnp_ransac: sample index out of range");
                return VIO_EINVAL;
            }
    auto al = [](size_t v) { return (v + 255) / 256 * 256; };
    const size_t bP = sizeof(float) * 3 * (size_t)n, bS = sizeof(int32_t) * 3 * (size_t)iters,
                 bH = sizeof(double) * 48 * (size_t)iters, bI = sizeof(int32_t) * (size_t)iters,
                 bR = sizeof(vio_pnp_ransac_result), bM = (size_t)n;
    const size_t total = 2 * al(bP) + al(bS) + al(bH) + 3 * al(bI) + al(bR) + al(bM);
    VIO_DEVICE(ctx);
    char* d = static_cast<char*>(ctx_buffer(ctx, kSlotPnpRansac, total));
    if (!d) {
        set_error(ctx, "vio_pnp_ransac: device allocation failed");
        return VIO_ENOMEM;
    }
    size_t off = 0;
    auto take = [&](size_t b) { char* q = d + off; off += al(b); return q; };
    PnpArgs a{};
    a.poses = reinterpret_cast<double*>(take(bH));
    float* dP = reinterpret_cast<float*>(take(bP));
    float* dB = reinterpret_cast<float*>(take(bP));
    int32_t* dS = reinterpret_cast<int32_t*>(take(bS));
    a.nsol = reinterpret_cast<int32_t*>(take(bI));
    a.count = reinterpret_cast<int32_t*>(take(bI));
    a.best_sol = reinterpret_cast<int32_t*>(take(bI));
    a.res = reinterpret_cast<vio_pnp_ransac_result*>(take(bR));
    a.mask = reinterpret_cast<uint8_t*>(take(bM));
    a.points = dP;
    a.bearings = dB;
    a.n = n;
    a.samples = dS;
    a.iters = iters;
    a.known = R_known ? 1 : 0;
    for (int q = 0; q < 9; ++q) a.Rk[q] = R_known ? (double)R_known[q] : 0.0;
    const double c = std::cos((double)p->inlier_thresh_rad), cp = std::cos((double)p->min_pair_angle_rad);
    a.c2 = c * c;
    a.cp2 = cp * cp;
    a.p = *p;
    hipStream_t st = ctx->stream;
    hipEvent_t* ev = ctx->ev + kEvPnp;
    if (int rc = events_ready(ctx, ev, 2)) return rc;
    VIO_HIP(ctx, hipMemcpyAsync(dP, points, bP, hipMemcpyHostToDevice, st));
    VIO_HIP(ctx, hipMemcpyAsync(dB, bearings, bP, hipMemcpyHostToDevice, st));
    VIO_HIP(ctx, hipMemcpyAsync(dS, samples, bS, hipMemcpyHostToDevice, st));
    VIO_HIP(ctx, hipEventRecord(ev[0], st));
    if (pnp_launch(st, a) != 0) {
        set_error(ctx, "vio_pnp_ransac: kernel launch failed");
        return VIO_EDEVICE;
    }
    VIO_HIP(ctx, hipEventRecord(ev[1], st));
    VIO_HIP(ctx, hipMemcpyAsync(res, a.res, bR, hipMemcpyDeviceToHost, st));
    if (mask) VIO_HIP(ctx, hipMemcpyAsync(mask, a.mask, bM, hipMemcpyDeviceToHost, st));
    if (counts) VIO_HIP(ctx, hipMemcpyAsync(counts, a.count, bI, hipMemcpyDeviceToHost, st));
    VIO_HIP(ctx, hipStreamSynchronize(st));
    return VIO_OK;
}

extern "C" int vio_pnp_ransac_kernel_ms(vio_ctx* ctx, double* ms) {
    return ctx ? events_ms(ctx, ctx->ev[kEvPnp], ctx->ev[kEvPnp + 1], ms) : VIO_EINVAL;
}

extern "C" int vio_pnp_correspondences(const vio_map_view* m, int frame, float* points, float* bearings, int32_t* feat,
                                       int cap, int* n) {
    if (!m || !n || cap < 0 || frame < 0 || frame >= m->num_frames || !m->feat_begin || m->width <= 0 || m->height <= 0)
        return VIO_EINVAL;
    const int g0 = m->feat_begin[frame], g1 = m->feat_begin[frame + 1];
    if (g1 > g0 && (!m->feat_uv || !m->feat_valid || !m->feat_mp || !m->mp_bad || !m->mp_pos)) return VIO_EINVAL;
    int cnt = 0;
    for (int g = g0; g < g1; ++g) {
        // the VIO_PNP gather's filters (ba_map_host.cpp): valid feature, MapPoint present and not bad, not near
        // the boundary (Camera::IsNearBoundary in f32)
        if (!m->feat_valid[g]) continue;
        const int mp = m->feat_mp[g];
        if (mp < 0 || mp >= m->num_mappoints || m->mp_bad[mp]) continue;
        const float* uv = m->feat_uv + 2 * g;
        if (m->boundary_margin > 0) {
            const float mg = static_cast<float>(m->boundary_margin);
            if (uv[0] < mg || uv[0] > static_cast<float>(m->width) - mg || uv[1] < mg ||
                uv[1] > static_cast<float>(m->height) - mg)
                continue;
        }
        if (cnt < cap) {
            if (feat) feat[cnt] = g;
            if (points)
                for (int q = 0; q < 3; ++q) points[3 * cnt + q] = m->mp_pos[3 * mp + q];
            if (bearings) {
                // Camera::PixelToBearing (Camera.cpp:22-47) in double
                const double lon = ((double)uv[0] / (double)m->width - 0.5) * 2.0 * M_PI;
                const double lat = -((double)uv[1] / (double)m->height - 0.5) * M_PI;
                const double cl = std::cos(lat);
                double b[3] = {cl * std::sin(lon), -std::sin(lat), cl * std::cos(lon)};
                const double nn = std::sqrt(b[0] * b[0] + b[1] * b[1] + b[2] * b[2]);
                for (int q = 0; q < 3; ++q) bearings[3 * cnt + q] = static_cast<float>(b[q] / nn);
            }
        }
        ++cnt;
    }
    *n = cnt;
    return cnt > cap ? VIO_EINVAL : VIO_OK;
}

extern "C" int vio_pnp_compose(const double R_cw[9], const double t_cw[3], const float T_cb[16], float T_wb[16]) {
    if (!R_cw || !t_cw || !T_cb || !T_wb) return VIO_EINVAL;
    // T_wc = [R^T  -R^T t], T_wb = T_wc * T_cb
    double Rw[9], tw[3];
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) Rw[3 * r + c] = R_cw[3 * c + r];
        tw[r] = -((R_cw[r] * t_cw[0] + R_cw[3 + r] * t_cw[1]) + R_cw[6 + r] * t_cw[2]);
    }
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 4; ++c) {
            double s = (Rw[3 * r] * (double)T_cb[c] + Rw[3 * r + 1] * (double)T_cb[4 + c]) + Rw[3 * r + 2] * (double)T_cb[8 + c];
            if (c == 3) s += tw[r];
            T_wb[4 * r + c] = static_cast<float>(s);
        }
    }
    T_wb[12] = T_wb[13] = T_wb[14] = 0.f;
    T_wb[15] = 1.f;
    return VIO_OK;
}
