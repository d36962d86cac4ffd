// frontend_host.cpp — erp_frontend: FeatureTracker::TrackFeatures (FeatureTracker.cpp:61-206) = the device numeric
// path (the tracker's helpers, tracker_host.h) + the reference's host bookkeeping, restated on plain structs
// instead of Frame / Feature.  The f32 expressions here are the reference's, bit for bit (-ffp-contract=off).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "mask.h"
#include "tracker_host.h"

using namespace vio360;

namespace {

struct FeatureRec {
    int32_t id;
    float x, y;
    int32_t track_count, age;
};

// Frame::AssignFeaturesToGrid + LimitFeaturesPerGrid (src/database/Frame.cpp:108-202)
void assign_and_limit(std::vector<FeatureRec>& feats, int W, int H, int gc, int gr, int max_per) {
    const float cw = (float)W / gc, ch = (float)H / gr;
    std::vector<std::vector<int>> grid((size_t)gc * gr);
    auto assign = [&]() {
        for (auto& c : grid) c.clear();
        for (size_t i = 0; i < feats.size(); ++i) {
            float x = feats[i].x, y = feats[i].y;
            if (x < 0 || x >= W || y < 0 || y >= H) continue;
            int gx = std::min((int)(x / cw), gc - 1), gy = std::min((int)(y / ch), gr - 1);
            grid[(size_t)gy * gc + gx].push_back((int)i);
        }
    };
    assign();
    for (auto& cell : grid) {
        if (cell.size() <= (size_t)max_per) continue;
        std::sort(cell.begin(), cell.end(),
                  [&](int a, int b) { return feats[a].track_count > feats[b].track_count; });
        cell.resize(max_per);
    }
    std::vector<char> keep(feats.size(), 0);
    for (auto& cell : grid)
        for (int i : cell) keep[i] = 1;
    std::vector<FeatureRec> out;
    for (size_t i = 0; i < feats.size(); ++i)
        if (keep[i]) out.push_back(feats[i]);
    feats.swap(out);
}

// FeatureTracker::RemoveClusteredFeatures (FeatureTracker.cpp:404-497), tracker grid 20 x 10
void remove_clustered(std::vector<FeatureRec>& feats, int W, int H, float ratio) {
    if (feats.size() < 4) return;
    const int gc = 20, gr = 10;  // m_grid_cols / m_grid_rows (FeatureTracker.cpp:39-40)
    const float cw = (float)W / gc, ch = (float)H / gr;
    const float thr = std::sqrt(cw * cw + ch * ch) * ratio;
    std::vector<std::vector<size_t>> cells((size_t)gc * gr);
    auto cell_of = [&](const FeatureRec& f) {
        int col = std::min((int)(f.x / cw), gc - 1), row = std::min((int)(f.y / ch), gr - 1);
        return (size_t)row * gc + col;
    };
    for (size_t i = 0; i < feats.size(); ++i) cells[cell_of(feats[i])].push_back(i);
    std::vector<char> clustered(cells.size(), 0);
    for (size_t c = 0; c < cells.size(); ++c) {
        if (cells[c].size() < 4) continue;
        float mx = 0.f, my = 0.f;
        for (size_t i : cells[c]) { mx += feats[i].x; my += feats[i].y; }
        mx /= cells[c].size();
        my /= cells[c].size();
        float var = 0.f;
        for (size_t i : cells[c]) {
            float dx = feats[i].x - mx, dy = feats[i].y - my;
            var += (dx * dx + dy * dy);
        }
        var /= cells[c].size();
        if (std::sqrt(var) < thr) clustered[c] = 1;
    }
    std::vector<FeatureRec> out;
    for (auto& f : feats)
        if (!clustered[cell_of(f)]) out.push_back(f);
    feats.swap(out);
}

}  // namespace

struct erp_frontend {
    erp_tracker* t = nullptr;
    erp_frontend_params p{};
    int W = 0, H = 0;
    int frame = 0;
    int32_t next_id = 0;
    int num_tracked = 0, num_detected = 0;
    std::vector<FeatureRec> feats;
    erp_equalize_params eq{};  // erp_frontend_set_equalize; mode VIO_EQ_NONE: off
    int seam = VIO_SEAM_CUT;   // erp_frontend_set_seam (the tracker's mode follows it)
    bool has_pred = false;     // erp_frontend_predict_rotation: R_cur_prev of the next track call only
    float pred_rot[9] = {};
    // erp_frontend_fb_stats: the round-trip check's counts in the last track call (zero when it ran no LK, or
    // the check was off)
    int fb_checked = 0, fb_back_lost = 0, fb_too_far = 0;
    erp_epi_params epi{};  // erp_frontend_set_epipolar; mode VIO_EPI_OFF: today's rotation RANSAC alone
    erp_epi_info epi_info{0, 0, -1, 0, {0.f, 0.f, 0.f}};  // erp_frontend_epi_stats: the stage in the last track call
};

namespace {

// GFTT on slot 1 with the DetectNewFeatures mask: polar ∧ boundary ∧ (discs around `feats`)
int frontend_detect(erp_frontend* f, std::vector<float>& corners) {
    erp_tracker* t = f->t;
    hipStream_t st = t->ctx->stream;
    int rc;
    const bool discs = !f->feats.empty();
    if (discs) {
        const int n = (int)f->feats.size();
        if (n > t->max_points) { set_error(t->ctx, "too many features for the disc mask"); return VIO_ENOSYS; }
        std::vector<float> xy(2 * (size_t)n);
        for (int i = 0; i < n; ++i) { xy[2 * i] = f->feats[i].x; xy[2 * i + 1] = f->feats[i].y; }
        VIO_HIP(t->ctx, hipMemcpyAsync(t->d_pts, xy.data(), sizeof(float) * 2 * n, hipMemcpyHostToDevice, st));
        const size_t disc_bytes = sizeof(uint32_t) * t->disc_words * t->H;
        if (t->has_mask) VIO_HIP(t->ctx, hipMemcpyAsync(t->d_disc, t->d_static, disc_bytes, hipMemcpyDeviceToDevice, st));
        else VIO_HIP(t->ctx, hipMemsetAsync(t->d_disc, 0, disc_bytes, st));
        const int radius = (int)f->p.min_distance;
        if ((rc = ensure_halfw(t, radius))) return rc;
        DiscArgs d{t->d_pts, nullptr, nullptr, nullptr, t->d_disc, t->disc_words, t->W, t->H, radius, t->d_halfw,
                   t->seam};
        hipError_t e = launch_disc_mask(d, n, st);
        if (e != hipSuccess) return hip_fail(t->ctx, e, "disc_mask_kernel");
    }
    GfttPlan plan;
    if ((rc = gftt_plan(t, nullptr, 0, f->p.max_features, (double)f->p.quality_level, (double)f->p.min_distance,
                        f->p.boundary_margin, 0.15f, discs, false, &plan)))
        return rc;
    if ((rc = enqueue_gftt(t, plan))) return rc;
    int n = 0;
    corners.resize(2 * (size_t)std::max(f->p.max_features, 1));
    if ((rc = read_corners(t, corners.data(), &n))) return rc;
    corners.resize(2 * (size_t)n);
    return VIO_OK;
}

// TrackFeatures on the frame now in slot 1
int frontend_track_slot1(erp_frontend* f, int* n_features) {
    erp_tracker* t = f->t;
    vio_ctx* ctx = t->ctx;
    VIO_DEVICE(ctx);
    hipStream_t st = ctx->stream;
    int rc;
    const erp_frontend_params& P = f->p;
    const bool predicted = f->has_pred;  // this call's prediction, consumed whatever the call does
    f->has_pred = false;
    f->fb_checked = f->fb_back_lost = f->fb_too_far = 0;
    f->epi_info = erp_epi_info{0, 0, -1, 0, {0.f, 0.f, 0.f}};
    if (f->eq.mode != VIO_EQ_NONE && (rc = erp_tracker_equalize(t, 1, &f->eq))) return rc;
    if (f->frame == 0 || f->feats.empty()) {
        // first frame (or nothing to track): detect only (:68-97)
        f->feats.clear();
        std::vector<float> c;
        if ((rc = frontend_detect(f, c))) return rc;
        for (size_t i = 0; i < c.size() / 2; ++i) f->feats.push_back({f->next_id++, c[2 * i], c[2 * i + 1], 0, 0});
        f->num_tracked = 0;
        f->num_detected = (int)(c.size() / 2);
        assign_and_limit(f->feats, f->W, f->H, P.grid_cols, P.grid_rows, P.max_features_per_grid);
    } else {
        // TrackOpticalFlow (:228-251)
        const int n = (int)f->feats.size();
        if (n > t->max_points) { set_error(ctx, "too many features"); return VIO_ENOSYS; }
        std::vector<float> prev(2 * (size_t)n), next(2 * (size_t)n);
        std::vector<uint8_t> status(n), usable, fb_state;
        for (int i = 0; i < n; ++i) { prev[2 * i] = f->feats[i].x; prev[2 * i + 1] = f->feats[i].y; }
        if ((rc = erp_tracker_set_points(t, prev.data(), n))) return rc;
        erp_klt_params kp{21, 3, 30, 0.01f, 0.01f, 0};  // FeatureTracker.cpp:33-35, 240
        if (predicted && (rc = tracker_set_rotation(t, f->pred_rot, "erp_frontend_predict_rotation"))) return rc;
        if ((rc = enqueue_lk(t, &kp, n))) return rc;
        VIO_HIP(ctx, hipMemcpyAsync(next.data(), t->d_next, sizeof(float) * 2 * n, hipMemcpyDeviceToHost, st));
        VIO_HIP(ctx, hipMemcpyAsync(status.data(), t->d_status, n, hipMemcpyDeviceToHost, st));
        if (t->fb_valid) {  // the round-trip check ran: status already holds its verdict, the states are for the stats
            fb_state.resize(n);
            VIO_HIP(ctx, hipMemcpyAsync(fb_state.data(), t->d_fb_state, n, hipMemcpyDeviceToHost, st));
        }
        if (t->has_mask) {  // the region mask's bit under every tracked point, gathered on the device
            usable.resize(n);
            VIO_HIP(ctx, launch_mask_gather(t->d_next, n, t->d_static, t->W, t->H, t->d_usable, st, f->seam));
            VIO_HIP(ctx, hipMemcpyAsync(usable.data(), t->d_usable, n, hipMemcpyDeviceToHost, st));
        }
        VIO_HIP(ctx, hipStreamSynchronize(st));
        for (const uint8_t s : fb_state) {
            f->fb_checked += s != VIO_FB_NOT_RUN;
            f->fb_back_lost += s == VIO_FB_BACK_LOST;
            f->fb_too_far += s == VIO_FB_TOO_FAR;
        }
        // status ∧ !IsInPolarRegion ∧ !IsNearBoundary (:117-126; Camera.cpp:120-139)
        std::vector<int> good;
        const float m = (float)P.boundary_margin;
        for (int i = 0; i < n; ++i) {
            float x = next[2 * i], y = next[2 * i + 1];
            float vr = y / (float)f->H;
            bool polar = vr < 0.15f || vr > (1.0f - 0.15f);
            // (seam wrap mode: no left / right margin, x is folded into [0, W))
            bool nearb = (!f->seam && (x < m || x > (float)f->W - m)) || y < m || y > (float)f->H - m;
            if (status[i] && !polar && !nearb && (usable.empty() || usable[i])) good.push_back(i);
        }
        std::vector<uint8_t> inl(good.size(), 1);
        const bool epi = f->epi.mode != VIO_EPI_OFF;
        const bool given = epi && predicted;  // the stage's rotation is this call's prediction
        if (epi && (good.size() >= 3 || (given && !good.empty()))) {
            // the epipolar stage in RANSAC's place: the rotation hypotheses (unless a rotation was predicted), then
            // the plane hypotheses on the first rows of the same sample stream
            const int ng = (int)good.size();
            const int rot_iters = given ? 0 : 1000, epi_iters = ng >= 3 ? f->epi.iters : 0;
            const int ns = ng >= 3 ? std::max(rot_iters, epi_iters) : 0;
            std::vector<int32_t> samples(3 * (size_t)std::max(ns, 1));
            if (ns) erp_ransac_samples(P.ransac_seed + (uint32_t)f->frame, ng, ns, samples.data());
            if ((rc = ensure_iters(t, std::max(ns, 1))) || (rc = ensure_epi(t))) return rc;
            std::vector<float> g0(2 * (size_t)ng), g1(2 * (size_t)ng);
            for (int j = 0; j < ng; ++j) {
                g0[2 * j] = prev[2 * good[j]]; g0[2 * j + 1] = prev[2 * good[j] + 1];
                g1[2 * j] = next[2 * good[j]]; g1[2 * j + 1] = next[2 * good[j] + 1];
            }
            VIO_HIP(ctx, hipMemcpyAsync(t->d_pts, g0.data(), sizeof(float) * 2 * ng, hipMemcpyHostToDevice, st));
            VIO_HIP(ctx, hipMemcpyAsync(t->d_next, g1.data(), sizeof(float) * 2 * ng, hipMemcpyHostToDevice, st));
            if (ns)
                VIO_HIP(ctx, hipMemcpyAsync(t->d_samples, samples.data(), sizeof(int32_t) * 3 * ns, hipMemcpyHostToDevice, st));
            RansacArgs r = ransac_args(t, ng, 0, ng >= 3 ? rot_iters : 0, 0, f->epi.rot_thresh_rad, 0.f, 0, t->d_pts,
                                       t->d_next);
            hipError_t e = launch_ransac_parts(r, false, !given, st);
            if (e == hipSuccess)
                e = launch_epipolar(epi_args(t, r, f->epi, epi_iters, 3, given ? f->pred_rot : nullptr), st);
            if (e != hipSuccess) return hip_fail(ctx, e, "epipolar kernels");
            VIO_HIP(ctx, hipMemcpyAsync(inl.data(), t->d_kept, ng, hipMemcpyDeviceToHost, st));
            if ((rc = epi_read_info(t, &f->epi_info))) return rc;
        } else if (good.size() >= 3) {  // RejectOutliersRotationRANSAC (:253-328)
            const int ng = (int)good.size();
            std::vector<int32_t> samples(3 * 1000);
            erp_ransac_samples(P.ransac_seed + (uint32_t)f->frame, ng, 1000, samples.data());
            std::vector<float> g0(2 * (size_t)ng), g1(2 * (size_t)ng);
            for (int j = 0; j < ng; ++j) {
                g0[2 * j] = prev[2 * good[j]]; g0[2 * j + 1] = prev[2 * good[j] + 1];
                g1[2 * j] = next[2 * good[j]]; g1[2 * j + 1] = next[2 * good[j] + 1];
            }
            VIO_HIP(ctx, hipMemcpyAsync(t->d_pts, g0.data(), sizeof(float) * 2 * ng, hipMemcpyHostToDevice, st));
            VIO_HIP(ctx, hipMemcpyAsync(t->d_next, g1.data(), sizeof(float) * 2 * ng, hipMemcpyHostToDevice, st));
            VIO_HIP(ctx, hipMemcpyAsync(t->d_samples, samples.data(), sizeof(int32_t) * 3000, hipMemcpyHostToDevice, st));
            const float thr = (float)(2.0f * M_PI / 180.0f);
            RansacArgs r = ransac_args(t, ng, 0, 1000, 0, thr, 0.f, 0, t->d_pts, t->d_next);
            hipError_t e = launch_ransac_parts(r, false, true, st);
            if (e != hipSuccess) return hip_fail(ctx, e, "ransac kernels");
            VIO_HIP(ctx, hipMemcpyAsync(inl.data(), t->d_kept, ng, hipMemcpyDeviceToHost, st));
            VIO_HIP(ctx, hipStreamSynchronize(st));
        }
        std::vector<FeatureRec> cur;
        for (size_t j = 0; j < good.size(); ++j) {
            if (!inl[j]) continue;
            const FeatureRec& pf = f->feats[good[j]];
            cur.push_back({pf.id, next[2 * good[j]], next[2 * good[j] + 1], pf.track_count + 1, pf.age + 1});
        }
        f->feats.swap(cur);
        f->num_tracked = (int)f->feats.size();
        if (P.remove_clustered) remove_clustered(f->feats, f->W, f->H, P.clustered_std_ratio);
        assign_and_limit(f->feats, f->W, f->H, P.grid_cols, P.grid_rows, P.max_features_per_grid);
        if ((int)f->feats.size() < P.max_features) {  // CreateFeatureMask + DetectNewFeatures (:176-199)
            std::vector<float> c;
            if ((rc = frontend_detect(f, c))) return rc;
            for (size_t i = 0; i < c.size() / 2; ++i) f->feats.push_back({f->next_id++, c[2 * i], c[2 * i + 1], 0, 0});
            f->num_detected = (int)(c.size() / 2);
            assign_and_limit(f->feats, f->W, f->H, P.grid_cols, P.grid_rows, P.max_features_per_grid);
        } else {
            f->num_detected = 0;
        }
    }
    erp_tracker_swap(t);  // m_prev_image = current (:202)
    f->frame++;
    if (n_features) *n_features = (int)f->feats.size();
    return VIO_OK;
}

int frontend_track_src(erp_frontend* f, const FrameSrc& src, const char* who, int* n_features) {
    if (!f) return VIO_EINVAL;
    const int rc = tracker_ingest(f->t, 1, src, who);
    return rc ? rc : frontend_track_slot1(f, n_features);
}

}  // namespace

extern "C" {

int erp_frontend_create(vio_ctx* ctx, int W, int H, const erp_frontend_params* p, erp_frontend** out) {
    if (!ctx || !p || !out || p->max_features <= 0 || p->grid_cols <= 0 || p->grid_rows <= 0 ||
        p->max_features_per_grid <= 0 || p->min_distance < 0 || p->quality_level <= 0)
        return VIO_EINVAL;
    *out = nullptr;
    VIO_DEVICE(ctx);
    erp_frontend* f = new erp_frontend();
    f->p = *p;
    f->W = W; f->H = H;
    const int cap = std::max(4096, 2 * p->max_features + p->grid_cols * p->grid_rows * p->max_features_per_grid);
    int rc = erp_tracker_create(ctx, W, H, cap, p->max_features, &f->t);
    if (rc) { delete f; return rc; }
    if ((rc = ensure_iters(f->t, 1000))) { erp_tracker_destroy(f->t); delete f; return rc; }
    *out = f;
    return VIO_OK;
}

void erp_frontend_destroy(erp_frontend* f) {
    if (!f) return;
    erp_tracker_destroy(f->t);
    delete f;
}

int erp_frontend_track(erp_frontend* f, const uint8_t* img, int stride, int* n_features) {
    if (!f) return VIO_EINVAL;
    return frontend_track_src(f, {img, VIO_PIX_GRAY8, 0, f->W, f->H, stride, nullptr}, "erp_frontend_track", n_features);
}

int erp_frontend_track_resized(erp_frontend* f, const uint8_t* img, int W, int H, int stride, int* n_features) {
    return frontend_track_src(f, {img, VIO_PIX_GRAY8, 0, W, H, stride, nullptr}, "erp_frontend_track_resized", n_features);
}

int erp_frontend_track_pixels(erp_frontend* f, const uint8_t* img, int format, int luma, int W, int H, int stride,
                              int* n_features) {
    return frontend_track_src(f, {img, format, luma, W, H, stride, nullptr}, "erp_frontend_track_pixels", n_features);
}

int erp_frontend_track_warped(erp_frontend* f, erp_warp* w, const uint8_t* img, int format, int luma, int stride,
                              int* n_features) {
    if (!w) return VIO_EINVAL;
    return frontend_track_src(f, {img, format, luma, 0, 0, stride, w}, "erp_frontend_track_warped", n_features);
}

int erp_frontend_set_equalize(erp_frontend* f, const erp_equalize_params* p) {
    if (!f) return VIO_EINVAL;
    if (!p || p->mode == VIO_EQ_NONE) {
        f->eq = erp_equalize_params{};
        return VIO_OK;
    }
    const int rc = erp_equalize_check(p, f->W, f->H, f->W, f->W);
    if (rc) return rc;
    f->eq = *p;
    return VIO_OK;
}

int erp_frontend_set_seam(erp_frontend* f, int seam) {
    if (!f) return VIO_EINVAL;
    // the front end's LK parameters (frontend_track_slot1) and its min_distance
    int rc = seam_mode_ok(f->t->ctx, seam, f->W, f->H, 21, 3, (double)f->p.min_distance, "erp_frontend_set_seam");
    if (rc) return rc;
    if ((rc = erp_tracker_set_seam(f->t, seam))) return rc;
    f->seam = seam;
    return VIO_OK;
}

int erp_frontend_set_fb(erp_frontend* f, const erp_fb_params* fb) {
    if (!f) return VIO_EINVAL;
    const int rc = fb_params_ok(f->t->ctx, fb, "erp_frontend_set_fb");
    return rc ? rc : erp_tracker_set_fb(f->t, fb);
}

int erp_frontend_set_epipolar(erp_frontend* f, const erp_epi_params* params) {
    if (!f) return VIO_EINVAL;
    const int rc = epi_params_ok(f->t->ctx, params, "erp_frontend_set_epipolar");
    if (rc) return rc;
    f->epi = *params;
    return VIO_OK;
}

int erp_frontend_epi_stats(erp_frontend* f, erp_epi_info* info) {
    if (!f || !info) return VIO_EINVAL;
    *info = f->epi_info;
    return VIO_OK;
}

int erp_frontend_fb_stats(erp_frontend* f, int* checked, int* back_lost, int* too_far) {
    if (!f) return VIO_EINVAL;
    if (checked) *checked = f->fb_checked;
    if (back_lost) *back_lost = f->fb_back_lost;
    if (too_far) *too_far = f->fb_too_far;
    return VIO_OK;
}

int erp_frontend_predict_rotation(erp_frontend* f, const float R_cur_prev[9]) {
    if (!f) return VIO_EINVAL;
    if (!R_cur_prev || !is_rotation(R_cur_prev)) {
        set_error(f->t->ctx, R_cur_prev ? "erp_frontend_predict_rotation: R_cur_prev is not a rotation"
                                        : "erp_frontend_predict_rotation: null R_cur_prev");
        return VIO_EINVAL;
    }
    std::copy(R_cur_prev, R_cur_prev + 9, f->pred_rot);
    f->has_pred = true;
    return VIO_OK;
}

int erp_frontend_set_mask(erp_frontend* f, const uint8_t* mask, int W, int H, int stride, const erp_mask_params* p) {
    return f ? erp_tracker_set_mask(f->t, mask, W, H, stride, p) : VIO_EINVAL;
}

int erp_frontend_set_mask_device(erp_frontend* f, const uint8_t* dmask, int W, int H, int stride,
                                 const erp_mask_params* p) {
    return f ? erp_tracker_set_mask_device(f->t, dmask, W, H, stride, p) : VIO_EINVAL;
}

int erp_frontend_set_mask_warped(erp_frontend* f, erp_warp* w, const uint8_t* src_mask, int stride,
                                 const erp_mask_params* p) {
    return f ? erp_tracker_set_mask_warped(f->t, w, src_mask, stride, p) : VIO_EINVAL;
}

int erp_frontend_features(erp_frontend* f, int32_t* ids, float* xy, int32_t* track_count, int32_t* age, int cap) {
    if (!f || cap < 0) return VIO_EINVAL;
    int n = std::min(cap, (int)f->feats.size());
    for (int i = 0; i < n; ++i) {
        const FeatureRec& r = f->feats[i];
        if (ids) ids[i] = r.id;
        if (xy) { xy[2 * i] = r.x; xy[2 * i + 1] = r.y; }
        if (track_count) track_count[i] = r.track_count;
        if (age) age[i] = r.age;
    }
    return VIO_OK;
}

int erp_frontend_stats(erp_frontend* f, int* num_tracked, int* num_detected) {
    if (!f) return VIO_EINVAL;
    if (num_tracked) *num_tracked = f->num_tracked;
    if (num_detected) *num_detected = f->num_detected;
    return VIO_OK;
}

}  // extern "C"
