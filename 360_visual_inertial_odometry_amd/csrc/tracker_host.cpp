// tracker_host.cpp — C-ABI of the ERP feature tracker (erp_*), host side.
//
// Owns the device state of a tracker (frame pyramids, point / RANSAC / GFTT buffers) and enqueues
// the tracker kernels (trk_lk.hip, trk_ransac.hip, trk_gftt.hip) on the context stream.  The standalone entry
// points erp_klt_track / erp_gftt / erp_rot_ransac mirror the three OpenCV / Eigen calls of FeatureTracker
// (src/processing/FeatureTracker.cpp:222-223, 238-240, 253-379); erp_tracker_run chains them for a
// frame pair without a host round trip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cmath>
#include <cstring>
#include <random>
#include <string>
#include <atomic>
#include <vector>

#include "frame_io.h"
#include "mask.h"
#include "resize.h"
#include "tracker_host.h"
#include "warp.h"

using namespace vio360;

namespace {

constexpr int kMaxIters = 1 << 16;

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// OpenCV imgproc/drawing.cpp Circle(..., fill=1): union of the midpoint-algorithm spans, as the
// half-width of the filled disc on every row offset 0..r
std::vector<int> circle_half_widths(int r) {
    std::vector<int> hw(r + 1, -1);
    int err = 0, dx = r, dy = 0, plus = 1, minus = (r << 1) - 1;
    while (dx >= dy) {
        hw[dy] = std::max(hw[dy], dx);  // rows cy±dy: [cx-dx, cx+dx]
        if (dx <= r) hw[dx] = std::max(hw[dx], dy);  // rows cy±dx: [cx-dy, cx+dy]
        dy++;
        err += plus;
        plus += 2;
        int mask = (err <= 0) - 1;
        err -= minus & mask;
        dx += mask;
        minus -= mask & 2;
    }
    return hw;
}

}  // namespace

namespace vio360 {

template <class T>
static int dalloc(erp_tracker* t, T** p, size_t bytes) {
    DeviceScope scope(t->ctx->device);  // every tracker buffer lives on the context's device
    void* q = nullptr;
    if (hipMalloc(&q, std::max<size_t>(bytes, 64)) != hipSuccess) {
        set_error(t->ctx, "hipMalloc failed in the tracker");
        return VIO_ENOMEM;
    }
    t->allocs.push_back(q);
    *p = (T*)q;
    return VIO_OK;
}

static void tracker_free(erp_tracker* t) {
    if (t->side) (void)hipStreamSynchronize(t->side);  // (the presel hand-off leaves the side stream unjoined)
    for (void* p : t->allocs) (void)hipFree(p);
    t->allocs.clear();
    for (auto& e : t->ev)
        if (e) (void)hipEventDestroy(e);
    if (t->side) (void)hipStreamDestroy(t->side);
    if (t->join) (void)hipEventDestroy(t->join);
    if (t->pyr_done) (void)hipEventDestroy(t->pyr_done);
}

int ensure_iters(erp_tracker* t, int iters) {
    if (iters <= t->iters_cap) return VIO_OK;
    if (iters > kMaxIters) { set_error(t->ctx, "ransac_iters too large"); return VIO_EINVAL; }
    int cap = std::max(iters, 1024);
    int rc;
    if ((rc = dalloc(t, &t->d_samples, sizeof(int32_t) * 3 * cap)) != VIO_OK) return rc;
    if ((rc = dalloc(t, &t->d_count, sizeof(int) * cap)) != VIO_OK) return rc;
    if ((rc = dalloc(t, &t->d_rot, sizeof(float) * 9 * cap)) != VIO_OK) return rc;
    if ((rc = dalloc(t, &t->d_epi_count, sizeof(int) * cap)) != VIO_OK) return rc;
    if ((rc = dalloc(t, &t->d_epi_resc, sizeof(int) * cap)) != VIO_OK) return rc;
    t->iters_cap = cap;
    return VIO_OK;
}

int ensure_halfw(erp_tracker* t, int radius) {
    if (radius == t->halfw_r) return VIO_OK;
    std::vector<int> hw = circle_half_widths(radius);
    int rc;
    if ((rc = dalloc(t, &t->d_halfw, sizeof(int) * (radius + 1)))) return rc;
    VIO_HIP(t->ctx, hipMemcpy(t->d_halfw, hw.data(), sizeof(int) * (radius + 1), hipMemcpyHostToDevice));
    t->halfw_r = radius;
    return VIO_OK;
}

// the GFTT selection grid (3 slots x 4 B per min-distance cell) lives in LDS up to this size, next
// to the selection kernel's ~14 KB of static LDS (config 1: 128 x 64 cells = 96 KB)
constexpr size_t kSelectGridLds = GF_SELECT_LDS_MAX;

static int ensure_gftt(erp_tracker* t, double min_dist) {
    int rc;
    if (!t->d_cand) {
        // NMS leaves at most one candidate per 2x2 block except on exact plateaus; W*H/4 (+slack)
        t->cand_cap = (unsigned int)std::min<size_t>((size_t)t->W * t->H / 4 + 4096, (size_t)1 << 26);
        if ((rc = dalloc(t, &t->d_cand, sizeof(unsigned long long) * t->cand_cap)) != VIO_OK) return rc;
        if ((rc = dalloc(t, &t->d_eig, sizeof(float) * (size_t)t->W * t->H)) != VIO_OK) return rc;
        if ((rc = dalloc(t, &t->d_cand_sorted, sizeof(unsigned long long) * t->cand_cap)) != VIO_OK) return rc;
        t->sort_tmp_bytes = gftt_sort_tmp_bytes(t->cand_cap);
        if ((rc = dalloc(t, (char**)&t->d_sort_tmp, t->sort_tmp_bytes)) != VIO_OK) return rc;
        t->topk_cap = std::min<unsigned int>(GF_TOPK_CAP, t->cand_cap);
        if ((rc = dalloc(t, &t->d_hist, sizeof(unsigned int) * GF_BUCKETS)) != VIO_OK) return rc;
        if ((rc = dalloc(t, &t->d_topk, sizeof(unsigned long long) * t->topk_cap)) != VIO_OK) return rc;
        if ((rc = dalloc(t, &t->d_topk_sorted, sizeof(unsigned long long) * t->topk_cap)) != VIO_OK) return rc;
        if ((rc = dalloc(t, &t->d_hist2, sizeof(unsigned int) * kPresortWords)) != VIO_OK) return rc;
        VIO_HIP(t->ctx, hipMemset(t->d_hist2, 0, sizeof(unsigned int) * kPresortWords));  // the hand-off counter
        if ((rc = dalloc(t, &t->d_topk2, sizeof(unsigned long long) * t->topk_cap)) != VIO_OK) return rc;
        if ((rc = dalloc(t, &t->d_topk2_sorted, sizeof(unsigned long long) * t->topk_cap)) != VIO_OK) return rc;
        t->tiles_x = (t->W + LM_TX - 1) / LM_TX;
        t->tiles_y = (t->H + LM_TY - 1) / LM_TY;
        const size_t nt = (size_t)t->tiles_x * t->tiles_y;
        if ((rc = dalloc(t, &t->d_lmax, sizeof(unsigned long long) * LM_CAP * nt)) != VIO_OK) return rc;
        if ((rc = dalloc(t, &t->d_lmax_n, sizeof(unsigned int) * nt)) != VIO_OK) return rc;
        if ((rc = dalloc(t, &t->d_tile_max, sizeof(uint32_t) * nt)) != VIO_OK) return rc;
        if ((rc = dalloc(t, &t->d_tile_dirty, nt)) != VIO_OK) return rc;
        if ((rc = dalloc(t, &t->d_tile_kmax, sizeof(uint32_t) * nt)) != VIO_OK) return rc;
        // dynamic-LDS limit of the single-workgroup selection kernel, once per tracker (its device is
        // current here): the selection grid and chain heads up to kSelectGridLds (larger grids live in
        // d_grid)
        hipError_t e = gftt_select_set_lds(kSelectGridLds);
        if (e != hipSuccess) return hip_fail(t->ctx, e, "hipFuncSetAttribute(gftt_select)");
    }
    if (min_dist >= 1) {
        int cell = (int)std::lrint(min_dist);
        int gw = (t->W + cell - 1) / cell, gh = (t->H + cell - 1) / cell;
        size_t bytes = (size_t)gw * gh * 3 * sizeof(uint32_t);
        if (bytes > kSelectGridLds && bytes > t->grid_bytes) {
            if ((rc = dalloc(t, &t->d_grid, bytes)) != VIO_OK) return rc;
            t->grid_bytes = bytes;
        }
    }
    return VIO_OK;
}

static int tracker_alloc(erp_tracker* t) {
    int rc;
    int w = t->W, h = t->H;
    t->nlev = 0;
    for (int l = 0; l < TRK_MAX_LEVELS; ++l) {
        t->lw[l] = w; t->lh[l] = h;
        t->lp[l] = (int)align_up(w, 128);
        for (int s = 0; s < 2; ++s)
            if ((rc = dalloc(t, &t->lvl[s][l], (size_t)t->lp[l] * h)) != VIO_OK) return rc;
        t->nlev = l + 1;
        if (w <= 2 || h <= 2) break;
        w = (w + 1) / 2; h = (h + 1) / 2;
    }
    const int P = std::max(t->max_points, 1);
    if ((rc = dalloc(t, &t->d_pts, sizeof(float) * 2 * P))) return rc;
    if ((rc = dalloc(t, &t->d_next, sizeof(float) * 2 * P))) return rc;
    if ((rc = dalloc(t, &t->d_err, sizeof(float) * P))) return rc;
    if ((rc = dalloc(t, &t->d_guess, sizeof(float) * 2 * P))) return rc;
    if ((rc = dalloc(t, &t->d_guess_out, sizeof(float) * 2 * P))) return rc;
    if ((rc = dalloc(t, &t->d_back, sizeof(float) * 2 * P))) return rc;
    if ((rc = dalloc(t, &t->d_fb_d2, sizeof(float) * P))) return rc;
    if ((rc = dalloc(t, &t->d_fb_state, P))) return rc;
    if ((rc = dalloc(t, &t->d_status, P))) return rc;
    if ((rc = dalloc(t, &t->d_kept, P))) return rc;
    if ((rc = dalloc(t, &t->d_gidx, sizeof(int) * P))) return rc;
    if ((rc = dalloc(t, &t->d_b0, sizeof(float) * 3 * P))) return rc;
    if ((rc = dalloc(t, &t->d_b1, sizeof(float) * 3 * P))) return rc;
    if ((rc = dalloc(t, &t->d_bear0, sizeof(float) * 3 * P))) return rc;
    if ((rc = dalloc(t, &t->d_bear1, sizeof(float) * 3 * P))) return rc;
    if ((rc = dalloc(t, &t->d_scal, sizeof(int) * TS_COUNT))) return rc;
    if ((rc = dalloc(t, &t->d_corners, sizeof(float) * 2 * std::max(t->max_corners, 1)))) return rc;
    t->disc_words = (t->W + 31) / 32;
    if ((rc = dalloc(t, &t->d_disc, sizeof(uint32_t) * t->disc_words * t->H))) return rc;
    if ((rc = ensure_iters(t, 1024))) return rc;
    if ((rc = dalloc(t, &t->d_raw, sizeof(uint32_t) * ransac_raw_words()))) return rc;
    for (auto& e : t->ev)
        if (hipEventCreate(&e) != hipSuccess) return hip_fail(t->ctx, hipErrorUnknown, "hipEventCreate");
    // pyr_done only orders GFTT pass 1 after the pyramids (contention, not data: pass 1 reads the uploaded level
    // 0), so it needs no system-scope fence -- the fence costs the main stream ~3 us before LK
    // (gpurun_out A/B, profiles/r6_notes.md); the join carries pass 1's results to the GFTT tail: default fences
    if (hipStreamCreateWithFlags(&t->side, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&t->join, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&t->pyr_done, hipEventDisableTiming | hipEventDisableSystemFence) != hipSuccess)
        return hip_fail(t->ctx, hipErrorUnknown, "side stream / events");
    return VIO_OK;
}

// the same walk on the sizes alone (tracker_alloc's levels), for erp_seam_check: the top level and its width
static int lk_top_level_of(int W, int H, int win, int max_level, int* top_w) {
    int w = W, h = H, lvl = 0;
    for (int l = 0; l <= max_level && l < TRK_MAX_LEVELS; ++l) {
        lvl = l;
        *top_w = w;
        if (w <= 2 || h <= 2) break;  // the last level tracker_alloc makes
        const int nw = (w + 1) / 2, nh = (h + 1) / 2;
        if (nw <= win || nh <= win || l + 1 >= TRK_MAX_LEVELS) break;
        w = nw; h = nh;
    }
    return lvl;
}

// top LK level: buildOpticalFlowPyramid stops when the next level would be <= winSize
static int lk_top_level(const erp_tracker* t, int win, int max_level) {
    int lvl = 0;
    for (int l = 0; l <= max_level && l < t->nlev; ++l) {
        lvl = l;
        int nw = (t->lw[l] + 1) / 2, nh = (t->lh[l] + 1) / 2;
        if (nw <= win || nh <= win || l + 1 >= t->nlev) break;
    }
    return lvl;
}

static int build_pyramids(erp_tracker* t, int top) {
    for (int l = 1; l <= top; ++l) {
        PyrLevelPair s{t->lvl[0][l - 1], t->lvl[1][l - 1], t->lw[l - 1], t->lh[l - 1], t->lp[l - 1], t->seam};
        PyrLevelPair d{t->lvl[0][l], t->lvl[1][l], t->lw[l], t->lh[l], t->lp[l], t->seam};
        hipError_t e = launch_pyr_down(s, d, 2, t->ctx->stream);
        if (e != hipSuccess) return hip_fail(t->ctx, e, "pyr_down_kernel");
    }
    return VIO_OK;
}

static int check_klt(vio_ctx* ctx, const erp_klt_params* p) {
    if (!p) { set_error(ctx, "null erp_klt_params"); return VIO_EINVAL; }
    if (p->win <= 2 || p->win > 21 || p->max_level < 0 || p->max_level >= TRK_MAX_LEVELS) {
        set_error(ctx, "unsupported LK window / level (win in [3,21], max_level < 8)");
        return VIO_ENOSYS;
    }
    return VIO_OK;
}

// aux (the tracker pipeline): extra workgroups of the LK launch (LkAux); the ev[1] stage marker between the
// pyramids and LK then only with stage timing (an event record costs the stream ~6 us before the next launch)
int enqueue_lk(erp_tracker* t, const erp_klt_params* p, int n, bool pyr_built, const LkAux* aux) {
    LkArgs a;
    std::memset(&a, 0, sizeof a);
    int top = lk_top_level(t, p->win, p->max_level);
    int rc = pyr_built ? VIO_OK : build_pyramids(t, top);
    if (rc) return rc;
    for (int l = 0; l <= top; ++l) a.lv[l] = LkLevel{t->lvl[0][l], t->lvl[1][l], t->lw[l], t->lh[l], t->lp[l]};
    a.levels = top;
    a.pts = t->d_pts;
    a.next = t->d_next;
    a.status = t->d_status;
    a.err = t->d_err;
    a.n = n;
    a.win = p->win;
    // TermCriteria clamps (lkpyramid.cpp): maxCount in [0,100], epsilon in [0,10], squared
    a.max_iters = std::min(std::max(p->max_iters, 0), 100);
    double eps = std::min(std::max((double)p->epsilon, 0.0), 10.0);
    a.eps2 = eps * eps;
    a.min_eig = p->min_eig_threshold;
    a.x_wrap = t->seam;
    if (aux) a.bear1 = t->d_bear1;  // the pipeline's RANSAC input (its previous points' bearings: aux workgroups)
    // a prediction belongs to this launch alone
    a.guided = t->pred;
    if (a.guided != LK_GUESS_NONE) {
        a.guess = t->d_guess;
        std::memcpy(a.rot, t->pred_rot, sizeof a.rot);
        a.guess_out = t->d_guess_out;
    }
    t->guess_out_valid = a.guided != LK_GUESS_NONE;
    t->pred = LK_GUESS_NONE;
    a.fb = t->fb.mode;
    if (a.fb != VIO_FB_OFF) {
        a.fb_max_dist = t->fb.max_dist;
        a.back = t->d_back;
        a.fb_state = t->d_fb_state;
        a.fb_d2 = t->d_fb_d2;
    }
    t->fb_valid = a.fb != VIO_FB_OFF;
    if (t->ev[1] && (!aux || t->stage_timing)) (void)hipEventRecord(t->ev[1], t->ctx->stream);
    hipError_t e = launch_lk(a, t->ctx->stream, aux);
    if (e != hipSuccess) return hip_fail(t->ctx, e, "lk_kernel");
    return VIO_OK;
}

RansacArgs ransac_args(erp_tracker* t, int n, int mode, int iters, uint32_t seed, float thr, float polar, int margin,
                       const float* p0, const float* p1) {
    RansacArgs r;
    std::memset(&r, 0, sizeof r);
    r.p0 = p0; r.p1 = p1; r.status = t->d_status;
    r.n = n; r.W = t->W; r.H = t->H; r.mode = mode;
    r.polar_ratio = polar; r.margin = margin;
    r.excl_bits = mode == 1 && t->has_mask ? t->d_static : nullptr;
    r.excl_words = t->disc_words;
    r.x_wrap = t->seam;
    r.gidx = t->d_gidx; r.n_good = t->d_scal + TS_N_GOOD;
    r.b0 = t->d_b0; r.b1 = t->d_b1;
    r.samples = t->d_samples; r.iters = iters; r.seed = seed; r.thresh = thr;
    r.cmin = reinterpret_cast<float*>(t->d_scal + TS_CMIN);
    r.raw = t->d_raw;
    r.count = t->d_count; r.rot = t->d_rot; r.kept = t->d_kept; r.n_in = t->d_scal + TS_N_IN;
    return r;
}

// The route of a detection and its GfArgs, every tracker-owned pointer and scalar slot wired once.
//   VIO_TRK_PRESEL=0: the pipeline takes the local-maximum route with the masked-maximum tail (no presort);
//   VIO_TRK_PRESEL_FLAG=0: the presort reaches the greedy pass through the stream join (~6-14 us of event latency
//   on the critical path) instead of the device counter.
int gftt_plan(erp_tracker* t, const uint8_t* mask, int mask_pitch, int max_corners, double quality, double min_dist,
              int margin, float polar, bool discs, bool pipeline, GfttPlan* out) {
    int rc = ensure_gftt(t, min_dist);
    if (rc) return rc;
    static const auto env_on = [](const char* name) {
        const char* v = std::getenv(name);
        return !(v && v[0] == '0');
    };
    static const bool presel_env = env_on("VIO_TRK_PRESEL"), flag_env = env_on("VIO_TRK_PRESEL_FLAG");
    GfttPlan pl;
    pl.pipeline = pipeline;
    // seam wrap mode takes the map path with the analytic mask (the kernels that know the periodic continuation)
    pl.route = mask || t->seam != VIO_SEAM_CUT ? GfRoute::Map : pipeline && presel_env ? GfRoute::Presel : GfRoute::Lmax;
    pl.resolved = pl.route;
    pl.handoff = pl.route == GfRoute::Presel && flag_env ? GfHandoff::Counter : GfHandoff::Join;
    if (pl.handoff == GfHandoff::Counter) ++t->presort_gen;
    GfArgs g;
    std::memset(&g, 0, sizeof g);
    g.img = t->lvl[1][0]; g.W = t->W; g.H = t->H; g.pitch = t->lp[0];
    // the analytic mask's static part: Camera::CreatePolarMask (Camera.cpp:100-118) + the left/right
    // boundary mask (FeatureTracker.cpp:49-58)
    g.top_rows = (int)((float)t->H * polar);
    g.bottom_start = (int)((float)t->H * (1.0f - polar));
    g.margin = margin;
    if (pl.route != GfRoute::Map) {
        g.lmax = t->d_lmax; g.lmax_n = t->d_lmax_n; g.tile_max = t->d_tile_max; g.tile_dirty = t->d_tile_dirty;
        g.tile_kmax = t->d_tile_kmax;
        g.tiles_x = t->tiles_x; g.tiles_y = t->tiles_y;
        g.lmax_over = t->d_scal + TS_LMAX_OVER;
        g.n_flat = (unsigned int*)(t->d_scal + TS_N_FLAT);
    }
    g.disc_words = t->disc_words;
    if (pipeline && pl.route != GfRoute::Map) {
        // the side stream's mask-independent pass 1 runs on what is wired so far, with the region mask as part of
        // its static region: a large mask then neither fills the presort's prefix with keys the greedy pass has
        // to skip nor raises the tile maxima the threshold is bounded by
        pl.pass1 = g;
        pl.pass1.static_bits = t->has_mask ? t->d_static : nullptr;
    }
    g.mask = mask; g.mask_pitch = mask_pitch;
    g.x_wrap = t->seam;
    // the exclusion plane: the discs stamped onto the region mask's plane, the mask's plane alone, or none
    g.disc_bits = discs ? t->d_disc : (t->has_mask ? t->d_static : nullptr);
    g.quality = quality; g.min_dist = min_dist; g.max_corners = max_corners;
    g.max_ord = (uint32_t*)(t->d_scal + TS_MAX_ORD);
    g.eig = t->d_eig;
    g.cand = t->d_cand; g.cand_sorted = t->d_cand_sorted;
    g.n_cand = (unsigned int*)(t->d_scal + TS_N_CAND);
    g.cand_cap = t->cand_cap;
    // minDistance < 1: every candidate is accepted in order (featureselect.cpp), no grid needed — one
    // cell covering the image keeps the selection kernel's conflict test trivially false
    g.cell = min_dist >= 1 ? (int)std::lrint(min_dist) : std::max(t->W, t->H);
    g.gw = (t->W + g.cell - 1) / g.cell;
    g.gh = (t->H + g.cell - 1) / g.cell;
    size_t lds = (size_t)g.gw * g.gh * 3 * sizeof(uint32_t);
    g.grid_global = lds > kSelectGridLds ? t->d_grid : nullptr;
    g.corners = t->d_corners;
    g.n_out = t->d_scal + TS_N_OUT;
    g.hist = t->d_hist;
    g.topk = t->d_topk;
    g.topk_sorted = t->d_topk_sorted;
    g.n_top = (unsigned int*)(t->d_scal + TS_N_TOP);
    g.cut = t->d_scal + TS_CUT;
    g.incomplete = t->d_scal + TS_INCOMPLETE;
    g.topk_cap = t->topk_cap;
    g.topk_target = (unsigned int)std::min<size_t>(t->topk_cap, std::max<size_t>(4096, 16 * (size_t)max_corners));
    pl.g = g;
    *out = pl;
    return VIO_OK;
}

// the presort of every local maximum of pass 1 (side stream): no disc bitmap, a zero masked maximum (every
// key passes the threshold test), the presort's own histogram / top-K / scalars
static GfArgs gf_presort_args(const erp_tracker* t, const GfttPlan& pl) {
    GfArgs g = pl.pass1;
    unsigned int* sc = t->d_hist2 + GF_BUCKETS;
    g.max_ord = sc + PS_MAX_ORD;
    g.n_cand = sc + PS_N_CAND;
    g.hist = t->d_hist2;
    g.topk = t->d_topk2;
    g.topk_sorted = t->d_topk2_sorted;
    g.n_top = sc + PS_N_TOP;
    g.cut = reinterpret_cast<int*>(sc + PS_CUT);
    g.smax = sc + PS_SMAX;
    if (pl.handoff == GfHandoff::Counter) g.done = sc + PS_DONE;
    g.topk_cap = t->topk_cap;
    // the discs remove the strongest keys near the tracked points: 8 keys per corner (config 1: the greedy pass
    // fills 300 corners from the first ~770 keys; the rank sort's cost grows with the square of the prefix)
    g.topk_target =
        (unsigned int)std::min<size_t>(t->topk_cap, std::max<size_t>(2048, 8 * (size_t)pl.g.max_corners));
    return g;
}

// the greedy pass over the presort's prefix: the run's arguments with the presort's cut ([1]: nothing below it),
// its static-region maximum and, for the counter hand-off, this run's target
static GfArgs gf_presel_args(const erp_tracker* t, const GfttPlan& pl) {
    GfArgs g = pl.g;
    unsigned int* sc = t->d_hist2 + GF_BUCKETS;
    g.presel = 1;
    g.cut = reinterpret_cast<int*>(sc + PS_CUT);
    g.smax = sc + PS_SMAX;
    if (pl.handoff == GfHandoff::Counter) {
        g.wait_ctr = sc + PS_DONE;
        g.wait_target = t->presort_gen * ((t->topk_cap + 63) / 64);
        // (VIO_TRK_TEST_PRESEL_TIMEOUT=1: the first hand-off of the process waits for a count it never
        // reaches -- the bounded wait's path, exercised by tests/test_tracker_gpu.py)
        static std::atomic<int> test_tmo{[] {
            const char* v = std::getenv("VIO_TRK_TEST_PRESEL_TIMEOUT");
            return v && v[0] == '1' ? 1 : 0;
        }()};
        if (test_tmo.exchange(0)) g.wait_target += 1u << 30;
    }
    return g;
}

// The pipeline has already enqueued the reset (LK launch) and, off the map route, pass 1 (and for Presel the
// presort, on the side stream: only the greedy pass over its prefix is enqueued here; read_corners runs the exact
// tail if that pass cannot decide).
int enqueue_gftt(erp_tracker* t, const GfttPlan& pl) {
    t->plan = pl;
    const GfArgs& g = pl.g;
    hipStream_t st = t->ctx->stream;
    hipError_t e = pl.pipeline ? hipSuccess : launch_gftt_reset(g, t->d_scal, st);
    if (pl.route == GfRoute::Map) {
        if (e == hipSuccess) e = launch_gftt_eig(g, st);
        if (e == hipSuccess) e = launch_gftt(g, st);
    } else {
        if (e == hipSuccess && !pl.pipeline) e = launch_gftt_lmax(g, st);
        if (e == hipSuccess)
            e = pl.route == GfRoute::Presel
                    ? launch_gftt_presel(gf_presel_args(t, pl), t->d_topk2_sorted, t->d_hist2 + GF_BUCKETS + PS_N_TOP, st)
                    : launch_gftt_after_lmax(g, st);
    }
    if (e != hipSuccess) return hip_fail(t->ctx, e, "gftt kernels");
    return VIO_OK;
}


static int upload_frame(erp_tracker* t, int slot, const uint8_t* img, int stride) {
    if (!img || stride < t->W) { set_error(t->ctx, "bad frame"); return VIO_EINVAL; }
    return upload_rows(t->ctx, t->lvl[slot][0], t->lp[0], img, stride, t->W, t->H);
}

// Brings the frame into slot `slot` as the tracker's W x H grey image, all on the context stream:
//   a grey frame of the tracker's size: the direct copy;
//   any other frame: staged, then luma + INTER_AREA in one pass (the convert-only pass at the tracker's size);
//   a warp of the tracker's size: staged, then remapped into the slot;
//   a larger warp: staged, remapped at the warp's size, then cv::resize(..., INTER_AREA) into the slot.
int tracker_ingest(erp_tracker* t, int slot, const FrameSrc& f, const char* who) {
    if (!t || slot < 0 || slot > 1 || !f.img) return VIO_EINVAL;
    vio_ctx* ctx = t->ctx;
    erp_warp* w = f.warp;
    const auto fail = [&](int rc, const char* why) {
        set_error(ctx, std::string(who) + ": " + why);
        return rc;
    };
    int rc;
    if (w) {
        if (w->ctx != ctx) return fail(VIO_EINVAL, "the warp belongs to another context");
        if ((rc = erp_warp_check(w, f.format, f.luma, f.stride, w->dW))) return rc;
        if (w->dW < t->W || w->dH < t->H)
            return fail(VIO_ENOSYS, "the warp's destination is smaller than the tracker's frame");
    }
    const int W = w ? w->sW : f.W, H = w ? w->sH : f.H, bpp = erp_pixel_bytes(f.format);
    const long long row = (long long)W * bpp;
    if (bpp < 0 || W <= 0 || H <= 0 || f.stride < row || row > (1 << 30))
        return fail(VIO_EINVAL, "unknown pixel format or bad sizes");
    if (!w && f.format == VIO_PIX_GRAY8 && W == t->W && H == t->H) return upload_frame(t, slot, f.img, f.stride);
    uint8_t* dst = t->lvl[slot][0];
    const int dp = t->lp[0];
    VIO_DEVICE(ctx);
    // source rows padded to 16 bytes: the resize fast path, dword loads for 4-byte pixels
    uint8_t *d_src = nullptr, *d_warp = nullptr;
    int sp = 0, wp = 0;
    if ((rc = stage_rows(ctx, kSlotResizeSrc, f.img, f.stride, row, H, 16, who, &d_src, &sp))) return rc;
    if (!w) return erp_ingest_device(ctx, d_src, f.format, f.luma, W, H, sp, 1, dst, t->W, t->H, dp);
    if (w->dW == t->W && w->dH == t->H) return erp_warp_apply_device(w, d_src, f.format, f.luma, sp, 1, dst, dp);
    if ((rc = scratch_rows(ctx, kSlotWarpDst, w->dW, w->dH, 16, who, &d_warp, &wp))) return rc;
    if ((rc = erp_warp_apply_device(w, d_src, f.format, f.luma, sp, 1, d_warp, wp))) return rc;
    return erp_resize_area_any_device(ctx, d_warp, w->dW, w->dH, wp, 1, dst, t->W, t->H, dp);
}

int read_corners(erp_tracker* t, float* out_xy, int* n_out) {
    GfttPlan& pl = t->plan;
    hipStream_t st = t->ctx->stream;
    int n = 0;
    int sc[TS_CMIN];  // the integer scalars (all before the f32 cosine bound)
    const auto fetch_scalars = [&]() -> int {
        VIO_HIP(t->ctx, hipMemcpyAsync(sc, t->d_scal, sizeof(sc), hipMemcpyDeviceToHost, st));
        VIO_HIP(t->ctx, hipStreamSynchronize(st));
        return VIO_OK;
    };
    int rc = fetch_scalars();
    if (rc) return rc;
    // the side stream's pass 1 / presort (the counter hand-off does not join it): the fallbacks below read them
    VIO_HIP(t->ctx, hipStreamSynchronize(t->side));
    GfArgs g = pl.g;
    if (pl.resolved == GfRoute::Map) g.lmax = nullptr;  // (also after an earlier download's escalation)
    if (pl.resolved != GfRoute::Map && sc[TS_LMAX_OVER]) {  // a tile held more local maxima than its slots
        pl.resolved = GfRoute::Map;
        g.lmax = nullptr;
        hipError_t e = launch_gftt_reset(g, t->d_scal, st);
        if (e == hipSuccess) e = launch_gftt_eig(g, st);
        if (e == hipSuccess) e = launch_gftt(g, st);
        if (e != hipSuccess) return hip_fail(t->ctx, e, "gftt map path");
        if ((rc = fetch_scalars())) return rc;
    }
    if (pl.resolved == GfRoute::Presel && sc[TS_INCOMPLETE]) {
        // the presorted prefix did not decide (threshold bound reached or prefix exhausted before max_corners):
        // the exact tail -- masked maximum, candidate top-K, greedy pass (its buffers are untouched by presel)
        hipError_t e = launch_gftt_after_lmax(g, st);
        if (e != hipSuccess) return hip_fail(t->ctx, e, "gftt exact tail");
        pl.resolved = GfRoute::Lmax;
        ++t->n_exact_tail;
        if ((rc = fetch_scalars())) return rc;
    }
    if ((unsigned int)sc[TS_N_CAND] > t->cand_cap) {  // NMS survivors beyond the candidate buffer: the corner set
        set_error(t->ctx, "GFTT candidate buffer overflow");  // would differ from goodFeaturesToTrack
        return VIO_ENOSYS;
    }
    if (sc[TS_INCOMPLETE]) {  // the top-K subset did not decide: exact pass over every candidate
        ++t->n_full_sort;
        hipError_t e = g.lmax ? launch_gftt_flatten(g, st) : hipSuccess;
        if (e == hipSuccess) e = launch_gftt_full(g, (unsigned int)sc[TS_N_CAND], t->d_sort_tmp, t->sort_tmp_bytes, st);
        if (e != hipSuccess) return hip_fail(t->ctx, e, "gftt exact fallback");
        VIO_HIP(t->ctx, hipMemsetAsync(t->d_scal + TS_INCOMPLETE, 0, sizeof(int), st));
    }
    VIO_HIP(t->ctx, hipMemcpyAsync(&n, t->d_scal + TS_N_OUT, sizeof(int), hipMemcpyDeviceToHost, st));
    VIO_HIP(t->ctx, hipStreamSynchronize(st));
    if (n > 0 && out_xy)
        VIO_HIP(t->ctx, hipMemcpy(out_xy, t->d_corners, sizeof(float) * 2 * n, hipMemcpyDeviceToHost));
    *n_out = n;
    return VIO_OK;
}

bool is_rotation(const float R[9]) {
    for (int i = 0; i < 9; ++i)
        if (!std::isfinite(R[i])) return false;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double s = 0.0;
            for (int k = 0; k < 3; ++k) s += (double)R[3 * k + i] * (double)R[3 * k + j];
            if (std::fabs(s - (i == j ? 1.0 : 0.0)) > 1e-3) return false;
        }
    const double det = (double)R[0] * ((double)R[4] * R[8] - (double)R[5] * R[7]) -
                       (double)R[1] * ((double)R[3] * R[8] - (double)R[5] * R[6]) +
                       (double)R[2] * ((double)R[3] * R[7] - (double)R[4] * R[6]);
    return det > 0.0;
}

int tracker_set_rotation(erp_tracker* t, const float R[9], const char* who) {
    if (!t) return VIO_EINVAL;
    if (!R || !is_rotation(R)) {
        set_error(t->ctx, std::string(who) + (R ? ": R_cur_prev is not a rotation" : ": null R_cur_prev"));
        return VIO_EINVAL;
    }
    std::memcpy(t->pred_rot, R, sizeof t->pred_rot);
    t->pred = LK_GUESS_ROT;
    return VIO_OK;
}

int fb_params_ok(vio_ctx* ctx, const erp_fb_params* fb, const char* who) {
    if (erp_fb_check(fb) != VIO_OK) {
        set_error(ctx, std::string(who) + (fb ? ": bad erp_fb_params (mode VIO_FB_OFF / VIO_FB_ON, max_dist finite and >= 0)"
                                              : ": null erp_fb_params"));
        return VIO_EINVAL;
    }
    return VIO_OK;
}

int epi_params_ok(vio_ctx* ctx, const erp_epi_params* p, const char* who) {
    if (erp_epi_check(p) != VIO_OK) {
        set_error(ctx, std::string(who) + (p ? ": bad erp_epi_params (mode, iters in [0, 65536], angles in (0, pi/2), "
                                               "min_support >= 0)"
                                             : ": null erp_epi_params"));
        return VIO_EINVAL;
    }
    return VIO_OK;
}

int ensure_epi(erp_tracker* t) {
    if (t->d_epi_scal) return VIO_OK;
    int rc;
    const int P = std::max(t->max_points, 1);
    if ((rc = dalloc(t, &t->d_epi_pa, sizeof(float4) * P))) return rc;
    if ((rc = dalloc(t, &t->d_epi_pn, sizeof(float4) * P))) return rc;
    return dalloc(t, &t->d_epi_scal, sizeof(int) * ES_COUNT);
}

EpiArgs epi_args(erp_tracker* t, const RansacArgs& r, const erp_epi_params& p, int iters, int min_n, const float* R) {
    EpiArgs e;
    std::memset(&e, 0, sizeof e);
    e.b0 = r.b0; e.b1 = r.b1; e.gidx = r.gidx; e.n_good = r.n_good; e.n_max = r.n;
    e.samples = r.samples; e.iters = iters; e.min_n = min_n;
    e.cmin = r.cmin;
    e.given = R ? 1 : 0;
    if (R) std::memcpy(e.rot, R, sizeof e.rot);
    e.rot_count = r.count; e.rot_all = r.rot; e.rot_iters = r.iters;
    // the thresholds, once, in double, rounded to float: the kernels evaluate no sin / cos
    const double se = std::sin((double)p.epi_thresh_rad), sp = std::sin((double)p.min_plane_angle_rad);
    e.s2_epi = (float)(se * se);
    e.s2_plane = (float)(sp * sp);
    e.cmax = (float)std::cos((double)p.max_parallax_rad);
    e.min_support = p.min_support;
    e.pa = t->d_epi_pa; e.pn = t->d_epi_pn;
    e.count = t->d_epi_count; e.resc = t->d_epi_resc;
    e.scal = t->d_epi_scal;
    e.kept = r.kept; e.n_in = r.n_in;
    return e;
}

int epi_read_info(erp_tracker* t, erp_epi_info* info) {
    static_assert(sizeof(erp_epi_info) == 7 * sizeof(int), "erp_epi_info is the stage's seven scalars");
    VIO_HIP(t->ctx, hipStreamSynchronize(t->ctx->stream));
    VIO_HIP(t->ctx, hipMemcpy(info, t->d_epi_scal + ES_INFO, sizeof *info, hipMemcpyDeviceToHost));
    return VIO_OK;
}

int seam_mode_ok(vio_ctx* ctx, int seam, int W, int H, int win, int max_level, double min_dist, const char* who) {
    if (seam != VIO_SEAM_CUT && seam != VIO_SEAM_WRAP) {
        set_error(ctx, std::string(who) + ": unknown seam mode");
        return VIO_EINVAL;
    }
    if (seam == VIO_SEAM_WRAP && erp_seam_check(W, H, win, max_level, min_dist) != VIO_OK) {
        set_error(ctx, std::string(who) + ": the frame size, LK levels or min_dist do not admit VIO_SEAM_WRAP (erp_seam_check)");
        return VIO_EINVAL;
    }
    return VIO_OK;
}

}  // namespace vio360

extern "C" {

int erp_ransac_samples(uint32_t seed, int n, int iters, int32_t* out) {
    if (n < 3 || iters < 0 || (iters > 0 && !out)) return VIO_EINVAL;
    std::mt19937 gen(seed);
    std::uniform_int_distribution<> dis(0, n - 1);
    for (int it = 0; it < iters; ++it) {
        int got[3], k = 0;
        while (k < 3) {
            int idx = dis(gen);
            bool dup = false;
            for (int q = 0; q < k; ++q) dup |= got[q] == idx;
            if (!dup) got[k++] = idx;
        }
        out[3 * it] = got[0]; out[3 * it + 1] = got[1]; out[3 * it + 2] = got[2];
    }
    return VIO_OK;
}

// min_side: erp_tracker_create's 8; 3 for the scratch tracker of erp_gftt, which admits W, H >= 3 (its kernels read
// level 0 only, through reflect101: 3x3 neighbourhoods need no more)
static int tracker_new(vio_ctx* ctx, int W, int H, int max_points, int max_corners, int min_side, erp_tracker** out) {
    if (!ctx || !out || W < min_side || H < min_side || W > 65535 || H > 65535 || max_points < 0 || max_corners < 0)
        return VIO_EINVAL;
    *out = nullptr;
    DeviceScope _vio_dev_scope(ctx->device);
    erp_tracker* t = new erp_tracker();
    t->ctx = ctx; t->W = W; t->H = H; t->max_points = max_points; t->max_corners = max_corners;
    int rc = tracker_alloc(t);
    if (rc) { tracker_free(t); delete t; return rc; }
    *out = t;
    return VIO_OK;
}

int erp_tracker_create(vio_ctx* ctx, int W, int H, int max_points, int max_corners, erp_tracker** out) {
    return tracker_new(ctx, W, H, max_points, max_corners, 8, out);
}

int erp_tracker_gftt_fallbacks(erp_tracker* t, int* exact_tail, int* full_sort) {
    if (!t || !exact_tail || !full_sort) return VIO_EINVAL;
    *exact_tail = t->n_exact_tail;
    *full_sort = t->n_full_sort;
    return VIO_OK;
}

void erp_tracker_destroy(erp_tracker* t) {
    if (!t) return;
    DeviceScope _vio_dev_scope(t->ctx->device);
    (void)hipStreamSynchronize(t->ctx->stream);
    tracker_free(t);
    delete t;
}

int erp_tracker_upload(erp_tracker* t, int slot, const uint8_t* img, int stride) {
    if (!t) return VIO_EINVAL;
    return tracker_ingest(t, slot, {img, VIO_PIX_GRAY8, 0, t->W, t->H, stride, nullptr}, "erp_tracker_upload");
}

int erp_tracker_upload_resized(erp_tracker* t, int slot, const uint8_t* img, int W, int H, int stride) {
    return tracker_ingest(t, slot, {img, VIO_PIX_GRAY8, 0, W, H, stride, nullptr}, "erp_tracker_upload_resized");
}

int erp_tracker_upload_pixels(erp_tracker* t, int slot, const uint8_t* img, int format, int luma, int W, int H,
                              int stride) {
    return tracker_ingest(t, slot, {img, format, luma, W, H, stride, nullptr}, "erp_tracker_upload_pixels");
}

int erp_tracker_upload_warped(erp_tracker* t, int slot, erp_warp* w, const uint8_t* img, int format, int luma,
                              int stride) {
    if (!w) return VIO_EINVAL;
    return tracker_ingest(t, slot, {img, format, luma, 0, 0, stride, w}, "erp_tracker_upload_warped");
}

int erp_tracker_equalize(erp_tracker* t, int slot, const erp_equalize_params* p) {
    if (!t || slot < 0 || slot > 1 || !p) return VIO_EINVAL;
    if (p->mode == VIO_EQ_NONE) return erp_equalize_check(p, t->W, t->H, t->lp[0], t->lp[0]);
    return erp_equalize_device(t->ctx, t->lvl[slot][0], t->W, t->H, t->lp[0], 1, p, t->lvl[slot][0], t->lp[0]);
}

int erp_tracker_device_frame(erp_tracker* t, int slot, uint8_t** dev_ptr, int* pitch) {
    if (!t || slot < 0 || slot > 1 || !dev_ptr || !pitch) return VIO_EINVAL;
    *dev_ptr = t->lvl[slot][0];
    *pitch = t->lp[0];
    return VIO_OK;
}

int erp_tracker_swap(erp_tracker* t) {
    if (!t) return VIO_EINVAL;
    for (int l = 0; l < t->nlev; ++l) std::swap(t->lvl[0][l], t->lvl[1][l]);
    return VIO_OK;
}

int erp_tracker_set_points(erp_tracker* t, const float* pts, int n) {
    if (!t || n < 0 || n > t->max_points || (n > 0 && !pts)) {
        if (t) set_error(t->ctx, "point count exceeds max_points");
        return VIO_EINVAL;
    }
    t->n_pts = n;
    VIO_DEVICE(t->ctx);
    if (n) VIO_HIP(t->ctx, hipMemcpyAsync(t->d_pts, pts, sizeof(float) * 2 * n, hipMemcpyHostToDevice, t->ctx->stream));
    return VIO_OK;
}

int erp_tracker_set_guess(erp_tracker* t, const float* guess, int n) {
    if (!t) return VIO_EINVAL;
    if (!guess || n != t->n_pts) {
        set_error(t->ctx, guess ? "erp_tracker_set_guess: n is not the erp_tracker_set_points count"
                                : "erp_tracker_set_guess: null guess");
        return VIO_EINVAL;
    }
    VIO_DEVICE(t->ctx);
    if (n)
        VIO_HIP(t->ctx, hipMemcpyAsync(t->d_guess, guess, sizeof(float) * 2 * n, hipMemcpyHostToDevice, t->ctx->stream));
    t->pred = LK_GUESS_PTS;
    return VIO_OK;
}

int erp_tracker_set_rotation(erp_tracker* t, const float R_cur_prev[9]) {
    return tracker_set_rotation(t, R_cur_prev, "erp_tracker_set_rotation");
}

int erp_tracker_download_guess(erp_tracker* t, float* guess) {
    if (!t) return VIO_EINVAL;
    if (!guess || !t->guess_out_valid) {
        set_error(t->ctx, guess ? "erp_tracker_download_guess: the last run had no prediction"
                                : "erp_tracker_download_guess: null guess");
        return VIO_EINVAL;
    }
    VIO_DEVICE(t->ctx);
    VIO_HIP(t->ctx, hipStreamSynchronize(t->ctx->stream));
    if (t->n_pts)
        VIO_HIP(t->ctx, hipMemcpy(guess, t->d_guess_out, sizeof(float) * 2 * t->n_pts, hipMemcpyDeviceToHost));
    return VIO_OK;
}

int erp_tracker_set_fb(erp_tracker* t, const erp_fb_params* fb) {
    if (!t) return VIO_EINVAL;
    const int rc = fb_params_ok(t->ctx, fb, "erp_tracker_set_fb");
    if (rc) return rc;
    t->fb = *fb;
    return VIO_OK;
}

int erp_tracker_download_fb(erp_tracker* t, float* back, uint8_t* fb_state, float* fb_d2) {
    if (!t) return VIO_EINVAL;
    if (!t->fb_valid) {
        set_error(t->ctx, "erp_tracker_download_fb: the last run had the round-trip check off");
        return VIO_EINVAL;
    }
    VIO_DEVICE(t->ctx);
    VIO_HIP(t->ctx, hipStreamSynchronize(t->ctx->stream));
    const int n = t->n_pts;
    if (n && back) VIO_HIP(t->ctx, hipMemcpy(back, t->d_back, sizeof(float) * 2 * n, hipMemcpyDeviceToHost));
    if (n && fb_state) VIO_HIP(t->ctx, hipMemcpy(fb_state, t->d_fb_state, n, hipMemcpyDeviceToHost));
    if (n && fb_d2) VIO_HIP(t->ctx, hipMemcpy(fb_d2, t->d_fb_d2, sizeof(float) * n, hipMemcpyDeviceToHost));
    return VIO_OK;
}

// the enqueue sequence of one pipeline run
static int enqueue_run(erp_tracker* t, const erp_klt_params* klt, const erp_tracker_params* p, int n, int radius,
                       const GfttPlan& pl) {
    int rc;
    hipStream_t st = t->ctx->stream;
    // seam wrap mode: detection takes the map route on the main stream (enqueue_gftt), no side work
    const bool side = pl.route != GfRoute::Map;
    // GFTT's candidate order is known before the disc mask: the side stream presorts every local maximum after
    // pass 1 and the tail after the hand-off is one greedy pass (Lmax: the masked-maximum tail after the join)
    const bool presel = pl.route == GfRoute::Presel;
    // epipolar stage: the run's rotation (erp_tracker_set_rotation) before enqueue_lk consumes it; the rotation test
    // then takes the stage's threshold, so that one cosine bound serves both
    const bool epi = t->epi.mode != VIO_EPI_OFF;
    const bool epi_given = epi && t->pred == LK_GUESS_ROT;
    float epi_rot[9];
    std::memcpy(epi_rot, t->pred_rot, sizeof epi_rot);
    const float rot_thresh = epi ? t->epi.rot_thresh_rad : p->ransac_thresh_rad;
    t->epi_valid = epi;
    // main stream: pyramids, then LK, whose launch also carries the RANSAC draws' raw stream (seed only),
    // the GFTT counters / histogram / top-K reset and the disc bitmap clear in extra workgroups (on the
    // side stream they cost the main stream a cross-stream wait before RANSAC); side stream: GFTT pass 1
    // (the eigenvalue map of the current frame does not depend on tracking) once the pyramids are built,
    // beside LK / RANSAC (from the start of the run, beside the pyramids: measured 6 % slower)
    {
        LkAux x;
        std::memset(&x, 0, sizeof x);
        x.raw = t->d_raw;
        x.seed = p->ransac_seed;
        x.thresh = rot_thresh;
        x.cmin = reinterpret_cast<float*>(t->d_scal + TS_CMIN);
        x.hist = t->d_hist;
        x.topk = t->d_topk;
        x.topk_cap = t->topk_cap;
        x.scal = t->d_scal;
        x.disc = t->d_disc;
        x.disc_words = (size_t)t->disc_words * t->H;
        x.disc_src = t->has_mask ? t->d_static : nullptr;
        x.pts = t->d_pts;
        x.bear0 = t->d_bear0;
        x.n = n;
        x.W = t->W;
        x.H = t->H;
        int top = lk_top_level(t, klt->win, klt->max_level);
        if ((rc = build_pyramids(t, top))) return rc;
        if (side) VIO_HIP(t->ctx, hipEventRecord(t->pyr_done, st));
        if ((rc = enqueue_lk(t, klt, n, true, &x))) return rc;
    }
    // The side stream (pass 1 + presort) is the longer path once the tail is one greedy pass, and the host's
    // enqueue order decides when the GPU first sees it (each launch costs the host a few microseconds, which the
    // GPU outruns): its work is enqueued after LK (pass 1 dispatched ~14 us after the pyramids; enqueued before
    // LK it delays LK for the same total, enqueued first 3-5 % slower: profiles/r6c_ab_side.log)
    if (side) {
        VIO_HIP(t->ctx, hipStreamWaitEvent(t->side, t->pyr_done, 0));
        GfArgs gl = pl.pass1;
        if (presel) {  // pass 1 clears the presort's histogram and scalars (ordered before the presort, and after
                       // the previous run's greedy pass through the pyramid event)
            gl.clear = t->d_hist2;
            gl.clear_n = kPresortClear;
        }
        hipError_t e = launch_gftt_lmax(gl, t->side);
        if (e != hipSuccess) return hip_fail(t->ctx, e, "gftt_lmax_kernel");
        if (presel) {
            e = launch_gftt_presort(gf_presort_args(t, pl), t->side);
            if (e != hipSuccess) return hip_fail(t->ctx, e, "gftt presort");
        }
        VIO_HIP(t->ctx, hipEventRecord(t->join, t->side));
    }
    if (t->stage_timing) VIO_HIP(t->ctx, hipEventRecord(t->ev[2], st));
    // (with a given rotation no rotation hypothesis is evaluated: the sampler draws the stage's rows only)
    const int epi_iters = std::min(t->epi.iters, p->ransac_iters);
    RansacArgs r = ransac_args(t, n, 1, epi_given ? epi_iters : p->ransac_iters, p->ransac_seed, rot_thresh,
                               p->polar_ratio, p->boundary_margin, t->d_pts, t->d_next);
    r.bear0 = t->d_bear0;  // formed by the LK launch
    r.bear1 = t->d_bear1;
    if (epi) {
        // the unfused tail: compaction + sampler (+ rotation hypotheses and selection), the epipolar kernels on
        // kept / TS_N_IN, then the discs around the final kept points
        DiscArgs d{t->d_next, t->d_kept, nullptr, nullptr, t->d_disc, t->disc_words, t->W, t->H, radius,
                   t->d_halfw, t->seam};
        hipError_t e = launch_ransac_parts(r, true, !epi_given, st);
        if (e == hipSuccess) e = launch_epipolar(epi_args(t, r, t->epi, epi_iters, 3, epi_given ? epi_rot : nullptr), st);
        if (e == hipSuccess && radius > 0) e = launch_disc_mask(d, n, st);
        if (e != hipSuccess) return hip_fail(t->ctx, e, "epipolar kernels");
    } else if (n > 0) {
        // RANSAC, then its selection and CreateFeatureMask's discs of radius (int)min_dist around every kept
        // point in one launch (bitmap cleared in the LK launch; radius 0: no discs)
        DiscArgs d{t->d_next, t->d_kept, nullptr, nullptr, t->d_disc, t->disc_words, t->W, t->H, radius,
                   t->d_halfw, t->seam};
        hipError_t e = launch_ransac_pipeline(r, d, st);
        if (e != hipSuccess) return hip_fail(t->ctx, e, "ransac kernels");
    } else {
        VIO_HIP(t->ctx, hipMemsetAsync(t->d_scal, 0, 2 * sizeof(int), st));
    }
    if (t->stage_timing) VIO_HIP(t->ctx, hipEventRecord(t->ev[3], st));
    if (side && pl.handoff == GfHandoff::Join) VIO_HIP(t->ctx, hipStreamWaitEvent(st, t->join, 0));
    return enqueue_gftt(t, pl);
}

static int tracker_run(erp_tracker* t, const erp_klt_params* klt, const erp_tracker_params* p);

int erp_tracker_run(erp_tracker* t, const erp_klt_params* klt, const erp_tracker_params* p) {
    if (!t || !p) return VIO_EINVAL;
    const int rc = tracker_run(t, klt, p);
    t->pred = LK_GUESS_NONE;  // a prediction belongs to this run, also when the run is refused
    return rc;
}

static int tracker_run(erp_tracker* t, const erp_klt_params* klt, const erp_tracker_params* p) {
    int rc = check_klt(t->ctx, klt);
    if (rc) return rc;
    if (p->ransac_iters < 0 || p->max_corners < 0 || p->max_corners > t->max_corners || p->quality <= 0 ||
        p->min_dist < 0) {
        set_error(t->ctx, "bad erp_tracker_params");
        return VIO_EINVAL;
    }
    if (t->seam != VIO_SEAM_CUT && erp_seam_check(t->W, t->H, klt->win, klt->max_level, p->min_dist) != VIO_OK) {
        set_error(t->ctx, "erp_tracker_run: the frame size, LK levels or min_dist do not admit VIO_SEAM_WRAP (erp_seam_check)");
        return VIO_EINVAL;
    }
    VIO_DEVICE(t->ctx);
    if ((rc = ensure_iters(t, std::max(p->ransac_iters, 1)))) return rc;
    if (t->epi.mode != VIO_EPI_OFF && (rc = ensure_epi(t))) return rc;
    const int radius = (int)p->min_dist;  // CreateFeatureMask's discs
    if ((rc = ensure_halfw(t, radius))) return rc;
    GfttPlan plan;
    if ((rc = gftt_plan(t, nullptr, 0, p->max_corners, p->quality, p->min_dist, p->boundary_margin, p->polar_ratio,
                        true, true, &plan)))
        return rc;
    hipStream_t st = t->ctx->stream;
    VIO_HIP(t->ctx, hipEventRecord(t->ev[0], st));
    if ((rc = enqueue_run(t, klt, p, t->n_pts, radius, plan))) return rc;
    VIO_HIP(t->ctx, hipEventRecord(t->ev[4], st));
    t->ran = true;
    t->timed_run = t->stage_timing;
    return VIO_OK;
}

int erp_tracker_sync(erp_tracker* t) {
    if (!t) return VIO_EINVAL;
    VIO_DEVICE(t->ctx);
    VIO_HIP(t->ctx, hipStreamSynchronize(t->ctx->stream));
    VIO_HIP(t->ctx, hipStreamSynchronize(t->side));  // (the presel hand-off leaves the side stream unjoined)
    return VIO_OK;
}

int erp_tracker_download(erp_tracker* t, float* next, uint8_t* status, uint8_t* kept, float* corners, int* n_corners) {
    if (!t) return VIO_EINVAL;
    VIO_DEVICE(t->ctx);
    VIO_HIP(t->ctx, hipStreamSynchronize(t->ctx->stream));
    const int n = t->n_pts;
    if (n && next) VIO_HIP(t->ctx, hipMemcpy(next, t->d_next, sizeof(float) * 2 * n, hipMemcpyDeviceToHost));
    if (n && status) VIO_HIP(t->ctx, hipMemcpy(status, t->d_status, n, hipMemcpyDeviceToHost));
    if (n && kept) VIO_HIP(t->ctx, hipMemcpy(kept, t->d_kept, n, hipMemcpyDeviceToHost));
    if (n_corners) {
        int nc = 0;
        int rc = read_corners(t, corners, &nc);
        if (rc) return rc;
        *n_corners = nc;
    }
    return VIO_OK;
}

int erp_tracker_set_stage_timing(erp_tracker* t, int on) {
    if (!t) return VIO_EINVAL;
    t->stage_timing = on != 0;
    return VIO_OK;
}

int erp_tracker_stage_ms(erp_tracker* t, double* pyr_ms, double* lk_ms, double* ransac_ms, double* gftt_ms,
                         double* total_ms) {
    if (!t || !t->ran) return VIO_EINVAL;
    VIO_DEVICE(t->ctx);
    VIO_HIP(t->ctx, hipEventSynchronize(t->ev[4]));
    float a = -1, b = -1, c = -1, d = -1, e = 0;
    if (t->timed_run) {
        VIO_HIP(t->ctx, hipEventElapsedTime(&a, t->ev[0], t->ev[1]));
        VIO_HIP(t->ctx, hipEventElapsedTime(&b, t->ev[1], t->ev[2]));
        VIO_HIP(t->ctx, hipEventElapsedTime(&c, t->ev[2], t->ev[3]));
        VIO_HIP(t->ctx, hipEventElapsedTime(&d, t->ev[3], t->ev[4]));
    }
    VIO_HIP(t->ctx, hipEventElapsedTime(&e, t->ev[0], t->ev[4]));
    if (pyr_ms) *pyr_ms = a;
    if (lk_ms) *lk_ms = b;
    if (ransac_ms) *ransac_ms = c;
    if (gftt_ms) *gftt_ms = d;
    if (total_ms) *total_ms = e;
    return VIO_OK;
}

int erp_fb_check(const erp_fb_params* fb) {
    if (!fb || (fb->mode != VIO_FB_OFF && fb->mode != VIO_FB_ON) || !std::isfinite(fb->max_dist) ||
        !(fb->max_dist >= 0.f))
        return VIO_EINVAL;
    return VIO_OK;
}

int erp_seam_check(int W, int H, int win, int max_level, double min_dist) {
    if (W <= 0 || H <= 0 || W > 65535 || H > 65535 || win <= 2 || win > LK_WIN_MAX || max_level < 0 ||
        max_level >= TRK_MAX_LEVELS || !(min_dist >= 0))
        return VIO_EINVAL;
    int top_w = W;
    const int top = lk_top_level_of(W, H, win, max_level, &top_w);
    if (W % (1 << top) != 0) return VIO_EINVAL;     // an odd level: its wrapped pyrDown is not the continuation's
    static_assert(LK_R >= LK_T, "the next-frame region is the wider LK staging tile");
    if (top_w < LK_R) return VIO_EINVAL;            // a staging tile would cross the seam twice
    if ((double)W <= 2.0 * min_dist) return VIO_EINVAL;  // a disc / min-distance neighbourhood would meet itself
    return VIO_OK;
}

int erp_klt_track(vio_ctx* ctx, const uint8_t* prev, const uint8_t* curr, int W, int H, int stride, const float* pts,
                  int n, float* next, uint8_t* status, float* err, const erp_klt_params* params) {
    return erp_klt_track_seam(ctx, prev, curr, W, H, stride, pts, n, next, status, err, params, VIO_SEAM_CUT);
}

// the one-shot LK calls: a tracker for the call, the two frames, the points, one LK launch.  guess / R: the guided
// forms (at most one of them); guess_out: the start positions used (guided only, may be null); fb: the round-trip
// check (null: off) and where its three arrays go (each may be null)
struct FbOut {
    const erp_fb_params* fb;
    float* back;
    uint8_t* state;
    float* d2;
};
static int klt_track_once(vio_ctx* ctx, const uint8_t* prev, const uint8_t* curr, int W, int H, int stride,
                          const float* pts, int n, float* next, uint8_t* status, float* err,
                          const erp_klt_params* params, int seam, const float* guess, const float* R,
                          float* guess_out, const char* who, const FbOut* fbo = nullptr) {
    int rc = check_klt(ctx, params);
    if (rc) return rc;
    if (fbo && (rc = fb_params_ok(ctx, fbo->fb, who))) return rc;
    if ((rc = seam_mode_ok(ctx, seam, W, H, params->win, params->max_level, 0.0, who))) return rc;
    if (R && !is_rotation(R)) {
        set_error(ctx, std::string(who) + ": R_cur_prev is not a rotation");
        return VIO_EINVAL;
    }
    VIO_DEVICE(ctx);
    erp_tracker* t = nullptr;
    if ((rc = erp_tracker_create(ctx, W, H, std::max(n, 1), 0, &t))) return rc;
    t->seam = seam;
    const bool fb_on = fbo && fbo->fb->mode != VIO_FB_OFF;
    if (fbo) t->fb = *fbo->fb;
    if (!(rc = upload_frame(t, 0, prev, stride)) && !(rc = upload_frame(t, 1, curr, stride)) &&
        !(rc = erp_tracker_set_points(t, pts, n)) && !(rc = guess ? erp_tracker_set_guess(t, guess, n) : VIO_OK) &&
        !(rc = R ? tracker_set_rotation(t, R, who) : VIO_OK) && !(rc = enqueue_lk(t, params, n))) {
        hipError_t e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) rc = hip_fail(ctx, e, "erp_klt_track");
        else if (n) {
            if (hipMemcpy(next, t->d_next, sizeof(float) * 2 * n, hipMemcpyDeviceToHost) != hipSuccess ||
                hipMemcpy(status, t->d_status, n, hipMemcpyDeviceToHost) != hipSuccess ||
                (err && hipMemcpy(err, t->d_err, sizeof(float) * n, hipMemcpyDeviceToHost) != hipSuccess) ||
                (guess_out &&
                 hipMemcpy(guess_out, t->d_guess_out, sizeof(float) * 2 * n, hipMemcpyDeviceToHost) != hipSuccess) ||
                (fb_on && fbo->back &&
                 hipMemcpy(fbo->back, t->d_back, sizeof(float) * 2 * n, hipMemcpyDeviceToHost) != hipSuccess) ||
                (fb_on && fbo->state && hipMemcpy(fbo->state, t->d_fb_state, n, hipMemcpyDeviceToHost) != hipSuccess) ||
                (fb_on && fbo->d2 &&
                 hipMemcpy(fbo->d2, t->d_fb_d2, sizeof(float) * n, hipMemcpyDeviceToHost) != hipSuccess))
                rc = hip_fail(ctx, hipErrorUnknown, "erp_klt_track download");
        }
    }
    erp_tracker_destroy(t);
    return rc;
}

int erp_klt_track_seam(vio_ctx* ctx, const uint8_t* prev, const uint8_t* curr, int W, int H, int stride,
                       const float* pts, int n, float* next, uint8_t* status, float* err, const erp_klt_params* params,
                       int seam) {
    if (!ctx || !prev || !curr || n < 0 || (n > 0 && (!pts || !next || !status))) return VIO_EINVAL;
    return klt_track_once(ctx, prev, curr, W, H, stride, pts, n, next, status, err, params, seam, nullptr, nullptr,
                          nullptr, "erp_klt_track_seam");
}

int erp_klt_track_guess(vio_ctx* ctx, const uint8_t* prev, const uint8_t* curr, int W, int H, int stride,
                        const float* pts, const float* guess, int n, float* next, uint8_t* status, float* err,
                        const erp_klt_params* params, int seam) {
    if (!ctx) return VIO_EINVAL;
    if (!prev || !curr || n < 0 || !guess || (n > 0 && (!pts || !next || !status))) {
        set_error(ctx, "erp_klt_track_guess: null frame, points, guess or output, or n < 0");
        return VIO_EINVAL;
    }
    return klt_track_once(ctx, prev, curr, W, H, stride, pts, n, next, status, err, params, seam, guess, nullptr,
                          nullptr, "erp_klt_track_guess");
}

int erp_klt_track_rot(vio_ctx* ctx, const uint8_t* prev, const uint8_t* curr, int W, int H, int stride,
                      const float* pts, int n, const float R_cur_prev[9], float* next, uint8_t* status, float* err,
                      float* guess_out, const erp_klt_params* params, int seam) {
    if (!ctx) return VIO_EINVAL;
    if (!prev || !curr || n < 0 || !R_cur_prev || (n > 0 && (!pts || !next || !status))) {
        set_error(ctx, "erp_klt_track_rot: null frame, points, rotation or output, or n < 0");
        return VIO_EINVAL;
    }
    return klt_track_once(ctx, prev, curr, W, H, stride, pts, n, next, status, err, params, seam, nullptr, R_cur_prev,
                          guess_out, "erp_klt_track_rot");
}

int erp_klt_track_fb(vio_ctx* ctx, const uint8_t* prev, const uint8_t* curr, int W, int H, int stride,
                     const float* pts, const float* guess, int n, float* next, uint8_t* status, float* err,
                     float* back, uint8_t* fb_state, float* fb_d2, const erp_klt_params* params, int seam,
                     const erp_fb_params* fb) {
    if (!ctx) return VIO_EINVAL;
    if (!prev || !curr || n < 0 || (n > 0 && (!pts || !next || !status))) {
        set_error(ctx, "erp_klt_track_fb: null frame, points or output, or n < 0");
        return VIO_EINVAL;
    }
    const FbOut fbo{fb, back, fb_state, fb_d2};
    return klt_track_once(ctx, prev, curr, W, H, stride, pts, n, next, status, err, params, seam, guess, nullptr,
                          nullptr, "erp_klt_track_fb", &fbo);
}

int erp_predict_from_preint(const vio_preint* pre, const float* T_BC, float R_cur_prev[9]) {
    if (!pre || !T_BC || !R_cur_prev) return VIO_EINVAL;
    float Rbc[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) Rbc[3 * i + j] = T_BC[4 * i + j];
    if (!is_rotation(pre->delta_R) || !is_rotation(Rbc)) return VIO_EINVAL;
    // R_cur_prev = R_BC^T delta_R^T R_BC in f64, rounded once
    double M[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double s = 0.0;
            for (int k = 0; k < 3; ++k) s += (double)pre->delta_R[3 * k + i] * (double)Rbc[3 * k + j];
            M[3 * i + j] = s;  // delta_R^T R_BC
        }
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double s = 0.0;
            for (int k = 0; k < 3; ++k) s += (double)Rbc[3 * k + i] * M[3 * k + j];
            R_cur_prev[3 * i + j] = (float)s;
        }
    return VIO_OK;
}

int erp_gftt(vio_ctx* ctx, const uint8_t* img, const uint8_t* mask, int W, int H, int stride, int max_corners,
             double quality, double min_dist, float* out_xy, int* n_out) {
    return erp_gftt_seam(ctx, img, mask, W, H, stride, max_corners, quality, min_dist, out_xy, n_out, VIO_SEAM_CUT);
}

int erp_gftt_seam(vio_ctx* ctx, const uint8_t* img, const uint8_t* mask, int W, int H, int stride, int max_corners,
                  double quality, double min_dist, float* out_xy, int* n_out, int seam) {
    if (!ctx || !img || !n_out || W < 3 || H < 3 || quality <= 0 || min_dist < 0 || max_corners < 0) return VIO_EINVAL;
    int rc = seam_mode_ok(ctx, seam, W, H, 3, 0, min_dist, "erp_gftt_seam");
    if (rc) return rc;
    if (max_corners == 0) max_corners = W * H;  // "no limit"
    VIO_DEVICE(ctx);
    erp_tracker* t = nullptr;
    rc = tracker_new(ctx, W, H, 1, max_corners, 3, &t);  // down to the W, H >= 3 checked above
    if (rc) return rc;
    t->seam = seam;
    uint8_t* dmask = nullptr;
    if (!(rc = upload_frame(t, 1, img, stride))) {
        if (mask) {
            if (!(rc = dalloc(t, &dmask, (size_t)t->lp[0] * H))) {
                rc = upload_rows(ctx, dmask, t->lp[0], mask, stride, W, H);
            }
        }
        GfttPlan plan;
        if (!rc) rc = gftt_plan(t, dmask, t->lp[0], max_corners, quality, min_dist, 0, 0.f, false, false, &plan);
        if (!rc) rc = enqueue_gftt(t, plan);
        if (!rc) rc = read_corners(t, out_xy, n_out);  // reports a candidate-buffer overflow
    }
    erp_tracker_destroy(t);
    return rc;
}

int erp_rot_ransac(vio_ctx* ctx, const float* p0, const float* p1, int n, int W, int H, const int32_t* samples,
                   int iters, float thresh_rad, uint8_t* mask, int* n_in) {
    if (!ctx || n < 0 || !mask || !n_in || iters < 0 || (n >= 3 && iters > 0 && !samples) || (n > 0 && (!p0 || !p1)))
        return VIO_EINVAL;
    if (n < 3) {  // FeatureTracker.cpp:130-134 / :258-260
        for (int i = 0; i < n; ++i) mask[i] = 1;
        *n_in = n;
        return VIO_OK;
    }
    for (int i = 0; i < 3 * iters; ++i)
        if (samples[i] < 0 || samples[i] >= n) { set_error(ctx, "RANSAC sample index out of range"); return VIO_EINVAL; }
    VIO_DEVICE(ctx);
    erp_tracker* t = nullptr;
    int rc = erp_tracker_create(ctx, std::max(W, 8), std::max(H, 8), n, 0, &t);
    if (rc) return rc;
    t->W = W; t->H = H;
    float* d_p1 = nullptr;
    if (!(rc = ensure_iters(t, std::max(iters, 1))) && !(rc = dalloc(t, &d_p1, sizeof(float) * 2 * n))) {
        hipStream_t st = ctx->stream;
        if (hipMemcpyAsync(t->d_pts, p0, sizeof(float) * 2 * n, hipMemcpyHostToDevice, st) != hipSuccess ||
            hipMemcpyAsync(d_p1, p1, sizeof(float) * 2 * n, hipMemcpyHostToDevice, st) != hipSuccess ||
            (iters && hipMemcpyAsync(t->d_samples, samples, sizeof(int32_t) * 3 * iters, hipMemcpyHostToDevice, st) !=
                          hipSuccess)) {
            rc = hip_fail(ctx, hipErrorUnknown, "ransac upload");
        } else {
            RansacArgs r = ransac_args(t, n, 0, iters, 0, thresh_rad, 0.f, 0, t->d_pts, d_p1);
            hipError_t e = launch_ransac_parts(r, false, true, st);
            if (e == hipSuccess) e = hipStreamSynchronize(st);
            if (e != hipSuccess) rc = hip_fail(ctx, e, "ransac kernels");
            else if (hipMemcpy(mask, t->d_kept, n, hipMemcpyDeviceToHost) != hipSuccess ||
                     hipMemcpy(n_in, t->d_scal + TS_N_IN, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess)
                rc = hip_fail(ctx, hipErrorUnknown, "ransac download");
        }
    }
    erp_tracker_destroy(t);
    return rc;
}

// ---- known-rotation epipolar RANSAC (epipolar.hip) ----

int erp_epi_check(const erp_epi_params* p) {
    if (!p || (p->mode != VIO_EPI_OFF && p->mode != VIO_EPI_ON) || p->iters < 0 || p->iters > kMaxIters ||
        p->min_support < 0)
        return VIO_EINVAL;
    const float half_pi = (float)(M_PI / 2);
    for (const float a : {p->epi_thresh_rad, p->rot_thresh_rad, p->max_parallax_rad, p->min_plane_angle_rad})
        if (!(a > 0.f && a < half_pi)) return VIO_EINVAL;  // (a NaN fails both)
    return VIO_OK;
}

int erp_epi_ransac(vio_ctx* ctx, const float* p0, const float* p1, int n, int W, int H, const float* R,
                   const int32_t* samples, int iters, const erp_epi_params* params, uint8_t* mask, int* n_inliers,
                   int32_t* counts, erp_epi_info* info) {
    if (!ctx || n < 0 || W <= 0 || H <= 0 || !mask || !n_inliers || !info || iters < 0 || iters > kMaxIters ||
        (n > 0 && (!p0 || !p1)))
        return VIO_EINVAL;
    int rc = epi_params_ok(ctx, params, "erp_epi_ransac");
    if (rc) return rc;
    if (R && !is_rotation(R)) { set_error(ctx, "erp_epi_ransac: R is not a rotation"); return VIO_EINVAL; }
    const int used = R ? 2 : 3;  // indices of a sample row that are read
    const bool sampled = n >= used && iters > 0;
    if (sampled && !samples) return VIO_EINVAL;
    for (int i = 0; counts && i < iters; ++i) counts[i] = -1;
    std::memset(info, 0, sizeof *info);
    info->best = -1;
    if (n == 0 || (!R && n < 3)) {  // no rotation to test against: everything is kept, as erp_rot_ransac does
        for (int i = 0; i < n; ++i) mask[i] = 1;
        *n_inliers = info->n_rot = n;
        return VIO_OK;
    }
    for (int it = 0; sampled && it < iters; ++it)
        for (int s = 0; s < used; ++s)
            if (samples[3 * it + s] < 0 || samples[3 * it + s] >= n) {
                set_error(ctx, "erp_epi_ransac: sample index out of range");
                return VIO_EINVAL;
            }
    VIO_DEVICE(ctx);
    erp_tracker* t = nullptr;
    rc = erp_tracker_create(ctx, std::max(W, 8), std::max(H, 8), n, 0, &t);
    if (rc) return rc;
    t->W = W; t->H = H;
    float* d_p1 = nullptr;
    if (!(rc = ensure_iters(t, std::max(iters, 1))) && !(rc = ensure_epi(t)) &&
        !(rc = dalloc(t, &d_p1, sizeof(float) * 2 * n))) {
        hipStream_t st = ctx->stream;
        if (hipMemcpyAsync(t->d_pts, p0, sizeof(float) * 2 * n, hipMemcpyHostToDevice, st) != hipSuccess ||
            hipMemcpyAsync(d_p1, p1, sizeof(float) * 2 * n, hipMemcpyHostToDevice, st) != hipSuccess ||
            (sampled && hipMemcpyAsync(t->d_samples, samples, sizeof(int32_t) * 3 * iters, hipMemcpyHostToDevice, st) !=
                            hipSuccess)) {
            rc = hip_fail(ctx, hipErrorUnknown, "epipolar upload");
        } else {
            // (rows that are not read are not uploaded: no hypothesis kernel runs on them)
            RansacArgs r = ransac_args(t, n, 0, sampled ? iters : 0, 0, params->rot_thresh_rad, 0.f, 0, t->d_pts, d_p1);
            hipError_t e = launch_ransac_parts(r, false, !R, st);
            if (e == hipSuccess) e = launch_epipolar(epi_args(t, r, *params, r.iters, 2, R), st);
            if (e == hipSuccess) e = hipStreamSynchronize(st);
            int have = 0;
            if (e != hipSuccess) rc = hip_fail(ctx, e, "epipolar kernels");
            else if (hipMemcpy(mask, t->d_kept, n, hipMemcpyDeviceToHost) != hipSuccess ||
                     hipMemcpy(n_inliers, t->d_scal + TS_N_IN, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess ||
                     hipMemcpy(&have, t->d_epi_scal + ES_HAVE_R, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess ||
                     (counts && have && r.iters > 0 &&
                      hipMemcpy(counts, t->d_epi_count, sizeof(int) * r.iters, hipMemcpyDeviceToHost) != hipSuccess))
                rc = hip_fail(ctx, hipErrorUnknown, "epipolar download");
            else rc = epi_read_info(t, info);
        }
    }
    erp_tracker_destroy(t);
    return rc;
}

int erp_tracker_set_epipolar(erp_tracker* t, const erp_epi_params* params) {
    if (!t) return VIO_EINVAL;
    const int rc = epi_params_ok(t->ctx, params, "erp_tracker_set_epipolar");
    if (rc) return rc;
    t->epi = *params;
    return VIO_OK;
}

int erp_tracker_download_epi(erp_tracker* t, erp_epi_info* info) {
    if (!t) return VIO_EINVAL;
    if (!info || !t->epi_valid) {
        set_error(t->ctx, info ? "erp_tracker_download_epi: the last run had the epipolar stage off"
                               : "erp_tracker_download_epi: null info");
        return VIO_EINVAL;
    }
    VIO_DEVICE(t->ctx);
    return epi_read_info(t, info);
}

// ---- seam mode ----

int erp_tracker_set_seam(erp_tracker* t, int seam) {
    if (!t) return VIO_EINVAL;
    if (seam != VIO_SEAM_CUT && seam != VIO_SEAM_WRAP) {
        set_error(t->ctx, "erp_tracker_set_seam: unknown seam mode");
        return VIO_EINVAL;
    }
    t->seam = seam;
    return VIO_OK;
}

// ---- region masks (mask.h; the kernels in mask.hip) ----

// d_src: a DEVICE mask (W x H), or with a warp its source-space mask or null
static int tracker_build_mask(erp_tracker* t, const uint8_t* d_src, int W, int H, long long stride, erp_warp* w,
                              const erp_mask_params* p) {
    int rc;
    if (!t->d_static) {
        if ((rc = dalloc(t, &t->d_static, sizeof(uint32_t) * t->disc_words * t->H))) return rc;
        if ((rc = dalloc(t, &t->d_usable, std::max(t->max_points, 1)))) return rc;
    }
    if ((rc = mask_enqueue(t->ctx, d_src, W, H, stride, w, t->W, t->H, p, t->d_static))) return rc;
    t->has_mask = true;
    return VIO_OK;
}

int erp_tracker_set_mask_device(erp_tracker* t, const uint8_t* dmask, int W, int H, int stride,
                                const erp_mask_params* p) {
    if (!t) return VIO_EINVAL;
    if (!dmask) {
        t->has_mask = false;
        return VIO_OK;
    }
    const int rc = erp_mask_check(W, H, stride, t->W, t->H, t->W, p);
    if (rc) {
        set_error(t->ctx, "erp_tracker_set_mask: bad sizes, stride, radius or border mode, or a mask smaller than the frame");
        return rc;
    }
    VIO_DEVICE(t->ctx);
    return tracker_build_mask(t, dmask, W, H, stride, nullptr, p);
}

int erp_tracker_set_mask(erp_tracker* t, const uint8_t* mask, int W, int H, int stride, const erp_mask_params* p) {
    if (!t) return VIO_EINVAL;
    if (!mask) {
        t->has_mask = false;
        return VIO_OK;
    }
    const int rc = erp_mask_check(W, H, stride, t->W, t->H, t->W, p);
    if (rc) {
        set_error(t->ctx, "erp_tracker_set_mask: bad sizes, stride, radius or border mode, or a mask smaller than the frame");
        return rc;
    }
    VIO_DEVICE(t->ctx);
    uint8_t* d_src = nullptr;
    int sp = 0;
    if (int e = mask_stage(t->ctx, mask, W, H, stride, "erp_tracker_set_mask", &d_src, &sp)) return e;
    return tracker_build_mask(t, d_src, W, H, sp, nullptr, p);
}

int erp_tracker_set_mask_warped(erp_tracker* t, erp_warp* w, const uint8_t* src_mask, int stride,
                                const erp_mask_params* p) {
    if (!t || !w) return VIO_EINVAL;
    vio_ctx* ctx = t->ctx;
    if (w->ctx != ctx) {
        set_error(ctx, "erp_tracker_set_mask_warped: the warp belongs to another context");
        return VIO_EINVAL;
    }
    const int rc = mask_warp_check(w, src_mask, stride, t->W, t->H, p);
    if (rc) {
        set_error(ctx, "erp_tracker_set_mask_warped: bad stride, radius or border mode, or a warp smaller than the frame");
        return rc;
    }
    VIO_DEVICE(ctx);
    uint8_t* d_src = nullptr;
    int sp = 0;
    if (src_mask)
        if (int e = mask_stage(ctx, src_mask, w->sW, w->sH, stride, "erp_tracker_set_mask_warped", &d_src, &sp)) return e;
    return tracker_build_mask(t, d_src, w->sW, w->sH, sp, w, p);
}

int erp_tracker_get_mask(erp_tracker* t, uint8_t* out, int stride) {
    if (!t || !out || stride < t->W) return VIO_EINVAL;
    if (!t->has_mask) {
        for (int y = 0; y < t->H; ++y) std::memset(out + (size_t)y * stride, 255, t->W);
        return VIO_OK;
    }
    vio_ctx* ctx = t->ctx;
    VIO_DEVICE(ctx);
    uint8_t* d_img = nullptr;
    int ip = 0;
    if (int e = scratch_rows(ctx, kSlotMaskDst, t->W, t->H, 1, "erp_tracker_get_mask", &d_img, &ip)) return e;
    VIO_HIP(ctx, launch_mask_unpack(t->d_static, t->W, t->H, d_img, ip, ctx->stream));
    return fetch_rows(ctx, d_img, ip, out, stride, t->W, t->H);
}

}  // extern "C"
