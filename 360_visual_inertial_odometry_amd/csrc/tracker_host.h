// tracker_host.h — what tracker_host.cpp (the tracker object, its pipeline and the GFTT routes) shares with
// frontend_host.cpp (erp_frontend_*).  Private to csrc/.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <vector>

#include "ctx.h"
#include "epipolar.h"
#include "tracker_types.h"

namespace vio360 {

// How one enqueued detection runs, decided once by gftt_plan and kept on the tracker for read_corners.
enum class GfRoute {
    Map,    // eigenvalue map, masked maximum, candidates: an explicit mask, or seam wrap mode
    Lmax,   // analytic mask: per-tile local maxima (pass 1), then the masked-maximum tail
    Presel  // pipeline: the side stream presorts every local maximum, the tail is one greedy pass over its prefix
};
enum class GfHandoff {
    Counter,  // the presort reaches the greedy pass through a device counter
    Join      // ... through the stream join (VIO_TRK_PRESEL_FLAG=0)
};
struct GfttPlan {
    GfRoute route = GfRoute::Map;
    GfHandoff handoff = GfHandoff::Join;  // (Presel)
    bool pipeline = false;  // erp_tracker_run enqueued the reset (LK launch) and, off the map route, pass 1 (side stream)
    GfArgs g{};             // the run's arguments: reset, pass 1, tail and the fallbacks
    GfArgs pass1{};         // pipeline, off the map route: the side stream's arguments (pass 1, the presort's base)
    GfRoute resolved = GfRoute::Map;  // read_corners: the route that produced the corners now in d_corners
};

// A host frame on its way into a tracker slot: any pixel format and size no smaller than the tracker's, as it is
// or through a warp (then the frame is the warp's sW x sH source, and W, H are not looked at).
struct FrameSrc {
    const uint8_t* img;
    int format, luma, W, H, stride;
    erp_warp* warp;
};

}  // namespace vio360

struct erp_tracker {
    vio_ctx* ctx = nullptr;
    int W = 0, H = 0, max_points = 0, max_corners = 0;
    int nlev = 0;                        // levels allocated (maxLevel + 1 upper bound)
    int lw[vio360::TRK_MAX_LEVELS], lh[vio360::TRK_MAX_LEVELS], lp[vio360::TRK_MAX_LEVELS];
    uint8_t* lvl[2][vio360::TRK_MAX_LEVELS] = {};
    // points
    float *d_pts = nullptr, *d_next = nullptr, *d_err = nullptr, *d_b0 = nullptr, *d_b1 = nullptr;
    float *d_bear0 = nullptr, *d_bear1 = nullptr;  // pipeline: bearings of every input / tracked point (LK launch)
    uint8_t *d_status = nullptr, *d_kept = nullptr;
    int *d_gidx = nullptr, *d_count = nullptr;
    float* d_rot = nullptr;
    int32_t* d_samples = nullptr;
    int iters_cap = 0;
    int n_pts = 0;
    int* d_scal = nullptr;  // device scalars, indexed by TrkScal
    // gftt
    unsigned long long *d_cand = nullptr, *d_cand_sorted = nullptr;
    uint32_t* d_raw = nullptr;  // tempered mt19937 words of the RANSAC seed (side stream)
    float* d_eig = nullptr;     // GFTT min-eigenvalue map (W x H f32)
    unsigned int cand_cap = 0;
    void* d_sort_tmp = nullptr;
    size_t sort_tmp_bytes = 0;
    uint32_t* d_grid = nullptr;
    size_t grid_bytes = 0;
    float* d_corners = nullptr;
    uint32_t* d_disc = nullptr;
    int disc_words = 0;
    int* d_halfw = nullptr;
    int halfw_r = -1;
    // region mask (erp_tracker_set_mask*): its exclusion plane in the disc plane's layout, what the disc plane
    // starts from and what the tracked-point filter tests; d_usable: the front end's per-point flags
    uint32_t* d_static = nullptr;
    bool has_mask = false;
    uint8_t* d_usable = nullptr;
    int seam = VIO_SEAM_CUT;  // erp_tracker_set_seam: VIO_SEAM_WRAP runs every stage on the periodic continuation
    // the prediction of the next LK launch (erp_tracker_set_guess / erp_tracker_set_rotation): enqueue_lk takes
    // the guided instance when one is held and clears it once the launch is enqueued
    int pred = vio360::LK_GUESS_NONE;
    float pred_rot[9] = {};
    float *d_guess = nullptr, *d_guess_out = nullptr;  // [max_points][2]: explicit guesses / start positions used
    bool guess_out_valid = false;                      // the last LK launch was guided and wrote d_guess_out
    // round-trip check (erp_tracker_set_fb): persistent like the seam mode; enqueue_lk takes the FB instance while
    // it is on, so the pipeline and the front end follow it
    erp_fb_params fb{VIO_FB_OFF, 0.5f};
    float *d_back = nullptr, *d_fb_d2 = nullptr;  // [max_points][2] / [max_points]
    uint8_t* d_fb_state = nullptr;                // [max_points] VIO_FB_*
    bool fb_valid = false;                        // the last LK launch ran the check and wrote the three
    // epipolar stage (erp_tracker_set_epipolar): persistent like the round-trip check.  Per-point terms and scalars
    // are allocated on first use (ensure_epi), the per-hypothesis arrays with the others (ensure_iters)
    erp_epi_params epi{};  // mode VIO_EPI_OFF
    float4 *d_epi_pa = nullptr, *d_epi_pn = nullptr;  // [max_points]
    int *d_epi_count = nullptr, *d_epi_resc = nullptr;  // [iters_cap]
    int* d_epi_scal = nullptr;                          // [ES_COUNT]
    bool epi_valid = false;                             // the last run had the stage on
    // GFTT top-K fast path
    unsigned int* d_hist = nullptr;
    unsigned long long *d_topk = nullptr, *d_topk_sorted = nullptr;
    unsigned int topk_cap = 0;
    // presort of every local maximum (pipeline, side stream) and the greedy pass over it after the discs:
    // histogram [GF_BUCKETS], then its scalars (PresortScal)
    unsigned int* d_hist2 = nullptr;
    unsigned long long *d_topk2 = nullptr, *d_topk2_sorted = nullptr;
    vio360::GfttPlan plan;         // the last enqueued detection (enqueue_gftt), resolved by read_corners
    unsigned int presort_gen = 0;  // runs with a counter hand-off: the counter's target is gen x the sort's grid
    int n_exact_tail = 0, n_full_sort = 0;  // fallbacks taken by read_corners (erp_tracker_gftt_fallbacks)
    // local-maximum path: per-tile local maxima, counts, static-region maxima, disc flags
    unsigned long long* d_lmax = nullptr;
    unsigned int* d_lmax_n = nullptr;
    uint32_t* d_tile_max = nullptr;
    uint8_t* d_tile_dirty = nullptr;
    uint32_t* d_tile_kmax = nullptr;
    int tiles_x = 0, tiles_y = 0;
    hipEvent_t ev[6] = {};
    // the GFTT eigenvalue map runs on a side stream, overlapped with pyramids / LK / RANSAC
    hipStream_t side = nullptr;
    hipEvent_t join = nullptr, pyr_done = nullptr;  // side stream: waits for the pyramids / joined before the GFTT tail
    bool stage_timing = true;  // record the per-stage events (each marker costs the stream a few us)
    bool timed_run = false;    // the last run recorded them
    bool ran = false;
    std::vector<void*> allocs;
};

namespace vio360 {

int ensure_iters(erp_tracker* t, int iters);
// CreateFeatureMask's disc half-widths for `radius` in d_halfw (a blocking upload when the radius changes)
int ensure_halfw(erp_tracker* t, int radius);
// R is a rotation: |R^T R - I| <= 1e-3 in every entry and det R > 0 (f64 on the f32 entries)
bool is_rotation(const float R[9]);
// the tracker's next LK launch starts every point at BearingToPixel(R_cur_prev * PixelToBearing(prev))
int tracker_set_rotation(erp_tracker* t, const float R_cur_prev[9], const char* who);
// erp_fb_check with the caller's name in the context's error
int fb_params_ok(vio_ctx* ctx, const erp_fb_params* fb, const char* who);
// erp_epi_check with the caller's name in the context's error
int epi_params_ok(vio_ctx* ctx, const erp_epi_params* p, const char* who);
// the stage's buffers (first use)
int ensure_epi(erp_tracker* t);
// The stage's arguments behind the compaction / rotation RANSAC described by r: `iters` rows of r.samples, R the
// given rotation or null (the rotation RANSAC's best over r.iters hypotheses)
EpiArgs epi_args(erp_tracker* t, const RansacArgs& r, const erp_epi_params& p, int iters, int min_n, const float* R);
// the stage's info of the last launch (waits for the stream)
int epi_read_info(erp_tracker* t, erp_epi_info* info);
int seam_mode_ok(vio_ctx* ctx, int seam, int W, int H, int win, int max_level, double min_dist, const char* who);
// Brings the frame into slot `slot` as the tracker's W x H grey image, all on the context stream.
int tracker_ingest(erp_tracker* t, int slot, const FrameSrc& f, const char* who);
// aux (the tracker pipeline): extra workgroups of the LK launch (LkAux)
int enqueue_lk(erp_tracker* t, const erp_klt_params* p, int n, bool pyr_built = false, const LkAux* aux = nullptr);
RansacArgs ransac_args(erp_tracker* t, int n, int mode, int iters, uint32_t seed, float thr, float polar, int margin,
                       const float* p0, const float* p1);
// The plan of a detection on slot 1: `mask` an explicit device mask or null for the analytic one (polar rows, side
// margins, the region mask, and with `discs` the disc plane); `pipeline`: erp_tracker_run's.  Allocates the
// GFTT buffers on first use; a counter hand-off takes the tracker's next presort generation.
int gftt_plan(erp_tracker* t, const uint8_t* mask, int mask_pitch, int max_corners, double quality, double min_dist,
              int margin, float polar, bool discs, bool pipeline, GfttPlan* out);
// enqueues what the plan leaves for the context stream and stores the plan on the tracker
int enqueue_gftt(erp_tracker* t, const GfttPlan& plan);
// waits for the tracker's last detection, runs the fallbacks its scalars ask for and copies the corners out
int read_corners(erp_tracker* t, float* out_xy, int* n_out);

}  // namespace vio360
