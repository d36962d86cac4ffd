/*
 * vio360.h — C-ABI of the MI355X-native hot path of 93won/360_visual_inertial_odometry.
 *
 * Pure C, caller-owned host buffers, no Eigen/OpenCV/torch types.  Each entry point replaces
 * one reference interface (cited file:line, paths relative to the reference repo root):
 *
 *   vio_ba_solve          Optimizer::RunLocalBA / RunBA / RunFullBA / RunVIBA / SolvePnP
 *                         (src/optimization/Optimizer.h:107-177, Optimizer.cpp:83-966)
 *                         = Ceres::Solve(SPARSE/DENSE_SCHUR, LM) over BAFactor/PnPFactor/
 *                         InertialFactorFixedGravity (src/optimization/Factors.cpp:33-612,1299-1485)
 *                         plus the chi^2 outlier tagging that follows each solve.
 *   vio_ba_solve_batched  many independent windows in one launch (config 4 / §8e).
 *   erp_klt_track         cv::calcOpticalFlowPyrLK call in FeatureTracker::TrackOpticalFlow
 *                         (src/processing/FeatureTracker.cpp:228-251)
 *   erp_gftt              cv::goodFeaturesToTrack call in FeatureTracker::DetectNewFeatures
 *                         (src/processing/FeatureTracker.cpp:208-226)
 *   vio_mono_init_solve   Initializer::TryMonocularInitialization (src/processing/Initializer.cpp:47-291)
 *   vio_window_*          Estimator::CreateKeyframe window slide / TriangulateNewMapPoints
 *                         (src/processing/Estimator.cpp:637-804, 1141-1318)
 *   erp_rot_ransac        FeatureTracker::RejectOutliersRotationRANSAC / EstimateRotation /
 *                         ComputeRotationInliers (src/processing/FeatureTracker.cpp:253-379)
 *
 * The gather of a window from the Frame/MapPoint graph and the write-back rules are the host
 * adapter's job; this ABI sees only flat arrays.
 *
 * Return convention: 0 on success, negative errno-style code on an API error (bad argument,
 * HIP failure).  A numerical failure of the solver is NOT an API error: it is reported through
 * vio_ba_summary.success = 0, exactly like Ceres Solver::Summary::IsSolutionUsable().
 */
#ifndef VIO360_H_
#define VIO360_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VIO360_ABI_VERSION 4

/* ----------------------------------------------------------------------------------------- */
/* error codes                                                                                */
#define VIO_OK 0
#define VIO_EINVAL (-22)   /* bad argument / inconsistent sizes */
#define VIO_ENOMEM (-12)   /* device allocation failed */
#define VIO_EDEVICE (-5)   /* HIP runtime error */
#define VIO_ENOSYS (-38)   /* variant not supported */

/* ----------------------------------------------------------------------------------------- */
/* context = device + stream + device scratch; one per host thread.                          */
typedef struct vio_ctx vio_ctx;

int vio_ctx_create(int device, vio_ctx** out);
/* destroy every batch / tracker / front-end created on the context first: they use its stream */
void vio_ctx_destroy(vio_ctx* ctx);
/* last error message of this context (or of the last failed vio_ctx_create when ctx==NULL) */
const char* vio_ctx_last_error(const vio_ctx* ctx);
int vio_abi_version(void);
/* VIO_OK when every translation unit of this library was compiled against the same layout of its
 * internal cross-TU argument structs (a stale object after a header change is reported as VIO_EDEVICE
 * here and by vio_ctx_create instead of faulting a kernel); needs no GPU */
int vio_layout_check(void);
/* The division-free lane geometry of the window-BA walk kernels, as the packer writes it into a window's
 * descriptor (needs no GPU; for tests): out = { LC = 256 / max(num_kf, 1) landmarks per chunk,
 * ceil(num_lm / LC) chunks, ceil(chunks / group_size) Schur groups, the reciprocal of max(num_kf, 1), the
 * reciprocal of LC }.  vio_ba_walk_div(t, recip) is the kernels' t / d for 0 <= t < 4096 given d's reciprocal
 * (VIO_EINVAL outside that range). */
int vio_ba_walk_geometry(int num_kf, int num_lm, int group_size, int32_t out[5]);
int vio_ba_walk_div(int t, int recip);
/* The LDS of the phase route's Schur kernel for one window shape (needs no GPU; for tests): num_kf keyframes,
 * num_lm landmarks, `tiles` 16-row tiles of the reduced pose system (1..6), group_size landmark chunks per
 * workgroup.  out = { dynamic LDS bytes of the launch, the kernel's static LDS bytes, 1 when the launch takes
 * the staged instance (the group's landmark values and rhs column kept in LDS; chosen only where two
 * workgroups per CU still fit) }. */
int vio_ba_schur_lds(int num_kf, int num_lm, int tiles, int group_size, int32_t out[3]);

/* Window-BA execution route of this context's later solves / batches (the routes give the same
   results to roundoff, each with its own fixed summation order; within a route results do not depend
   on the batch):
   AUTO (default) = the cluster route for batches of up to 32 LocalBA / BA / VIBA windows (when the
   device can hold every workgroup of the batch at once), the phase kernels for larger batches; PnP
   windows always run single-kernel.
   PHASES / SINGLE_KERNEL / CLUSTER force one route for every non-PnP window (CLUSTER falls back to the
   phase kernels when the batch does not fit the device at once). */
#define VIO_BA_ROUTE_AUTO 0
#define VIO_BA_ROUTE_PHASES 1
#define VIO_BA_ROUTE_SINGLE_KERNEL 2
#define VIO_BA_ROUTE_CLUSTER 3
int vio_ctx_set_ba_route(vio_ctx* ctx, int route);

/* Device Lie maths of the BA factors, evaluated for n inputs with the same device code
   the solvers inline, for parity tests against Ceres' rotation known answers
   (thirdparty/ceres-solver/internal/ceres/rotation_test.cc:406-589).  Rotations row-major.
     VIO_LIE_SO3_EXP   in 3 (phi)        -> out 9   SO3d::Exp as the window factors evaluate it
                                                    (LieUtils.cpp:203-219; no re-projection)
     VIO_LIE_SE3_EXP   in 6 ([rho, phi]) -> out 12  SE3d::exp: R (9) | t (3) (LieUtils.cpp:305-333)
     VIO_LIE_IMU_LOG   in 9 (R)          -> out 3   InertialFactorFixedGravity::log_SO3 (Factors.cpp:1507-1519)
     VIO_LIE_SO3D_EXP  in 3              -> out 9   SO3d::Exp + the SO3d constructor's projection (IMU init)
     VIO_LIE_SO3D_LOG  in 9              -> out 3   SO3d::Log with its theta ~ pi branch (LieUtils.cpp:221-273) */
#define VIO_LIE_SO3_EXP 0
#define VIO_LIE_SE3_EXP 1
#define VIO_LIE_IMU_LOG 2
#define VIO_LIE_SO3D_EXP 3
#define VIO_LIE_SO3D_LOG 4
int vio_lie_eval(vio_ctx* ctx, int op, const double* in, int n, double* out);

/* ----------------------------------------------------------------------------------------- */
/* Bundle adjustment / PnP                                                                    */

/* rigid transform, row-major rotation, f64 (reference keeps f32 Eigen::Matrix4f and casts) */
typedef struct {
    double R[9];
    double t[3];
} vio_pose;

/* IMUPreintegration (src/processing/IMUPreintegrator.h:40-69), f32 fields as in the reference */
typedef struct {
    float delta_R[9];   /* row-major */
    float delta_V[3];
    float delta_P[3];
    float J_Rg[9], J_Vg[9], J_Va[9], J_Pg[9], J_Pa[9];
    float cov9[81];     /* covariance.block<9,9>(0,0), row-major */
    float gyro_bias[3];
    float accel_bias[3];
    float _pad[2];
    double dt_total;
} vio_preint;

/* Device evaluation of n InertialFactorFixedGravity factors (Factors.cpp:1299-1485) with the device
   functions the solvers call, for tests against an independent reference: one launch, one 64-lane
   workgroup per factor.  Per factor f: preint[f], gravity[3f..], the raw (f32 -> f64) initial poses
   T_wb_i_init[f] / T_wb_j_init[f] (projected as the solvers' setup projects them), the parameter blocks
   delta_i[6f..] ([rho, phi]), v_i[3f..], bg[3f..], ba[3f..], delta_j[6f..], v_j[3f..].
   out[315 f ..] = sqrt_info (81, row-major 9x9) | r (9) | J (9x12 row-major, columns [v_i | bg | ba | v_j];
   the pose Jacobians are identically zero) from the serial evaluation, then r (9) | J (108) from the
   wave-parallel evaluation. */
int vio_imu_factor_eval(vio_ctx* ctx, int n, const vio_preint* preint, const double* gravity,
                        const vio_pose* T_wb_i_init, const vio_pose* T_wb_j_init, const double* delta_i,
                        const double* v_i, const double* bg, const double* ba, const double* delta_j,
                        const double* v_j, double* out);

/* which Optimizer entry point the problem mirrors (selects constants and fixing rules) */
enum {
    VIO_BA_LOCAL = 0, /* RunLocalBA: pose 0 constant (if observed), marginalised MPs constant,
                         chi2 threshold 5.99146 (Optimizer.cpp:726-966) */
    VIO_BA_FULL = 1,  /* RunBA(fix_first, fix_last): chi2 threshold 5.991 (Optimizer.cpp:304-486) */
    VIO_BA_VI = 2,    /* RunVIBA: + InertialFactorFixedGravity (Optimizer.cpp:493-724) */
    VIO_PNP = 3       /* SolvePnP: pose-only, 4 rounds of outlier tagging (Optimizer.cpp:83-302) */
};

/* Ceres termination types (ceres/types.h), mirrored */
enum { VIO_TERM_CONVERGENCE = 0, VIO_TERM_NO_CONVERGENCE = 1, VIO_TERM_FAILURE = 2 };

/*
 * One window = one Ceres problem.  Observation o links keyframe obs_kf[o] to landmark obs_lm[o]
 * with pixel obs_uv[2o..2o+1] (the f32 Feature::GetPixelCoord()).  Every observation given here
 * becomes one residual block (the adapter already dropped near-boundary features).
 *
 * Constant blocks: kf_const[k] != 0 → pose k is SetParameterBlockConstant; lm_const[l] != 0 →
 * point l constant.  For VIO_PNP all points are constant and lm_const marks *marginalised*
 * MapPoints (never tagged as outliers, Optimizer.cpp:219-220).  For every variant lm_marg[l]
 * marks marginalised MapPoints (exempt from outlier counting / SetBad); may be NULL.
 */
typedef struct {
    int32_t variant;          /* VIO_BA_* */
    int32_t num_kf;           /* K */
    int32_t num_lm;           /* L */
    int32_t num_obs;          /* N */
    double cols, rows;        /* ERP size (CameraParameters) */
    double huber_delta;       /* HuberLoss(δ) — 1.0 in the reference (Optimizer.cpp:28) */
    double info[4];           /* 2x2 information matrix, row-major (identity in the reference) */
    double chi2_threshold;    /* 5.99146 (LocalBA) or 5.991 (BA/VIBA/PnP) */
    const vio_pose* T_cb;     /* K entries: Frame::GetTCB() of each keyframe (raw f32->f64) */
    const vio_pose* T_wb_init;/* K entries: Frame::GetTwb() (raw f32->f64) */
    const uint8_t* kf_const;  /* K */
    const uint8_t* lm_const;  /* L */
    const uint8_t* lm_marg;   /* L, may be NULL */
    const double* lm_xyz;     /* L*3 initial positions (f32 -> f64) */
    const int32_t* obs_kf;    /* N */
    const int32_t* obs_lm;    /* N */
    const float* obs_uv;      /* 2N */
    /* VIO_BA_VI only (else NULL) */
    const vio_preint* preint; /* K entries; preint[k] links keyframe k-1 -> k (entry 0 unused) */
    const uint8_t* preint_valid; /* K; 0 → factor k-1->k missing (RunVIBA skips it) */
    const double* vel;        /* K*3 initial velocities */
    double bg[3], ba[3];      /* initial shared biases */
    double gravity[3];        /* fixed gravity in world */
    /* solver controls */
    int32_t max_iterations;   /* 50 in the reference (Optimizer.cpp:30) */
    int32_t fixed_iterations; /* != 0 → benchmark mode: run exactly max_iterations LM iterations
                                 with all convergence tests disabled */
    int32_t num_rounds;       /* VIO_PNP: outlier rounds (4); ignored otherwise */
    int32_t _pad0;
} vio_ba_problem;

typedef struct {
    int32_t success;          /* Summary::IsSolutionUsable() (and PnP inlier gate) */
    int32_t termination;      /* VIO_TERM_* of the (last) solve */
    int32_t iterations;       /* summary.iterations.size() (PnP: sum over rounds) */
    int32_t num_successful_steps;
    int32_t num_unsuccessful_steps;
    int32_t num_inliers;      /* chi2 <= threshold after the solve */
    int32_t num_outliers;
    int32_t num_bad_lm;       /* MapPoints to SetBad(): inliers==0 && outliers>=2 && !marg */
    double initial_cost;      /* summary.initial_cost (includes fixed cost) */
    double final_cost;        /* summary.final_cost  (PnP: mean inlier chi2 of last round) */
    double fixed_cost;        /* cost of residual blocks whose parameters are all constant */
    double _pad1;
} vio_ba_summary;

/* One entry of Ceres Solver::Summary::iterations (ceres/iteration_callback.h IterationSummary), pushed
   where TrustRegionMinimizer::FinalizeIterationAndCheckIfMinimizerCanContinue pushes it
   (trust_region_minimizer.cc:313-348): iteration 0 (IterationZero :195-229), every valid, invalid
   (HandleInvalidStep :453-486), accepted (HandleSuccessfulStep :806-826) or rejected (:118-129) step;
   an iteration that ends the solve on the parameter / function tolerance is not pushed (:108-114).
   The reference reads Summary::iterations.size() (src/optimization/Optimizer.cpp:481-483). */
typedef struct {
    int32_t iteration;
    int32_t step_is_valid;
    int32_t step_is_successful;
    int32_t _pad;
    double cost;                /* x or candidate cost + fixed cost */
    double cost_change;         /* x_cost - candidate_cost (0 for an invalid step) */
    double gradient_max_norm;   /* |x - Plus(x, -g)|_inf of the last linearisation */
    double step_norm;           /* |x - candidate| */
    double relative_decrease;   /* TrustRegionStepEvaluator::StepQuality */
    double trust_region_radius; /* after the step's radius update */
    double model_cost_change;   /* -(J h)^T (r + J h / 2); not an IterationSummary field (margin analysis) */
} vio_ba_iteration;

/* outputs, caller-owned; any pointer may be NULL if not wanted */
typedef struct {
    vio_pose* T_wb;           /* K: SE3(T_wb_init) * exp(delta) (constant poses: SE3(T_wb_init)) */
    double* lm_xyz;           /* L*3 final point parameters */
    double* obs_chi2;         /* N: compute_chi_square at the solution */
    uint8_t* obs_outlier;     /* N: chi2 > threshold (PnP: also !marginalised) */
    uint8_t* lm_bad;          /* L: SetBad decision */
    double* vel;              /* K*3 (VI) */
    double* bg;               /* 3 (VI) */
    double* ba;               /* 3 (VI) */
    vio_ba_summary* summary;  /* 1 */
    /* per-iteration trace (Summary::iterations): up to trace_cap entries, summary->iterations of them
       (PnP: the rounds' traces one after another); may be NULL */
    vio_ba_iteration* trace;
    int32_t trace_cap;
    int32_t _pad2;
} vio_ba_output;

/* Any window size: windows whose reduced system fits one workgroup (LocalBA / FullBA / PnP with
   K <= 16, VIBA with K <= 10) run on the windowed solver; larger ones (RunBA over hundreds of keyframes,
   RunVIBA beyond 10 keyframes: Optimizer.cpp:304-486, 493-724) on the multi-kernel global path. */
int vio_ba_solve(vio_ctx* ctx, const vio_ba_problem* prob, vio_ba_output* out);

/* n independent windows in ONE device launch (one workgroup per window); problems beyond the windowed
   path's bounds are solved one by one on the global path */
int vio_ba_solve_batched(vio_ctx* ctx, const vio_ba_problem* probs, vio_ba_output* outs, int n);

/*
 * Device-resident batched interface for benchmarking and multi-GPU sharding: upload once,
 * then vio_ba_batch_run() solves all windows from the resident copy with no host transfer.
 */
typedef struct vio_ba_batch vio_ba_batch;
/* windowed path only: VIO_ENOSYS for a window beyond its bounds (K > 16, VIBA K > 10) */
int vio_ba_batch_create(vio_ctx* ctx, const vio_ba_problem* probs, int n, vio_ba_batch** out);
int vio_ba_batch_run(vio_ba_batch* b);          /* async on the context stream */
int vio_ba_batch_sync(vio_ba_batch* b);
/* replace the IMU preintegrations of a VIO_BA_VI batch before the next run: src holds the batch's
   total keyframe count of entries, window after window in creation order (entry k of a window links
   keyframe k-1 -> k; entry 0 unused), from host (on_device = 0) or device memory (on_device = 1,
   e.g. the output of vio_imu_preintegrate_device).  The validity pattern given at creation stays
   in force.  Async on the context stream. */
int vio_ba_batch_set_preint(vio_ba_batch* b, const vio_preint* src, int count, int on_device);
int vio_ba_batch_download(vio_ba_batch* b, vio_ba_output* outs);
/* average device time (ms) of the solver kernel over the runs since the last reset */
int vio_ba_batch_kernel_ms(vio_ba_batch* b, double* avg_ms, int* count);
/* the route the batch's LocalBA / BA / VIBA windows run on (VIO_BA_ROUTE_PHASES / _SINGLE_KERNEL /
   _CLUSTER; fixed at vio_ba_batch_create), and for the cluster route the workgroups per window */
int vio_ba_batch_route(vio_ba_batch* b, int* route, int* workgroups_per_window);
void vio_ba_batch_destroy(vio_ba_batch* b);
/* diagnostics: per-phase shader-clock accounting of the solver kernel (sum over windows of the
   last run; VIO_BA_PROF_SLOTS slots, named in the Python mirror's BaBatch.PHASES) */
int vio_ba_batch_profile(vio_ba_batch* b, int enable);
#define VIO_BA_PROF_SLOTS 32
int vio_ba_batch_phase_cycles(vio_ba_batch* b, unsigned long long* out /* [VIO_BA_PROF_SLOTS] */);

/*
 * Packed per-window result records, for gathering the windows of a sharded batch over RCCL
 * (config 4: 256 windows over 8 GPUs, one ncclAllGather of the records).  A record is
 * self-describing and position-independent: {int32 K, L, N, version; int32 summary[8] (success,
 * termination, iterations, successful, unsuccessful, inliers, outliers, bad MPs); f64 summary[4]
 * (initial, final, fixed cost, 0); f64 T_wb[12K] (R row-major | t); f64 lm_xyz[3L]; f64 vel[3K];
 * f64 bias[6] (bg | ba); u8 obs_outlier[N] in the caller's observation order; u8 lm_bad[L]}, padded
 * to a multiple of 16 bytes.  Every record of a batch takes vio_ba_batch_record_bytes (the largest).
 */
#define VIO_BA_RECORD_VERSION 1
size_t vio_ba_record_bytes(int num_kf, int num_lm, int num_obs);
int vio_ba_batch_record_bytes(vio_ba_batch* b, size_t* bytes);
/* the batch's n records back to back into dst (on_device != 0: a device buffer of this context's
   device, written asynchronously on the context stream by a pack kernel; else host memory, blocking) */
int vio_ba_batch_pack(vio_ba_batch* b, void* dst, int on_device);
/* decode one record (host memory, record_bytes readable bytes) into caller-owned outputs (NULL fields
   skipped; obs_chi2 and trace are not carried: left untouched).  Records arrive from other ranks:
   VIO_EINVAL when the header is malformed or its K/L/N layout does not fit in record_bytes. */
int vio_ba_record_unpack(const void* record, size_t record_bytes, vio_ba_output* out);

/*
 * Problem assembly and write-back of the Optimizer entry points (SURVEY §8 a3 host half / a4) on a
 * flat view of the reference's Frame / Feature / MapPoint graph.  Host-only, no device work.
 *
 * The view holds the frames vector handed to RunBA / RunVIBA / RunLocalBA (window order; for
 * SolvePnP the one frame) and the MapPoints their features reference:
 *   frame f's features are [feat_begin[f], feat_begin[f+1]) in Frame::GetFeatures() order; feature
 *   g has GetPixelCoord() = feat_uv[2g..2g+1], IsValid() = feat_valid[g] (a null Feature: 0) and
 *   GetMapPoint() = feat_mp[g] (an index into the MapPoint table, -1 for none);
 *   MapPoint m has IsBad() = mp_bad[m], IsMarginalized() = mp_marg[m], GetPosition() = mp_pos[3m..];
 *   mp_key[m] orders the MapPoints as the reference's std::set<shared_ptr<MapPoint>> does (pointer
 *   order there, any unique key here, e.g. the MapPoint id); RunLocalBA also walks
 *   MapPoint::GetObservations(): entries [mp_obs_begin[m], mp_obs_begin[m+1]) with the observing
 *   frame's slot in this view (-1: expired weak_ptr or a frame outside the window) and the
 *   feature index inside that frame.
 * IsNearBoundary (Optimizer.cpp:41-46 -> Camera.cpp:134-139): margin > 0 and x < margin or
 * x > width - margin or y < margin or y > height - margin, in f32.
 */
typedef struct {
    int32_t num_frames;
    int32_t num_mappoints;
    const float* frame_Twb;      /* 16 per frame: Frame::GetTwb(), row-major 4x4 */
    const float* frame_Tcb;      /* 16 per frame: Frame::GetTCB(), row-major 4x4 */
    const int32_t* feat_begin;   /* num_frames + 1 */
    const float* feat_uv;
    const uint8_t* feat_valid;
    const int32_t* feat_mp;
    const int64_t* mp_key;
    const uint8_t* mp_bad;
    const uint8_t* mp_marg;
    const float* mp_pos;
    const int32_t* mp_obs_begin; /* num_mappoints + 1 (RunLocalBA only, else may be NULL) */
    const int32_t* mp_obs_frame;
    const int32_t* mp_obs_feat;
    int32_t width, height;       /* Camera / Frame size (CameraParameters cols, rows) */
    int32_t boundary_margin;     /* Optimizer::m_boundary_margin (20, Optimizer.cpp:33) */
    int32_t _pad;
} vio_map_view;

/* vio_ba_gather status (> 0: the reference returns its default, unsuccessful result) */
enum {
    VIO_GATHER_OK = 0,
    VIO_GATHER_FEW_FRAMES = 1,   /* frames.size() < 2 (Optimizer.cpp:307-310, 497-500, 729-732) */
    VIO_GATHER_NO_MAPPOINTS = 2, /* mappoints.empty() (:328-331, 519-522, 757-760) */
    VIO_GATHER_FEW_OBS = 3       /* SolvePnP: observations.size() < 6 (:127-130) */
};

/* The assembled problem, caller-owned arrays.  Capacities: landmarks <= num_mappoints; observations
   <= feat_begin[num_frames] (RunBA / RunVIBA / SolvePnP) or mp_obs_begin[num_mappoints] (RunLocalBA). */
typedef struct {
    int32_t status;              /* VIO_GATHER_* */
    int32_t num_lm, num_obs;
    int32_t cap_lm, cap_obs;     /* in */
    int32_t _pad;
    int32_t* lm_mp;              /* cap_lm: landmark -> MapPoint index, std::set order */
    uint8_t* lm_const;           /* cap_lm: SetParameterBlockConstant (RunLocalBA: marginalised) */
    uint8_t* lm_marg;            /* cap_lm: marginalised (exempt from SetBad / PnP outliers) */
    double* lm_xyz;              /* 3 cap_lm: GetPosition() cast to f64 */
    int32_t* obs_kf;             /* cap_obs: frame slot */
    int32_t* obs_lm;             /* cap_obs */
    float* obs_uv;               /* 2 cap_obs */
    int32_t* obs_feat;           /* cap_obs: global feature index g (AddResidualBlock order) */
    uint8_t* kf_const;           /* num_frames */
    uint8_t* kf_in_problem;      /* num_frames: the pose block has a residual (poses_in_problem, :848-852) */
    vio_pose* T_wb_init;         /* num_frames (may be NULL): GetTwb().cast<double>() */
    vio_pose* T_cb;              /* num_frames (may be NULL): GetTCB().cast<double>() */
} vio_ba_gather_out;

/* MapPoint / frame collection + residual-block filters of one entry point (variant VIO_BA_LOCAL:
   Optimizer.cpp:726-851; VIO_BA_FULL: :303-409 with fix_first / fix_last; VIO_BA_VI: :493-636
   (fix_first; the IMU factors, velocities and biases are the caller's direct copies); VIO_PNP:
   :83-130, frame 0 only, every MapPoint constant).  Fills `out` and returns VIO_OK (check
   out->status) or VIO_EINVAL. */
int vio_ba_gather(const vio_map_view* map, int variant, int fix_first, int fix_last, vio_ba_gather_out* out);

/* What the entry point writes back into the graph after the solve (caller-owned arrays; NULL
   skipped).  Frames: SetTwb(T.matrix().cast<float>()) where frame_set; VIO_BA_VI: SetVelocity for
   every frame, SetGyroBias / SetAccelBias (bias = gyro | accel) for every frame.  MapPoints:
   SetBad() where mp_set_bad, SetPosition() where mp_set.  result: BAResult / PnPResult fields. */
typedef struct {
    float* frame_Twb;            /* 16 per frame, row-major */
    uint8_t* frame_set;          /* num_frames */
    float* frame_vel;            /* 3 per frame */
    float* bias;                 /* 6 */
    float* mp_pos;               /* 3 per MapPoint */
    uint8_t* mp_set;             /* num_mappoints */
    uint8_t* mp_set_bad;         /* num_mappoints */
    int32_t success, num_inliers, num_outliers, num_poses_optimized, num_points_optimized, num_iterations;
    double initial_cost, final_cost;
} vio_ba_map_update;

/* Write-back rules (RunBA :459-474, RunVIBA :684-712, RunLocalBA :917-954, SolvePnP :272-297): `g`
   is the gather of the same view and variant, `res` the solver's output for the problem built from
   it (T_wb, lm_xyz, lm_bad, summary; vel/bg/ba for VIO_BA_VI).  A gather with status > 0 writes
   nothing and gives the reference's default result. */
int vio_ba_write_back(const vio_map_view* map, int variant, const vio_ba_gather_out* g, const vio_ba_output* res,
                      vio_ba_map_update* upd);

/* ----------------------------------------------------------------------------------------- */
/* ERP feature tracking                                                                       */

typedef struct {
    int32_t win;              /* LK window (21, FeatureTracker.cpp:33) */
    int32_t max_level;        /* 3 */
    int32_t max_iters;        /* 30 */
    float epsilon;            /* 0.01 (criteria.epsilon; squared internally) */
    float min_eig_threshold;  /* 0.01 (the reference passes epsilon here, :240) */
    int32_t _pad;
} erp_klt_params;

/* prev/curr: u8 W x H, row stride `stride` bytes, host memory.  Returns next/status/err. */
int erp_klt_track(vio_ctx* ctx, const uint8_t* prev, const uint8_t* curr, int W, int H, int stride,
                  const float* pts, int n, float* next, uint8_t* status, float* err,
                  const erp_klt_params* params);

/* goodFeaturesToTrack(img, max_corners, quality, min_dist, mask, blockSize 3, useHarris false).
   mask may be NULL and shares the image's row stride.  W, H >= 3.  out_xy holds up to max_corners float2
   (W * H for max_corners 0: no limit), *n_out the count. */
int erp_gftt(vio_ctx* ctx, const uint8_t* img, const uint8_t* mask, int W, int H, int stride,
             int max_corners, double quality, double min_dist, float* out_xy, int* n_out);

/* rotation-only RANSAC on ERP bearings with an injected sample stream (iters*3 indices, each
   triple distinct, as FeatureTracker.cpp:280-288 draws them).  mask[n] = best hypothesis' inliers
   (all ones when no hypothesis has an inlier), *n_in = its inlier count. */
int erp_rot_ransac(vio_ctx* ctx, const float* p0, const float* p1, int n, int W, int H,
                   const int32_t* samples, int iters, float thresh_rad, uint8_t* mask, int* n_in);

/* the reference's RANSAC sample stream made deterministic: std::mt19937(seed) +
   std::uniform_int_distribution<>(0, n-1), three distinct indices per iteration
   (FeatureTracker.cpp:273-288; the reference seeds from std::random_device).  Host-only helper. */
int erp_ransac_samples(uint32_t seed, int n, int iters, int32_t* out);

/* ------------------------------------------------------------------------------------------ */
/* Device-resident frame pipeline = the numeric part of FeatureTracker::TrackFeatures
   (FeatureTracker.cpp:61-206) for one frame pair, all on the GPU with no host round trip:
     pyramids of both frames -> pyramidal LK of the previous frame's points -> status / polar /
     boundary filter (:117-126) -> rotation RANSAC on the survivors with the in-pipeline sample
     stream of erp_ransac_samples(ransac_seed, n_good, ransac_iters) (:130-134) -> GFTT
     re-detection on the current frame masked by polar ∧ boundary ∧ discs of radius
     (int)min_dist around the kept points (CreateFeatureMask :386-402, DetectNewFeatures :208-226).
   The host-side feature bookkeeping between those steps in the reference (RemoveClusteredFeatures,
   Frame::LimitFeaturesPerGrid, feature ids) is the adapter's job; the in-pipeline
   disc mask is built from every kept point. */
typedef struct erp_tracker erp_tracker;
int erp_tracker_create(vio_ctx* ctx, int W, int H, int max_points, int max_corners, erp_tracker** out);
/* copy a host frame into slot 0 (prev) or 1 (curr); erp_tracker_device_frame gives the device
   buffer of a slot (pitch *pitch bytes) for producers that write frames on the device */
int erp_tracker_upload(erp_tracker* t, int slot, const uint8_t* img, int stride);
int erp_tracker_device_frame(erp_tracker* t, int slot, uint8_t** dev_ptr, int* pitch);
/* the demo's frame path (app/main.cpp:199-204): upload a W x H u8 camera frame and resize it on the
   device with INTER_AREA (erp_resize_area_any_device) into slot's tracker resolution; any downscale
   (enlarging is VIO_ENOSYS), a frame already at tracker resolution is uploaded as is */
int erp_tracker_upload_resized(erp_tracker* t, int slot, const uint8_t* img, int W, int H, int stride);
/* swap slots 0 and 1 (the current frame becomes the previous one, m_prev_image = current) */
int erp_tracker_swap(erp_tracker* t);
typedef struct {
    int32_t ransac_iters;     /* 1000 (FeatureTracker.cpp:36) */
    float ransac_thresh_rad;  /* 2 deg (:37, 2.0f * M_PI / 180.0f) */
    uint32_t ransac_seed;     /* seed of the in-pipeline mt19937 sample stream */
    int32_t max_corners;      /* goodFeaturesToTrack maxCorners (feature_detection.max_features) */
    double quality;           /* qualityLevel (0.01) */
    double min_dist;          /* minDistance (30); disc radius (int)min_dist */
    int32_t boundary_margin;  /* camera.boundary_margin (20) */
    float polar_ratio;        /* 0.15 (Camera::CreatePolarMask / IsInPolarRegion default) */
} erp_tracker_params;
/* previous-frame points (pixel coordinates) to track */
int erp_tracker_set_points(erp_tracker* t, const float* pts, int n);
/* enqueue the whole pipeline on the context stream (asynchronous) */
int erp_tracker_run(erp_tracker* t, const erp_klt_params* klt, const erp_tracker_params* p);
int erp_tracker_sync(erp_tracker* t);
/* results of the last run: per input point next position, LK status and kept flag
   (status ∧ !polar ∧ !boundary ∧ RANSAC inlier); the new corners (≤ max_corners float2) */
int erp_tracker_download(erp_tracker* t, float* next, uint8_t* status, uint8_t* kept, float* corners,
                         int* n_corners);
/* device time (ms) of the pipeline stages of the last run (the stage values are -1 when the run did not
   record its stage events, see erp_tracker_set_stage_timing; total_ms is always measured) */
int erp_tracker_stage_ms(erp_tracker* t, double* pyr_ms, double* lk_ms, double* ransac_ms, double* gftt_ms,
                         double* total_ms);
/* on (default): runs record the per-stage events; off: only the pipeline's start and end (each event
   marker costs the stream a few microseconds) */
int erp_tracker_set_stage_timing(erp_tracker* t, int on);
/* GFTT fallbacks taken by erp_tracker_download since the tracker was created: exact_tail = runs whose greedy
   pass over the presorted local maxima could not decide (the masked-maximum tail ran after the download's
   sync), full_sort = runs whose top-K candidate prefix could not decide (every candidate sorted) */
int erp_tracker_gftt_fallbacks(erp_tracker* t, int* exact_tail, int* full_sort);
void erp_tracker_destroy(erp_tracker* t);

/* ------------------------------------------------------------------------------------------ */
/* FeatureTracker::TrackFeatures as a whole (src/processing/FeatureTracker.cpp:61-206): the device
   numeric path above plus the reference's host bookkeeping — feature ids (survivors keep theirs,
   new detections take m_next_feature_id++ in GFTT order), track counts / ages,
   RemoveClusteredFeatures (:404-497, gated by visualization.highlight_clustered_grid),
   Frame::AssignFeaturesToGrid / LimitFeaturesPerGrid (src/database/Frame.cpp:108-202, std::sort by
   track count) and CreateFeatureMask discs (:386-402).  One object per camera stream. */
typedef struct erp_frontend erp_frontend;
typedef struct {
    int32_t max_features;         /* feature_detection.max_features (1000) */
    float min_distance;           /* feature_detection.min_distance (30) */
    float quality_level;          /* feature_detection.quality_level (0.01) */
    int32_t boundary_margin;      /* camera.boundary_margin (20) */
    int32_t grid_cols, grid_rows; /* Frame grid: feature_detection.grid_cols/rows (20, 10) */
    int32_t max_features_per_grid;/* feature_detection.max_features_per_grid (10) */
    int32_t remove_clustered;     /* visualization.highlight_clustered_grid (1) */
    float clustered_std_ratio;    /* visualization.clustered_std_ratio (0.25 in the yaml) */
    uint32_t ransac_seed;         /* frame f uses erp_ransac_samples(ransac_seed + f, ...) */
} erp_frontend_params;
int erp_frontend_create(vio_ctx* ctx, int W, int H, const erp_frontend_params* p, erp_frontend** out);
/* process the next frame (u8 W x H); *n_features = features of this frame after the call */
int erp_frontend_track(erp_frontend* f, const uint8_t* img, int stride, int* n_features);
/* the same on a camera-resolution frame (u8 W x H), resized on the device to the front end's size as
   erp_tracker_upload_resized does */
int erp_frontend_track_resized(erp_frontend* f, const uint8_t* img, int W, int H, int stride, int* n_features);
/* current frame's features in Frame order: id, pixel, track count, age (any pointer may be NULL) */
int erp_frontend_features(erp_frontend* f, int32_t* ids, float* xy, int32_t* track_count, int32_t* age, int cap);
/* GetTrackingStats (FeatureTracker.h): features after tracking, new detections of the last frame */
int erp_frontend_stats(erp_frontend* f, int* num_tracked, int* num_detected);
void erp_frontend_destroy(erp_frontend* f);

/* ------------------------------------------------------------------------------------------ */
/* IMU preintegration: the producer of vio_preint, on device.                   */

/* IMUData (src/processing/Estimator.h:32-36) */
typedef struct {
    double timestamp;         /* seconds */
    float ax, ay, az;         /* m/s^2 */
    float gx, gy, gz;         /* rad/s */
} vio_imu_data;

/* IMUPreintegrator noise densities (IMUPreintegrator.cpp:64-67 defaults 1e-4, 1e-3, 1e-6, 1e-5;
   SetNoiseParameters :131-140) */
typedef struct {
    float gyro_noise, accel_noise, gyro_bias_noise, accel_bias_noise;
} vio_imu_noise;

/*
 * IMUPreintegrator::Preintegrate (src/processing/IMUPreintegrator.cpp:143-193, with
 * IntegrateMeasurement :195-236 and UpdateCovariance :238-274) for n intervals in one launch:
 * interval i integrates the samples with t_start[i] <= timestamp < t_end[i] under the biases
 * gyro_bias[3i..], accel_bias[3i..] (the preintegrator's m_gyro_bias / m_accel_bias; NULL = 0).
 * imu[] must be sorted by non-decreasing timestamp (VIO_EINVAL otherwise).  valid[i] = 0 where
 * the reference returns nullptr (no sample in range — a NaN bound keeps none, ±inf bounds compare
 * as usual; out[i] is then zeroed).  cov_bias_diag
 * (n*6, may be NULL) receives covariance(9..14, 9..14)'s diagonal, the random-walk block.
 * noise NULL = the reference defaults.  Blocking; out / valid / cov_bias_diag are host buffers.
 */
int vio_imu_preintegrate(vio_ctx* ctx, const vio_imu_data* imu, int n_imu, const double* t_start,
                         const double* t_end, int n, const float* gyro_bias, const float* accel_bias,
                         const vio_imu_noise* noise, vio_preint* out, uint8_t* valid, float* cov_bias_diag);
/* the same on DEVICE buffers (imu, t_start, t_end, biases, out, valid, cov_bias_diag — the last is
   required here), asynchronous on the context stream; imu must be sorted (not checked) */
int vio_imu_preintegrate_device(vio_ctx* ctx, const vio_imu_data* imu, int n_imu, const double* t_start,
                                const double* t_end, int n, const float* gyro_bias, const float* accel_bias,
                                const vio_imu_noise* noise, vio_preint* out, uint8_t* valid, float* cov_bias_diag);
/* device time (ms) of the last vio_imu_preintegrate[_device] kernel on this context (waits for it) */
int vio_imu_preintegrate_kernel_ms(vio_ctx* ctx, double* ms);

/* ------------------------------------------------------------------------------------------ */
/* IMU initialisation: Optimizer::OptimizeIMUInit (src/optimization/            */
/* Optimizer.cpp:972-1257) — stage 1 gravity direction (2) + scale, stage 2 velocities + shared */
/* biases with BiasPriorFactor (Factors.h:366-396), both over InertialGravityScaleFactor        */
/* (Factors.cpp:981-1293) with HuberLoss(sqrt(16)), DENSE_QR, default Solver::Options.          */
/* Reproduced quirks: the pose blocks are constant zero perturbations in both stages and the    */
/* factor applies SE3d::exp to them without the keyframe poses, so every factor sees identity  */
/* poses (Factors.cpp:1024-1042, Optimizer.cpp:1084-1092); the factor's square-root            */
/* information is built but never applied to the residual.  One workgroup per problem.          */

enum {
    VIO_IMU_INIT_OK = 0,
    VIO_IMU_INIT_FEW_FRAMES = 1,   /* frames.size() < 3 (:977-981) */
    VIO_IMU_INIT_NO_PREINT = 2,    /* a frame after the first lacks its preintegration (:984-989) */
    VIO_IMU_INIT_NO_FACTORS = 3    /* stage 1 kept no factor (0.001 <= dt <= 2.0, :1060-1086) */
};

typedef struct {
    int32_t num_frames;          /* keyframes, 3 .. 64 */
    int32_t max_iterations;      /* per stage: 50 (Solver::Options default) */
    const vio_pose* T_wb;        /* num_frames: GetTwb().cast<double>() (velocity initialisation) */
    const vio_preint* preint;    /* num_frames: entry i = frame i's preintegration from the last keyframe */
    const uint8_t* preint_valid; /* num_frames (entry 0 ignored) */
    double gravity_magnitude;    /* 9.81 */
    double huber_delta;          /* sqrt(16) = 4 */
    double bias_prior_weight;    /* 1.0 */
} vio_imu_init_problem;

typedef struct {
    int32_t success;             /* IMUInitResult::success */
    int32_t status;              /* VIO_IMU_INIT_* */
    int32_t iterations[2];       /* Summary::iterations.size() of stage 1 / 2 */
    int32_t termination[2];      /* VIO_TERM_* of stage 1 / 2 */
    double gravity[3];           /* R_wg (0, 0, -9.81) */
    double Rwg[9];               /* row-major */
    double gravity_dir[2];       /* the stage-1 parameters (theta_x, theta_y) */
    double scale;
    double gyro_bias[3], accel_bias[3];
    double initial_cost;         /* stage 1 Summary::initial_cost */
    double final_cost;           /* stage 2 Summary::final_cost */
    double* velocities;          /* caller-owned 3 * num_frames, may be NULL */
} vio_imu_init_result;

int vio_imu_init_solve(vio_ctx* ctx, const vio_imu_init_problem* probs, vio_imu_init_result* results, int n);

/* ------------------------------------------------------------------------------------------ */
/* Two-view triangulation: Estimator::TriangulateSinglePoint                   */
/* (src/processing/Estimator.cpp:1082-1137) for n candidates in one launch.                   */

/*
 * T_cw: n_poses world-to-camera transforms, 4x4 row-major f32 (the reference's
 * kf->GetTwc().inverse(), Estimator.cpp:1163-1164).  Candidate i triangulates bearings
 * bearings[6i..6i+2] (in camera pose_pair[2i]) and bearings[6i+3..6i+5] (in camera pose_pair[2i+1])
 * (Feature::GetBearing, unit f32).  points: 3n f32; valid[i] = TriangulateSinglePoint's return
 * (|v(3)| >= 1e-10 and a finite point; a candidate whose bearings or poses hold a NaN or an inf is
 * invalid); invalid candidates get point 0 and error 0; pixel_err (2n, may be NULL) = the reprojection angle errors
 * in pixels TriangulateNewMapPoints computes (:1233-1248) with `width` = GetWidth().  Blocking; host
 * buffers.  The 4x4 SVD is an f64 one-sided Jacobi on the f32-built A (reference: Eigen's f32
 * JacobiSVD; the null vector is unique up to sign, which the division cancels).
 */
int vio_triangulate(vio_ctx* ctx, const float* T_cw, int n_poses, const int32_t* pose_pair, const float* bearings,
                    int n, int width, float* points, uint8_t* valid, float* pixel_err);
/* the same on DEVICE buffers, asynchronous on the context stream (no validation of pose_pair) */
int vio_triangulate_device(vio_ctx* ctx, const float* T_cw, int n_poses, const int32_t* pose_pair,
                           const float* bearings, int n, int width, float* points, uint8_t* valid,
                           float* pixel_err);
/* device time (ms) of the last triangulation kernel on this context (waits for it) */
int vio_triangulate_kernel_ms(vio_ctx* ctx, double* ms);

/* ------------------------------------------------------------------------------------------ */
/* Dataset formats and frame preprocessing, app/main.cpp:30-119, 199-204.        */

/* LoadCameraTimestamps (app/main.cpp:30-48): one double per line.  Writes min(cap, count) values,
   *n = count (call with cap = 0 to size the buffer).  VIO_EINVAL if the file cannot be opened. */
int vio_load_camera_timestamps(const char* path, double* out, int cap, int* n);
/* LoadIMUData (app/main.cpp:50-90): header line, then "t,ax,ay,az,gx,gy,gz" rows; malformed rows
   are skipped exactly as the reference skips them.  Same sizing convention. */
int vio_load_imu_csv(const char* path, vio_imu_data* out, int cap, int* n);

/* cv::resize(img, img, Size(dW, dH), 0, 0, INTER_AREA) of a u8 grayscale frame (app/main.cpp:203),
   integer downscale factors only (W % dW == 0, H % dH == 0; else VIO_ENOSYS).  Blocking; host buffers. */
int erp_resize_area(vio_ctx* ctx, const uint8_t* src, int W, int H, int stride, uint8_t* dst, int dW, int dH,
                    int dst_stride);
/* the same for n_frames DEVICE frames (frame f at src + f*stride*H, dst + f*dst_stride*dH), async on
   the context stream */
int erp_resize_area_device(vio_ctx* ctx, const uint8_t* src, int W, int H, int stride, int n_frames, uint8_t* dst,
                           int dW, int dH, int dst_stride);
/* device time (ms) of the last resize kernel on this context (waits for it) */
int erp_resize_area_kernel_ms(vio_ctx* ctx, double* ms);
/* cv::resize(..., INTER_AREA) to any size dW <= W, dH <= H (4096x2048 or 5376x2688 -> 960x480, ...).
   Integer factors on both axes run erp_resize_area's kernels (bitwise the same result); every other size runs
   OpenCV's general area path: per-axis tap tables (computeResizeAreaTab, built on the host in double and cached
   on the context per (W, dW, H, dH)), f32 accumulation in tap order, round half to even.  Enlarging on either
   axis is VIO_ENOSYS.  Blocking; host buffers. */
int erp_resize_area_any(vio_ctx* ctx, const uint8_t* src, int W, int H, int stride, uint8_t* dst, int dW, int dH,
                        int dst_stride);
/* the same for n_frames DEVICE frames (laid out as for erp_resize_area_device), async on the context stream
   (a call with sizes other than the previous general call's first uploads their tap tables and waits for that) */
int erp_resize_area_any_device(vio_ctx* ctx, const uint8_t* src, int W, int H, int stride, int n_frames,
                               uint8_t* dst, int dW, int dH, int dst_stride);
/* host only: one axis' tap table of the general path (ssize -> dsize <= ssize), taps ordered by output index
   and then by source index: output index di[i] += alpha[i] * source index si[i].  Writes min(cap, count) taps,
   *n = count (call with cap = 0 to size the buffers). */
int erp_resize_area_tab(int ssize, int dsize, int32_t* di, int32_t* si, float* alpha, int cap, int* n);

/* Colour and packed-YUV camera frames: luma + INTER_AREA in one pass (csrc/resize.hip).
   Pixel formats, 1 / 3 / 3 / 4 / 4 / 2 / 2 bytes per pixel; alpha is ignored.  YUYV / UYVY (packed 4:2:2, W
   even): the luma byte of pixel x is byte 2x / 2x + 1 of the row, taken as is (OpenCV's COLOR_YUV2GRAY_YUY2 /
   _UYVY); `luma` is ignored, as it is for GRAY8.  NV12 / I420: pass the Y plane as VIO_PIX_GRAY8 with the
   plane's stride. */
enum { VIO_PIX_GRAY8 = 0, VIO_PIX_BGR8 = 1, VIO_PIX_RGB8 = 2, VIO_PIX_BGRA8 = 3, VIO_PIX_RGBA8 = 4,
       VIO_PIX_YUYV = 5, VIO_PIX_UYVY = 6 };
/* Luma rules of the BGR / RGB formats, integer arithmetic only (restatements: OpenCV is not available to this
   project, parity with it is unpinned, as for the resize):
     VIO_LUMA_CVTCOLOR  (3735 B + 19235 G + 9798 R + 16384) >> 15   OpenCV 4.x cvtColor(BGR2GRAY) for u8
     VIO_LUMA_IMREAD    (1868 B +  9617 G + 4899 R +  8192) >> 14   imread(IMREAD_GRAYSCALE) of a colour PNG,
                                                                    the reference's own path (app/main.cpp:162,199)
   Both map (v, v, v) to v; they differ, by 1, on 43 864 of the 2^24 triples. */
enum { VIO_LUMA_CVTCOLOR = 0, VIO_LUMA_IMREAD = 1 };
/* host only: bytes per pixel of a format; VIO_EINVAL for an unknown format */
int erp_pixel_bytes(int format);
/* host only: the luma of n packed pixels (n even for the 4:2:2 formats) */
int erp_luma_u8(int format, int luma, const uint8_t* px, int n, uint8_t* out);
/* erp_resize_area_any of the grey image that the luma rule makes of a packed W x H frame, bit for bit, without
   that image ever being stored (GRAY8: erp_resize_area_any itself).  stride is in bytes, >= W * bytes per pixel.
   dW == W and dH == H converts only.  Enlarging on either axis is VIO_ENOSYS; an unknown format or luma rule, an
   odd W for 4:2:2 and bad sizes are VIO_EINVAL.  Blocking; host buffers. */
int erp_ingest(vio_ctx* ctx, const uint8_t* src, int format, int luma, int W, int H, int stride, uint8_t* dst,
               int dW, int dH, int dst_stride);
/* host only: the argument check of erp_ingest* (one frame) without a context: VIO_OK, or the code they return */
int erp_ingest_check(int format, int luma, int W, int H, int stride, int dW, int dH, int dst_stride);
/* the same for n_frames DEVICE frames (frame f at src + f*stride*H, dst + f*dst_stride*dH), async on the context
   stream; no alignment is required of src or stride.  erp_resize_area_kernel_ms times these launches too. */
int erp_ingest_device(vio_ctx* ctx, const uint8_t* src, int format, int luma, int W, int H, int stride, int n_frames,
                      uint8_t* dst, int dW, int dH, int dst_stride);
/* Execution route of later erp_ingest* calls on this context (diagnostics, tools/ingest_time.py): AUTO picks per
   format and path what measured faster, FUSED always runs the one-pass kernels, TWO_PASS converts
   to a grey plane in a context buffer and runs erp_resize_area_any_device on it, FUSED_BYTES runs the one-pass
   kernels' byte-load variants whatever the format and alignment.  The bytes are the same. */
enum { VIO_INGEST_ROUTE_AUTO = 0, VIO_INGEST_ROUTE_FUSED = 1, VIO_INGEST_ROUTE_TWO_PASS = 2,
       VIO_INGEST_ROUTE_FUSED_BYTES = 3 };
int erp_ingest_set_route(vio_ctx* ctx, int route);
/* erp_tracker_upload_resized for a packed colour / 4:2:2 frame: upload, then erp_ingest_device into slot's frame
   (a convert-only pass when the frame is already at the tracker's size) */
int erp_tracker_upload_pixels(erp_tracker* t, int slot, const uint8_t* img, int format, int luma, int W, int H,
                              int stride);
/* erp_frontend_track_resized for a packed colour / 4:2:2 frame */
int erp_frontend_track_pixels(erp_frontend* f, const uint8_t* img, int format, int luma, int W, int H, int stride,
                              int* n_features);

/* Lens-to-ERP warp: cv::remap(src, dst, map_x, map_y, INTER_LINEAR) restated in exact integer arithmetic and
   fused with the luma rules above (csrc/warp.hip).  The map gives destination pixel (x, y) of a
   dW x dH u8 frame the source coordinate (map_x, map_y)[y * map_stride + x] as float32.  OpenCV is not available
   to this project: parity with it is unpinned, as for the resize and the luma rules; the contract is this text
   and tests/warp_oracle.py, which the GPU matches bitwise.
     quantisation (host, once per map)   q = lrint((double)s * 32.0), round half to even; i = q >> 5 (floor),
                                         a = q & 31; a non-finite map_x or map_y makes the pixel invalid
     borders, per axis                   X_WRAP: tap columns modulo sW (a full ERP source), q reduced to
                                         [0, 32 sW); Y_REPLICATE: tap rows clamped to [0, sH); CONSTANT: a tap
                                         outside the source reads border_value (q clamped to [-32, 32 S], which
                                         changes no result); an invalid pixel is border_value whatever the modes
     taps                                p00 = (ix, iy), p01 = (ix + 1, iy), p10 = (ix, iy + 1), p11 = (ix + 1,
                                         iy + 1), each the luma (erp_luma_u8) of that source pixel; a, b the
                                         fractional bits of x and y
     pixel                               ((32-a)(32-b) p00 + a(32-b) p01 + (32-a)b p10 + ab p11 + 512) >> 10
   (OpenCV's INTER_BITS = 5 fixed-point bilinear weights with the common factor 32 divided out: the four weights
   are exact integers that sum to 1024.)  So warp(frame) == warp(grey(frame)) bit for bit, and the grey image is
   never stored. */
enum { VIO_WARP_X_CONSTANT = 0, VIO_WARP_X_WRAP = 1 };
enum { VIO_WARP_Y_CONSTANT = 0, VIO_WARP_Y_REPLICATE = 2 };
/* device-resident quantised map, bound to a context; destroy it before the context */
typedef struct erp_warp erp_warp;
/* map_stride in floats, >= dW; dH at most 65535; sW x sH the source frame in pixels (each at most 2^25); border_x a VIO_WARP_X_*,
   border_y a VIO_WARP_Y_*, border_value in [0, 255].  Blocking (quantises on the host, uploads the map).  ctx ==
   NULL gives a host-only object (no map is kept) that erp_warp_check and erp_warp_destroy accept and every other
   call refuses with VIO_EINVAL: the argument checks then need no device. */
int erp_warp_create(vio_ctx* ctx, const float* map_x, const float* map_y, int dW, int dH, int map_stride, int sW,
                    int sH, int border_x, int border_y, int border_value, erp_warp** out);
void erp_warp_destroy(erp_warp* w);
/* host only: the quantisation of n coordinates of one axis of size S under border_mode (a VIO_WARP_X_* or
   VIO_WARP_Y_*): q[i], and valid[i] = 0 (with q[i] = 0) for a non-finite coordinate */
int erp_warp_quantize(const float* s, int n, int S, int border_mode, int32_t* q, uint8_t* valid);
/* host only: the argument check of erp_warp_apply* (format, luma, stride in bytes, dst_stride): VIO_OK, or the
   code they return (unknown format or luma rule, odd sW for 4:2:2, stride < sW * bytes per pixel, dst_stride < dW) */
int erp_warp_check(const erp_warp* w, int format, int luma, int stride, int dst_stride);
/* one sW x sH frame of `format` -> dst (dW x dH u8).  Blocking; host buffers. */
int erp_warp_apply(erp_warp* w, const uint8_t* src, int format, int luma, int stride, uint8_t* dst, int dst_stride);
/* the same for n_frames DEVICE frames (frame f at src + f*stride*sH, dst + f*dst_stride*dH) in one launch that
   reads the map once, async on the context stream; no alignment is required of src, stride or dst, and the
   padding of the destination rows is not written */
int erp_warp_apply_device(erp_warp* w, const uint8_t* src, int format, int luma, int stride, int n_frames,
                          uint8_t* dst, int dst_stride);
/* device time (ms) of the last warp launch of this object (waits for it) */
int erp_warp_kernel_ms(erp_warp* w, double* ms);
/* Execution route of later applies of this object (diagnostics, tools/warp_time.py): AUTO loads the two taps of a
   source row as one pair of neighbouring pixels (every format, any alignment; sources one pixel wide run SINGLE),
   SINGLE loads every tap on its own (4-byte pixels: one aligned dword when src and stride are multiples of 4, else
   byte loads).  The bytes are the same. */
enum { VIO_WARP_ROUTE_AUTO = 0, VIO_WARP_ROUTE_SINGLE = 1 };
int erp_warp_set_route(erp_warp* w, int route);

/* Map generators: host only, computed in double, written as float32 map_x / map_y of dW * dH entries (row-major,
   stride dW).  Destination pixel (x, y) has the bearing of Camera::PixelToBearing (src/database/Camera.cpp:22-47)
   at u = x, v = y, no half-pixel offset (as the tracker reads coordinates); R_dst (9 doubles, row-major, NULL =
   identity) rotates it into the source rig frame: b = R_dst * bearing.  Bad sizes or tables are VIO_EINVAL. */
/* a rotated / resampled ERP source: Camera::BearingToPixel (Camera.cpp:49-67) into sW x sH; use with X_WRAP +
   Y_REPLICATE (e.g. R_dst = Rwg of vio_imu_init_solve: a gravity-aligned frame) */
int erp_warp_map_erp(int sW, int sH, const double* R_dst, int dW, int dH, float* map_x, float* map_y);
/* equidistant fisheye lenses (dual-fisheye 360 cameras: two lenses, side by side in one image or one table per
   image).  R is rig -> lens, the lens looks along +Z, X right, Y down: bl = R b, h = hypot(bl.x, bl.y), theta =
   atan2(h, bl.z); the pixel takes the lens of smallest theta among those with theta <= theta_max (ties: lowest
   index): sx = cx + f theta bl.x / h, sy = cy + f theta bl.y / h ((cx, cy) at h = 0); no lens: NaN (invalid).  The
   seam between lenses is hard (no blending). */
typedef struct {
    double R[9];
    double cx, cy, f, theta_max; /* centre (px), focal length (px / rad), half field of view (rad) */
} erp_fisheye_lens;
int erp_warp_map_fisheye(const erp_fisheye_lens* lenses, int n, const double* R_dst, int dW, int dH, float* map_x,
                         float* map_y);
/* cubemap faces, any layout (3x2, 6x1, cross) as a face table: R is rig -> face, the face looks along +Z and
   fills the w x h rectangle at (x0, y0) of the sW x sH source.  The pixel takes the face of largest (R b).z (ties:
   lowest index; NaN if none is positive): u = bx / bz, v = by / bz, with eac != 0 each becomes (4/pi) atan(.)
   (equi-angular cubemap); sx = x0 + (u + 1) w / 2 - 0.5 clamped to [x0, x0 + w - 1], sy likewise: every tap stays
   inside the face.  A face outside the source is VIO_EINVAL. */
typedef struct {
    double R[9];
    int32_t x0, y0, w, h;
} erp_cube_face;
int erp_warp_map_cubemap(const erp_cube_face* faces, int n, int eac, int sW, int sH, const double* R_dst, int dW,
                         int dH, float* map_x, float* map_y);

/* erp_tracker_upload for a frame that needs a warp first: img is the warp's sW x sH source frame (host), and the
   warped frame lands in slot's frame without a host round trip.  A warp of the tracker's size writes the slot
   directly; a larger one (supersampling: a 5.7K fisheye pair taken to 960x480 with bilinear taps alone would
   alias) is warped into a context buffer and erp_resize_area_any_device takes it into the slot, i.e. remap then
   resize(INTER_AREA); a warp smaller than the tracker on either axis is VIO_ENOSYS; a warp of another context is
   VIO_EINVAL. */
int erp_tracker_upload_warped(erp_tracker* t, int slot, erp_warp* w, const uint8_t* img, int format, int luma,
                              int stride);
/* erp_frontend_track on such a frame */
int erp_frontend_track_warped(erp_frontend* f, erp_warp* w, const uint8_t* img, int format, int luma, int stride,
                              int* n_features);

/* Contrast equalisation of a u8 frame on the device: cv::equalizeHist and cv::CLAHE::apply (8-bit) restated
   (csrc/equalize.hip).  KLT front ends apply one of them to the frame before tracking; the reference
   does not, so it is off unless asked for.  OpenCV is not available to this project: parity with it is unpinned,
   as for the resize, the luma rules and the warp; the contract is this text and tests/equalize_oracle.py, which the
   GPU matches bitwise.  All float arithmetic is float32, each operation rounded on its own (no FMA), division
   correctly rounded; round() is round half to even, then a clamp to [0, 255].
     VIO_EQ_HIST   hist[256] over the W x H frame, i0 its first non-empty bin.  hist[i0] == W H: every pixel is i0.
                   Otherwise scale = 255.f / (float)(W H - hist[i0]), lut[i <= i0] = 0, and for i > i0:
                   sum += hist[i], lut[i] = round((float)sum * scale); dst = lut[src].
     VIO_EQ_CLAHE  tiling: tiles_x x tiles_y tiles over the frame if W % tiles_x == 0 and H % tiles_y == 0; else over
                   the frame extended on the right by tiles_x - W % tiles_x columns and at the bottom by tiles_y -
                   H % tiles_y rows with BORDER_REFLECT_101 (both axes as soon as one is not divisible: a divisible
                   axis grows by a whole tiles count, as in OpenCV).  tw x th = extended size / tiles, area = tw th.
                   LUT of a tile: its histogram; if clip_limit > 0: c = max((int)(clip_limit * area / 256), 1), the
                   excess above c is cut from each bin and summed, batch = excess / 256, resid = excess - 256 batch,
                   every bin += batch, and if resid > 0 the bins 0, step, 2 step, ... (step = max(256 / resid, 1))
                   get +1 each while i < 256 and resid-- > 0; lut[i] = round((float)cumsum[i] * (255.f / (float)area)).
                   Pixel (x, y) of the W x H frame, v = src: txf = (float)x * (1.f / (float)tw) - 0.5f, tx1 =
                   floor(txf), tx2 = tx1 + 1, xa = txf - (float)tx1, xa1 = 1.f - xa, then tx1 = max(tx1, 0), tx2 =
                   min(tx2, tiles_x - 1); y likewise; dst = round((L[ty1][tx1][v] * xa1 + L[ty1][tx2][v] * xa) * ya1 +
                   (L[ty2][tx1][v] * xa1 + L[ty2][tx2][v] * xa) * ya), in that order.
                   border_x = VIO_EQ_X_WRAP takes tx1 = -1 to tiles_x - 1 and tx2 = tiles_x to 0 instead: the mapping
                   is continuous across the seam of a 360 degree frame.  It needs both axes divisible.
   A call is valid if W, H >= 2, W H <= 2^30, stride and dst_stride >= W, the mode is known and, for CLAHE, 1 <=
   tiles_x <= W / 2, 1 <= tiles_y <= H / 2 (one reflection suffices), clip_limit >= 0 and finite (0 = no clipping),
   border_x known and WRAP only with both axes divisible; otherwise VIO_EINVAL.  VIO_EQ_NONE is a copy. */
enum { VIO_EQ_NONE = 0, VIO_EQ_HIST = 1, VIO_EQ_CLAHE = 2 };
enum { VIO_EQ_X_CLAMP = 0, VIO_EQ_X_WRAP = 1 };
typedef struct {
    int32_t mode;              /* VIO_EQ_* */
    int32_t tiles_x, tiles_y;  /* CLAHE: tilesGridSize (8, 8) */
    int32_t border_x;          /* CLAHE: VIO_EQ_X_* (CLAMP is OpenCV's behaviour) */
    double clip_limit;         /* CLAHE: clipLimit (VINS-style trackers: 3.0) */
} erp_equalize_params;
/* host only: the argument check of erp_equalize* (one frame) without a context: VIO_OK, or VIO_EINVAL */
int erp_equalize_check(const erp_equalize_params* p, int W, int H, int stride, int dst_stride);
/* host only: the LUT rule of one tile of `area` pixels (CLAHE) or of a frame of `area` pixels (HIST; clip_limit is
   ignored; a single-bin frame gives lut[i] = i0 for every i) from its 256-bin histogram */
int erp_equalize_lut(int mode, const uint32_t* hist, int area, double clip_limit, uint8_t* lut);
/* one W x H frame -> dst.  Blocking; host buffers. */
int erp_equalize(vio_ctx* ctx, const uint8_t* src, int W, int H, int stride, const erp_equalize_params* p,
                 uint8_t* dst, int dst_stride);
/* the same for n_frames (at most 65535) DEVICE frames, laid out as erp_resize_area_any_device lays them out (frame f
   at src + f*stride*H, dst + f*dst_stride*H), each equalised on its own, async on the context stream.  No alignment
   is required of src, dst or the strides, and the padding of the destination rows is not written.  dst may be src
   (with dst_stride == stride): the bytes are those of the out-of-place call; any other overlap is undefined.  More
   tiles than one launch holds (2^21 workgroups) is VIO_ENOSYS. */
int erp_equalize_device(vio_ctx* ctx, const uint8_t* src, int W, int H, int stride, int n_frames,
                        const erp_equalize_params* p, uint8_t* dst, int dst_stride);
/* device time (ms) of the last erp_equalize_device launches on this context, all three stages (waits for them) */
int erp_equalize_kernel_ms(vio_ctx* ctx, double* ms);
/* diagnostics (tools/equalize_time.py): on = later launches also record an event between the stages (each marker
   costs the stream a few microseconds; off by default), and erp_equalize_stage_ms gives the last such launch's
   histogram, LUT and apply times (VIO_EINVAL if it recorded none) */
int erp_equalize_set_stage_timing(vio_ctx* ctx, int on);
int erp_equalize_stage_ms(vio_ctx* ctx, double* hist_ms, double* lut_ms, double* apply_ms);
/* equalise slot's frame in place, after any erp_tracker_upload* and before erp_tracker_run; asynchronous */
int erp_tracker_equalize(erp_tracker* t, int slot, const erp_equalize_params* p);
/* equalise every later frame of the front end before anything reads it, whichever erp_frontend_track* brings it
   (upload, resize, luma, warp: all of them compose with it); p == NULL or VIO_EQ_NONE: off (the default; no kernel
   is launched).  The parameters are checked against the front end's size: VIO_EINVAL leaves the setting as it was. */
int erp_frontend_set_equalize(erp_frontend* f, const erp_equalize_params* p);

/* Region masks (csrc/mask.hip): which pixels of a 360 degree frame are not the scene -- the operator,
   the rig, the holes of a dual-fisheye warp, the objects a segmentation network marks per frame.  A usable-region
   mask is a u8 image, nonzero = usable (OpenCV's convention, that of erp_gftt's mask), given at the tracker's size,
   at the camera's, or in the source coordinates of an erp_warp.  It is reduced conservatively to the tracker's size
   on the device, optionally eroded, and held by a tracker or front end as a static exclusion plane.  The reference
   has the hook (FeatureTracker.cpp:47-58 builds m_mask, :117-126 filters) and nothing to put into it.  Everything
   is integer; the contract is this text and tests/mask_oracle.py, which the GPU matches bit for bit.
     reduce   sW x sH -> dW x dH, dW <= sW and dH <= sH (enlarging on either axis: VIO_ENOSYS).  Per axis the
              footprint of destination index d is the set of source indices si with an entry (d, si, alpha) in
              erp_resize_area_tab(ssize, dsize): the taps the frame's own INTER_AREA resize reads.  A destination
              pixel is usable iff every source pixel of footprint_x x footprint_y is nonzero: a tracker pixel that
              contains any excluded camera pixel is excluded.  Equal sizes: the identity.
     erode    radius r in [0, 255], in tracker pixels: usable'(x, y) = AND of usable(x + dx, y + dy) over |dx|,
              |dy| <= r.  Rows outside the image count as usable (cv::erode's default border: the image edge does not
              erode); columns outside count as usable under VIO_MASK_X_CLAMP and are taken modulo dW under
              VIO_MASK_X_WRAP (the seam of a 360 degree frame).  r >= dW or r >= dH is legal, r = 0 a no-op.
     warp     for an erp_warp (destination wW x wH, source sW x sH) and a source-space mask, sW x sH u8 or NULL (every
              source pixel usable): a warp pixel is usable iff its map entry is valid and each of its four taps p00,
              p01, p10, p11 is usable, whatever their weights; a tap column under X_WRAP is taken modulo sW and a tap
              row under Y_REPLICATE is clamped, and the mask is read there; under a CONSTANT border a tap outside the
              source is not usable.  With a NULL mask: no border_value and no invalid pixel enters the output.  A warp
              larger than the plane asked for is then reduced as above, erosion comes last; a warp smaller on either
              axis is VIO_ENOSYS, a warp of another context VIO_EINVAL.
   A call is valid if every size is in [1, 65535], stride >= the source width, dst_stride >= dW, r in [0, 255] and
   border_x known; otherwise VIO_EINVAL.  The output is 0 / 255.
   Held by a tracker or front end, a mask has two effects: (1) the GFTT mask of erp_tracker_run and of the front
   end's first-frame detection and re-detection is polar AND boundary AND usable AND NOT discs; (2) a tracked point
   survives iff status AND NOT polar AND NOT boundary AND usable(xi, yi), xi = (int)rintf(x), yi = (int)rintf(y)
   (round half to even, as the disc centres; a rounded position outside [0, W) x [0, H) is not usable), before
   RANSAC: its sample stream is erp_ransac_samples(seed, n_good, iters) with the new n_good.  Without a mask nothing
   changes and no extra kernel is launched.  Equalisation histograms still see masked pixels and LK still reads
   them: erosion keeps LK windows off the mask's edge. */
enum { VIO_MASK_X_CLAMP = 0, VIO_MASK_X_WRAP = 1 };
typedef struct {
    int32_t erode_radius;  /* r, tracker pixels */
    int32_t border_x;      /* VIO_MASK_X_* */
} erp_mask_params;
/* host only: the argument check of erp_mask_build* without a context: VIO_OK, VIO_EINVAL or VIO_ENOSYS */
int erp_mask_check(int sW, int sH, int stride, int dW, int dH, int dst_stride, const erp_mask_params* p);
/* sW x sH mask -> dW x dH 0 / 255.  Blocking; host buffers. */
int erp_mask_build(vio_ctx* ctx, const uint8_t* mask, int sW, int sH, int stride, int dW, int dH,
                   const erp_mask_params* p, uint8_t* dst, int dst_stride);
/* the same for DEVICE buffers, async on the context stream; no alignment is required of the pointers or the strides
   and the padding of the destination rows is not written.  (The first call with a new pair of sizes uploads the
   footprint tables after draining the stream; later calls with those sizes do not wait.) */
int erp_mask_build_device(vio_ctx* ctx, const uint8_t* mask, int sW, int sH, int stride, int dW, int dH,
                          const erp_mask_params* p, uint8_t* dst, int dst_stride);
/* through a warp: src_mask is sW x sH of the warp's source (host) or NULL; dst is dW x dH, dW <= wW, dH <= wH.
   Blocking. */
int erp_mask_build_warped(erp_warp* w, const uint8_t* src_mask, int stride, int dW, int dH, const erp_mask_params* p,
                          uint8_t* dst, int dst_stride);
/* device time (ms) of the last build's launches on this context, a tracker's or front end's included (waits) */
int erp_mask_kernel_ms(vio_ctx* ctx, double* ms);
/* The tracker's mask: W x H is the tracker's size or larger (a camera-resolution mask is reduced).  mask == NULL
   clears it: back to the maskless pipeline, bitwise.  A failed call leaves the previous mask in place.  Setting or
   clearing applies to every later erp_tracker_run. */
int erp_tracker_set_mask(erp_tracker* t, const uint8_t* mask, int W, int H, int stride, const erp_mask_params* p);
/* the same from a DEVICE mask, async on the context stream and without a host synchronisation (per-frame masks of a
   network on the same GPU); the mask must stay unchanged until the stream has passed the build */
int erp_tracker_set_mask_device(erp_tracker* t, const uint8_t* dmask, int W, int H, int stride,
                                const erp_mask_params* p);
/* the usable region of `w`'s destination (src_mask: host, the warp's source size, or NULL), reduced to the tracker's
   size when the warp is larger: the mask that goes with erp_tracker_upload_warped */
int erp_tracker_set_mask_warped(erp_tracker* t, erp_warp* w, const uint8_t* src_mask, int stride,
                                const erp_mask_params* p);
/* the mask in use as 0 / 255 at the tracker's size (host, stride >= W); all 255 when none is set.  Blocking. */
int erp_tracker_get_mask(erp_tracker* t, uint8_t* out, int stride);
/* the front end's mask: applies to every later frame, whichever erp_frontend_track* brings it, and composes with
   the equalisation; the arguments and rules are those of erp_tracker_set_mask* */
int erp_frontend_set_mask(erp_frontend* f, const uint8_t* mask, int W, int H, int stride, const erp_mask_params* p);
int erp_frontend_set_mask_device(erp_frontend* f, const uint8_t* dmask, int W, int H, int stride,
                                 const erp_mask_params* p);
int erp_frontend_set_mask_warped(erp_frontend* f, erp_warp* w, const uint8_t* src_mask, int stride,
                                 const erp_mask_params* p);

/* Seam mode: an equirectangular frame is a cylinder, column W - 1 is adjacent to column 0.
   VIO_SEAM_CUT (the default) is the reference's flat picture: REFLECT_101 columns, a point whose window leaves the
   frame sideways is lost, boundary_margin columns are cut at the left and right, distances are flat.
   VIO_SEAM_WRAP: every operation of the tracking path is the CUT operation applied to the horizontally periodic
   continuation of the frame, and resulting x coordinates are folded into [0, W).  The y axis keeps every rule.
     pyramids   the pyrDown border columns come from the opposite side of the level
     LK         template, Scharr neighbours and next-frame window take columns modulo the level width; only the y
                parts of the "left the frame" tests remain; the iteration runs in unwrapped coordinates and only the
                final next.x is folded, by one f32 +-W (a fold that rounds to W gives 0; a point further than W
                from the frame, or not a number, is lost: status 0)
     filter     no left / right margin (top, bottom and polar stay); the region mask is read at the folded column
     discs      CreateFeatureMask's disc columns are taken modulo W
     GFTT       Sobel, 3x3 box and 3x3 NMS with wrapped neighbours; no left / right margin; candidates at every
                x in [0, W), y in [1, H - 2]; threshold, sort and tie order unchanged; a candidate is rejected when
                min(|dx|, W - |dx|)^2 + dy^2 < min_dist^2 against an accepted corner
   The front end's grid assignment, RemoveClusteredFeatures and LimitFeaturesPerGrid stay flat (cells at the seam
   are separate cells), and vio_ba_gather still drops observations within its boundary_margin of the left and right
   edges.  Every frame entry (upload, resized, pixels, warped, equalised, masked) composes with the mode.
   erp_seam_check (host only) is the check every WRAP call makes before it launches anything; VIO_EINVAL when
     W is not divisible by 2^top, top = the pyramid level LK really uses for (W, H, win, max_level): only then is
       a wrapped pyrDown the pyrDown of the continuation;
     the top level is narrower than the LK staging tiles (38 columns);
     W <= 2 min_dist (a disc or a min-distance neighbourhood would meet itself);
   or when an argument is out of range.  erp_gftt_seam checks (W, H, 3, 0, min_dist). */
enum { VIO_SEAM_CUT = 0, VIO_SEAM_WRAP = 1 };
int erp_seam_check(int W, int H, int win, int max_level, double min_dist);
/* erp_klt_track / erp_gftt with a seam mode; VIO_SEAM_CUT is erp_klt_track / erp_gftt bit for bit */
int erp_klt_track_seam(vio_ctx* ctx, const uint8_t* prev, const uint8_t* curr, int W, int H, int stride,
                       const float* pts, int n, float* next, uint8_t* status, float* err,
                       const erp_klt_params* params, int seam);
int erp_gftt_seam(vio_ctx* ctx, const uint8_t* img, const uint8_t* mask, int W, int H, int stride,
                  int max_corners, double quality, double min_dist, float* out_xy, int* n_out, int seam);
/* the pipeline's mode, from the next erp_tracker_run on (which then makes the check with its own parameters and
   returns VIO_EINVAL without a launch when it fails).  WRAP runs take the exact route through detection: the
   eigenvalue map, its masked maximum and the candidate sort on the main stream. */
int erp_tracker_set_seam(erp_tracker* t, int seam);
/* the front end's mode, from the next frame on: LK, the boundary filter, the discs and detection follow it.  The
   check is made here, with the front end's LK parameters (21 / 3) and min_distance. */
int erp_frontend_set_seam(erp_frontend* f, int seam);

/* Guided LK: the search of a point starts at a predicted position instead of its previous one, so the
   tracker survives an inter-frame rotation beyond the pyramid's reach (about 40 px per frame at win 21, 3 levels).
     explicit guesses  cv::calcOpticalFlowPyrLK(..., OPTFLOW_USE_INITIAL_FLOW): at the top pyramid level the search
                       starts at guess * (float)(1. / (1 << level)) instead of prev * that; window sums, iteration,
                       status and err rules and the level hand-down next * 2 are unchanged.  guess == pts gives the
                       unguided result bit for bit (in VIO_SEAM_WRAP: for points inside [0, W), see the fold below).
     rotation          R_cur_prev (3x3 f32, row-major) takes a bearing of the previous camera frame into the current
                       one; the guess of a point is BearingToPixel(R_cur_prev * PixelToBearing(prev)) with
                       Camera.cpp:22-67's conventions (theta = atan2(x, z), phi = -asin(y / |b|),
                       u = W (0.5 + theta / 2pi), v = H (0.5 - phi / pi)), formed in f32 on the device by the
                       point's own LK workgroup.  VIO_EINVAL unless R_cur_prev is a rotation: every entry of
                       R^T R - I within 1e-3 and det R > 0.
     seam modes        VIO_SEAM_WRAP folds a guess's x into [0, W) by one f32 +-W (a fold that rounds to W gives 0);
                       VIO_SEAM_CUT takes it as it is, and a guess outside the frame ends the level as the
                       "left the frame" tests end it.
     bad guesses       a guess that is not finite, or lies outside [-W, 2W) x [-H, 2H), counts as absent: that point
                       starts at its previous position.  A DEVIATION from OpenCV, which would index with it; it
                       keeps every tile origin within the ranges the index arithmetic was written for.
     lifetime          on a tracker or a front end a prediction belongs to one frame pair: the next run / track call
                       consumes it and clears it.  Without one every entry point behaves as it always did.
   Argument errors (a null pointer, a wrong n, a non-rotation, an unknown seam mode, a size the seam mode does not
   admit) return VIO_EINVAL before anything is launched. */
/* one-shot, like erp_klt_track_seam; guess[n][2] */
int erp_klt_track_guess(vio_ctx* ctx, const uint8_t* prev, const uint8_t* curr, int W, int H, int stride,
                        const float* pts, const float* guess, int n, float* next, uint8_t* status, float* err,
                        const erp_klt_params* params, int seam);
/* the same, seeded by a rotation; guess_out[n][2] (may be NULL): the start position each point used, after the fold
   and the bad-guess rule */
int erp_klt_track_rot(vio_ctx* ctx, const uint8_t* prev, const uint8_t* curr, int W, int H, int stride,
                      const float* pts, int n, const float R_cur_prev[9], float* next, uint8_t* status, float* err,
                      float* guess_out, const erp_klt_params* params, int seam);
/* device pipeline: for the next erp_tracker_run only.  n must be the erp_tracker_set_points count; the later of
   set_guess / set_rotation wins. */
int erp_tracker_set_guess(erp_tracker* t, const float* guess, int n);
int erp_tracker_set_rotation(erp_tracker* t, const float R_cur_prev[9]);
/* the start positions of the last run [n][2]; VIO_EINVAL when that run had no prediction */
int erp_tracker_download_guess(erp_tracker* t, float* guess);
/* front end: for the next erp_frontend_track* call only (a call that only detects consumes it too) */
int erp_frontend_predict_rotation(erp_frontend* f, const float R_cur_prev[9]);
/* host only: R_cur_prev = R_BC^T * delta_R^T * R_BC from the preintegration between the two frames
   (delta_R = R_b(prev)^T R_b(cur), IMUPreintegrator.cpp:227; T_BC camera-to-body 4x4 row-major,
   T_wc = T_wb * T_BC, Frame.cpp:87), formed in f64 and rounded once.  VIO_EINVAL when delta_R or T_BC's rotation
   block is not a rotation (the test above). */
int erp_predict_from_preint(const vio_preint* between_frames, const float* T_BC, float R_cur_prev[9]);

/* Round-trip check (forward-backward LK; VINS-Fusion's FLOW_BACK): status == 1 only says that the
   window stayed in the frame and was textured.  With the check on, a found point is tracked back into the previous
   frame and kept only if it lands where it started.  Off by default; with it off every entry point is bit for bit
   what it is without this section.  With it on, for every point, inside the point's one LK workgroup:
     forward    the search the call would make without the check (unguided, explicit guess or rotation, either seam
                mode); next, err and guess_out are its results, unchanged.  In VIO_SEAM_WRAP next.x is folded first,
                and a point the fold declares lost counts as forward-lost.
     backward   only for points the forward search found:
                cv::calcOpticalFlowPyrLK(curr, prev, next, back, ..., OPTFLOW_USE_INITIAL_FLOW) with back = pts --
                the template and Scharr derivatives from curr's pyramid at next, the search window from prev's, the
                guess the point's previous position under the guided search's rules (the bad-guess rule, the fold in
                WRAP), the erp_klt_params and the seam mode of the forward search.  It is
                erp_klt_track_guess(curr, prev, next, guess = pts) on the forward-found subset, bit for bit.
     test       f32, no contraction: dx = back.x - pts.x, dy = back.y - pts.y; in WRAP the short way round
                (dx > W/2: dx -= W; dx < -W/2: dx += W; W/2 = (float)W * 0.5f); d2 = dx*dx + dy*dy.  The point
                passes iff the backward status is 1 and d2 <= max_dist * max_dist (an f32 product); a NaN fails.
     results    status = forward AND pass.  fb_state: VIO_FB_NOT_RUN (forward lost), VIO_FB_PASS, VIO_FB_BACK_LOST,
                VIO_FB_TOO_FAR.  back is (0, 0) where the backward search was not run, and where it was run what
                that search returned.  fb_d2 is d2 in squared pixels (no square root: bit-defined), 0 where the
                search was not run or lost the point.  Everything downstream (filter, RANSAC, discs, the front end's
                feature list) sees only status.
   erp_fb_check (host only) is the check every entry point makes before anything is launched: VIO_EINVAL for a null
   pointer, an unknown mode, or a max_dist that is not finite or is negative. */
enum { VIO_FB_OFF = 0, VIO_FB_ON = 1 };
enum { VIO_FB_NOT_RUN = 0, VIO_FB_PASS = 1, VIO_FB_BACK_LOST = 2, VIO_FB_TOO_FAR = 3 };
typedef struct erp_fb_params {
    int32_t mode;   /* VIO_FB_OFF / VIO_FB_ON */
    float max_dist; /* pixels; VINS-Fusion's 0.5 is the usual value */
} erp_fb_params;
int erp_fb_check(const erp_fb_params* fb);
/* one-shot, like erp_klt_track_guess; guess may be NULL (unguided forward search); back[n][2], fb_state[n] and
   fb_d2[n] may each be NULL.  With fb->mode == VIO_FB_OFF it is the unchecked call and the three are not written. */
int erp_klt_track_fb(vio_ctx* ctx, const uint8_t* prev, const uint8_t* curr, int W, int H, int stride,
                     const float* pts, const float* guess, int n, float* next, uint8_t* status, float* err,
                     float* back, uint8_t* fb_state, float* fb_d2, const erp_klt_params* params, int seam,
                     const erp_fb_params* fb);
/* device pipeline: persistent, like erp_tracker_set_seam; erp_tracker_run's LK stage follows it, and composes with
   erp_tracker_set_guess / erp_tracker_set_rotation (which stay one-shot), the seam mode, masks and equalisation */
int erp_tracker_set_fb(erp_tracker* t, const erp_fb_params* fb);
/* the last run's back[n][2], fb_state[n], fb_d2[n] (each may be NULL); VIO_EINVAL when that run had the check off */
int erp_tracker_download_fb(erp_tracker* t, float* back, uint8_t* fb_state, float* fb_d2);
/* front end: from the next frame on */
int erp_frontend_set_fb(erp_frontend* f, const erp_fb_params* fb);
/* the check's counts in the last erp_frontend_track* call: points tracked back, of them lost on the way back, of
   them landed too far (each may be NULL); all zero when that call ran no LK or the check was off */
int erp_frontend_fb_stats(erp_frontend* f, int* checked, int* back_lost, int* too_far);

/* Known-rotation epipolar RANSAC: the rotation test keeps a track when one rotation carries its
   previous bearing to within rot_thresh of its current one, so under translation it drops every near point.  With
   the rotation R = R_cur_prev known (the gyro's, or the rotation RANSAC's best), two-view geometry leaves the
   direction of translation: each track gives one plane through it, two tracks fix it, and every other track is
   tested against its epipolar plane and the direction of flow.  Off by default; with the mode off every entry
   point is bit for bit what it is without this section.  The rule, f32 without contraction, sums in the written
   order:
     inputs     the n points that pass the stage's input filter, their unit bearings b0[k], b1[k] (PixelToBearing of
                the previous and the current pixel), R row-major, iters sample rows (i, j, .) of which the first two
                indices are used, the parameters below.  The thresholds are formed once on the host in double and
                rounded to float: s2_epi = sin^2(epi_thresh_rad), s2_plane = sin^2(min_plane_angle_rad),
                cmax = cos(max_parallax_rad); cmin is the rotation test's cosine bound of rot_thresh_rad (the
                smallest float c with (float)acos((double)c) < rot_thresh_rad).
     per point  a = R b0 (each row (R0*x + R1*y) + R2*z); c = (a0*q0 + a1*q1) + a2*q2 with q = b1;
                nrm = a x q = (a1*q2 - a2*q1, a2*q0 - a0*q2, a0*q1 - a1*q0); nn = (nrm0^2 + nrm1^2) + nrm2^2;
                rin = clamp(c, -1, 1) >= cmin (the rotation test); par_ok = c >= cmax.
     hypothesis (i, j): skipped (count -1) when rin[i] or rin[j], or when, with t = nrm[i] x nrm[j] and
                tt = (t0^2 + t1^2) + t2^2, tt >= s2_plane * (nn[i] * nn[j]) does not hold.  Otherwise every point k
                with !rin[k] and par_ok[k] forms m = t x a[k], mm = (m0^2 + m1^2) + m2^2,
                e = (t0*nrm0 + t1*nrm1) + t2*nrm2, on_plane = mm > 1e-6f * tt && e * e < s2_epi * mm,
                s = -((nrm0*m0 + nrm1*m1) + nrm2*m2), and votes pos when on_plane && s > 0, neg when
                on_plane && s < 0.  rescued = max(pos, neg), sigma = pos >= neg ? +1 : -1,
                count = (number of rin) + rescued.
     selection  the first hypothesis with the strictly greatest count >= 0.  When there is none, or its
                rescued < min_support: mask = rin, model_valid = 0, best = -1 (none) or its index, t_dir = 0.
                Otherwise mask[k] = rin[k] || (on_plane with the sign sigma) under the best t, model_valid = 1 and
                t_dir = -sigma * t / sqrtf(tt): the camera's direction of translation in the current camera frame
                (bearings flow away from it).
     small n    hypotheses are evaluated from n >= 2 in erp_epi_ransac and from n >= 3 in the tracker and the front
                end (their sample stream erp_ransac_samples needs three points); below that, and with iters == 0,
                the result is the rotation mask rin.  Without a given R the rotation RANSAC runs first on the same
                sample rows (all three indices); when it finds no rotation (n < 3, iters == 0, every hypothesis
                degenerate) everything is kept as erp_rot_ransac does, n_rot = the count it reports, best = -1.
   erp_epi_check (host only) is the check every entry point makes before anything is launched: VIO_EINVAL for a null
   pointer, an unknown mode, a negative or NaN field, iters above 65536 (the tracker's hypothesis cap), or an angle
   outside (0, pi/2). */
enum { VIO_EPI_OFF = 0, VIO_EPI_ON = 1 };
typedef struct erp_epi_params {
    int32_t mode;              /* VIO_EPI_OFF / VIO_EPI_ON */
    int32_t iters;             /* hypotheses: the first iters rows of the sample stream (256) */
    float epi_thresh_rad;      /* angle of b1 to the epipolar plane (0.25 deg) */
    float rot_thresh_rad;      /* the rotation test's angle (2 deg) */
    float max_parallax_rad;    /* a rescued track's angle between R b0 and b1 is at most this (20 deg) */
    float min_plane_angle_rad; /* the two sample planes must differ by at least this (1 deg) */
    int32_t min_support;       /* a model needs this many rescued tracks (10) */
} erp_epi_params;
typedef struct erp_epi_info {
    int32_t n_rot;       /* tracks the rotation test keeps (rin) */
    int32_t n_rescued;   /* tracks only the epipolar model keeps (0 when model_valid == 0) */
    int32_t best;        /* the chosen hypothesis, -1: none */
    int32_t model_valid; /* 1: the mask is rin || epipolar; 0: the mask is the rotation stage's */
    float t_dir[3];      /* unit direction of translation, 0 when model_valid == 0 */
} erp_epi_info;
int erp_epi_check(const erp_epi_params* params);
/* one-shot, like erp_rot_ransac: p0, p1 [n][2] pixels, R 9 floats (R_cur_prev) or NULL (the rotation RANSAC's best
   over `samples`), samples [iters][3] (indices < n; with R given only the first two of a row are read).  Of params,
   iters (the argument counts) and mode are not looked at.  Outputs: mask[n], *n_inliers, counts[iters] (may be
   NULL; -1: skipped, or no hypothesis was evaluated), info.  Blocking. */
int erp_epi_ransac(vio_ctx* ctx, const float* p0, const float* p1, int n, int W, int H, const float* R,
                   const int32_t* samples, int iters, const erp_epi_params* params, uint8_t* mask, int* n_inliers,
                   int32_t* counts, erp_epi_info* info);
/* device pipeline: persistent, like erp_tracker_set_fb.  With the mode on erp_tracker_run's RANSAC stage is followed
   by the epipolar stage on the first min(iters, ransac_iters) rows of the run's sample stream; R is the rotation of
   erp_tracker_set_rotation for that run when there is one (the rotation hypotheses are then not evaluated), else
   the rotation RANSAC's best.  kept, and the discs around kept points, follow the final mask. */
int erp_tracker_set_epipolar(erp_tracker* t, const erp_epi_params* params);
/* the last run's info; VIO_EINVAL when that run had the mode off */
int erp_tracker_download_epi(erp_tracker* t, erp_epi_info* info);
/* front end: from the next frame on; R is that call's erp_frontend_predict_rotation when one was given, else the
   rotation RANSAC's best; the sample stream is erp_ransac_samples(ransac_seed + frame, n_good, .) */
int erp_frontend_set_epipolar(erp_frontend* f, const erp_epi_params* params);
/* the stage's info in the last erp_frontend_track* call; all zero (best -1) when that call did not run it */
int erp_frontend_epi_stats(erp_frontend* f, erp_epi_info* info);


/* ------------------------------------------------------------------------------------------ */
/* Monocular initialisation: Initializer::TryMonocularInitialization           */
/* (src/processing/Initializer.cpp:47-291) — essential-matrix RANSAC (:458-621), pose recovery */
/* (:623-697, :785-835), mid-point triangulation (:699-783), validation (:889-995), scale      */
/* normalisation (:997-1048).  Config: initialization.* (config/default_config.yaml:33-41).    */

typedef struct {
    int32_t width, height;          /* m_camera_width / m_camera_height (reprojection pixels) */
    int32_t min_features;           /* initialization.min_features (100) */
    int32_t ransac_iterations;      /* initialization.ransac_iterations (200) */
    float ransac_threshold;         /* initialization.ransac_threshold (0.1) on |b2^T E b1| */
    float max_reprojection_error;   /* initialization.max_reprojection_error (5.0 px) */
} vio_mono_init_params;

/* status: where TryMonocularInitialization returned false (0 = success) */
#define VIO_INIT_OK 0
#define VIO_INIT_TOO_FEW_BEARINGS 1   /* fewer than 5 bearing pairs (:117-120) */
#define VIO_INIT_ESSENTIAL_FAILED 2   /* best RANSAC inlier count < min_features (:579-581) */
#define VIO_INIT_POSE_FAILED 3        /* no cheirality candidate with >= min_features good points (:688-690) */
#define VIO_INIT_TRIANGULATION 4      /* triangulated points < min_features (:151-154) */
#define VIO_INIT_VALIDATION 5         /* validated points < min_features, or none (:962-992) */

typedef struct {
    int32_t status;                 /* VIO_INIT_* */
    int32_t best_hypothesis;        /* first RANSAC iteration with the (strictly) largest inlier count */
    int32_t num_inliers;            /* its inlier count */
    int32_t pose_candidate;         /* chosen (R, t) candidate 0..3 (:659-663) */
    int32_t candidate_good[4];      /* TestPoseCandidate good-point counts */
    int32_t num_triangulated;       /* TriangulatePoints successes */
    int32_t num_valid;              /* ValidateInitialization valid_count */
    float mean_reproj_error;        /* ValidateInitialization mean_error (px) */
    float scale_factor;             /* NormalizeScale: 1 / median distance */
    float E[9];                     /* refined essential matrix, row-major */
    float R[9];                     /* R_c2c1 (frame 1 -> frame 2), row-major */
    float t[3];                     /* t_c2c1 after scale normalisation */
} vio_mono_init_result;

/*
 * bearings1/2: n unit bearings (Feature::GetBearing, f32 xyz) of the selected features in the
 * first / last frame of the window; samples: ransac_iterations x 8 indices (the reference draws
 * them from mt19937 seeded by std::random_device, :477-494 — inject vio_mono_init_samples).
 * Outputs (host, caller-owned): res; inlier_mask (n, may be NULL) = the best hypothesis' inliers;
 * points (3n f32, may be NULL) = the scaled mid-point triangulations in camera-1 coordinates
 * (zero where triangulation failed), before the T_BC transform of :220-224.  1 <= n <= 4096.
 * The 8x9 / nx9 null vectors and the 3x3 SVDs are f64 Jacobi on the f32-built systems (reference:
 * Eigen f32 JacobiSVD); per-point arithmetic is the reference's f32.  Blocking.
 */
int vio_mono_init_solve(vio_ctx* ctx, const float* bearings1, const float* bearings2, int n, const int32_t* samples,
                        const vio_mono_init_params* params, vio_mono_init_result* res, uint8_t* inlier_mask,
                        float* points);
/* device time (ms) of the last vio_mono_init_solve's kernels on this context (waits for them) */
int vio_mono_init_kernel_ms(vio_ctx* ctx, double* ms);
/* the reference's RANSAC sample stream with an injected seed: iters x 8 distinct indices drawn by
   std::mt19937(seed) + std::uniform_int_distribution<>(0, n-1) with duplicate rejection (:477-494) */
int vio_mono_init_samples(uint32_t seed, int n, int iters, int32_t* out);

/* Host helpers of the same path (no device work). */
/* Initializer::SelectFeaturesForInit (:351-433) on a flat view of the last frame's features:
   uv (n x 2 pixel coords), obs_count (n, Feature::GetObservationCount).  Writes the selected
   feature indices in the reference's order to out_idx (capacity n), *n_out = count (0 when fewer
   than min_features candidates have >= min_observations observations). */
int vio_init_select_features(const float* uv, const int32_t* obs_count, int n, int width, int height, int grid_cols,
                             int grid_rows, int min_observations, int min_features, int32_t* out_idx, int* n_out);
/* Initializer::ComputeParallax (:293-349): median pixel displacement of features matched by id
   (first match in frame 2 for each frame-1 feature); 0 when nothing matches. */
int vio_init_parallax(const int32_t* ids1, const float* uv1, int n1, const int32_t* ids2, const float* uv2, int n2,
                      float* parallax);
/* Frame poses of :184-204 from T_BC (4x4 row-major, camera-to-body) and the result's R, t:
   T_wb1 = I, T_wb2 = T_BC * T_c1c2^-1 * T_BC^-1 (f32); also maps points (3n, camera-1 frame) to
   the world frame in place (p <- R_BC p + t_BC, :217-224) when points != NULL. */
int vio_init_compose(const float* T_BC, const float* R, const float* t, float* T_wb1, float* T_wb2, float* points,
                     int n);


/* ------------------------------------------------------------------------------------------ */
/* Absolute-pose RANSAC on map points (beyond the reference).  Optimizer::SolvePnP  */
/* (Optimizer.cpp:83-302, here VIO_PNP) refines the predicted pose and tags outliers around it;  */
/* a prediction outside its basin, or many wrong map-point links, get no answer.  This stage is  */
/* the hypothesise-and-verify step before it: minimal poses from sampled 3D-2D pairs, scored by  */
/* the angle between each bearing and R p + t.  Nothing calls it by itself.  The rule, f64 on    */
/* the f32 inputs, no contraction, sums in the written order:
     inputs     n world points p[k] (MapPoint::GetPosition) and bearings b[k] (Feature::GetBearing, unit to f32
                rounding), iters sample rows (i, j, k) (erp_ransac_samples), the parameters below, and in mode B a
                rotation R_known.  Formed once on the host in double: c2 = cos^2(inlier_thresh_rad),
                cp2 = cos^2(min_pair_angle_rad).
     inlier     x = R p + t (each row ((R0*p0 + R1*p1) + R2*p2) + t), d = b.x:  d > 0 && d*d >= c2 * (x.x).  A
                non-finite point or bearing is never an inlier.
     skipped    a row gets count -1 when, over the indices it reads (three in mode A, the first two in mode B),
                  an index repeats, or a sampled point or bearing has a non-finite component or a zero bearing; or
                  two sampled bearings are close: e = bi.bj, e > 0 && e*e >= cp2 * ((bi.bi) * (bj.bj)); or
                  (mode A) the world points are coincident or collinear: with e1 = p2 - p1, e2 = p3 - p1,
                  c = e1 x e2, c.c > 1e-10 * ((e1.e1) * (e2.e2)) does not hold; or
                  the solver has no real solution with positive depths (below).
     mode A     R_known == NULL, P3P.  With y = b / |b|, a12 = |p1 - p2|^2 (a13, a23 alike) and b12 = y1.y2 (b13,
                b23 alike) the depths l satisfy l1^2 + l2^2 - 2 b12 l1 l2 = a12 and its two siblings.  The solver
                takes one real root gamma of det(D1 + gamma D2) = 0 (D1 = a23 M12 - a12 M23, D2 = a23 M13 - a13 M23,
                M the constraints' quadratic forms; 40 Newton steps from outside the cubic's stationary points),
                splits the degenerate conic D1 + gamma D2 into its two lines in (l1 : l2 : l3) by the adjugate
                method, cuts each line with D2 (|gamma| < 1) or D1, scales by the sum of the three constraints,
                polishes each candidate with 5 Gauss-Newton steps on the three constraints, and keeps the
                candidates whose depths are finite and positive: up to four, in that order (first line's roots,
                then the second's).  No real line pair, a negative discriminant or no positive candidate: no
                solution.  Pose of a candidate: R = Y X^-1 with X = [p1-p2, p2-p3, (p1-p2) x (p2-p3)] and Y the same
                of the scaled bearings l y; t = l1 y1 - R p1.  The row's count is the largest of its poses' counts,
                best_solution the first pose with that count.  Only + - * / and sqrt are used.
     mode B     R_known given (it must pass erp_tracker_set_rotation's test, else VIO_EINVAL).  a = R_known p,
                (I - y y^T)(a + t) = 0 for the row's first two points: N t = -sum (I - y y^T) a with
                N = sum (I - y y^T), solved by the adjugate; no solution when det N > 0 does not hold, t is not
                finite, or y.(a + t) > 0 fails for either point.  One pose per row, R0 = R_known.
     selection  the first row with the strictly greatest count >= 0.  None: status NO_MODEL, zero pose, empty mask.
                Its count below min_inliers: FEW_INLIERS, pose and mask still reported.  n < 4 (mode A) or n < 3
                (mode B) or iters == 0: TOO_FEW, nothing launched, zero pose, empty mask, counts -1.
     refit      when the winner counts at least 3 inliers: refit_iters Gauss-Newton steps on them (the set is fixed):
                residual unit(R p + t) - b, x <- x + w x x + v, update R <- Q R, t <- Q t + v with Q the rotation of
                the quaternion (1, w / 2) normalised.  The 27 sums of J^T J and J^T r: lane l of 128 sums points
                i = l mod 128 in increasing i, the partials are summed in lane order; 6x6 Cholesky in one lane (a
                non-positive pivot stops the refit at the previous iterate).  In both modes all six parameters are
                free.  The refit pose is recounted with the same test and kept when it counts at least as many
                inliers as the minimal pose (refit_kept = 1); mask, num_inliers and rms_angle_rad (the RMS of
                atan2(|b x x|, b.x) over the inliers) follow the returned pose.
   The same inputs give bitwise the same outputs, run to run and across contexts. */
enum { VIO_PNPR_OK = 0, VIO_PNPR_TOO_FEW = 1, VIO_PNPR_NO_MODEL = 2, VIO_PNPR_FEW_INLIERS = 3 };
typedef struct vio_pnp_ransac_params {
    float inlier_thresh_rad;   /* angle between the bearing and R p + t (0.5 deg) */
    float min_pair_angle_rad;  /* two sampled bearings must differ by at least this (1 deg) */
    int32_t min_inliers;       /* below this the status is FEW_INLIERS (10, SolvePnP's own gate) */
    int32_t refit_iters;       /* Gauss-Newton iterations on the winner's inliers, 0..10 (5) */
} vio_pnp_ransac_params;
typedef struct vio_pnp_ransac_result {
    int32_t status;              /* VIO_PNPR_* */
    int32_t best_hypothesis;     /* the winning row, -1: none */
    int32_t best_solution;       /* its pose 0..3, -1: none */
    int32_t num_inliers_sample;  /* the winning minimal pose's count */
    int32_t num_inliers;         /* of the returned pose (after the refit when it is kept) */
    int32_t refit_kept;          /* 1: R_cw / t_cw are the refit, 0: the minimal pose */
    double R_cw[9], t_cw[3];     /* x_c = R_cw x_w + t_cw, row-major */
    double R0_cw[9], t0_cw[3];   /* the winning minimal pose */
    double rms_angle_rad;        /* over the returned pose's inliers */
} vio_pnp_ransac_result;

/* host only, and the first thing every entry point does: VIO_EINVAL for a null pointer, a NaN or negative field,
   an angle outside (0, pi/2), refit_iters outside 0..10, n or iters negative or above 4096 */
int vio_pnp_ransac_check(const vio_pnp_ransac_params* p, int n, int iters);
/* points [n][3] world, bearings [n][3], R_cw_known 9 floats row-major or NULL, samples [iters][3] with indices
   < n (mode B reads the first two of a row), mask [n] and counts [iters] may be NULL (-1: skipped).  Blocking. */
int vio_pnp_ransac(vio_ctx* ctx, const float* points, const float* bearings, int n, const float* R_cw_known,
                   const int32_t* samples, int iters, const vio_pnp_ransac_params* p, vio_pnp_ransac_result* res,
                   uint8_t* mask, int32_t* counts);
/* device time (ms) of the last vio_pnp_ransac's three kernels on this context (waits for them) */
int vio_pnp_ransac_kernel_ms(vio_ctx* ctx, double* ms);
/* Host helpers (no device work). */
/* The 3D-2D pairs of frame `frame` of the view: exactly the observation set and order of
   vio_ba_gather(map, VIO_PNP, ...) for that frame (valid feature, MapPoint not bad, not near the boundary;
   the gather itself looks at frame 0).  feat[k] is that gather's obs_feat, points its mp_pos, bearings
   Camera::PixelToBearing (Camera.cpp:22-47) of feat_uv, evaluated in double and rounded to f32.  Writes at most
   cap entries; *n is the full count (VIO_EINVAL when it exceeds cap; any output may be NULL with cap 0). */
int vio_pnp_correspondences(const vio_map_view* map, int frame, float* points, float* bearings, int32_t* feat, int cap,
                            int* n);
/* T_wb = T_cw^-1 * T_cb as a row-major f32 4x4 (products in double), ready for vio_ba_problem.T_wb_init of the
   VIO_PNP solve that follows */
int vio_pnp_compose(const double R_cw[9], const double t_cw[3], const float T_cb[16], float T_wb[16]);


/* ------------------------------------------------------------------------------------------ */
/* Estimator sliding-window bookkeeping on a host-side keyframe / MapPoint graph:  */
/* Estimator::CreateKeyframe's observation update and window slide (src/processing/Estimator.cpp: */
/* 671-754: reference-keyframe transfer, marginalisation, SetBad, RemoveObservation),             */
/* LinkMapPointsFromPreviousFrame (:806-843) and TriangulateNewMapPoints (:1141-1318, the          */
/* triangulation itself on device through vio_triangulate).  MapPoints are handles 0, 1, ... in   */
/* creation order; frames are identified by Frame::GetFrameId().  Not thread-safe.                */

typedef struct vio_window vio_window;

/* a keyframe handed to vio_window_add_keyframe (copied; the caller keeps its buffers) */
typedef struct {
    int32_t frame_id;
    int32_t num_features;
    int32_t width;               /* Frame::GetWidth (pixel error scale of the triangulation check) */
    int32_t _pad;
    const float* T_wb;           /* 16, row-major: Frame::GetTwb() */
    const float* T_bc;           /* 16, row-major: Frame::GetTBC() (camera-to-body) */
    const int32_t* feature_id;   /* n: Feature::GetFeatureId() */
    const float* uv;             /* 2n: GetPixelCoord() (carried for the BA map view) */
    const float* bearing;        /* 3n: GetBearing() */
    const uint8_t* valid;        /* n: IsValid() */
    const int32_t* mappoint;     /* n: GetMapPoint() handle (-1: none), e.g. from vio_window_link_mappoints */
    /* Feature::GetObservations() of each feature (its track): CSR, entries (frame id, feature index);
       may be NULL (no track history) */
    const int32_t* track_begin;  /* n + 1 */
    const int32_t* track_frame;
    const int32_t* track_feat;
} vio_window_frame;

typedef struct {
    int32_t obs_added;           /* observations the new keyframe added (:679-690) */
    int32_t transferred;         /* reference-keyframe transfers (marginalised MapPoints, :720-725) */
    int32_t deleted;             /* referenced MapPoints no other keyframe observes, set bad (:726-729);
                                    MapPoints left without observations (:747-749) also turn bad */
    int32_t removed_frame;       /* frame id of the keyframe slid out (-1: none) */
    int32_t num_keyframes;       /* window size after the call */
    int32_t _pad;
} vio_window_kf_stats;

typedef struct {
    float pos[3];
    int32_t bad, marginalized, triangulated;
    int32_t reference_frame;     /* reference keyframe id, -1 none */
    int32_t num_observations;
} vio_window_mappoint_info;

int vio_window_create(int max_keyframes, vio_window** out);   /* max_keyframes: 10 (:693) */
void vio_window_destroy(vio_window* win);
/* new MapPoint at pos (e.g. Initializer::CreateMapPoints); reference_frame -1 for none */
int vio_window_add_mappoint(vio_window* win, const float* pos, int32_t reference_frame, int32_t* handle);
/* MapPoint::AddObservation(frame, feat) + Frame::SetMapPoint(feat, mp) for a keyframe of the store */
int vio_window_add_observation(vio_window* win, int32_t mp, int32_t frame_id, int32_t feat);
/* LinkMapPointsFromPreviousFrame: curr_mp[i] = the previous frame's (valid, last-by-id) feature's
   MapPoint if it exists and is not bad, else -1 */
int vio_window_link_mappoints(const vio_window* win, const int32_t* prev_id, const uint8_t* prev_valid,
                              const int32_t* prev_mp, int n_prev, const int32_t* curr_id, int n_curr, int32_t* curr_mp);
/* CreateKeyframe: append the keyframe, add its MapPoint observations, slide the window */
int vio_window_add_keyframe(vio_window* win, const vio_window_frame* frame, vio_window_kf_stats* stats);
/* TriangulateNewMapPoints(kf1, kf2) in two host halves around the device triangulation:
   candidates: matched (kf1 index, kf2 index) pairs in kf2 order, their bearings (6 per pair) and the
   two world-to-camera transforms GetTwc().inverse() (T_cw, 32 floats) -> vio_triangulate;
   commit: creates a MapPoint per valid triangulation (reference kf1, observations kf1, kf2 and the
   in-window keyframes of kf2's feature track) and returns the handles in new_mp (-1 where invalid).
   vio_window_triangulate does both with the device in between; *n_new = new MapPoints. */
int vio_window_triangulation_candidates(const vio_window* win, int32_t kf1_id, int32_t kf2_id, int32_t* pairs,
                                        float* bearings, float* T_cw, int cap, int* n);
int vio_window_commit_triangulation(vio_window* win, int32_t kf1_id, int32_t kf2_id, const int32_t* pairs,
                                    const float* points, const uint8_t* valid, int n, int32_t* new_mp, int* n_new);
int vio_window_triangulate(vio_window* win, vio_ctx* ctx, int32_t kf1_id, int32_t kf2_id, int* n_new);
/* queries */
int vio_window_keyframes(const vio_window* win, int32_t* frame_ids, int cap, int* n);   /* oldest first */
int vio_window_num_mappoints(const vio_window* win);
int vio_window_mappoint(const vio_window* win, int32_t mp, vio_window_mappoint_info* info);
/* MapPoint::GetObservations() in order: (frame id, feature index) pairs */
int vio_window_mappoint_observations(const vio_window* win, int32_t mp, int32_t* frame_ids, int32_t* feats, int cap,
                                     int* n);
int vio_window_frame_mappoints(const vio_window* win, int32_t frame_id, int32_t* mp, int cap, int* n);
/* BA over the window: a vio_map_view of the window's keyframes (oldest first) and every MapPoint
   (arrays owned by the window, valid until its next mutating call), for vio_ba_gather /
   vio_ba_write_back; then the write-back applied to the window (frame poses, MapPoint positions,
   SetBad) */
int vio_window_map_view(vio_window* win, int height, int boundary_margin, vio_map_view* view);
int vio_window_apply_update(vio_window* win, const vio_ba_map_update* upd);

#ifdef __cplusplus
}
#endif
#endif /* VIO360_H_ */
