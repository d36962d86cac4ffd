// ba_phases.inc — the batched window solver as a sequence of phase kernels (included at the end of
// ba_kernel.hip, whose device maths it shares).
//
// ba_window_kernel runs a whole Ceres solve in one workgroup per window: every phase then runs at
// one wave per SIMD (its ~130 KB of LDS admits one workgroup per CU), and the observation walks
// are latency-bound.  Here one LM iteration is split at its data-parallel seams:
//   ph_lin    (window x landmark chunk)  BAFactor::Evaluate + J^T J / J^T r partials   [small LDS]
//   ph_prep   (window)                   partial sums, IMU normal equations, Ceres bookkeeping,
//                                        FinalizeIterationAndCheckIfMinimizerCanContinue
//   ph_schur  (window x chunk group)     V~ = L L^T per landmark, split-k Schur partials (MFMA)
//   ph_solve  (window)                   reduced system assembly + blocked Cholesky, candidates
//   ph_back   (window x landmark chunk)  back-substitution, model change, candidate cost
//   (ph_prep of the next slot first runs the step acceptance, ph_ctrl_run: trust_region_minimizer.cc:313-448)
// All LM state lives in the window's workspace between launches; every reduction over chunks or
// groups is a fixed-order loop, so results are bitwise reproducible and independent of the batch.
// The host enqueues max_iterations + 1 slots of these launches between ph_setup and ph_post (the last
// slot only its ph_prep, which ends every window); a window that has terminated skips the remaining
// launches.
namespace vio360 {

#ifndef PH_SCHUR_OCC
#define PH_SCHUR_OCC 2  // ph_schur_kernel waves per SIMD (launch bound)
#endif
constexpr int PH_GS_MIN = 1;  // smallest BaWin::gs (landmark chunks per Schur workgroup): workspace sizing
// A linearisation keeps per observation its scaled residual r (2) and Jacobian scale (1: the Huber scale,
// 0 where the Jacobian is zero); the compressed Jacobian A / Pb is rebuilt where it is used
// (factor_ap_at) from the landmark position and the pose cache at the linearisation point, PL24 doubles
// per keyframe (pose_cache_one's Rbw tbw Rcw tcw)
constexpr int PL24 = 24;

// Values that cross workgroups inside the persistent cluster route (ph_cluster_kernel, below): chunk /
// group partials, the Jacobi scaling, the candidate pose cache and step.  Written through to memory
// (sc1 stores) and read past the L1 (sc1 global loads), the protocol of MI355X_MICROARCH.md "Valid
// forms", row 1: every storing wave waits vmcnt(0), a workgroup barrier, then one lane's agent-scope
// counter add; the consumer polls with sc1 loads and loads after its poll / a workgroup barrier.  The
// phase route uses the same accesses (its kernel boundaries order them anyway).
typedef __attribute__((address_space(1))) double ph_gdouble;
typedef __attribute__((address_space(1))) int ph_gint;
#ifndef PH_PLAIN_X_EXPERIMENT
__device__ __forceinline__ void st_x(double* p, double v) {
    __hip_atomic_store((ph_gdouble*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ double ld_x(const double* p) {
    return __hip_atomic_load((const ph_gdouble*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
#else  // A/B build only (the cluster route is then unsafe): plain accesses
__device__ __forceinline__ void st_x(double* p, double v) { *p = v; }
__device__ __forceinline__ double ld_x(const double* p) { return *p; }
#endif
// The same accesses 16 B wide (two doubles): "Valid forms" row 1 admits 16-B sc1 stores and loads, and 8-B sc1
// accesses move at 0.54-0.70x the 16-B rate (a 16-B sc1 store costs about a plain one; an 8-B one leaves L2
// as a fabric write of its own).  Buffer forms (buffer_load / buffer_store_dwordx4 sc1, cache-policy bit 16
// = sc1 on gfx950): base is a wave-uniform, 16-B aligned pointer (the resource), i the even element index.
using ph_d2 = __attribute__((ext_vector_type(2))) double;
using ph_u4 = __attribute__((ext_vector_type(4))) unsigned;
__device__ __forceinline__ __amdgpu_buffer_rsrc_t ph_rsrc(const double* base) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<double*>(base), (short)0, 0x7fffffff, 0x00020000);
}
__device__ __forceinline__ ph_d2 ld_x2(__amdgpu_buffer_rsrc_t r, int i) {
    return __builtin_bit_cast(ph_d2, __builtin_amdgcn_raw_buffer_load_b128(r, i * 8, 0, 16));
}
__device__ __forceinline__ void st_x2(__amdgpu_buffer_rsrc_t r, int i, ph_d2 v) {
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(ph_u4, v), r, i * 8, 0, 16);
}
// n doubles of a cross-workgroup region (ld_x values) into LDS: 16-B pair loads where src is 16-B aligned
// and n even, else 8-B loads
__device__ __forceinline__ void ph_ld_block(double* dst, const double* src, int n) {
    if (((uintptr_t)src & 15) == 0 && (n & 1) == 0) {
        const __amdgpu_buffer_rsrc_t rs = ph_rsrc(src);
        for (int p = threadIdx.x; 2 * p < n; p += BA_THREADS) {
            const ph_d2 v = ld_x2(rs, 2 * p);
            dst[2 * p] = v.x;
            dst[2 * p + 1] = v.y;
        }
    } else {
        for (int e = threadIdx.x; e < n; e += BA_THREADS) dst[e] = ld_x(src + e);
    }
}
// threadIdx.x as an opaque value: per-thread addresses derived from it are recomputed where they are used
// instead of being hoisted out of the cluster route's persistent member loop and kept live (spilled to
// scratch) across it
__device__ __forceinline__ int ph_tid() {
    int t = (int)threadIdx.x;
    asm volatile("" : "+v"(t));
    return t;
}
// a partial that crosses workgroups inside the cluster route's persistent launch (WT: written through, st_x)
// or only a kernel boundary in the phase route (a plain store: the boundary orders it; sc1 stores of 8 B
// leave L2 one fabric write each and doubled the phase route's write traffic)
template <bool WT>
__device__ __forceinline__ void st_w(double* p, double v) {
    if constexpr (WT) st_x(p, v);
    else *p = v;
}
// the matching read: sc1 when the value comes from another workgroup of the same launch (cluster route),
// plain when an earlier launch wrote it (phase route: the launch boundary orders it, and a plain read may
// hit this XCD's L2 instead of going out to memory)
template <bool WT>
__device__ __forceinline__ double ld_w(const double* p) {
    if constexpr (WT) return ld_x(p);
    else return *p;
}

// what a step kernel needs of the window's LM state: in the phase route read from PhState at kernel
// start, in the cluster route from the leader's published records (ph_cluster_kernel)
struct PhView {
    int cur, done, step_valid;
    double radius;
    const double* rlin;  // pose cache at the linearisation point [K][24] (PL24; null: read from the phase region)
};

// diagnostic shader-clock accounting of the single-workgroup phase kernels (BaPools::prof, phase
// route): thread 0 adds the cycles since the previous mark to slot `slot` of the window
struct PhStamp {
    unsigned long long* prof;
    unsigned long long last;
    int win;  // the window's slot row (blockIdx.x of the per-window kernels)
    __device__ __forceinline__ PhStamp(unsigned long long* p, int w)
        : prof(p), last(p ? __builtin_amdgcn_s_memtime() : 0), win(w) {}
    __device__ __forceinline__ void operator()(int slot) {
        if (prof && threadIdx.x == 0) {
            const unsigned long long t = __builtin_amdgcn_s_memtime();
            prof[PF_NSLOT * win + slot] += t - last;
            last = t;
        }
    }
    __device__ __forceinline__ void reset() {
        if (prof) last = __builtin_amdgcn_s_memtime();
    }
};

struct PhState {
    LmState st;
    int need_lin, first, step_valid, lin_fail;
    int cur;                   // which of the two parameter / IMU-Jacobian sets is the current point
    int ctrl_pending;          // a step was attempted in this slot: the next ph_prep runs its control first
    int _p3, _p4;
    double lin_cost, imu_cost, imu_cand_cost, pad;
};

struct PhLayout {
    int64_t st, pinit, rcb, rlin, pcc, fv, U, upart, cpart, bpart, imuJ, imur, imuJc, imurc, spart, stot, imurec;
    // the second linearisation set (the candidate's, written by ph_back; swaps roles with the first
    // on acceptance like the parameter sets): obs r / Jacobian scale (a2's first N doubles; pb2 unused),
    // landmark V / g_l, chunk pose partials, chunk linearisation partials (cost, max |g_l|, failure) of
    // both sets
    int64_t r2, a2, pb2, v2, gl2, upart2, lpart, lpart2, himu2, total;
    int LC, nch, ng;
};
// phase region of a window (doubles, after ba_ws_layout().total + ba_ws_extra_doubles())
// (LC, nch, ng: the walk geometry, which the kernels take from the window descriptor instead of dividing)
__host__ __device__ inline PhLayout ph_layout_at(int K, int L, int N, int T, int LC, int nch, int ng) {
    PhLayout p;
    const int k = K > 0 ? K : 1;
    p.LC = LC;
    p.nch = nch;
    p.ng = ng;
    const int nt = T * (T + 1) / 2;
    int64_t o = 0;
    p.st = o; o += 64;
    p.pinit = o; o += 24 * k;
    p.rcb = o; o += 9 * k;
    p.rlin = o; o += PL24 * k;                     // pose cache at the linearisation point (Rbw tbw Rcw tcw)
    p.pcc = o; o += 36 * k;
    p.fv = o; o += 5 * BA_NF_MAX;                  // s_f g_f colsq_f D_f b
    p.U = o; o += 27 * k;
    p.upart = o; o += (int64_t)27 * k * p.nch;      // [chunk][K][27]
    p.cpart = o; o += (int64_t)8 * (p.nch + 1);     // back: mc sn xn ccost cfail fin per chunk; [nch]: IMU mc, cost
    p.bpart = o; o += (int64_t)8 * p.ng;            // schur: bad
    p.imuJ = o; o += 108 * k;
    p.imur = o; o += 9 * k;
    p.imuJc = o; o += 108 * k;                     // IMU Jacobians / residuals at the candidate
    p.imurc = o; o += 9 * k;
    o = (o + 1) & ~(int64_t)1;                      // 16-B aligned: the cluster route moves these in pairs (ld_x2)
    p.spart = o; o += (int64_t)(nt * 256 + 16 * T) * p.ng;  // [group][lower tiles | rhs]
    p.stot = o; o += (int64_t)nt * 256 + 16 * T + 8;         // cluster route: their sum over all groups | any failure
    p.imurec = o; o += 8;                                     // cluster route: the IMU member's solve record
    p.r2 = o; o += 2 * (int64_t)N;
    p.a2 = o; o += 6 * (int64_t)N;
    p.pb2 = o; o += 3 * (int64_t)N;
    p.v2 = o; o += 6 * (int64_t)L;
    p.gl2 = o; o += 3 * (int64_t)L;
    p.upart2 = o; o += (int64_t)27 * k * p.nch;
    p.lpart = o; o += (int64_t)4 * p.nch;
    p.lpart2 = o; o += (int64_t)4 * p.nch;
    p.himu2 = o; o += NI_MAX * NI_MAX + NI_MAX;      // IMU normal equations (H, g) of the second set
    p.total = (o + 31) & ~(int64_t)31;
    return p;
}
__host__ __device__ inline PhLayout ph_layout(int K, int L, int N, int T, int gs) {
    const int LC = BA_THREADS / (K > 0 ? K : 1), nch = (L + LC - 1) / LC;
    return ph_layout_at(K, L, N, T, LC, nch, (nch + gs - 1) / gs);
}
__host__ __device__ inline PhLayout ph_layout(const BaWin& w) {
    return ph_layout_at(w.K, w.L, w.N, w.T, w.LC, w.nch, w.ng);
}

static_assert(1500 + 3 * BA_THREADS <= 9 * BA_THREADS && 8 + NI_MAX * NI_MAX + NI_MAX + (BA_KMAX * NI_MAX) / 8 <= 1500,
              "ph_prep's staging areas inside PhShared::buf");
struct __align__(16) PhShared {
    double pc[BA_KMAX][36];
    double Rcb_raw[BA_KMAX][9];
    double Rlin[BA_KMAX][PL24];  // pose cache at the linearisation point (Rbw tbw Rcw tcw)
    double red[BA_THREADS / 64 + 4];
    double redm[BA_THREADS / 64 + 4];
    double redv[(BA_THREADS / 64) * 8];  // block_reduce exchange
    double buf[9 * BA_THREADS];
    double dlt[BA_NF_MAX];       // the f-space step (ph_back)
    LmState st;
    int posef[BA_KMAX];
    int pvalid[BA_KMAX];
    int8_t icol[BA_KMAX][12];
    int flag[8];
    // last: ph_back_kernel allocates PhShared up to here (kPhBackLds)
    double imu_J[VI_KMAX][108];
    double imu_r[VI_KMAX][9];
};
constexpr size_t kPhBackLds = offsetof(PhShared, imu_J);  // the IMU arrays: ph_back_x's IMU workgroup, ph_prep, ph_solve

struct PhCtx {
    WinCtx c;
    PhLayout ph;
    double* pr;  // phase region base
    PhState* gs;
    // the current point x and the candidate (the workspace's two parameter sets swap roles when a
    // step is accepted: no copy), and the IMU residuals / Jacobians at each
    double *xp, *xl, *xv, *xb, *cp, *cl, *cv, *cb;
    double *imuJ, *imur, *imuJc, *imurc;
    double *himu, *himuc;  // IMU normal equations [NI_MAX^2 | NI_MAX] at the current point / the candidate
    // linearisation sets: current (at x) and candidate (at the candidate, ph_back): residuals r [2][N],
    // Jacobian scales [N], landmark V / g_l, chunk pose and linearisation partials
    double *lr, *la, *lv, *lg, *lup, *llp;
    double *cr, *ca, *cvv, *cgl, *cup, *clp;
};

// PnP windows (outlier rounds inside a solve) stay on ba_window_kernel
__device__ inline bool ph_skip(const BaPools& P, int wi) { return P.win[wi].is_pnp != 0; }
// the window of a per-window (x) / per-window-row (y) workgroup: a launch covers the windows
// [win_base, win_base + grid extent) of the batch (one sub-batch per stream, launch_ba_phases)
__device__ inline int ph_wx(const BaPools& P) { return P.win_base + (int)blockIdx.x; }
// A per-window-row launch of `per` workgroups for each of n windows has the grid (gx, per, n / gx) of ph_grid,
// gx = 8 where n % 8 == 0: linear block ids (x fastest) are dealt round robin over the 8 XCDs, so every
// workgroup of local window i = x + gx z runs on XCD i % 8, where the window's ph_prep / ph_solve workgroup
// (block i of n) reads its partials; any other n: gx = 1, the plain (per, n) order.  Placement only: nothing
// relies on it.  ph_sub: the workgroup's chunk / group index within its window
__device__ inline int ph_wy(const BaPools& P) { return P.win_base + (int)(blockIdx.x + gridDim.x * blockIdx.z); }
__device__ inline int ph_sub() { return (int)blockIdx.y; }

// the cluster leader's LDS copy of its window's PhState: right after the leader's BaShared and PhClusterSh in
// the kernel's dynamic LDS (ph_cluster_lds_bytes)
struct PhClusterSh;
__device__ __forceinline__ PhState* ph_lds_state();
__device__ __forceinline__ void ph_ctx_view(PhCtx& x, bool sw);

// LS: the window's PhState lives in LDS (the cluster route's leader keeps its LM state on chip for the whole
// solve, ph_cluster_kernel); otherwise in the window's phase region
template <bool LS = false>
__device__ __forceinline__ PhCtx ph_ctx(const BaPools& P, int wi, int cur_override = -1) {
    PhCtx x;
    WinCtx& c = x.c;
    const BaWin& w = P.win[wi];
    c.w = &w;
    c.L = ba_ws_layout(w.K, w.L, w.N);
    c.pose_raw = P.pose_raw + 24 * w.o_pose;
    c.kf_const = P.kf_const + w.o_pose;
    c.lm_xyz0 = P.lm_xyz0 + 3 * w.o_lm;
    c.lm_var = P.lm_var + w.o_lm;
    c.lm_marg = P.lm_marg + w.o_lm;
    c.lm_ptr = P.lm_ptr + w.o_lmptr;
    c.obs_kf = P.obs_kf + w.o_obs;
    c.obs_lm = P.obs_lm + w.o_obs;
    c.obs_uv = P.obs_uv + 2 * w.o_obs;
    c.kf_ptr = P.kf_ptr + w.o_kfptr;
    c.kf_obs = P.kf_obs + w.o_obs;
    c.preint = P.preint + w.o_pose;
    c.preint_valid = P.preint_valid + w.o_pose;
    c.vel0 = P.vel0 + 3 * w.o_pose;
    c.ws = P.ws + w.o_ws;
    c.sqi = c.ws + c.L.total;
    c.Himu = c.sqi + 81 * BA_KMAX;
    c.gimu = c.Himu + NI_MAX * NI_MAX;
    c.outlier = P.out_u8 + w.o_obs;
    c.trace = P.out_trace + w.o_tr;
    x.ph = ph_layout(w);
    x.pr = c.ws + c.L.total + ba_ws_extra();
    x.gs = LS ? ph_lds_state() : reinterpret_cast<PhState*>(x.pr + x.ph.st);
    ph_ctx_view(x, (cur_override >= 0 ? cur_override : x.gs->cur) != 0);
    return x;
}
// the same window's context with parameter set `cur` as the current point (only the view differs: a kernel
// that has built one context derives the other from it instead of building it again)
__device__ __forceinline__ PhCtx ph_ctx_at(const PhCtx& x0, int cur) {
    PhCtx x = x0;
    ph_ctx_view(x, cur != 0);
    return x;
}
// sw: parameter / linearisation set 1 is the current point, set 0 the candidate
__device__ __forceinline__ void ph_ctx_view(PhCtx& x, bool sw) {
    const WinCtx& c = x.c;
    double* s0[4] = {c.ws + c.L.x_pose, c.ws + c.L.x_lm, c.ws + c.L.x_vel, c.ws + c.L.x_bias};
    double* s1[4] = {c.ws + c.L.c_pose, c.ws + c.L.c_lm, c.ws + c.L.c_vel, c.ws + c.L.c_bias};
    double** X = sw ? s1 : s0;
    double** Cd = sw ? s0 : s1;
    x.xp = X[0]; x.xl = X[1]; x.xv = X[2]; x.xb = X[3];
    x.cp = Cd[0]; x.cl = Cd[1]; x.cv = Cd[2]; x.cb = Cd[3];
    x.imuJ = x.pr + (sw ? x.ph.imuJc : x.ph.imuJ);
    x.imur = x.pr + (sw ? x.ph.imurc : x.ph.imur);
    x.imuJc = x.pr + (sw ? x.ph.imuJ : x.ph.imuJc);
    x.imurc = x.pr + (sw ? x.ph.imur : x.ph.imurc);
    x.himu = sw ? x.pr + x.ph.himu2 : c.Himu;
    x.himuc = sw ? c.Himu : x.pr + x.ph.himu2;
    double* l0[6] = {c.ws + c.L.r, c.ws + c.L.jp, c.ws + c.L.V, c.ws + c.L.gl, x.pr + x.ph.upart, x.pr + x.ph.lpart};
    double* l1[6] = {x.pr + x.ph.r2, x.pr + x.ph.a2, x.pr + x.ph.v2, x.pr + x.ph.gl2, x.pr + x.ph.upart2, x.pr + x.ph.lpart2};
    double** LC_ = sw ? l1 : l0;
    double** LN_ = sw ? l0 : l1;
    x.lr = LC_[0]; x.la = LC_[1]; x.lv = LC_[2]; x.lg = LC_[3]; x.lup = LC_[4]; x.llp = LC_[5];
    x.cr = LN_[0]; x.ca = LN_[1]; x.cvv = LN_[2]; x.cgl = LN_[3]; x.cup = LN_[4]; x.clp = LN_[5];
}

// keyframe tables of a window into LDS
__device__ __forceinline__ void ph_tables(PhShared& sh, const PhCtx& x) {
    const BaWin& w = *x.c.w;
    for (int k = threadIdx.x; k < BA_KMAX; k += BA_THREADS) {
        sh.posef[k] = k < w.K ? w.pose_f[k] : -1;
        sh.pvalid[k] = k < w.K ? x.c.preint_valid[k] : 0;
    }
    for (int e = threadIdx.x; e < 12 * BA_KMAX; e += BA_THREADS) {
        const int k = e / 12, cc = e - 12 * k;
        sh.icol[k][cc] = (int8_t)((w.is_vi && k >= 1 && k < w.K) ? imu_col(w, k, cc) : -1);
    }
    for (int e = threadIdx.x; e < 9 * w.K; e += BA_THREADS) sh.Rcb_raw[e / 9][e % 9] = x.pr[x.ph.rcb + e];
}

// pose cache at xp (pinit from the phase region)
__device__ __forceinline__ void ph_pose_cache(PhShared& sh, const PhCtx& x, const double* xp) {
    const int K = x.c.w->K;
    for (int k = threadIdx.x; k < K; k += BA_THREADS) pose_cache_one(x.pr + x.ph.pinit + 24 * k, xp + 6 * k, sh.pc[k]);
}

// IMU factors of the window (one lane per factor) at the poses in sh.pc
// INL: the IMU factor code inlined (the cluster route's kernel stays free of calls and of their stack)
template <bool INL = false>
__device__ __forceinline__ double ph_imu_factors(PhShared& sh, const PhCtx& x, const double* xv, const double* xb, bool want_jac) {
    const int tid = ph_tid();
    const BaWin& w = *x.c.w;
    double cost = 0.0;
    if (!w.is_vi) return 0.0;
    for (int k = 1 + tid; k < w.K; k += BA_THREADS) {
        if (!x.c.preint_valid[k]) continue;
        double r[9];
        (INL ? imu_eval_inl : imu_eval)(x.c.preint[k], x.c.sqi + 81 * k, w.gravity, sh.pc[k - 1], sh.pc[k], xv + 3 * (k - 1), xb, xb + 3,
                 xv + 3 * k, want_jac, r, sh.imu_J[k]);
        double sq = 0.0;
        for (int i = 0; i < 9; ++i) {
            sq += r[i] * r[i];
            if (want_jac) sh.imu_r[k][i] = r[i];
        }
        cost += 0.5 * sq;
    }
    return cost;
}

// IMU normal equations of the window's factors in factor order (each entry accumulates its factor-k
// terms for k ascending; the (p, q) pairs of one factor are distinct): H [ni][ni] and g [ni] into the LDS
// scratch Hs (NI_MAX^2 + NI_MAX doubles) from the factors' Jacobians / residuals in LDS (J[k][9x12],
// r[k][9]) and the factors' column table icol (LDS, imu_col of every (k, c); PhShared::icol, ph_tables).
// All threads call it; it ends with a barrier.
__device__ __forceinline__ void imu_normal_eq(double* Hs, const double (*J)[108], const double (*r)[9], const BaWin& w,
                                              const int* pvalid, const int8_t (*icol)[12]) {
    const int ni = w.ni, K = w.K;
    double* gs = Hs + NI_MAX * NI_MAX;
    for (int e = threadIdx.x; e < NI_MAX * NI_MAX + NI_MAX; e += BA_THREADS) Hs[e] = 0.0;
    __syncthreads();
    for (int k = 1; k < K; ++k) {
        if (!pvalid[k]) continue;
        const int e = threadIdx.x;
        if (e < 144) {
            const int cpp = e / 12, cq = e - 12 * (e / 12);
            const int p = icol[k][cpp], q = icol[k][cq];
            if (p >= 0 && q >= 0) {
                double h = 0.0;
#pragma unroll
                for (int i = 0; i < 9; ++i) h += J[k][12 * i + cpp] * J[k][12 * i + cq];
                Hs[p * ni + q] += h;
            }
        } else if (e < 156) {
            const int cpp = e - 144;
            const int p = icol[k][cpp];
            if (p >= 0) {
                double gg = 0.0;
#pragma unroll
                for (int i = 0; i < 9; ++i) gg += J[k][12 * i + cpp] * r[k][i];
                gs[p] += gg;
            }
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------
// setup: projected input rotations, IMU sqrt-information, (landmark, keyframe) table, initial
// parameters, fixed cost, Ceres minimizer state (trust_region_minimizer.cc:67-134)
template <bool INL = false>
__device__ __forceinline__ void ph_setup_body(const BaPools& P, int wi, PhShared& sh) {
    const PhCtx x = ph_ctx(P, wi, 0);  // PhState is not initialised yet: parameter set 0
    const WinCtx& c = x.c;
    const BaWin& w = *c.w;
    const int K = w.K, L = w.L, N = w.N;
    {
        const int job = threadIdx.x >> 6, k = threadIdx.x & 63;
        if (k < K) {
            const double* pr = c.pose_raw + 24 * k;
            double* pi = x.pr + x.ph.pinit + 24 * k;
            if (job == 0) {
                (INL ? polar3_inl : polar3)(pr, pi);
                for (int i = 0; i < 3; ++i) pi[9 + i] = pr[9 + i];
            } else if (job == 1) {
                (INL ? polar3_inl : polar3)(pr + 12, pi + 12);
                for (int i = 0; i < 3; ++i) pi[21 + i] = pr[21 + i];
                for (int i = 0; i < 9; ++i) x.pr[x.ph.rcb + 9 * k + i] = pr[12 + i];
            }
        }
        if (w.is_vi)  // then every wave, one IMU factor at a time (wave j: factors 1 + j, 5 + j, ...)
            for (int kk = 1 + job; kk < K; kk += BA_THREADS / 64)
                if (c.preint_valid[kk]) (INL ? imu_sqrt_info_wave_inl : imu_sqrt_info_wave)(c.preint[kk], c.sqi + 81 * kk);
    }
    for (int o = threadIdx.x; o < N; o += BA_THREADS) c.outlier[o] = 0;
    {
        int* lk = reinterpret_cast<int*>(c.ws + c.L.lk);
        for (int e = threadIdx.x; e < 16 * L; e += BA_THREADS) lk[e] = -1;
        __syncthreads();
        fill_lk(lk, c.obs_lm, c.obs_kf, N);
    }
    double* ws = c.ws;  // a solve starts on parameter set 0 (PhState::cur = 0 below)
    for (int e = threadIdx.x; e < 6 * K; e += BA_THREADS) ws[c.L.x_pose + e] = 0.0;
    copy_strided(ws + c.L.x_lm, c.lm_xyz0, 3 * L);
    for (int e = threadIdx.x; e < 3 * K; e += BA_THREADS) ws[c.L.x_vel + e] = w.is_vi ? c.vel0[e] : 0.0;
    for (int e = threadIdx.x; e < 6; e += BA_THREADS) ws[c.L.x_bias + e] = e < 3 ? w.bg0[e] : w.ba0[e - 3];
    __syncthreads();
    ph_tables(sh, x);
    ph_pose_cache(sh, x, ws + c.L.x_pose);
    __syncthreads();
    const double fc = fixed_cost(c, sh.posef, sh.pc, sh.Rcb_raw);
    const double fct = block_sum(fc, sh.red);
    bool any_free = w.nf > 0;
    if (threadIdx.x == 0) {
        if (!any_free)
            for (int l = 0; l < L && !any_free; ++l) any_free = c.lm_var[l];
        PhState& g = *x.gs;
        LmState& s = g.st;
        s.radius = 1e4;
        s.decrease_factor = 2.0;
        s.x_norm = -1.0;
        s.min_cost = DBL_MAX;
        s.iteration = 0;
        s.nsucc = s.nunsucc = 0;
        s.consecutive_invalid = 0;
        s.termination = VIO_TERM_NO_CONVERGENCE;
        s.done = 0;
        s.fail = 0;
        s.fixed_cost = fct;
        s.tr_n = 0;
        g.cur = 0;
        g.ctrl_pending = 0;
        g.need_lin = 1;
        g.first = 1;
        g.step_valid = 0;
        if (!any_free) {  // nothing to optimise (the monolithic kernel's no-free-parameter branch)
            s.termination = VIO_TERM_CONVERGENCE;
            s.initial_cost = s.final_cost = fct;
            s.nsucc = s.nunsucc = 0;
            s.done = 1;
            g.need_lin = 0;
        }
    }
}
#ifndef VIO_BA_CLUSTER_TU
__global__ void __launch_bounds__(BA_THREADS) ph_setup_kernel(BaPools P) {
    const int wi = ph_wx(P);
    if (ph_skip(P, wi)) return;
    __shared__ PhShared sh;
    ph_setup_body(P, wi, sh);
}
#endif

// ------------------------------------------------------------------------------------------
// linearisation of one landmark chunk: residuals, compressed Jacobians (A, Pb), V/g per landmark,
// pose J^T J / J^T r partials of the chunk (the IMU factors are evaluated by ph_prep, which keeps
// this kernel's registers and its workgroups small)
// (the first linearisation only; later ones are the accepted candidates', ph_back, speculatively; the
// caller checks that the window needs it)
template <bool WT = true>
__device__ __forceinline__ void ph_lin_body(const BaPools& P, int wi, int ci, PhShared& sh) {
    const PhCtx x = ph_ctx(P, wi, 0);  // the first linearisation is at parameter set 0
    const WinCtx& c = x.c;
    const BaWin& w = *c.w;
    if (ci >= x.ph.nch) return;
    const int N = w.N, K = w.K, L = w.L;
    const bool first = true;
    double* ws = c.ws;
    const double* xp = x.xp;
    const double* xl = x.xl;
    ph_tables(sh, x);
    ph_pose_cache(sh, x, xp);
    __syncthreads();
    const Walk g = walk_geom(w);
    const int pf = g.on ? sh.posef[g.kf] : -1;
    const int* lk = reinterpret_cast<const int*>(ws + c.L.lk);
    double* r0 = x.lr;
    double* as = x.la;
    double* V = x.lv;
    double* gl = x.lg;
    double* sl = ws + c.L.s_l;
    double acc[27];
#pragma unroll
    for (int i = 0; i < 27; ++i) acc[i] = 0.0;
    double cost = 0.0, gm = 0.0, v9[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) v9[i] = 0.0;
    int fail = 0;
    const int l0 = ci * g.LC, l = l0 + g.jf;
    const int o = (g.on && l < L) ? lk[16 * l + g.kf] : -1;
    if (o >= 0) {
        const bool lv = c.lm_var[l] != 0;
        if (pf >= 0 || lv) {
            double Pw[3] = {xl[3 * l], xl[3 * l + 1], xl[3 * l + 2]};
            double r[2], Aj[6], Pb[3];
            bool jz;
            const int f = factor_eval_ap(sh.pc[g.kf], sh.Rcb_raw[g.kf], Pw, (double)c.obs_uv[2 * o],
                                         (double)c.obs_uv[2 * o + 1], w.cols, w.rows, w.Lw, c.outlier[o] != 0,
                                         w.is_pnp, r, Aj, Pb, jz);
            if (f) {
                fail = 1;
            } else {
                double cst, sc;
                huber(w.huber, r[0] * r[0] + r[1] * r[1], cst, sc);
                cost += cst;
                const double ra = r[0] * sc, rb = r[1] * sc;
                r0[o] = ra;
                r0[N + o] = rb;
                as[o] = jz ? 0.0 : sc;
#pragma unroll
                for (int i = 0; i < 6; ++i) Aj[i] = jz ? 0.0 : Aj[i] * sc;
#pragma unroll
                for (int i = 0; i < 3; ++i) Pb[i] = jz ? 0.0 : Pb[i];
                double Jp[12], Jl[6];
                jac_from_ap(Aj, Pb, sh.pc[g.kf] + 12, Jp, Jl);
                if (pf >= 0) {
                    int idx = 0;
#pragma unroll
                    for (int i = 0; i < 6; ++i)
#pragma unroll
                        for (int j = i; j < 6; ++j) acc[idx++] = Jp[i] * Jp[j] + Jp[6 + i] * Jp[6 + j];
#pragma unroll
                    for (int i = 0; i < 6; ++i) acc[21 + i] = Jp[i] * ra + Jp[6 + i] * rb;
                }
                if (lv) {
                    const double* la = Jl;
                    const double* lb = Jl + 3;
                    v9[0] = la[0] * la[0] + lb[0] * lb[0];
                    v9[1] = la[0] * la[1] + lb[0] * lb[1];
                    v9[2] = la[0] * la[2] + lb[0] * lb[2];
                    v9[3] = la[1] * la[1] + lb[1] * lb[1];
                    v9[4] = la[1] * la[2] + lb[1] * lb[2];
                    v9[5] = la[2] * la[2] + lb[2] * lb[2];
                    v9[6] = la[0] * ra + lb[0] * rb;
                    v9[7] = la[1] * ra + lb[1] * rb;
                    v9[8] = la[2] * ra + lb[2] * rb;
                }
            }
        }
    }
    // landmark sums over the slot's K lanes
#pragma unroll
    for (int i = 0; i < 9; ++i) sh.buf[i * BA_THREADS + threadIdx.x] = v9[i];
    __syncthreads();
    gm = lm_sums9(sh.buf, l0, g, K, L, c.lm_var, xl, V, gl, sl, first, gm);
    __syncthreads();
    // pose partials of the chunk: 27 sums per keyframe over its LC lanes, 9 at a time through LDS
    double* up = x.lup + (int64_t)ci * 27 * K;
    for (int part = 0; part < 3; ++part) {
#pragma unroll
        for (int i = 0; i < 9; ++i) sh.buf[i * BA_THREADS + threadIdx.x] = acc[9 * part + i];
        __syncthreads();
        for (int e = threadIdx.x; e < 9 * K; e += BA_THREADS) {
            const int k = walk_div(e, walk_recip(9)), i = e - 9 * k;  // (e < 9 K <= 144: exact, full-rate multiply)
            double s = 0.0;
            for (int j = 0; j < g.LC; ++j) s += sh.buf[i * BA_THREADS + j * K + k];
            st_w<WT>(up + 27 * k + 9 * part + i, s);
        }
        __syncthreads();
    }
    double rv[3] = {cost, gm, (double)fail};
    block_reduce<1, 2>(rv, sh.redv);
    const double tc = rv[0], tg = rv[1], tf = rv[2];
    if (threadIdx.x == 0) {
        double* lp = x.llp + 4 * ci;
        st_w<WT>(lp, tc);
        st_w<WT>(lp + 1, tg);
        st_w<WT>(lp + 2, tf);
    }
}
#ifndef VIO_BA_CLUSTER_TU
__global__ void __launch_bounds__(BA_THREADS) ph_lin_kernel(BaPools P) {
    const int wi = ph_wy(P);
    if (ph_skip(P, wi)) return;
    __shared__ PhShared sh;
    const PhState& gst = *ph_ctx(P, wi, 0).gs;
    if (gst.st.done || !gst.need_lin || !gst.first) return;
    ph_lin_body<false>(P, wi, ph_sub(), sh);
}
#endif

// ------------------------------------------------------------------------------------------
// step evaluation and acceptance of the step attempted in the previous slot (trust_region_minimizer.cc:
// 313-448, 649-826), at the head of the next ph_prep (same workgroup: no cross-workgroup hand-off);
// lanes 0-63 work, every thread calls it.  Returns (every thread) the current parameter set afterwards.
template <bool LS = false>
__device__ __forceinline__ int ph_ctrl_run(const BaPools& P, int wi, double (*cps)[6], int& s_accept, int& s_cur) {
    const PhCtx x = ph_ctx<LS>(P, wi);
    const WinCtx& c = x.c;
    const BaWin& w = *c.w;
    PhState& gst = *x.gs;
    PhStamp stamp(P.prof, wi);  // diagnostic slots: 21 control lane, 22 accepted-step copies
    const int t = (int)threadIdx.x;
    // the back-substitution's chunk partials (6 per chunk) staged by all 64 lanes, then summed by lane 0
    // in chunk order onto ph_solve's f-space partials.  The step's validity, lane 0's IMU partials and the
    // first 64 chunks' partials are requested in one batch before the first barrier (the partials are read
    // whatever the validity and unused when invalid); lane 0 updates the LM state in place.  No local copy
    // of LmState: SROA leaves part of one on the stack, and the first scratch access of a workgroup that
    // is alone on its CU cost ≈ 25 k cycles (phase route: 256-window ph_prep 37-48 µs -> 25 µs)
    const int nch = x.ph.nch;
    double v0[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) v0[i] = (t < 64 && t < nch) ? ld_w<LS>(x.pr + x.ph.cpart + 8 * t + i) : 0.0;
    double mc = 0.0, sn = 0.0, xn = 0.0, fin = 0.0, cc = 0.0, icc = 0.0;
    double mc0 = 0.0, icc0 = 0.0;
    int fixed0 = 0;
    if (threadIdx.x == 0) {
        const double* ex = x.pr + x.ph.cpart + 8 * x.ph.nch;  // ph_back's extra workgroup / the IMU member
        mc0 = ld_w<LS>(ex);
        icc0 = ld_w<LS>(ex + 3);
        if constexpr (!LS) fixed0 = w.fixed_iter;
    }
    const bool valid0 = gst.step_valid != 0;
    int cfail = 0;
    if (threadIdx.x == 0 && valid0) {  // the IMU model change and ph_solve's f-space partials start the sums
        mc = mc0;
        icc = icc0;
        sn = gst.st.step_norm;
        xn = gst.st.cand_x_norm2;
    }
    if (valid0) {
        for (int q0 = 0; q0 < nch; q0 += 64) {
            const int q = q0 + t;
            double v[6];
#pragma unroll
            for (int i = 0; i < 6; ++i) v[i] = q0 == 0 ? v0[i] : (t < 64 && q < nch) ? ld_w<LS>(x.pr + x.ph.cpart + 8 * q + i) : 0.0;
            __syncthreads();
            if (t < 64) {
#pragma unroll
                for (int i = 0; i < 6; ++i) cps[t][i] = v[i];
            }
            __syncthreads();
            if (threadIdx.x == 0)
#pragma unroll 4
                for (int u = 0; u < 64 && q0 + u < nch; ++u) {
                    mc += cps[u][0];
                    sn += cps[u][1];
                    xn += cps[u][2];
                    cc += cps[u][3];
                    cfail |= cps[u][4] > 0.0;
                    fin = fmax(fin, cps[u][5]);
                }
        }
    }
    if (threadIdx.x == 0) {
        LmState& s = gst.st;  // (in place: a local copy of the state puts part of it on the stack)
        const bool fixed = (LS ? w.fixed_iter : fixed0) != 0;
        bool valid = valid0;
        if (valid) {
            cc += icc;
            gst.imu_cand_cost = icc;
            s.model_change = mc;
            s.step_norm = sqrt(sn);
            s.cand_x_norm2 = xn;
            if (fin == 0.0) s.tr_model = mc;  // a finite step: its model change is recorded, valid or not
            valid = fin == 0.0 && mc > 0.0;
        }
        int accept = 0;
        if (!valid) {
            if (++s.consecutive_invalid >= 5) {
                s.termination = VIO_TERM_FAILURE;
                s.done = 1;
            } else {
                s.radius /= s.decrease_factor;
                s.decrease_factor *= 2.0;
                s.step_ok = 0;
                s.iter_cost = s.x_cost + s.fixed_cost;
            }
        } else {
            s.consecutive_invalid = 0;
            s.cand_cost = cfail ? DBL_MAX : cc;
            s.fail = 0;
            s.tr_valid = 1;
            s.tr_step_norm = s.step_norm;
            s.tr_cost_change = s.x_cost - s.cand_cost;
            if (!fixed && s.step_norm <= 1e-8 * (s.x_norm + 1e-8)) { s.termination = VIO_TERM_CONVERGENCE; s.done = 1; }
            else if (!fixed && fabs(s.x_cost - s.cand_cost) <= 1e-6 * s.x_cost) { s.termination = VIO_TERM_CONVERGENCE; s.done = 1; }
            else {
                const double rel = s.cand_cost >= DBL_MAX ? -DBL_MAX : (s.step_eval_current - s.cand_cost) / s.model_change;
                s.rel = rel;
                s.tr_rel = rel;
                s.step_ok = rel > 1e-3;
                if (!s.step_ok) {
                    s.iter_cost = s.cand_cost + s.fixed_cost;
                    s.radius /= s.decrease_factor;
                    s.decrease_factor *= 2.0;
                }
            }
            accept = !s.done && s.step_ok;
            if (accept) {  // the trust region after an accepted step (trust_region_minimizer.cc:706-770):
                           // final here, so the next step's Schur groups need nothing of ph_prep
                const double q = s.rel;
                s.radius = s.radius / fmax(1.0 / 3.0, 1.0 - pow(2.0 * q - 1.0, 3.0));
                s.radius = fmin(1e16, s.radius);
                s.decrease_factor = 2.0;
            }
        }
        gst.need_lin = accept;
        gst.step_valid = 0;
        gst.ctrl_pending = 0;
        s_accept = accept;
        s_cur = accept ? gst.cur ^ 1 : gst.cur;
    }
    __syncthreads();
    stamp(21);
    if (s_accept) {  // x <- candidate: the parameter and IMU-Jacobian sets swap roles
        const int K = w.K;
        // the next linearisation's R_bw is the candidate's (ph_solve's pose cache)
        for (int e = t; e < PL24 * K; e += (int)blockDim.x)
            st_w<LS>(x.pr + x.ph.rlin + e, ld_w<LS>(x.pr + x.ph.pcc + 36 * (e / PL24) + 12 + e % PL24));
        if (threadIdx.x == 0) {
            gst.imu_cost = gst.imu_cand_cost;
            gst.cur ^= 1;
        }
    }
    __syncthreads();
    stamp(22);
    return s_cur;
}

// ------------------------------------------------------------------------------------------
// after a linearisation: chunk partials in order, IMU normal equations, gradient / column norms,
// the Ceres bookkeeping of IterationZero or of an accepted step; then the iteration finalisation
// and the f-space part of the step (LM diagonal, rhs)
// step control of the previous slot's step (when one is pending); returns the current parameter set
template <bool LS = false>
__device__ __forceinline__ int ph_prep_ctrl(const BaPools& P, int wi, PhShared& sh) {
    const PhState& g0 = *ph_ctx<LS>(P, wi).gs;
    if (g0.st.done) return g0.cur;
    int cur = g0.cur;
    if (g0.ctrl_pending)  // the previous slot's step: accept / reject it first (may swap the sets)
        cur = ph_ctrl_run<LS>(P, wi, reinterpret_cast<double(*)[6]>(sh.buf), sh.flag[2], sh.flag[3]);
    return cur;
}
// sU: BA_KMAX * 27 doubles of LDS (U, the chunk sums, for the gradient / column norms); after ph_prep_ctrl
// hctr / htarget / herr (cluster route, LS): the IMU member's gradient-record counter (PS_G), the count this
// iteration needs and the window's error word (a bounded wait; on time-out the error word is set)
template <bool LS = false>
__device__ __forceinline__ void ph_prep_rest(const BaPools& P, int wi, PhShared& sh, double* sU, int cur,
                                             const int* hctr = nullptr, int htarget = 0, int* herr = nullptr) {
    const PhCtx x = ph_ctx<LS>(P, wi, cur);
    const WinCtx& c = x.c;
    const BaWin& w = *c.w;
    PhState& gst = *x.gs;
    const int K = w.K;
    const bool fixed = w.fixed_iter != 0;
    // diagnostic slots: 0 U partial sums, 1 IMU factors (first) / load, 2 cost partials, 3 IMU normal
    // equations, 4 gradient + norms, 5 finalisation + LM diagonal
    PhStamp stamp(P.prof, wi);
    // the window's state (lane 0 wrote it in the control: read back by lane 0) and the tables in one round
    // trip; a finished solve stops here
    if (threadIdx.x == 0) {
        sh.flag[5] = gst.st.done;
        sh.st = gst.st;
        sh.flag[0] = gst.need_lin;
        sh.flag[1] = gst.first;
    }
    ph_tables(sh, x);
    __syncthreads();
    if (sh.flag[5]) return;
    const bool lin = sh.flag[0] != 0, first = sh.flag[1] != 0;
    double* s_f = x.pr + x.ph.fv;
    double* g_f = s_f + BA_NF_MAX;
    double* colsq = s_f + 2 * BA_NF_MAX;
    double* D_f = s_f + 3 * BA_NF_MAX;
    double* bb = s_f + 4 * BA_NF_MAX;
    if (lin) {
        const int nch = x.ph.nch;
        const double* cp = x.llp;  // linearisation partials (cost, max |g_l|, failure) per chunk
        // U = sum of the chunk partials (chunk order)
        double* U = x.pr + x.ph.U;
        const int E27 = 27 * K;
        if ((E27 & 1) == 0 && ((uintptr_t)x.lup & 15) == 0) {
            // 16-B pairs (E27 even, the partials 16-B aligned): twenty-four chunks' loads in flight
            const __amdgpu_buffer_rsrc_t rs = ph_rsrc(x.lup);
            for (int p = threadIdx.x; 2 * p < E27; p += BA_THREADS) {
                ph_d2 s2 = {0.0, 0.0};
                for (int q0 = 0; q0 < nch; q0 += 24) {
                    ph_d2 v[24];
#pragma unroll
                    for (int u = 0; u < 24; ++u) v[u] = q0 + u < nch ? ld_x2(rs, (q0 + u) * E27 + 2 * p) : ph_d2{0.0, 0.0};
#pragma unroll
                    for (int u = 0; u < 24; ++u)
                        if (q0 + u < nch) s2 += v[u];
                }
                U[2 * p] = s2.x;
                U[2 * p + 1] = s2.y;
                sU[2 * p] = s2.x;
                sU[2 * p + 1] = s2.y;
            }
        } else {
            for (int e = threadIdx.x; e < E27; e += BA_THREADS) {
                double s = 0.0;
                for (int q0 = 0; q0 < nch; q0 += 16) {  // sixteen chunks' loads in flight, summed in chunk order
                    double v[16];
#pragma unroll
                    for (int u = 0; u < 16; ++u)
                        v[u] = q0 + u < nch ? ld_x(x.lup + (int64_t)(q0 + u) * E27 + e) : 0.0;
#pragma unroll
                    for (int u = 0; u < 16; ++u)
                        if (q0 + u < nch) s += v[u];
                }
                U[e] = s;
                sU[e] = s;
            }
        }
        stamp(0);
        // IMU factors with Jacobians at this linearisation point (one lane per factor) and R_bw there:
        // evaluated here for the first linearisation only; after an accepted step they are the
        // candidate's (ph_solve evaluates them with Jacobians, ph_ctrl promotes them), bitwise the
        // same values at the same point
        double tic;
        if (first) {
            ph_pose_cache(sh, x, x.xp);
            __syncthreads();
            tic = block_sum(ph_imu_factors<true>(sh, x, x.xv, x.xb, true), sh.red);
            for (int e = threadIdx.x; e < 108 * K; e += BA_THREADS)
                if (e / 108 < VI_KMAX) st_x(x.imuJ + e, sh.imu_J[e / 108][e % 108]);
            for (int e = threadIdx.x; e < 9 * K; e += BA_THREADS)
                if (e / 9 < VI_KMAX) st_x(x.imur + e, sh.imu_r[e / 9][e % 9]);
            for (int e = threadIdx.x; e < PL24 * K; e += BA_THREADS) st_x(x.pr + x.ph.rlin + e, sh.pc[e / PL24][12 + e % PL24]);
        } else {
            tic = gst.imu_cost;
            for (int e = threadIdx.x; e < 108 * K; e += BA_THREADS)
                if (e / 108 < VI_KMAX && !P.csync) sh.imu_J[e / 108][e % 108] = x.imuJ[e];
            for (int e = threadIdx.x; e < 9 * K; e += BA_THREADS)
                if (e / 9 < VI_KMAX && !P.csync) sh.imu_r[e / 9][e % 9] = x.imur[e];
        }
        stamp(1);
        {   // chunk partials (cost, max |g_l|, failure) staged by all lanes, summed in chunk order by lane 0
            double cost = 0.0, gm = 0.0, fl = 0.0;
            double* stg = sh.buf + 1500;  // [BA_THREADS][3]: clear of buf[0..2] and of the IMU block area
            for (int q0 = 0; q0 < nch; q0 += BA_THREADS) {
                const int q = q0 + (int)threadIdx.x;
                double v[3];
#pragma unroll
                for (int i = 0; i < 3; ++i) v[i] = q < nch ? ld_x(cp + 4 * q + i) : 0.0;
                __syncthreads();
#pragma unroll
                for (int i = 0; i < 3; ++i) stg[3 * threadIdx.x + i] = v[i];
                __syncthreads();
                if (threadIdx.x == 0)
                    for (int u = 0; u < BA_THREADS && q0 + u < nch; ++u) {
                        cost += stg[3 * u];
                        gm = fmax(gm, stg[3 * u + 1]);
                        fl = fmax(fl, stg[3 * u + 2]);
                    }
            }
            if (threadIdx.x == 0) {
                sh.buf[0] = cost + tic;
                sh.buf[1] = gm;
                sh.buf[2] = fl;
            }
        }
        __syncthreads();
        stamp(2);
        double gmx = sh.buf[1];
        // IMU normal equations (factor order), then the f-space gradient and column norms.
        // pcode[p]: 3 m + c for component c of velocity m, 1000 + c / 2000 + c for bg / ba
        int* pcode = reinterpret_cast<int*>(sh.buf + 8 + NI_MAX * NI_MAX + NI_MAX);
        if (w.is_vi) {
            double* Hs = sh.buf + 8;                 // [ni][ni] | g [ni]
            for (int m = threadIdx.x; m < K; m += BA_THREADS)
                if (w.vel_f[m] >= 0)
                    for (int cc = 0; cc < 3; ++cc) pcode[w.vel_f[m] - w.np + cc] = 3 * m + cc;
            if (threadIdx.x < 3) {
                if (w.bg_f >= 0) pcode[w.bg_f - w.np + threadIdx.x] = 1000 + threadIdx.x;
                if (w.ba_f >= 0) pcode[w.ba_f - w.np + threadIdx.x] = 2000 + threadIdx.x;
            }
            if (first || !(P.csync || P.imu_in_back)) {  // else the accepted candidate's, formed by the cluster
                                                         // route's IMU member / ph_back_x's extra workgroup
                imu_normal_eq(Hs, sh.imu_J, sh.imu_r, w, sh.pvalid, sh.icol);
                for (int e = threadIdx.x; e < NI_MAX * NI_MAX + NI_MAX; e += BA_THREADS) st_x(x.himu + e, Hs[e]);
            } else if (LS) {
                // the cluster leader after the first iteration: the IMU rows' gradient, column norms, LM
                // diagonal and solve are the IMU member's (ph_imu_solve); only its gradient maximum is
                // needed here, below
            } else {
                if (hctr && threadIdx.x == 0) {  // (ph_imu_spec_normal_eq; its sc1 stores drained before the count)
                    const unsigned long long t0 = wait_clock();
                    while (__hip_atomic_load((const ph_gint*)hctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < htarget) {
                        if (wait_expired(t0) ||
                            __hip_atomic_load((const ph_gint*)herr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) {
                            __hip_atomic_store((ph_gint*)herr, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            break;
                        }
                        __builtin_amdgcn_s_sleep(1);
                    }
                }
                __syncthreads();
                for (int e = threadIdx.x; e < NI_MAX * NI_MAX + NI_MAX; e += BA_THREADS) Hs[e] = ld_x(x.himu + e);
            }
        }
        __syncthreads();
        stamp(3);
        const bool imu_off = LS && w.is_vi && !first;  // the IMU rows are the IMU member's (ph_imu_solve)
        const int nfl = imu_off ? w.np : w.nf;
        for (int f = threadIdx.x; f < nfl; f += BA_THREADS) {
            double gg, cs, xval;
            if (f < w.np) {
                int k = 0;
                for (int kk = 0; kk < K; ++kk)
                    if (sh.posef[kk] >= 0 && f >= sh.posef[kk] && f < sh.posef[kk] + 6) k = kk;
                const int i = f - sh.posef[k];
                gg = sU[27 * k + 21 + i];
                cs = sU[27 * k + i * 6 - (i * (i - 1)) / 2];
                xval = x.xp[6 * k + i];
            } else {
                const int p = f - w.np;
                gg = sh.buf[8 + NI_MAX * NI_MAX + p];
                cs = sh.buf[8 + p * w.ni + p];
                const int code = pcode[p];
                xval = code >= 2000 ? x.xb[3 + code - 2000] : code >= 1000 ? x.xb[code - 1000] : x.xv[code];
            }
            g_f[f] = gg;
            colsq[f] = cs;
            gmx = fmax(gmx, grad_term(xval, gg));
            if (first) st_x(s_f + f, 1.0 / (1.0 + sqrt(cs)));
        }
        if (imu_off && threadIdx.x == 0) {  // the IMU member's gradient maximum of the IMU rows (PS_G)
            const unsigned long long t0 = wait_clock();
            while (__hip_atomic_load((const ph_gint*)hctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < htarget) {
                if (wait_expired(t0) ||
                    __hip_atomic_load((const ph_gint*)herr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) {
                    __hip_atomic_store((ph_gint*)herr, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    break;
                }
                __builtin_amdgcn_s_sleep(1);
            }
            gmx = fmax(gmx, ld_x(x.pr + x.ph.imurec));
        }
        const double gmax = block_max(gmx, sh.redm);
        stamp(4);
        if (threadIdx.x == 0) {
            LmState& s = sh.st;
            const double cost = sh.buf[0];
            const bool fail = sh.buf[2] > 0.0;
            s.gmax = gmax;
            if (first) {  // IterationZero
                if (fail) {
                    s.termination = VIO_TERM_FAILURE;
                    s.initial_cost = s.fixed_cost;
                    s.final_cost = s.fixed_cost;
                    s.done = 1;
                } else {
                    s.x_cost = cost;
                    s.initial_cost = cost + s.fixed_cost;
                    s.final_cost = s.initial_cost;
                    s.step_eval_current = cost;
                    s.step_ok = 1;
                    s.iter_cost = cost + s.fixed_cost;
                    trace_begin(s);  // IterationZero (:195-229): valid and successful
                    s.tr_valid = 1;
                }
            } else {  // after an accepted step (trust_region_minimizer.cc:706-770)
                if (fail) {
                    s.termination = VIO_TERM_FAILURE;
                    s.done = 1;
                } else {  // (the radius update ran in ph_ctrl_run)
                    s.x_norm = sqrt(s.cand_x_norm2);
                    s.x_cost = cost;
                    s.step_eval_current = s.cand_cost;
                    s.iter_cost = cost + s.fixed_cost;
                }
            }
        }
        __syncthreads();
    }
    // FinalizeIterationAndCheckIfMinimizerCanContinue
    if (threadIdx.x == 0) {
        LmState& s = sh.st;
        if (!s.done) {
            if (s.step_ok) {
                s.nsucc++;
                if (s.x_cost < s.min_cost) s.min_cost = s.x_cost;
            } else {
                s.nunsucc++;
            }
            s.final_cost = fmin(s.final_cost, s.iter_cost);
            trace_push(c, s);
            if (s.iteration >= w.max_iter) { s.termination = VIO_TERM_NO_CONVERGENCE; s.done = 1; }
            else if (!fixed && s.step_ok && s.gmax <= 1e-10) { s.termination = VIO_TERM_CONVERGENCE; s.done = 1; }
            else if (!fixed && s.radius <= 1e-32) { s.termination = VIO_TERM_CONVERGENCE; s.done = 1; }
            if (!s.done) {
                s.iteration++;
                trace_begin(s);
            }
        }
    }
    __syncthreads();
    // f-space LM diagonal and rhs (levenberg_marquardt_strategy.cc:76-88)
    if (!sh.st.done) {
        const double radius = sh.st.radius;
        for (int f = threadIdx.x; f < (LS && w.is_vi && !first ? w.np : w.nf); f += BA_THREADS) {
            double d = colsq[f] * s_f[f] * s_f[f];
            d = fmin(fmax(d, 1e-6), 1e32);
            D_f[f] = sqrt(d / radius);
            bb[f] = s_f[f] * g_f[f];
        }
    }
    if (threadIdx.x == 0) {
        gst.st = sh.st;
        gst.need_lin = 0;
        gst.first = 0;
        gst.step_valid = 0;
        gst.ctrl_pending = sh.st.done ? 0 : 1;  // this slot's step kernels follow
    }
    stamp(5);
}
__device__ __forceinline__ void ph_prep_body(const BaPools& P, int wi, PhShared& sh, double* sU) {
    const int cur = ph_prep_ctrl(P, wi, sh);
    ph_prep_rest(P, wi, sh, sU, cur);
}
#ifndef VIO_BA_CLUSTER_TU
__global__ void __launch_bounds__(BA_THREADS) ph_prep_kernel(BaPools P) {
    const int wi = ph_wx(P);
    if (ph_skip(P, wi)) return;
    __shared__ PhShared sh;
    __shared__ double sU[BA_KMAX * 27];
    ph_prep_body(P, wi, sh, sU);
}
#endif

// ------------------------------------------------------------------------------------------
// Schur partials of a group of landmark chunks: V~ = s V s + D^2 factored per landmark (L^-1
// kept for the back-substitution), Z = W~ L^-T on the k-major LDS panel, the lower T(T+1)/2 tiles
// of Z Z^T and Z h on the matrix cores (k-steps split over the 4 waves, partials combined in order)
// the cluster route's one-barrier wave combine of a Schur group (ph_schur_body): four partial areas of
// NT 256 + 16 T doubles in the member's dynamic LDS (what follows PhSchurSh inside the kernel's BaShared-sized
// allotment); larger tile counts keep the wave-by-wave combine
//
// ST, the phase route's staged instance (ph_schur_staged_doubles: where two workgroups per CU still fit):
// the group's per-landmark values stay in LDS instead of coming back through memory once per chunk and
// keyframe lane.  The thread that factors landmark slot s = l - lbeg of the group keeps s_l and L^-1 in
// gcol[gsc KC + i GL + s] (i < 9, GL = gsc LC slots, gsc = min(gs, nch) chunks) and forms the slot's rhs
// entries h = L^-1 (g s) once, at gcol[KC chunk + 3 j] (every chunk's column padded to KC with zeros); the
// fill and the MFMA phase read them there, and the prefetch carries the observation's own values only.
// The four waves' partials are combined with two barriers: waves 0 and 1 write theirs to two areas over
// the dead panel, wave 2 folds both and its own into the first, wave 3 adds its own and writes the group's
// partials to memory from its MFMA layout (64 contiguous doubles per tile row).  Every expression and every
// summation order is that of the unstaged form: bitwise the same partials.
// The staged instance's combine of the four waves' partials (acc: the wave's lower tiles in MFMA layout, bacc:
// its rhs rows, already summed over the wave's k-lanes) with two barriers: waves 0 and 1 write theirs to two
// areas of E = NT 256 + 16 T doubles at comb (the dead panel), wave 2 folds both and its own into the first,
// wave 3 adds its own and writes the group's partials to sp from its MFMA layout (tile t, row 4e+kk, col r16 is
// element 256 t + 64 e + lane: 64 contiguous doubles per wave and store).  Every element is summed
// (((0 + p0) + p1) + p2) + p3, the order of the wave-by-wave combine.
template <int T, bool WT>
__device__ __forceinline__ void ph_schur_combine2(const d4* acc, const double* bacc, double* comb, double* sp) {
    static_assert(BA_THREADS / 64 == 4, "written for four waves");
    constexpr int NT = T * (T + 1) / 2, E = NT * 256 + 16 * T;
    const int wid = wave_id(), lane = threadIdx.x & 63, r16 = lane & 15, kk = lane >> 4;
    if (wid < 2) {
        double* mine = comb + wid * E;
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int e = 0; e < 4; ++e) mine[t * 256 + 64 * e + lane] = acc[t][e];
#pragma unroll
        for (int r = 0; r < T; ++r)
            if (kk == 0) mine[NT * 256 + 16 * r + r16] = bacc[r];
    }
    __syncthreads();
    if (wid == 2) {
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                double* d = comb + t * 256 + 64 * e + lane;
                *d = ((0.0 + *d) + d[E]) + acc[t][e];
            }
#pragma unroll
        for (int r = 0; r < T; ++r) {
            double* d = comb + NT * 256 + 16 * r + r16;
            if (kk == 0) *d = ((0.0 + *d) + d[E]) + bacc[r];
        }
    }
    __syncthreads();
    if (wid == 3) {
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int i = t * 256 + 64 * e + lane;
                st_w<WT>(sp + i, comb[i] + acc[t][e]);
            }
#pragma unroll
        for (int r = 0; r < T; ++r) {
            const int i = NT * 256 + 16 * r + r16;
            if (kk == 0) st_w<WT>(sp + i, comb[i] + bacc[r]);
        }
    }
}
struct PhSchurSh;
__host__ __device__ constexpr bool ph_schur_fast_combine(int T);
template <int T, bool WT = true, bool ST = false>
__device__ __forceinline__ void ph_schur_body(const PhCtx& x, int gi, double radius, double* Zt, double* gcol,
                                              const int* posef, const double* s_f, const double* rlin_k,
                                              const double* rcb_k, double* red, double* redm, PhStamp& stamp) {
    const WinCtx& c = x.c;
    const BaWin& w = *c.w;
    const int N = w.N, L = w.L, K = w.K, np = w.np;
    constexpr int KS = schur_ks(T);
    constexpr int NT = T * (T + 1) / 2;
    constexpr int NW = BA_THREADS / 64;
    const int LC = x.ph.LC;
    const int KC = schur_kc(LC);
    const int wid = wave_id(), lane = threadIdx.x & 63;
    const int r16 = lane & 15, kk = lane >> 4;
    double* ws = c.ws;
    const double* V = x.lv;
    const double* gl = x.lg;
    const double* sl = ws + c.L.s_l;
    double* Li = ws + c.L.Vi;
    const double* as = x.la;
    const double* xl = x.xl;
    const int* lk = reinterpret_cast<const int*>(ws + c.L.lk);
    const int lbeg = gi * w.gs * LC, lend = min(L, lbeg + w.gs * LC);
    const int jf = threadIdx.x / K, kf = threadIdx.x - jf * K;
    const int pf = jf < LC ? posef[kf] : -1;
    // the fill inputs of a lane are loaded one chunk ahead (in flight during the previous chunk's
    // MFMA phase), its observation index two chunks ahead: no global round trip between barriers
    auto obs_of = [&](int l0c) -> int {
        const int l = l0c + jf;
        return (pf >= 0 && l0c < lend && l < min(l0c + LC, L)) ? lk[16 * l + kf] : -1;
    };
    double pas, ppw[3], psv[3], pli[6];
    double hg[3], hs[3], hl[6];  // the rhs column's inputs (lanes < LC: landmark l0c + lane), likewise ahead
    bool pon = false, hon = false;
    auto fetch_at = [&](int l, int o, bool var) {
        pon = var;
        if (pon) {
            pas = as[o];
#pragma unroll
            for (int i = 0; i < 3; ++i) ppw[i] = xl[3 * l + i];
            if constexpr (!ST) {
#pragma unroll
                for (int i = 0; i < 3; ++i) psv[i] = sl[(int64_t)i * L + l];
#pragma unroll
                for (int i = 0; i < 6; ++i) pli[i] = Li[(int64_t)i * L + l];
            }
        }
    };
    auto fetch = [&](int l0c, int o) {
        const int l = l0c + jf;
        fetch_at(l, o, o >= 0 && c.lm_var[l]);
        if constexpr (!ST) {
            const int lg = l0c + (int)threadIdx.x;
            hon = (int)threadIdx.x < LC && lg < min(l0c + LC, L) && c.lm_var[lg];
            if (T <= 4 && hon) {  // (larger tile counts: no registers to spare, loaded in the chunk's turn)
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    hg[i] = gl[(int64_t)i * L + lg];
                    hs[i] = sl[(int64_t)i * L + lg];
                }
#pragma unroll
                for (int i = 0; i < 6; ++i) hl[i] = Li[(int64_t)i * L + lg];
            }
        }
    };
    const int gsc = min(w.gs, w.nch), GL = gsc * LC;  // staged: chunks and landmark slots of a group
    double* sst = gcol + gsc * KC;
    // staged: the lane's landmark values of chunk l0c from the group's LDS copy (into registers a chunk ahead,
    // like the rest of the fill's inputs: the fill itself then waits for no LDS read)
    auto staged = [&](int l0c) {
        if (pon) {
            const double* sv = sst + (l0c - lbeg + jf);
#pragma unroll
            for (int i = 0; i < 3; ++i) psv[i] = sv[i * GL];
#pragma unroll
            for (int i = 0; i < 6; ++i) pli[i] = sv[(3 + i) * GL];
        }
    };
    // staged: nothing the first fill reads from memory waits for the landmark blocks -- the first two chunks'
    // observation indices and the first chunk's landmark flags are requested with the blocks' own inputs, the
    // observation's values as soon as its index is there, and arrive while the blocks are factored
    int o_nxt = -1, o_first = -1, var_first = 0;
    bool first_done = !ST;
    if constexpr (ST) {
        o_first = obs_of(lbeg);
        o_nxt = obs_of(lbeg + LC);
        var_first = c.lm_var[min(lbeg + jf, L - 1)];
        // the panel is zeroed under those loads; the barriers of the blocks' reduction order it before the fills
        for (int e = threadIdx.x; e < KC * KS; e += BA_THREADS) Zt[e] = 0.0;
    }
    // (1) landmark blocks of the group
    int bad = 0;
    for (int l = lbeg + threadIdx.x; l < (ST ? lbeg + GL : lend); l += BA_THREADS) {
        double s0, s1, s2, v[6], g[3];
        double* hc = nullptr;
        if constexpr (ST) {
            // every slot's rhs entries and its chunk's padding start at zero; the loads in one batch
            const int s = l - lbeg, ci = walk_div(s, w.rLC), j = s - ci * LC;
            hc = gcol + ci * KC + 3 * j;
            hc[0] = hc[1] = hc[2] = 0.0;
            if (j == LC - 1)
                for (int e = 3 * LC; e < KC; ++e) gcol[ci * KC + e] = 0.0;
            const int lq = min(l, lend - 1);
            const int var = c.lm_var[lq];
            s0 = sl[lq], s1 = sl[(int64_t)L + lq], s2 = sl[2 * (int64_t)L + lq];
            for (int i = 0; i < 6; ++i) v[i] = V[(int64_t)i * L + lq];
            for (int i = 0; i < 3; ++i) g[i] = gl[(int64_t)i * L + lq];
            if (!first_done) {
                fetch_at(lbeg + jf, o_first, o_first >= 0 && var_first);
                first_done = true;
            }
            if (l >= lend || !var) continue;
        } else {
            if (!c.lm_var[l]) continue;
            s0 = sl[l], s1 = sl[(int64_t)L + l], s2 = sl[2 * (int64_t)L + l];
            for (int i = 0; i < 6; ++i) v[i] = V[(int64_t)i * L + l];
        }
        double a00 = v[0] * s0 * s0, a01 = v[1] * s0 * s1, a02 = v[2] * s0 * s2;
        double a11 = v[3] * s1 * s1, a12 = v[4] * s1 * s2, a22 = v[5] * s2 * s2;
        a00 += fmin(fmax(a00, 1e-6), 1e32) / radius;
        a11 += fmin(fmax(a11, 1e-6), 1e32) / radius;
        a22 += fmin(fmax(a22, 1e-6), 1e32) / radius;
        if (!(a00 > 0.0)) { bad = 1; continue; }
        double l00 = sqrt(a00), l10 = a01 / l00, l20 = a02 / l00;
        double t11 = a11 - l10 * l10;
        if (!(t11 > 0.0)) { bad = 1; continue; }
        double l11 = sqrt(t11), l21 = (a12 - l20 * l10) / l11;
        double t22 = a22 - l20 * l20 - l21 * l21;
        if (!(t22 > 0.0)) { bad = 1; continue; }
        double l22 = sqrt(t22);
        double i00 = 1.0 / l00, i11 = 1.0 / l11, i22 = 1.0 / l22;
        double i10 = -l10 * i00 * i11, i21 = -l21 * i11 * i22;
        double i20 = -(l20 * i00 + l21 * i10) * i22;
        Li[l] = i00;
        Li[(int64_t)L + l] = i10;
        Li[2 * (int64_t)L + l] = i11;
        Li[(int64_t)3 * L + l] = i20;
        Li[(int64_t)4 * L + l] = i21;
        Li[(int64_t)5 * L + l] = i22;
        if constexpr (ST) {
            double* sv = sst + (l - lbeg);
            sv[0] = s0; sv[GL] = s1; sv[2 * GL] = s2;
            sv[3 * GL] = i00; sv[4 * GL] = i10; sv[5 * GL] = i11;
            sv[6 * GL] = i20; sv[7 * GL] = i21; sv[8 * GL] = i22;
            const double g0 = g[0] * s0, g1 = g[1] * s1, g2 = g[2] * s2;
            // h = L^-1 (g s) with the fused operations spelled out, as every unstaged instance contracts the
            // per-chunk expressions below (left to the compiler here, h1 came out with the other product fused)
            hc[0] = i00 * g0;
            hc[1] = fma(i10, g0, i11 * g1);
            hc[2] = fma(i22, g2, fma(i20, g0, i21 * g1));
        }
    }
    if (!first_done) fetch_at(lbeg + jf, o_first, o_first >= 0 && var_first);  // (a thread without a slot)
    const double anybad = block_max((double)bad, redm);
    if (threadIdx.x == 0) st_w<WT>(x.pr + x.ph.bpart + 8 * gi, anybad);
    stamp(6);
    // (2) panels
    d4 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = d4{0.0, 0.0, 0.0, 0.0};
    double bacc[T];
#pragma unroll
    for (int r = 0; r < T; ++r) bacc[r] = 0.0;
    const double* rbw = rlin_k + PL24 * (kf < BA_KMAX ? kf : 0);  // LDS (keeps the fill's registers low)
    const double* rcb = rcb_k + 9 * (kf < BA_KMAX ? kf : 0);
    if constexpr (!ST) {
        for (int e = threadIdx.x; e < KC * KS; e += BA_THREADS) Zt[e] = 0.0;
        for (int e = threadIdx.x; e < KC; e += BA_THREADS) gcol[e] = 0.0;
        __syncthreads();
    }
    stamp(15);
    if (!anybad) {
        if constexpr (ST) {
            staged(lbeg);
        } else {
            fetch(lbeg, obs_of(lbeg));
            o_nxt = obs_of(lbeg + LC);
        }
        const double* gch = gcol;  // the chunk's rhs column
        for (int l0 = lbeg; l0 < lend; l0 += LC) {
            const int l1 = min(l0 + LC, L);
            // fill
            if (pf >= 0) {
                double* zt = Zt + 3 * jf * KS + pf;  // Zt[(3 jf + cc) KS + pf + i] = Z[i][cc]
                if (pon) {
                    double pj[12], lj[6], paj[6], ppb[3];
                    factor_ap_at(rbw, rcb, ppw, w.cols, w.rows, w.Lw, pas, paj, ppb);
                    jac_from_ap(paj, ppb, rbw, pj, lj);
                    const double b0 = lj[0] * psv[0], b1 = lj[1] * psv[1], b2 = lj[2] * psv[2];
                    const double d0 = lj[3] * psv[0], d1 = lj[4] * psv[1], d2 = lj[5] * psv[2];
#pragma unroll
                    for (int i = 0; i < 6; ++i) {
                        const double sp = s_f[pf + i];
                        const double a = pj[i] * sp, e = pj[6 + i] * sp;
                        const double W0 = a * b0 + e * d0, W1 = a * b1 + e * d1, W2 = a * b2 + e * d2;
                        zt[i] = W0 * pli[0];
                        zt[KS + i] = W0 * pli[1] + W1 * pli[2];
                        zt[2 * KS + i] = W0 * pli[3] + W1 * pli[4] + W2 * pli[5];
                    }
                } else {
#pragma unroll
                    for (int cc = 0; cc < 3; ++cc)
#pragma unroll
                        for (int i = 0; i < 6; ++i) zt[cc * KS + i] = 0.0;
                }
            }
            if (!ST && (int)threadIdx.x < LC) {
                double h0 = 0.0, h1 = 0.0, h2 = 0.0;
                if (hon) {
                    if constexpr (T > 4) {
                        const int lg = l0 + threadIdx.x;
#pragma unroll
                        for (int i = 0; i < 3; ++i) {
                            hg[i] = gl[(int64_t)i * L + lg];
                            hs[i] = sl[(int64_t)i * L + lg];
                        }
#pragma unroll
                        for (int i = 0; i < 6; ++i) hl[i] = Li[(int64_t)i * L + lg];
                    }
                    const double g0 = hg[0] * hs[0], g1 = hg[1] * hs[1], g2 = hg[2] * hs[2];
                    const double i00 = hl[0], i10 = hl[1], i11 = hl[2];
                    const double i20 = hl[3], i21 = hl[4], i22 = hl[5];
                    h0 = i00 * g0;
                    h1 = i10 * g0 + i11 * g1;
                    h2 = i20 * g0 + i21 * g1 + i22 * g2;
                }
                gcol[3 * threadIdx.x] = h0;
                gcol[3 * threadIdx.x + 1] = h1;
                gcol[3 * threadIdx.x + 2] = h2;
            }
            __syncthreads();
            stamp(7);
            if (l0 + LC < lend) {  // the next chunk's inputs, loading while this chunk's MFMAs run
                fetch(l0 + LC, o_nxt);
                if constexpr (ST) staged(l0 + LC);
                o_nxt = obs_of(l0 + 2 * LC);
            }
            const int nsteps = (3 * (l1 - l0) + 3) >> 2;
            for (int st = wid; st < nsteps; st += NW) {
                const int kr = (4 * st + kk) * KS;
                double f[T];
#pragma unroll
                for (int r = 0; r < T; ++r) f[r] = Zt[kr + 16 * r + r16];
                const double gq = gch[4 * st + kk];
#pragma unroll
                for (int r = 0, t = 0; r < T; ++r)
#pragma unroll
                    for (int q = 0; q <= r; ++q, ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(f[r], f[q], acc[t], 0, 0, 0);
#pragma unroll
                for (int r = 0; r < T; ++r) bacc[r] += f[r] * gq;
            }
            __syncthreads();
            stamp(13);
            if constexpr (ST) gch += KC;
        }
    }
    // combine the 4 waves' partials in order (in LDS, over the dead panel), then one global write
    if constexpr (!ST) __syncthreads();  // (staged: the last barrier above, on either path, already ended every use)
    double* comb = Zt;
#pragma unroll
    for (int r = 0; r < T; ++r) {
        bacc[r] += __shfl_xor(bacc[r], 16, 64);
        bacc[r] += __shfl_xor(bacc[r], 32, 64);
    }
    constexpr int E = NT * 256 + 16 * T;
    if constexpr (WT && ph_schur_fast_combine(T)) {
        // cluster route (the whole member LDS is free here): every wave writes its partial to an area of its
        // own, one barrier, then each element is summed ((((0 + p0) + p1) + p2) + p3, the order of the
        // wave-by-wave combine below) by all threads at once and written out in 16-B pairs
        double* mine = comb + wid * E;
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int e = 0; e < 4; ++e) mine[t * 256 + (4 * e + kk) * 16 + r16] = acc[t][e];
#pragma unroll
        for (int r = 0; r < T; ++r)
            if (kk == 0) mine[NT * 256 + 16 * r + r16] = bacc[r];
        __syncthreads();
        double* sp = x.pr + x.ph.spart + (int64_t)gi * E;
        const __amdgpu_buffer_rsrc_t rs = ph_rsrc(sp);
        for (int e = 2 * threadIdx.x; e < E; e += 2 * BA_THREADS) {
            ph_d2 v = {0.0, 0.0};
#pragma unroll
            for (int wv = 0; wv < NW; ++wv) v += *reinterpret_cast<const ph_d2*>(comb + wv * E + e);
            st_x2(rs, e, v);
        }
        stamp(14);
        return;
    }
    if constexpr (ST) {
        ph_schur_combine2<T, WT>(acc, bacc, comb, x.pr + x.ph.spart + (int64_t)gi * E);
        stamp(14);
        return;
    }
    for (int wv = 0; wv < NW; ++wv) {
        if (wid == wv) {
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    double* dst = comb + t * 256 + (4 * e + kk) * 16 + r16;  // tile t, row 4e+kk, col r16
                    *dst = (wv == 0 ? 0.0 : *dst) + acc[t][e];
                }
#pragma unroll
            for (int r = 0; r < T; ++r) {
                double* dst = comb + NT * 256 + 16 * r + r16;
                if (kk == 0) *dst = (wv == 0 ? 0.0 : *dst) + bacc[r];
            }
        }
        __syncthreads();
    }
    double* sp = x.pr + x.ph.spart + (int64_t)gi * (NT * 256 + 16 * T);
    if constexpr (WT) {  // pairs (the group's extent NT 256 + 16 T is even, sp 16-B aligned)
        const __amdgpu_buffer_rsrc_t rs = ph_rsrc(sp);
        for (int e = 2 * threadIdx.x; e < NT * 256 + 16 * T; e += 2 * BA_THREADS)
            st_x2(rs, e, *reinterpret_cast<const ph_d2*>(comb + e));
    } else {
        for (int e = threadIdx.x; e < NT * 256 + 16 * T; e += BA_THREADS) *(sp + e) = comb[e];
    }
    stamp(14);
    (void)np;
    (void)red;
}

// dynamic LDS of ph_schur_kernel for a tile count: the panel + rhs column, or the wave-combine area
__host__ __device__ inline int ph_schur_lds_doubles(int T, int LC) {
    const int a = schur_kc(LC) * schur_ks(T) + schur_kc(LC);
    const int b = T * (T + 1) / 2 * 256 + 16 * T;
    return a > b ? a : b;
}

// tile-count instance of a window (the monolithic kernel's switch: 1..5, anything else 6)
__host__ __device__ constexpr int ph_schur_t(int T) { return T >= 1 && T <= 5 ? T : 6; }

// the small LDS inputs of a Schur group (per window: pose blocks, Jacobi scaling, R_bw at the linearisation)
struct PhSchurSh {
    int posef[BA_KMAX];
    double s_f[BA_NF_MAX];
    double rlin[BA_KMAX * PL24];  // pose cache at the linearisation point
    double rcb[BA_KMAX * 9];      // R_cb_raw
    double red[BA_THREADS / 64 + 4], redm[BA_THREADS / 64 + 4];
};
__host__ __device__ constexpr bool ph_schur_fast_combine(int T) {
    return ((sizeof(PhSchurSh) + 15) & ~(size_t)15) + sizeof(double) * (BA_THREADS / 64) * (T * (T + 1) / 2 * 256 + 16 * T) <=
           sizeof(BaShared);
}
// The staged instance of ph_schur_kernel (ph_schur_body's ST) for a window's tile count, chunk size and
// chunks per group gsc = min(gs, nch): its dynamic LDS in doubles -- the panel, the group's rhs columns
// (gsc KC) and landmark values (9 gsc LC), or the two combine areas where those are larger -- or 0 where
// the instance does not apply: T = 6 (its combine areas alone exceed the panel's allotment), or two
// workgroups per CU no longer fit the CU's 160 KB (each workgroup's static + dynamic LDS rounded up to 2 KB,
// above any allocation granule).  Without two workgroups a CU's matrix cores idle through every fill.
constexpr int PH_LDS_CU = 160 * 1024, PH_LDS_ROUND = 2048;
__host__ __device__ inline int ph_schur_staged_doubles(int T, int LC, int gsc) {
    if (T < 1 || T > 5 || gsc < 1) return 0;
    const int KC = schur_kc(LC);
    const int64_t a = (int64_t)KC * schur_ks(T) + (int64_t)gsc * KC + (int64_t)9 * gsc * LC;
    const int64_t b = 2 * (T * (T + 1) / 2 * 256 + 16 * T);
    const int64_t d = a > b ? a : b;
    const int64_t wg = ((int64_t)sizeof(PhSchurSh) + 8 * d + PH_LDS_ROUND - 1) / PH_LDS_ROUND * PH_LDS_ROUND;
    return 2 * wg <= PH_LDS_CU && (int64_t)gsc * LC < WALK_TMAX ? (int)d : 0;
}
__device__ __forceinline__ void ph_schur_inputs(PhSchurSh& ss, const PhCtx& x, const double* rlin) {
    const BaWin& w = *x.c.w;
    for (int k = threadIdx.x; k < BA_KMAX; k += BA_THREADS) ss.posef[k] = k < w.K ? w.pose_f[k] : -1;
    for (int f = threadIdx.x; f < BA_NF_MAX; f += BA_THREADS) ss.s_f[f] = f < w.nf ? ld_x(x.pr + x.ph.fv + f) : 0.0;
    if (rlin) {
        for (int e = threadIdx.x; e < PL24 * w.K; e += BA_THREADS) ss.rlin[e] = rlin[e];
    } else {
        ph_ld_block(ss.rlin, x.pr + x.ph.rlin, PL24 * w.K);
    }
    for (int e = threadIdx.x; e < 9 * w.K; e += BA_THREADS) ss.rcb[e] = x.pr[x.ph.rcb + e];
}
// group gi of window x at trust-region radius `radius`; dyn: the panel LDS (ph_schur_lds_doubles)
template <int TI, bool WT = true, bool ST = false>
__device__ __forceinline__ void ph_schur_group(const BaPools& P, const PhCtx& x, int wi, int gi, double radius,
                                               PhSchurSh& ss, double* dyn) {
    const BaWin& w = *x.c.w;
    const int KC = schur_kc(x.ph.LC);
    double* Zt = dyn;
    double* gcol = dyn + KC * schur_ks(w.T);
    // diagnostic slots (group 0 of each window): 6 landmark blocks, 15 panel zeroing, 7 fills, 13 MFMA
    // phases, 14 wave combine + partial write
    PhStamp stamp(gi == 0 ? P.prof : nullptr, wi);
    ph_schur_body<TI, WT, ST>(x, gi, radius, Zt, gcol, ss.posef, ss.s_f, ss.rlin, ss.rcb, ss.red, ss.redm, stamp);
}
#ifndef VIO_BA_CLUSTER_TU
// ST: the staged instance (every window of the launch's tile count fits it, ph_extents).  Its head asks for
// the LM state and the small inputs, none of whose addresses depend on the state, in one round trip, and
// selects the current parameter set's view afterwards
template <int TI, bool ST>
__global__ void __launch_bounds__(BA_THREADS, PH_SCHUR_OCC) ph_schur_kernel(BaPools P) {
    const int wi = ph_wy(P);
    if (ph_skip(P, wi) || ph_schur_t(P.win[wi].T) != TI) return;
    extern __shared__ __align__(16) double ph_dyn[];
    __shared__ PhSchurSh ss;
    if constexpr (ST) {
        const PhCtx x0 = ph_ctx(P, wi, 0);
        if (ph_sub() >= x0.ph.ng) return;
        const int cur = x0.gs->cur, done = x0.gs->st.done;
        const double radius = x0.gs->st.radius;
        ph_schur_inputs(ss, x0, nullptr);
        if (done) return;
        __syncthreads();
        ph_schur_group<TI, false, true>(P, ph_ctx_at(x0, cur), wi, ph_sub(), radius, ss, ph_dyn);
    } else {
        const PhCtx x = ph_ctx(P, wi);
        if (ph_sub() >= x.ph.ng) return;
        if (x.gs->st.done) return;
        ph_schur_inputs(ss, x, nullptr);
        __syncthreads();
        ph_schur_group<TI, false>(P, x, wi, ph_sub(), x.gs->st.radius, ss, ph_dyn);
    }
}
template <bool ST>
static const void* ph_schur_fn_of(int TI) {
    switch (TI) {
        case 1: return (const void*)ph_schur_kernel<1, ST>;
        case 2: return (const void*)ph_schur_kernel<2, ST>;
        case 3: return (const void*)ph_schur_kernel<3, ST>;
        case 4: return (const void*)ph_schur_kernel<4, ST>;
        case 5: return (const void*)ph_schur_kernel<5, ST>;
        default: return ST ? nullptr : (const void*)ph_schur_kernel<6, false>;  // (no staged instance of 6)
    }
}
static const void* ph_schur_fn(int TI, bool staged) { return staged ? ph_schur_fn_of<true>(TI) : ph_schur_fn_of<false>(TI); }
template <bool ST>
static void ph_schur_launch_of(int TI, dim3 grid, size_t lds, hipStream_t stream, const BaPools& P) {
    switch (TI) {
        case 1: hipLaunchKernelGGL((ph_schur_kernel<1, ST>), grid, dim3(BA_THREADS), lds, stream, P); break;
        case 2: hipLaunchKernelGGL((ph_schur_kernel<2, ST>), grid, dim3(BA_THREADS), lds, stream, P); break;
        case 3: hipLaunchKernelGGL((ph_schur_kernel<3, ST>), grid, dim3(BA_THREADS), lds, stream, P); break;
        case 4: hipLaunchKernelGGL((ph_schur_kernel<4, ST>), grid, dim3(BA_THREADS), lds, stream, P); break;
        case 5: hipLaunchKernelGGL((ph_schur_kernel<5, ST>), grid, dim3(BA_THREADS), lds, stream, P); break;
        default:
            if constexpr (!ST) hipLaunchKernelGGL((ph_schur_kernel<6, false>), grid, dim3(BA_THREADS), lds, stream, P);
            break;
    }
}
static void ph_schur_launch(int TI, bool staged, dim3 grid, size_t lds, hipStream_t stream, const BaPools& P) {
    if (staged) ph_schur_launch_of<true>(TI, grid, lds, stream, P);
    else ph_schur_launch_of<false>(TI, grid, lds, stream, P);
}
#endif

// ------------------------------------------------------------------------------------------
// The IMU terms at the candidate, at the end of ph_solve: the IMU part of the model change
// (-(J d)^T (r + J d / 2) per factor, trust_region_minimizer.cc:424-439) and the IMU factors at the
// candidate with their Jacobians (the next linearisation point if the step is accepted): thread
// 12(k-1) + j evaluates factor k's common part and Jacobian column j (imu_eval_wave), then thread k-1
// sums factor k's squared residuals in row order (imu_eval's caller's order).  Partials go to slot nch
// of the chunk partials.  sh.pc holds the candidate pose cache, dlt the f-space step, rst is 9 K doubles
// of scratch.  (In ph_back_kernel, 4 waves per SIMD, the call of the IMU factor code gave the kernel a
// scratch segment, which slowed the whole back-substitution walk.)
template <bool INL = false, class SH>
__device__ __forceinline__ void ph_imu_terms(SH& sh, const PhCtx& x, const double* dlt, double* rst, bool use_icol,
                                             PhStamp* st = nullptr) {
    const int tid = ph_tid();
    const WinCtx& c = x.c;
    const BaWin& w = *c.w;
    const int K = w.K;
    double mc = 0.0, icc = 0.0;
    // diagnostic slots (st): 24 loads, 26 factors at the candidate beside the model change, 27 cost
    auto mark = [&](int slot) { if (st) (*st)(slot); };
    static_assert(BA_THREADS >= 128 + 9 * (VI_KMAX - 1), "model-change lanes on waves 2-3");
    if (w.is_vi) {
        for (int e = tid; e < 108 * K; e += BA_THREADS)
            if (e / 108 < VI_KMAX) sh.imu_J[e / 108][e % 108] = ld_x(x.imuJ + e);
        for (int e = tid; e < 9 * K; e += BA_THREADS)
            if (e / 9 < VI_KMAX) sh.imu_r[e / 9][e % 9] = ld_x(x.imur + e);
        // the candidate velocities / biases (ph_solve's) staged through LDS
        double* cvb = rst + 1600;  // [3K velocities | 6 biases]
        for (int e = tid; e < 3 * K + 6; e += BA_THREADS) cvb[e] = ld_x(e < 3 * K ? x.cv + e : x.cb + e - 3 * K);
        __syncthreads();
        mark(24);
        if (tid < 128) {
            // waves 0-1: factor k at the candidate with its Jacobian, thread 12 (k - 1) + column (imu_eval_wave)
            const int k = 1 + tid / 12, col = tid % 12;
            if (k < K && c.preint_valid[k]) {
                double r;
                (INL ? imu_eval_wave_inl : imu_eval_wave)(c.preint[k], c.sqi + 81 * k, w.gravity, sh.pc[k - 1], sh.pc[k], cvb + 3 * (k - 1), cvb + 3 * K,
                              cvb + 3 * K + 3, cvb + 3 * k, col, r, x.imuJc + 108 * k);
                if (col < 9) {
                    x.imurc[9 * k + col] = r;
                    rst[9 * k + col] = r;
                }
            }
        } else {
            // waves 2-3 meanwhile: the IMU part of the model change, thread 128 + 9 (k - 1) + i for residual row i
            // of factor k: m = (J delta)_i, mc -= m (r_i + m / 2)
            const int u = tid - 128, k = 1 + u / 9, i = u % 9;
            if (k < K && c.preint_valid[k]) {
                double m = 0.0;
                for (int cpp = 0; cpp < 12; ++cpp) {
                    const int p = use_icol ? sh.icol[k][cpp] : imu_col(w, k, cpp);
                    if (p >= 0) m += sh.imu_J[k][12 * i + cpp] * dlt[w.np + p];
                }
                mc -= m * (sh.imu_r[k][i] + m / 2.0);
            }
        }
        __syncthreads();
        mark(26);
        const int kf = 1 + tid;
        if (kf < K && c.preint_valid[kf]) {
            double sq = 0.0;
            for (int i = 0; i < 9; ++i) sq += rst[9 * kf + i] * rst[9 * kf + i];
            icc += 0.5 * sq;
        }
        mark(27);
    }
    double rv[2] = {mc, icc};
    block_reduce<2, 0>(rv, sh.redv);
    if (tid == 0) {
        double* cp = x.pr + x.ph.cpart + 8 * x.ph.nch;
        st_x(cp, rv[0]);
        st_x(cp + 1, 0.0);
        st_x(cp + 2, 0.0);
        st_x(cp + 3, rv[1]);
        st_x(cp + 4, 0.0);
        st_x(cp + 5, 0.0);
    }
}
// the candidate's IMU normal equations (speculative, like the candidate linearisation of the walks: ph_prep
// takes them when the step is accepted instead of forming them on its serial path); the cluster route's
// IMU member after its ph_imu_terms (rst: the candidate residuals it left in LDS), while the leader runs the
// step control
template <class SH>
__device__ __forceinline__ void ph_imu_spec_normal_eq(SH& sh, const PhCtx& x, double* rst) {
    const BaWin& w = *x.c.w;
    const int K = w.K;
    __syncthreads();
    for (int e = threadIdx.x; e < 108 * K; e += BA_THREADS)
        if (e / 108 < VI_KMAX) sh.imu_J[e / 108][e % 108] = x.imuJc[e];
    for (int e = threadIdx.x; e < 9 * K; e += BA_THREADS)
        if (e / 9 < VI_KMAX) sh.imu_r[e / 9][e % 9] = rst[e];
    __syncthreads();
    double* Hs = rst + 256;
    imu_normal_eq(Hs, sh.imu_J, sh.imu_r, w, sh.pvalid, sh.icol);
    for (int e = threadIdx.x; e < NI_MAX * NI_MAX + NI_MAX; e += BA_THREADS) st_x(x.himuc + e, Hs[e]);
}

// ------------------------------------------------------------------------------------------
// reduced system: U~ + IMU block + D^2, minus the Schur partials (group order); blocked Cholesky
// and solve; candidates of poses / velocities / biases, pose cache at the candidate, IMU model
// change and IMU candidate cost
// mode 0: the whole phase (phase route); the cluster route splits it around its wait for the Schur groups:
// mode 1 assembles everything but the Schur partials into S / b (before the wait), mode 2 subtracts the
// partials in group-block order -- the same operations in the same order as mode 0's per-element
// base - p_0 - p_1 - ... -- and continues with the factorisation (after the wait)
template <bool LS = false>
// (LS, VI windows: the velocity / bias block is the IMU member's, ph_imu_solve; ictr / itarget / ierr: its
// solve-record counter PS_I, the count this iteration needs, the error word -- mode 2 waits for it at the end)
__device__ __forceinline__ void ph_solve_body(const BaPools& P, int wi, BaShared& sh, int mode = 0,
                                              const int* ictr = nullptr, int itarget = 0, int* ierr = nullptr) {
    const bool do_pre = mode != 2, do_post = mode != 1;
    const PhCtx x = ph_ctx<LS>(P, wi);
    const WinCtx& c = x.c;
    const BaWin& w = *c.w;
    PhState& gst = *x.gs;
    if (gst.st.done) return;
    // the system this workgroup solves: every block, or (cluster route, VI) the pose block only
    const bool imu_off = LS && w.is_vi;
    const int K = w.K, nf = imu_off ? w.np : w.nf, np = w.np, ls = s_ld(nf), npS = 16 * ((nf + 15) >> 4);
    // (cluster route, diagnostic slots 29 / 30: mode 1's and mode 2's time up to the assembly loop)
    const int head_slot = mode == 1 ? 29 : mode == 2 ? 30 : -1;
    // diagnostic slots: 16 assembly, 17 Cholesky + solves, 18 candidates + pose cache, 19 IMU model
    // change + candidate factors, 20 reductions
    PhStamp stamp(P.prof, wi);
    const double* s_f = x.pr + x.ph.fv;
    const double* D_f = s_f + 3 * BA_NF_MAX;
    const double* bb = s_f + 4 * BA_NF_MAX;
    double* ws = c.ws;
    // assemble the lower 16x16 tiles of S, each element written once: (U~ or the IMU block) + D^2,
    // minus the Schur partials of the landmark groups in group order (the same operation order as
    // assemble_S + schur_gemm's wave combine); every global input is loaded before any is used
    const int nb = (nf + 15) >> 4, ntile = nb * (nb + 1) / 2;
    const int ni = w.ni, T = w.T, NT = T * (T + 1) / 2, ng = x.ph.ng;
    // global inputs requested together, in the order they are consumed (a wait for the first ones leaves
    // the later ones in flight): the groups' failure flags, the small inputs (s_f, D_f, rhs, U, the IMU
    // block), the first round of the Schur partials (10 tile elements per thread x 4 groups) and the rhs
    // partials
    int bad = 0;
    if (do_post && LS)  // the members' reduce-scatter leaves the groups' failure flag after the total
        bad = ld_x(x.pr + x.ph.stot + (int64_t)NT * 256 + 16 * T) > 0.0;
    else if (do_post)
        for (int q = 0; q < ng; ++q) bad |= ld_x(x.pr + x.ph.bpart + 8 * q) > 0.0;
    const double* U = x.pr + x.ph.U;
    const int nsm = 3 * nf + 27 * K + (w.is_vi && !imu_off ? ni * ni : 0);
    auto small_in = [&](int e) -> double {  // phase-region f vectors: s_f (0), D_f (3), rhs s_f g_f (4) x BA_NF_MAX
        return e >= nsm ? 0.0 : e < 3 * nf ? s_f[(e < nf ? 0 : e < 2 * nf ? 3 : 4) * BA_NF_MAX + e % nf]
                                : e < 3 * nf + 27 * K ? U[e - 3 * nf] : ld_x(x.himu + e - 3 * nf - 27 * K);
    };
    double sm0[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) sm0[u] = do_pre ? small_in(threadIdx.x + u * BA_THREADS) : 0.0;
    // the Schur partials to subtract, in group order: every group's (phase route) or, in the cluster route
    // (LS), their sum over all groups, formed by the members (ph_cluster_kernel's reduce-scatter)
    const double* sp0 = x.pr + (LS ? x.ph.stot : x.ph.spart);
    const int ngp = LS ? 1 : ng;
    const int64_t gstride = (int64_t)NT * 256 + 16 * T;
    constexpr int EU = 10;
    static_assert(EU % 2 == 0, "element pairs");
    // element u of a thread's round starting at r0, in 16-B pairs (thread t, pair u / 2: elements
    // 2 (t + (u / 2) BA_THREADS) + {0, 1}): the first round's partials of up to four groups (the cluster
    // route: their total) are requested as 16-B loads (gstride and NT 256 even, the partials 16-B aligned)
    auto eid = [&](int r0, int u) -> int { return r0 + 2 * ((u >> 1) * BA_THREADS + (int)threadIdx.x) + (u & 1); };
    double pre[EU][4], pr4[4];
    {
        const __amdgpu_buffer_rsrc_t rs = ph_rsrc(sp0);
#pragma unroll
        for (int u = 0; u < EU; u += 2) {
            const int e = eid(0, u);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const ph_d2 v = (do_post && e < NT * 256 && q < ngp) ? ld_x2(rs, q * (int)gstride + e) : ph_d2{0.0, 0.0};
                pre[u][q] = v.x;
                pre[u + 1][q] = v.y;
            }
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
        pr4[q] = (do_post && (int)threadIdx.x < np && q < ngp) ? ld_x(sp0 + q * gstride + NT * 256 + threadIdx.x) : 0.0;
    if (bad) {
        if (threadIdx.x == 0) gst.step_valid = 0;
        return;
    }
    if (mode == 2) stamp(25);  // (diagnostic: the groups' failure flags are in)
    if (head_slot >= 0 && P.prof) {  // (diagnostic: the requested loads complete here)
        double z = sm0[0] + pre[0][0] + pr4[0];
        if (z == 12345.678 && threadIdx.x == 999) sh.b[0] = z;
        stamp(head_slot);
    }
    // the reduced system is block diagonal (poses | velocities and biases): each block by one wave
    // the reduced system is block diagonal (poses | velocities and biases, the reference's IMU pose
    // Jacobians being zero): both blocks by one 6x6-blocked LLT (chol6_solve2), the IMU block padded to a
    // multiple of 6 with identity rows
    const int ni6 = imu_off ? 0 : (ni + 5) / 6 * 6;
    const bool split = np % 6 == 0 && np + ni6 <= BA_NF_MAX;
    {
        // (1) small inputs into LDS: s_f, D_f, rhs (nf each), U (27K), the IMU block (ni^2, into the stage
        // area, free until the Cholesky), pose-block -> keyframe table
        double* Hs = sh.stage;
        for (int e0 = threadIdx.x; do_pre && e0 < nsm; e0 += 8 * BA_THREADS) {
            double v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = e0 == (int)threadIdx.x ? sm0[u] : small_in(e0 + u * BA_THREADS);
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int e = e0 + u * BA_THREADS;
                if (e >= nsm) continue;
                if (e < nf) sh.s_f[e] = v[u];
                else if (e < 2 * nf) sh.g_f[e - nf] = v[u];          // D_f (g_f is free here)
                else if (e < 3 * nf) sh.colsq_f[e - 2 * nf] = v[u];  // rhs s_f * g_f
                else if (e < 3 * nf + 27 * K) sh.U[(e - 3 * nf) / 27][(e - 3 * nf) % 27] = v[u];
                else Hs[e - 3 * nf - 27 * K] = v[u];
            }
        }
        if (threadIdx.x < BA_KMAX && do_pre) sh.posef[threadIdx.x] = -1;
        __syncthreads();
        if (threadIdx.x < K && w.pose_f[threadIdx.x] >= 0 && do_pre) sh.posef[w.pose_f[threadIdx.x] / 6] = threadIdx.x;
        __syncthreads();
        stamp(18);  // (diagnostic: small inputs + tables)
        // (2) element value of the reduced system at (row, col), Schur partials excluded.  Branch-free
        // (clamped LDS addresses and selects), so that the loads of all of a thread's elements go out
        // together instead of one dependent LDS round trip per element under its own exec mask
        auto base = [&](int row, int col) -> double {
            const bool inr = row < nf && col < nf;
            const int br = (row * 171) >> 10, bc = (col * 171) >> 10;  // row / 6, col / 6 (< 128)
            const bool same = row < np && col < np && br == bc;        // a pose's diagonal block
            const bool imu = inr && row >= np && col >= np;
            const int i = row - 6 * br, j = col - 6 * bc, a = min(i, j), bq = max(i, j);
            const int kf = sh.posef[same ? br : 0];
            const double uv = sh.U[same && kf >= 0 ? kf : 0][same ? a * 6 - (a * (a - 1)) / 2 + (bq - a) : 0];
            const double hv = Hs[imu ? (row - np) * ni + (col - np) : 0];
            const int rr = inr ? row : 0, cc = inr ? col : 0;
            const double sr = sh.s_f[rr], sc = sh.s_f[cc], gr = sh.g_f[rr];
            double v = same ? uv * sr * sc : imu ? hv * sr * sc : 0.0;
            v = row == col ? v + gr * gr : v;
            return inr ? v : (row == col ? 1.0 : 0.0);
        };
        // lower tile t = e / 256 -> (tile row I, tile column J), row-major over the lower triangle (t < 21)
        auto rowcol = [](int e, int& row, int& col) {
            const int t = e >> 8;
            const int I = (t >= 1) + (t >= 3) + (t >= 6) + (t >= 10) + (t >= 15);
            const int J = t - I * (I + 1) / 2;
            row = 16 * I + ((e >> 4) & 15);
            col = 16 * J + (e & 15);
        };
        // (2a) tiles of the pose tile-rows (I < T): the Schur partials of every landmark group, 10 tile
        // elements per thread per round with all their loads in flight (static register indices).
        // Subtracting 0.0 where a partial does not apply leaves the value's bits as they are.
        for (int r0 = 0; r0 < NT * 256; r0 += EU * BA_THREADS) {
            double part[EU][4];
#pragma unroll
            for (int u = 0; u < EU; ++u) {
                const int e = eid(r0, u);
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    part[u][q] = r0 == 0 ? pre[u][q] : (e < NT * 256 && q < ngp) ? ld_x(sp0 + q * gstride + e) : 0.0;
            }
            double v[EU];
            bool pose[EU], in[EU];
            int addr[EU];
#pragma unroll
            for (int u = 0; u < EU; ++u) {
                const int e = eid(r0, u);
                in[u] = e < NT * 256;
                int row, col;
                rowcol(in[u] ? e : 0, row, col);
                addr[u] = row * ls + col;
                v[u] = do_pre ? base(row, col) : sh.S[addr[u]];  // mode 2: mode 1's base
                pose[u] = do_post && row < np && col < np;
#pragma unroll
                for (int q = 0; q < 4; ++q) v[u] -= (pose[u] && q < ngp) ? part[u][q] : 0.0;
            }
            // groups 4.. (the phase route's groups beyond the first four): four groups' loads of all EU
            // elements in flight per round, subtracted in group order
            for (int q0 = 4; do_post && q0 < ngp; q0 += 4) {
#pragma unroll
                for (int u = 0; u < EU; ++u) {
                    const int e = eid(r0, u);
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        part[u][q] = (e < NT * 256 && q0 + q < ngp) ? ld_x(sp0 + (q0 + q) * gstride + e) : 0.0;
                }
#pragma unroll
                for (int u = 0; u < EU; ++u)
#pragma unroll
                    for (int q = 0; q < 4; ++q) v[u] -= (pose[u] && q0 + q < ngp) ? part[u][q] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < EU; ++u)
                if (in[u]) sh.S[addr[u]] = v[u];
        }
        stamp(19);  // (diagnostic: pose tiles with the Schur partials)
        // (2b) the remaining lower tiles (I >= T: IMU-space and padding rows, no Schur partials), EU
        // elements per thread per round
        for (int r0 = NT * 256; do_pre && r0 < ntile * 256; r0 += EU * BA_THREADS) {
            double v[EU];
            bool in[EU];
            int addr[EU];
#pragma unroll
            for (int u = 0; u < EU; ++u) {
                const int e = r0 + u * BA_THREADS + (int)threadIdx.x;
                in[u] = e < ntile * 256;
                int row, col;
                rowcol(in[u] ? e : 0, row, col);
                addr[u] = row * ls + col;
                v[u] = base(row, col);
            }
#pragma unroll
            for (int u = 0; u < EU; ++u)
                if (in[u]) sh.S[addr[u]] = v[u];
        }
        // rhs: s_f g_f minus the groups' Z h partials (pose rows)
        if (threadIdx.x < 96) {
            const int f = threadIdx.x;
            double v = do_pre ? (f < nf ? sh.colsq_f[f] : 0.0) : sh.b[f];
            if (f < np && do_post) {
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (q < ngp) v -= pr4[q];
                for (int q = 4; q < ngp; ++q) v -= ld_x(sp0 + q * gstride + NT * 256 + f);
            }
            sh.b[f] = v;
        }
        if (threadIdx.x == 0) sh.chol_bad = 0;
        __syncthreads();
        if (!do_post) return;
        if (split) {  // right-hand sides as row np (poses) / row np + ni6 (IMU block); IMU padding rows
            for (int f = threadIdx.x; f < np; f += BA_THREADS) sh.S[np * ls + f] = sh.b[f];
            for (int f = threadIdx.x; f < ni6; f += BA_THREADS) sh.S[(np + ni6) * ls + np + f] = f < ni ? sh.b[np + f] : 0.0;
            for (int e = threadIdx.x; e < (ni6 - ni) * ni6; e += BA_THREADS) {
                const int f = ni + e / ni6, c = e % ni6;
                sh.S[(np + f) * ls + np + c] = c == f ? 1.0 : 0.0;
            }
            __syncthreads();
        }
        if (!split && (nf & 15)) {  // the right-hand side rides through the factorisation as row nf (cholesky_solve_rhs)
            for (int f = threadIdx.x; f <= nf; f += BA_THREADS) sh.S[nf * ls + f] = f < nf ? sh.b[f] : kRhsPivot;
            __syncthreads();
        }
    }
    stamp(16);
    bool ok = true;
    if (split) {
        // S = blockdiag(pose block, velocity/bias block); row np + ni6 of S may be the first row past it
        // (the stage area follows S): the inverse diagonals go further into the stage area
        static_assert(BA_STAGE >= 128 + 2 * BA_NF_MAX, "chol6 scratch in the stage area");
        static_assert(BA_STAGE >= 128 + 2 * BA_NF_MAX + 256, "chol_mw scratch in the stage area");
        static_assert(BA_STAGE >= 128 + chol_tile_scratch_doubles(), "chol_tile scratch in the stage area");
        const int tg = 10 * chol_tile_rows(np) + chol_tile_rows(ni6);  // tile geometry (T0, T1)
        if (P.chol_variant == 2 && tg == 43)  // config-3 VI windows: 54 pose rows + 36 velocity / bias rows
            ok = chol_tile_solve2<4, 3>(sh.S, np, sh.S + np * ls + np, ni6, ls, sh.b, sh.b + np, sh.stage + 128, &sh.chol_bad);
        else if (P.chol_variant == 2 && tg == 40)  // 10-keyframe visual windows (config 2)
            ok = chol_tile_solve2<4, 0>(sh.S, np, sh.S + np * ls + np, 0, ls, sh.b, sh.b + np, sh.stage + 128, &sh.chol_bad);
        else
            ok = chol6_solve2<BA_THREADS>(sh.S, np, sh.S + np * ls + np, ni6, ls, sh.b, sh.b + np, sh.stage + 128,
                                          sh.stage + 128 + BA_NF_MAX, &sh.chol_bad);
    } else if (nf > 0) {
        auto mark = [&](int slot) { stamp(slot); };
        ok = (nf & 15) ? cholesky_solve_rhs(sh, nf, mark) : cholesky_solve(sh, nf, mark);
    }
    stamp(17);
    if (!ok) {
        if (threadIdx.x == 0) gst.step_valid = 0;
        return;
    }
    // delta_f, candidates and norms of the f-space blocks
    double* Dd = x.pr + x.ph.fv + 3 * BA_NF_MAX;  // D_f is no longer needed: holds delta_f from here
    for (int f = threadIdx.x; f < nf; f += BA_THREADS) st_w<LS>(Dd + f, -sh.b[f] * s_f[f]);  // (phase route: plain)
    for (int f = threadIdx.x; f < nf; f += BA_THREADS) sh.D_f[f] = -sh.b[f] * s_f[f];
    __syncthreads();
    double sn = 0.0, xn = 0.0, fin = 0.0;
    for (int f = threadIdx.x; f < nf; f += BA_THREADS)
        if (!isfinite(sh.b[f])) fin = 1.0;
    double* xp = x.xp; double* cp_ = x.cp;
    double* xv = x.xv; double* cv = x.cv;
    double* xb = x.xb; double* cb = x.cb;
    for (int e = threadIdx.x; e < 6 * K; e += BA_THREADS) {
        int k = e / 6, i = e % 6;
        int pfk = w.pose_f[k];
        double xx = xp[e];
        double cnd = pfk >= 0 ? xx + sh.D_f[pfk + i] : xx;
        cp_[e] = cnd;
        sh.stage[e] = cnd;
        if (pfk >= 0) { double d = xx - cnd; sn += d * d; xn += cnd * cnd; }
    }
    if (w.is_vi && !imu_off) {
        for (int e = threadIdx.x; e < 3 * K; e += BA_THREADS) {
            int k = e / 3, cc = e % 3;
            int vf = w.vel_f[k];
            double xx = xv[e];
            double cnd = vf >= 0 ? xx + sh.D_f[vf + cc] : xx;
            st_w<LS>(cv + e, cnd);
            if (vf >= 0) { double d = xx - cnd; sn += d * d; xn += cnd * cnd; }
        }
        for (int e = threadIdx.x; e < 6; e += BA_THREADS) {
            int f = e < 3 ? w.bg_f + e : w.ba_f + e - 3;
            bool a = e < 3 ? w.bg_f >= 0 : w.ba_f >= 0;
            double xx = xb[e];
            double cnd = a ? xx + sh.D_f[f] : xx;
            st_w<LS>(cb + e, cnd);
            if (a) { double d = xx - cnd; sn += d * d; xn += cnd * cnd; }
        }
    }
    // the pose cache at the candidate poses (the back-substitution walk's and the next linearisation's
    // R_bw); the IMU part of the model change and the IMU factors at the candidate run in ph_back's
    // extra workgroup
    __syncthreads();
    for (int k = threadIdx.x; k < K; k += BA_THREADS) pose_cache_one(x.pr + x.ph.pinit + 24 * k, sh.stage + 6 * k, sh.pc[k]);
    __syncthreads();
    for (int e = threadIdx.x; e < 36 * K; e += BA_THREADS) st_w<LS>(x.pr + x.ph.pcc + e, sh.pc[e / 36][e % 36]);
    if (LS || P.imu_in_back) {  // (the cluster route always: its IMU member)
        // small batches: ph_back_x_kernel's extra workgroup evaluates them beside the walk
    } else if (w.is_vi) {
        ph_imu_terms<true>(sh, x, sh.D_f, sh.stage, false);  // (inlined: one workgroup per CU, registers to spare)
    } else if (threadIdx.x == 0) {
        double* cp = x.pr + x.ph.cpart + 8 * x.ph.nch;
        for (int i = 0; i < 6; ++i) st_x(cp + i, 0.0);
    }
    double rv[3] = {sn, xn, fin};
    block_reduce<2, 1>(rv, sh.redv);
    double tsn = rv[0], txn = rv[1], tfin = rv[2];
    stamp(20);
    if (threadIdx.x == 0) {
        if (imu_off && ictr) {  // the velocity / bias block's step (ph_imu_solve's record)
            const unsigned long long t0 = wait_clock();
            while (__hip_atomic_load((const ph_gint*)ictr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < itarget) {
                if (wait_expired(t0) ||
                    __hip_atomic_load((const ph_gint*)ierr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) {
                    __hip_atomic_store((ph_gint*)ierr, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    break;
                }
                __builtin_amdgcn_s_sleep(1);
            }
            const double* rec = x.pr + x.ph.imurec;
            tsn += ld_x(rec + 1);
            txn += ld_x(rec + 2);
            tfin = fmax(tfin, ld_x(rec + 3));
            if (ld_x(rec + 4) > 0.0) tfin = 1.0;  // a non-positive pivot of the IMU block: no valid step
        }
        gst.st.step_norm = tsn;       // partial: the back-substitution walk adds the landmarks
        gst.st.cand_x_norm2 = txn;
        gst.step_valid = tfin > 0.0 ? 0 : 1;
    }
}


#ifndef VIO_BA_CLUSTER_TU
__global__ void __launch_bounds__(BA_THREADS, 1) ph_solve_kernel(BaPools P) {
    const int wi = ph_wx(P);
    if (ph_skip(P, wi)) return;
    extern __shared__ __align__(16) unsigned char smem_raw[];
    ph_solve_body(P, wi, *reinterpret_cast<BaShared*>(smem_raw));
}
#endif


// ------------------------------------------------------------------------------------------
// ------------------------------------------------------------------------------------------
// back-substitution of one landmark chunk (y_l = V~^-1 (g~_l - W~^T y_p)), the chunk's part of
// the model change and of the candidate cost
// EXTRA (small batches, ph_back_x_kernel): workgroup nch of each window evaluates the IMU candidate
// terms (ph_imu_terms) beside the walk instead of ph_solve, off the serial path of a single window; the
// call of the IMU factor code costs that kernel 4-waves-per-SIMD occupancy and a scratch segment, which
// large batches (ph_back_kernel) cannot afford
// (the caller checks the window's state: a valid step of a running solve; chunk ci of window wi, or the
// extra IMU workgroup ci == nch when EXTRA)
// The step-independent part of a chunk's walk lane: its observation, the inputs of the landmark step and the
// observation's Jacobian at the linearisation point (factor_ap_at + jac_from_ap need only the linearisation
// point's pose cache).  The cluster route's chunk members form it while the leader solves the reduced
// system (ph_back_pre, between their B arrival and the step's F record) and ph_back_body takes it as is.
struct WalkJac {  // what crosses the cluster member's wait for the step: the linearisation-point Jacobian
    double p12[12], j6[6];
};
struct WalkLane {
    int o;
    bool lv, out_o, lane_lm, lvj;
    double ra, rb, uo, vo;
    double sv[3], glj[3], li[6], xlj[3];
    WalkJac J;
};
// the lane inputs of chunk ci (o, landmark lanes) from memory (no tables needed); o_pre >= -1: the lane's
// observation index already read (ph_back_launch requests it with the window state: the landmark-keyframe
// table does not depend on the parameter set)
__device__ __forceinline__ void ph_walk_lm_inputs(const PhCtx& x, const Walk& g, int ci, WalkLane& wl);
// (lm_now false: the landmark lanes' step inputs are left for ph_walk_lm_inputs, called just before the step)
// (g: the window's walk geometry, formed once per workgroup by the caller -- walk_geom reads the descriptor)
__device__ __forceinline__ void ph_walk_inputs(const PhCtx& x, const Walk& g, int ci, WalkLane& wl, double (&pw)[3],
                                               double& a_o, int o_pre = -2, bool lm_now = true) {
    const WinCtx& c = x.c;
    const BaWin& w = *c.w;
    const int N = w.N, K = w.K, L = w.L;
    const int l0 = ci * g.LC, l = l0 + g.jf;
    wl.o = o_pre >= -1 ? o_pre : (g.on && l < L) ? reinterpret_cast<const int*>(c.ws + c.L.lk)[16 * l + g.kf] : -1;
    wl.lv = wl.out_o = false;
    wl.ra = wl.rb = wl.uo = wl.vo = 0.0;
    pw[0] = pw[1] = pw[2] = 0.0;
    a_o = 0.0;
    if (wl.o >= 0) {
        const int o = wl.o;
        wl.lv = c.lm_var[l] != 0;
#pragma unroll
        for (int i = 0; i < 3; ++i) pw[i] = x.xl[3 * l + i];
        a_o = x.la[o];
        wl.ra = x.lr[o];
        wl.rb = x.lr[N + o];
        wl.uo = (double)c.obs_uv[2 * o];
        wl.vo = (double)c.obs_uv[2 * o + 1];
        wl.out_o = c.outlier[o] != 0;
    }
    if (lm_now) ph_walk_lm_inputs(x, g, ci, wl);
}
// the landmark lanes' inputs of the landmark step (lane j < LC: landmark l0 + j): Jacobi scale, gradient,
// V~^-1 factor, position
__device__ __forceinline__ void ph_walk_lm_inputs(const PhCtx& x, const Walk& g, int ci, WalkLane& wl) {
    const WinCtx& c = x.c;
    const BaWin& w = *c.w;
    const int L = w.L;
    const int l0 = ci * g.LC;
    const int lj = l0 + (int)threadIdx.x;
    wl.lane_lm = (int)threadIdx.x < g.LC && lj < L;
    wl.lvj = false;
#pragma unroll
    for (int cc = 0; cc < 3; ++cc) wl.sv[cc] = wl.glj[cc] = wl.xlj[cc] = 0.0;
#pragma unroll
    for (int i = 0; i < 6; ++i) wl.li[i] = 0.0;
    if (wl.lane_lm) {
        const double* sl = c.ws + c.L.s_l;
        const double* Li = c.ws + c.L.Vi;
        wl.lvj = c.lm_var[lj] != 0;
#pragma unroll
        for (int cc = 0; cc < 3; ++cc) {
            wl.sv[cc] = sl[(int64_t)cc * L + lj];
            wl.glj[cc] = x.lg[(int64_t)cc * L + lj];
            wl.xlj[cc] = x.xl[3 * lj + cc];
        }
#pragma unroll
        for (int i = 0; i < 6; ++i) wl.li[i] = Li[(int64_t)i * L + lj];
    }
}
// the observation's Jacobian at the linearisation point (sh.Rlin, sh.Rcb_raw in LDS)
__device__ __forceinline__ void ph_walk_jac(const PhShared& sh, const BaWin& w, const Walk& g, WalkLane& wl,
                                            const double (&pw)[3], double a_o) {
#pragma unroll
    for (int i = 0; i < 6; ++i) wl.J.j6[i] = 0.0;
#pragma unroll
    for (int i = 0; i < 12; ++i) wl.J.p12[i] = 0.0;
    if (wl.o >= 0) {
        double a6[6], pb[3];
        factor_ap_at(sh.Rlin[g.kf], sh.Rcb_raw[g.kf], pw, w.cols, w.rows, w.Lw, a_o, a6, pb);
        jac_from_ap(a6, pb, sh.Rlin[g.kf], wl.J.p12, wl.J.j6);
    }
}
// the prelude itself (every thread; chunk ci of window wi at parameter set cur): the tables and the
// linearisation point's pose cache into LDS, the lane inputs, the Jacobian
// (jl: 18 x BA_THREADS doubles of LDS outside PhShared, element i of thread t at jl[i BA_THREADS + t]: the
// Jacobian waits there, not in registers, through the wait for the step)
__device__ __forceinline__ void ph_back_pre(const BaPools& P, PhShared& sh, int wi, int ci, int cur, double* jl) {
    const PhCtx x = ph_ctx(P, wi, cur);
    double pw[3], a_o;
    WalkLane wl;
    const Walk g = walk_geom(*x.c.w);
    ph_walk_inputs(x, g, ci, wl, pw, a_o);
    ph_tables(sh, x);
    ph_ld_block(&sh.Rlin[0][0], x.pr + x.ph.rlin, PL24 * x.c.w->K);
    __syncthreads();
    ph_walk_jac(sh, *x.c.w, g, wl, pw, a_o);
#pragma unroll
    for (int i = 0; i < 12; ++i) jl[i * BA_THREADS + threadIdx.x] = wl.J.p12[i];
#pragma unroll
    for (int i = 0; i < 6; ++i) jl[(12 + i) * BA_THREADS + threadIdx.x] = wl.J.j6[i];
}

// pose-partial term q < 21 of ph_back_body: the pair (a, b), a <= b, in row-major upper-triangle order
__host__ __device__ constexpr int ph_pair_a(int q) {
    int a = 0;
    while (a < 6 && q >= 6 - a) { q -= 6 - a; ++a; }
    return a < 6 ? a : 0;
}
__host__ __device__ constexpr int ph_pair_b(int q) {
    int a = 0;
    while (a < 6 && q >= 6 - a) { q -= 6 - a; ++a; }
    return a < 6 ? a + q : 0;
}
static_assert(ph_pair_a(0) == 0 && ph_pair_b(5) == 5 && ph_pair_a(6) == 1 && ph_pair_b(6) == 1 && ph_pair_a(20) == 5 &&
                  ph_pair_b(20) == 5, "pair order");
// jl (non-null): the lanes' Jacobians from the prelude (ph_back_pre; the tables and sh.Rlin are in LDS too)
// (x, g: the window's context at parameter set v.cur and its walk geometry, built once per workgroup)
template <bool EXTRA, bool WT = true>
__device__ __forceinline__ void ph_back_body_at(const BaPools& P, PhShared& sh, const PhCtx& x, const Walk& g, int wi,
                                                int ci, const PhView& v, const double* jl = nullptr, int o_pre = -2) {
    const bool pre = jl != nullptr;
    const WinCtx& c = x.c;
    const BaWin& w = *c.w;
    if (ci > x.ph.nch || (!EXTRA && ci == x.ph.nch)) return;
    const int N = w.N, K = w.K, L = w.L, nf = w.nf;
    const unsigned long long wstart = P.prof ? __builtin_amdgcn_s_memtime() : 0;
    // the lane's observation and its linearisation inputs, requested before the window tables (one memory
    // round trip for both instead of two in sequence) -- or the cluster member's prelude (ph_back_pre)
    const int l0 = ci * g.LC;
    WalkLane wl;
    double pw[3], a_o;
    // (with the prelude: the same loads again, its Jacobian kept; phase route: the landmark lanes' inputs
    // requested after the Jacobian, so that they are not live across it -- no spill at five waves per SIMD)
    ph_walk_inputs(x, g, ci, wl, pw, a_o, o_pre, WT);
    const int o = wl.o, lj = l0 + (int)threadIdx.x;
    const bool lv = wl.lv, out_o = wl.out_o;
    const double uo = wl.uo, vo = wl.vo;
    if (!pre) ph_tables(sh, x);
    // the pose cache at the candidate poses (ph_solve's output), the linearisation point's, the step delta_f
    ph_ld_block(&sh.pc[0][0], x.pr + x.ph.pcc, 36 * K);
    if (pre) {
        // (the prelude's: sh.Rlin and the tables in LDS already)
    } else if (v.rlin) {
        for (int e = threadIdx.x; e < PL24 * K; e += BA_THREADS) sh.Rlin[e / PL24][e % PL24] = v.rlin[e];
    } else {
        ph_ld_block(&sh.Rlin[0][0], x.pr + x.ph.rlin, PL24 * K);
    }
    ph_ld_block(sh.dlt, x.pr + x.ph.fv + 3 * BA_NF_MAX, nf);
    __syncthreads();
    if (EXTRA && ci == x.ph.nch) {
        if (w.is_vi) {
            PhStamp ist(P.csync ? P.prof : nullptr, wi);
            ph_imu_terms<EXTRA>(sh, x, sh.dlt, sh.buf, true, &ist);
            // phase route: the candidate's IMU normal equations too, off the serial path (ph_prep takes them
            // after an accepted step, like the cluster route's IMU member's)
#ifndef VIO_BA_CLUSTER_TU
            if (!P.csync) ph_imu_spec_normal_eq(sh, x, sh.buf);
#endif
        } else if (threadIdx.x == 0) {
            double* cp = x.pr + x.ph.cpart + 8 * x.ph.nch;
            for (int i = 0; i < 6; ++i) st_x(cp + i, 0.0);
        }
        return;
    }
    const int pf = g.on ? sh.posef[g.kf] : -1;
    double* ws = c.ws;
    const double* xl = x.xl;
    double* cl = x.cl;
    const double* sl = ws + c.L.s_l;
    const double* gl = x.lg;
    const double* Li = ws + c.L.Vi;
    double* red = sh.buf;
    double* dls = sh.buf + 3 * BA_THREADS;
    double* cps = sh.buf + 6 * BA_THREADS;
    double fin = 0.0, mc = 0.0, sn = 0.0, xn = 0.0, ccost = 0.0;
    int cfail = 0;
    const bool act = o >= 0 && (pf >= 0 || lv);
    if (pre) {
#pragma unroll
        for (int i = 0; i < 12; ++i) wl.J.p12[i] = jl[i * BA_THREADS + threadIdx.x];
#pragma unroll
        for (int i = 0; i < 6; ++i) wl.J.j6[i] = jl[(12 + i) * BA_THREADS + threadIdx.x];
    } else {
        ph_walk_jac(sh, w, g, wl, pw, a_o);
    }
    const double* p12 = wl.J.p12;
    const double* j6 = wl.J.j6;
    const double ra = wl.ra, rb = wl.rb;
    double e0 = 0.0, e1 = 0.0;
    if (o >= 0) {
        if (act && pf >= 0) {
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                const double d = sh.dlt[pf + i];
                e0 += p12[i] * d;
                e1 += p12[6 + i] * d;
            }
        }
    }
    const bool contrib = lv && pf >= 0;
    if (!WT) ph_walk_lm_inputs(x, g, ci, wl);
    const bool lane_lm = wl.lane_lm, lvj = wl.lvj;
    const double* sv = wl.sv;
    const double* glj = wl.glj;
    const double* li = wl.li;
    const double* xlj = wl.xlj;
#pragma unroll
    for (int cc = 0; cc < 3; ++cc) red[cc * BA_THREADS + threadIdx.x] = contrib ? j6[cc] * e0 + j6[3 + cc] * e1 : 0.0;
    __syncthreads();
    if (lane_lm) {
        {
            double d[3] = {0.0, 0.0, 0.0};
            if (lvj) {
                double rhs[3];
#pragma unroll
                for (int cc = 0; cc < 3; ++cc) {
                    double t = 0.0;
#pragma unroll
                    for (int kf = 0; kf < BA_KMAX; ++kf)
                        if (kf < K) t += red[cc * BA_THREADS + threadIdx.x * K + kf];
                    rhs[cc] = glj[cc] * sv[cc] + sv[cc] * t;
                }
                const double t0 = li[0] * rhs[0];
                const double t1 = li[1] * rhs[0] + li[2] * rhs[1];
                const double t2 = li[3] * rhs[0] + li[4] * rhs[1] + li[5] * rhs[2];
                const double y0 = li[0] * t0 + li[1] * t1 + li[3] * t2;
                const double y1 = li[2] * t1 + li[4] * t2;
                const double y2 = li[5] * t2;
                if (!isfinite(y0) || !isfinite(y1) || !isfinite(y2)) fin = 1.0;
                d[0] = -y0 * sv[0];
                d[1] = -y1 * sv[1];
                d[2] = -y2 * sv[2];
            }
#pragma unroll
            for (int cc = 0; cc < 3; ++cc) {
                const double xx = xlj[cc];
                const double cnd = lvj ? xx + d[cc] : xx;
                cl[3 * lj + cc] = cnd;
                if (lvj) {
                    const double dd = xx - cnd;
                    sn += dd * dd;
                    xn += cnd * cnd;
                }
                dls[3 * threadIdx.x + cc] = d[cc];
                cps[3 * threadIdx.x + cc] = cnd;
            }
        }
    }
    __syncthreads();
    if (P.csync && ci == 0 && P.prof && threadIdx.x == 0) {  // (diagnostic, cluster member of chunk 0: walk head)
        PhStamp wst(P.prof, wi);
        wst.last = wstart;
        wst(31);
    }
    // the model change of the observation, then the residual block at the candidate WITH its Jacobian:
    // the candidate's linearisation (residuals, compressed Jacobians, landmark V / g_l, pose partials)
    // goes to the second linearisation set, which becomes the current one if ph_ctrl accepts the step
    // (the same values the first-linearisation code computes at that point: no re-evaluation)
    // (the 27 pose-partial terms are formed per pass from jpk / rsk below: 14 live values instead of 27 across
    // the landmark sums, 121 -> 110 VGPRs; the same expressions, contracted into FMAs in another order, so
    // the partials can differ in the last bit from the round-5 build)
    // (the lane's model change waits in LDS across the candidate evaluation, not in two of ph_back_kernel's 96
    // registers: red's slots are free from the barrier above to the one below; the compiler barrier before the
    // reload keeps it from forwarding the value in a register all the same)
    double* mcs = red;
    mcs[threadIdx.x] = 0.0;
    double jpk[12], rsk[2] = {0.0, 0.0}, v9[9];
#pragma unroll
    for (int i = 0; i < 12; ++i) jpk[i] = 0.0;
#pragma unroll
    for (int i = 0; i < 9; ++i) v9[i] = 0.0;
    if (act) {
        double m0 = e0, m1 = e1;
        if (lv) {
#pragma unroll
            for (int cc = 0; cc < 3; ++cc) {
                const double d = dls[3 * g.jf + cc];
                m0 += j6[cc] * d;
                m1 += j6[3 + cc] * d;
            }
        }
        mc -= m0 * (ra + m0 / 2.0) + m1 * (rb + m1 / 2.0);
        mcs[threadIdx.x] = mc;
        double Pc[3] = {cps[3 * g.jf], cps[3 * g.jf + 1], cps[3 * g.jf + 2]};
        double r[2], Pcam[3], Lc = 0.0, iLc = 0.0;
        bool tail;
        // (factor_eval_ap split around the loss: its Jacobian tail after huber, so A / Pb are not live across
        // it -- one spill-free register budget at four waves per SIMD)
        if (factor_eval_res(sh.pc[g.kf], Pc, uo, vo, w.cols, w.rows, w.Lw, out_o, w.is_pnp, r, Pcam, Lc, iLc, tail)) {
            cfail = 1;
        } else {
            double cst, sc;
            huber(w.huber, r[0] * r[0] + r[1] * r[1], cst, sc);
            ccost += cst;
            const double rsa = r[0] * sc, rsb = r[1] * sc;
            x.cr[o] = rsa;
            x.cr[N + o] = rsb;
            double Aj[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, Pb[3] = {0.0, 0.0, 0.0};
            const bool jz = !tail || !factor_ap_tail(Pcam[0], Pcam[1], Pcam[2], Lc, iLc, sh.pc[g.kf] + 12,
                                                     sh.pc[g.kf] + 21, Pc, sh.Rcb_raw[g.kf], w.cols, w.rows, w.Lw,
                                                     Aj, Pb);
            x.ca[o] = jz ? 0.0 : sc;
#pragma unroll
            for (int i = 0; i < 6; ++i) Aj[i] = jz ? 0.0 : Aj[i] * sc;
#pragma unroll
            for (int i = 0; i < 3; ++i) Pb[i] = jz ? 0.0 : Pb[i];
            double Jp[12], Jl[6];
            jac_from_ap(Aj, Pb, sh.pc[g.kf] + 12, Jp, Jl);
            if (pf >= 0) {
#pragma unroll
                for (int i = 0; i < 12; ++i) jpk[i] = Jp[i];
                rsk[0] = rsa;
                rsk[1] = rsb;
            }
            if (lv) {
                const double* la = Jl;
                const double* lb = Jl + 3;
                v9[0] = la[0] * la[0] + lb[0] * lb[0];
                v9[1] = la[0] * la[1] + lb[0] * lb[1];
                v9[2] = la[0] * la[2] + lb[0] * lb[2];
                v9[3] = la[1] * la[1] + lb[1] * lb[1];
                v9[4] = la[1] * la[2] + lb[1] * lb[2];
                v9[5] = la[2] * la[2] + lb[2] * lb[2];
                v9[6] = la[0] * rsa + lb[0] * rsb;
                v9[7] = la[1] * rsa + lb[1] * rsb;
                v9[8] = la[2] * rsa + lb[2] * rsb;
            }
        }
    }
    asm volatile("" ::: "memory");
    mc = mcs[threadIdx.x];
    __syncthreads();  // buf (red / dls / cps) is reused below
    // landmark sums of the candidate linearisation (the chunk's landmarks), gradient terms at the
    // candidate points (cl, written above by this workgroup's landmark lanes)
#pragma unroll
    for (int i = 0; i < 9; ++i) sh.buf[i * BA_THREADS + threadIdx.x] = v9[i];
    __syncthreads();
    double gm = lm_sums9(sh.buf, l0, g, K, L, c.lm_var, cl, x.cvv, x.cgl, nullptr, false, 0.0);
    __syncthreads();
    // pose partials of the chunk at the candidate: 27 sums per keyframe over its LC lanes
    double* up = x.cup + (int64_t)ci * 27 * K;
    static_for<3>([&](auto Part) {
        constexpr int part = decltype(Part)::value;
        static_for<9>([&](auto I) {  // term q = 9 part + i: the upper-triangle pairs (i <= j) in order, then the gradient
            constexpr int q = 9 * part + decltype(I)::value;
            constexpr int a = ph_pair_a(q), b = ph_pair_b(q);
            const double v = q < 21 ? jpk[a] * jpk[b] + jpk[6 + a] * jpk[6 + b] : jpk[q - 21] * rsk[0] + jpk[6 + q - 21] * rsk[1];
            sh.buf[decltype(I)::value * BA_THREADS + threadIdx.x] = v;
        });
        __syncthreads();
        for (int e = threadIdx.x; e < 9 * K; e += BA_THREADS) {
            const int k = walk_div(e, walk_recip(9)), i = e - 9 * k;  // (e < 9 K <= 144: exact, full-rate multiply)
            double s = 0.0;
            for (int j = 0; j < g.LC; ++j) s += sh.buf[i * BA_THREADS + j * K + k];
            st_w<WT>(up + 27 * k + 9 * part + i, s);
        }
        __syncthreads();
    });
    double rv[7] = {mc, sn, xn, ccost, (double)cfail, fin, gm};
    block_reduce<4, 3>(rv, sh.redv);
    const double tmc = rv[0], tsn = rv[1], txn = rv[2], tcc = rv[3], tcf = rv[4], tfi = rv[5], tgm = rv[6];
    if (threadIdx.x == 0) {
        double* cp = x.pr + x.ph.cpart + 8 * ci;
        st_w<WT>(cp, tmc);
        st_w<WT>(cp + 1, tsn);
        st_w<WT>(cp + 2, txn);
        st_w<WT>(cp + 3, tcc);
        st_w<WT>(cp + 4, tcf);
        st_w<WT>(cp + 5, tfi);
        double* lp = x.clp + 4 * ci;  // the candidate linearisation's partials (ph_prep after acceptance)
        st_w<WT>(lp, tcc);
        st_w<WT>(lp + 1, tgm);
        st_w<WT>(lp + 2, tcf);
    }
}

template <bool EXTRA, bool WT = true>
__device__ __forceinline__ void ph_back_body(const BaPools& P, PhShared& sh, int wi, int ci, const PhView& v,
                                             const double* jl = nullptr, int o_pre = -2) {
    const PhCtx x = ph_ctx(P, wi, v.cur);
    ph_back_body_at<EXTRA, WT>(P, sh, x, walk_geom(*x.c.w), wi, ci, v, jl, o_pre);
}

template <bool EXTRA>
__device__ __forceinline__ void ph_back_launch(const BaPools& P, PhShared& sh) {
    const int wi = ph_wy(P);
    if (ph_skip(P, wi)) return;
    const PhCtx x0 = ph_ctx(P, wi, 0);
    // the lane's observation index, requested with the window state (one round trip for both; the walk's
    // other inputs depend on the current parameter set, i.e. on the state)
    const BaWin& w0 = *x0.c.w;
    const Walk g0 = walk_geom(w0);
    const int ci = ph_sub(), l = ci * g0.LC + g0.jf;
    const int o_pre = (g0.on && ci < x0.ph.nch && l < w0.L)
                          ? reinterpret_cast<const int*>(x0.c.ws + x0.c.L.lk)[16 * l + g0.kf] : -1;
    const PhState& gst = *x0.gs;
    if (gst.st.done || !gst.step_valid) return;
    PhView v{gst.cur, 0, 1, 0.0, nullptr};
    // one context per workgroup: the view at the current parameter set from the one built above
    ph_back_body_at<EXTRA, false>(P, sh, ph_ctx_at(x0, gst.cur), g0, wi, ci, v, nullptr, o_pre);
}
#ifndef VIO_BA_CLUSTER_TU
__global__ void __launch_bounds__(BA_THREADS, 4) ph_back_kernel(BaPools P) {
    // PhShared without its trailing IMU arrays (no IMU terms here): 28.3 KB, so LDS admits five workgroups per
    // CU, and with the landmark lanes' inputs requested after the Jacobian (ph_back_body) the kernel needs 95
    // VGPRs: five waves per SIMD (110 VGPRs / four before: 256 windows 107.2 -> 97.6 us per launch,
    // profiles/r6g_ab_back.log; tests/test_build.py keeps it at <= 96)
    __shared__ __align__(16) unsigned char sh_raw[kPhBackLds];
    ph_back_launch<false>(P, *reinterpret_cast<PhShared*>(sh_raw));
}
#endif
#ifndef VIO_BA_CLUSTER_TU
__global__ void __launch_bounds__(BA_THREADS) ph_back_x_kernel(BaPools P) {
    __shared__ PhShared sh;
    ph_back_launch<true>(P, sh);
}
#endif

// ------------------------------------------------------------------------------------------
// chi2 / outliers / bad landmarks and outputs (Optimizer.cpp:425-456, 888-928)
template <bool LS = false>
__device__ __forceinline__ void ph_post_body(const BaPools& P, int wi, PhShared& sh) {
    const PhCtx x = ph_ctx<LS>(P, wi);
    const WinCtx& c = x.c;
    const BaWin& w = *c.w;
    const int K = w.K, L = w.L, N = w.N;
    double* ws = c.ws;
    if (threadIdx.x == 0) sh.st = x.gs->st;
    __syncthreads();
    if (sh.st.termination == VIO_TERM_FAILURE) {  // the solve failed: parameters back to their inputs
        for (int e = threadIdx.x; e < 6 * K; e += BA_THREADS) x.xp[e] = 0.0;
        copy_strided(x.xl, c.lm_xyz0, 3 * L);
        for (int e = threadIdx.x; e < 3 * K; e += BA_THREADS) x.xv[e] = w.is_vi ? c.vel0[e] : 0.0;
        for (int e = threadIdx.x; e < 6; e += BA_THREADS) x.xb[e] = e < 3 ? w.bg0[e] : w.ba0[e - 3];
        __syncthreads();
    }
    ph_tables(sh, x);
    ph_pose_cache(sh, x, x.xp);
    __syncthreads();
    int32_t* si = P.out_i32 + SI_COUNT * wi;
    double* sd = P.out_sum + SD_COUNT * wi;
    const BaOutLayout OL = ba_out_layout(K, L, N);
    double* out = P.out + w.o_out;
    const double* xl = x.xl;
    double cin = 0.0, cout_ = 0.0, cbad = 0.0;
    for (int l = threadIdx.x; l < L; l += BA_THREADS) {
        int li = 0, lo = 0;
        for (int o = c.lm_ptr[l]; o < c.lm_ptr[l + 1]; ++o) {
            int k = c.obs_kf[o];
            double Pw[3] = {xl[3 * l], xl[3 * l + 1], xl[3 * l + 2]};
            double ch = factor_chi2(sh.pc[k], Pw, (double)c.obs_uv[2 * o], (double)c.obs_uv[2 * o + 1], w.cols, w.rows,
                                    w.info, false, false);
            bool is_out = ch > w.chi2_thr;
            out[OL.chi2 + o] = ch;
            c.outlier[o] = is_out;
            if (is_out) lo++; else li++;
        }
        bool bad = !c.lm_marg[l] && li == 0 && lo >= 2;
        P.out_bad[w.o_lm + l] = bad;
        cin += li;
        cout_ += lo;
        cbad += bad;
    }
    double tin = block_sum(cin, sh.red);
    double tout = block_sum(cout_, sh.red);
    double tbad = block_sum(cbad, sh.red);
    if (threadIdx.x == 0) {
        const LmState& s = sh.st;
        si[SI_SUCCESS] = s.termination != VIO_TERM_FAILURE;
        si[SI_TERM] = s.termination;
        si[SI_ITERS] = s.nsucc + s.nunsucc;
        si[SI_NSUCC] = s.nsucc;
        si[SI_NUNSUCC] = s.nunsucc;
        si[SI_NIN] = (int)tin;
        si[SI_NOUT] = (int)tout;
        si[SI_NBAD] = (int)tbad;
        sd[SD_INIT] = s.initial_cost;
        sd[SD_FINAL] = s.final_cost;
        sd[SD_FIXED] = s.fixed_cost;
    }
    for (int k = threadIdx.x; k < K; k += BA_THREADS) {
        for (int i = 0; i < 9; ++i) out[OL.T_wb + 12 * k + i] = sh.pc[k][i];
        for (int i = 0; i < 3; ++i) out[OL.T_wb + 12 * k + 9 + i] = sh.pc[k][9 + i];
    }
    for (int e = threadIdx.x; e < 3 * L; e += BA_THREADS) out[OL.lm + e] = x.xl[e];
    for (int e = threadIdx.x; e < 3 * K; e += BA_THREADS) out[OL.vel + e] = x.xv[e];
    for (int e = threadIdx.x; e < 6; e += BA_THREADS) out[OL.bias + e] = x.xb[e];
}
#ifndef VIO_BA_CLUSTER_TU
__global__ void __launch_bounds__(BA_THREADS) ph_post_kernel(BaPools P) {
    const int wi = ph_wx(P);
    if (ph_skip(P, wi)) return;
    __shared__ PhShared sh;
    ph_post_body(P, wi, sh);
}
#endif

// ------------------------------------------------------------------------------------------
// Cluster route (small batches, ph_cluster_kernel): ONE persistent launch per batch.  Window w runs on C
// co-resident workgroups ("members") for its whole solve, with no kernel boundary between phases:
//   member 0, the leader: setup, ph_prep (with the step control of the previous step), ph_solve, the
//     IMU candidate terms, post -- the per-window serial work;
//   members 1..C-1: landmark chunks ci = m - 1 (+ k (C - 1)): the first linearisation, Schur group ci
//     (one chunk per group: a group's landmarks are its member's own, so the per-observation
//     linearisation, V~^-1 and the landmark blocks never leave the member) and the back-substitution
//     walk with the speculative candidate linearisation.
// Per LM iteration: leader prep (step control first) -> record R {done, cur, radius} -> members' Schur
// groups (concurrent with the rest of the leader's prep) -> counter B -> leader solve -> record F
// {step_valid} -> members' walks (the leader evaluates the IMU candidate terms meanwhile) -> counter A ->
// the leader's next prep.  Only the partials / records cross workgroups (sc1 stores and loads, st_x /
// ld_x); setup's outputs and the final landmark positions cross once behind agent-scope release /
// acquire fences.  Every wait is bounded (a timed-out wait sets the window's error word and ends the
// launch; the host reports VIO_EDEVICE).  Members of a window are dealt to blocks b with equal b % 8
// (one XCD under round-robin placement: speed only, never assumed for correctness).
// Bits: the cluster and phase routes agree to roundoff, not bit for bit -- the leader subtracts one summed
// Schur total from the reduce-scatter (base - (p0 + ... + pn), where the phase route subtracts the partials
// one by one) and the IMU member factors the velocity / bias block on its own (chol_tile_solve2<3,0>, the
// phase route the joint <4,3> system).  Within the cluster route the results are bitwise the same whatever
// the member count (the reduce-scatter sums every element in group order).
enum { PS_A = 0, PS_B = 32, PS_R = 64, PS_F = 96, PS_S = 128, PS_E = 160, PS_ERR = 192, PS_H = 224, PS_REC = 256,
       PS_WB = 320, PS_G = 352, PS_I = 384 };  // ints, 128-B lines; PS_WB: the chunk members' own barrier;
                                               // PS_G / PS_I: the IMU member's gradient / solve records
static_assert(PS_ERR == PH_SYNC_ERR, "the host reads the error word at PH_SYNC_ERR (ba_types.h)");
struct PhClusterSh {
    int ok;        // a wait's outcome (lane 0 -> all)
    int rec[8];    // the last record read
    double radius;
};
// the cluster route's reduce-scatter: member r of nm sums elements [r E / nm, (r + 1) E / nm) of the nparts
// partial records (stride E doubles at src) in record order into dst; a record's elements are read with
// all parts in flight (16 at a time)
// (in pairs: E even, src / dst 16-B aligned; member r's slice is the pairs [r E/2 / nm, (r + 1) E/2 / nm))
__device__ __forceinline__ void ph_reduce_groups(const double* src, double* dst, int64_t E, int nparts, int r, int nm) {
    const int E2 = (int)(E / 2), p0 = E2 * r / nm, p1 = E2 * (r + 1) / nm;
    const __amdgpu_buffer_rsrc_t rs = ph_rsrc(src), rd = ph_rsrc(dst);
    for (int pp = p0 + threadIdx.x; pp < p1; pp += BA_THREADS) {
        ph_d2 v = {0.0, 0.0};
        for (int q0 = 0; q0 < nparts; q0 += 8) {
            ph_d2 p[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) p[u] = q0 + u < nparts ? ld_x2(rs, (int)((q0 + u) * E) + 2 * pp) : ph_d2{0.0, 0.0};
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (q0 + u < nparts) v = (q0 + u == 0) ? p[u] : v + p[u];
        }
        st_x2(rd, 2 * pp, v);
    }
}

// arrive at a counter for every wave of this workgroup (their stores drained first: sc1 values leave
// with the wait; MICROARCH "Valid forms" row 1)
__device__ __forceinline__ void ph_arrive(int* ctr) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_fetch_add((ph_gint*)ctr, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// wait until *ctr >= target (all threads; false on time-out, which also sets the error word)
__device__ __forceinline__ bool ph_wait(const int* ctr, int target, int* err, PhClusterSh& cs) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this workgroup's own sc1 values before it reads others'
    if (threadIdx.x == 0) {
        int ok = 1;
        const unsigned long long t0 = wait_clock();  // bounded by wall clock (chol_dev.h)
        while (__hip_atomic_load((const ph_gint*)ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
            if (wait_expired(t0) ||
                __hip_atomic_load((const ph_gint*)err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) {
                ok = 0;
                __hip_atomic_store((ph_gint*)err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                break;
            }
            __builtin_amdgcn_s_sleep(2);
        }
        cs.ok = ok;
    }
    __syncthreads();
    return cs.ok != 0;
}
// publish a record (lane 0's values, sc1) then its generation flag
__device__ __forceinline__ void ph_publish(int* flag, int* rec, int gen, const int* vals, int nv, const double* dv,
                                           int ndv) {
    if (threadIdx.x == 0) {
        for (int i = 0; i < nv; ++i) __hip_atomic_store((ph_gint*)(rec + i), vals[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        for (int i = 0; i < ndv; ++i) st_x(reinterpret_cast<double*>(rec + 8) + i, dv[i]);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store((ph_gint*)flag, gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void ph_read_rec(const int* rec, int nv, PhClusterSh& cs, bool with_radius) {
    if (threadIdx.x == 0) {
        for (int i = 0; i < nv; ++i) cs.rec[i] = __hip_atomic_load((const ph_gint*)(rec + i), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (with_radius) cs.radius = ld_x(reinterpret_cast<const double*>(rec + 8));
    }
    __syncthreads();
}
// release every store of this workgroup to other CUs (all waves' stores drained, L2 written back)
__device__ __forceinline__ void ph_release_arrive(int* ctr, bool add) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (add) __hip_atomic_fetch_add((ph_gint*)ctr, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else __hip_atomic_store((ph_gint*)ctr, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}
__device__ __forceinline__ void ph_acquire() {
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
}
// dynamic LDS of the cluster kernel: the largest role (the leader's ph_solve), the wait scratch and the
// leader's on-chip PhState
__host__ __device__ constexpr size_t ph_cluster_state_off() { return (sizeof(BaShared) + sizeof(PhClusterSh) + 15) & ~(size_t)15; }
__host__ __device__ constexpr size_t ph_cluster_lds_bytes() { return ph_cluster_state_off() + sizeof(PhState) + 64; }
static_assert(ph_cluster_lds_bytes() <= 160 * 1024, "cluster kernel LDS");
__device__ __forceinline__ PhState* ph_lds_state() {
    extern __shared__ __align__(16) unsigned char ph_lds_dyn[];
    return reinterpret_cast<PhState*>(ph_lds_dyn + ph_cluster_state_off());
}
static_assert(sizeof(PhShared) + sizeof(double) * BA_KMAX * 27 <= sizeof(BaShared), "prep LDS inside the solve's");
// (a Schur group's panel, ph_schur_lds_doubles, is checked against sizeof(BaShared) by ba_cluster_members)

// Cluster route, VI windows: the IMU member solves the velocity / bias block of the reduced system while the
// leader solves the pose block (the reference's IMU pose Jacobians are zero, Factors.cpp:1415-1419, 1471-1475:
// S is block diagonal, and this block has no Schur term).  After the step control's record R: the IMU normal
// equations at the current point (the IMU member's own speculative ones, or the leader's first), the
// gradient terms, column norms and LM diagonal of the IMU rows (ph_prep_rest's f-loop and finalisation for f
// >= np) -- the gradient maximum published at once (PS_G, the leader's prep takes it) -- then s H s + D^2
// with the right-hand side s g as its last row, its Cholesky solve, the IMU rows of the f-space step, the
// velocity / bias candidates and their step / candidate norms (record + PS_I, the leader's solve takes
// them).  The same operations as the leader's split solve performs on this block.
__device__ __forceinline__ void ph_imu_solve(const BaPools& P, int wi, int cur, double radius, BaShared& sh,
                                             int* sync) {
    const PhCtx x = ph_ctx(P, wi, cur);
    const BaWin& w = *x.c.w;
    const int np = w.np, ni = w.ni, ni6 = (ni + 5) / 6 * 6, K = w.K;
    const int ls = (16 * ((ni6 + 15) >> 4)) | 1;
    const double* s_f = x.pr + x.ph.fv;
    double* Dd = x.pr + x.ph.fv + 3 * BA_NF_MAX;
    double* rec = x.pr + x.ph.imurec;
    double* Hs = sh.stage;  // H [ni][ni] (row stride ni) | g at NI_MAX^2: the chol scratch once S is built
    for (int e = threadIdx.x; e < ni * ni; e += BA_THREADS) Hs[e] = ld_x(x.himu + e);
    for (int p = threadIdx.x; p < ni; p += BA_THREADS) {
        Hs[NI_MAX * NI_MAX + p] = ld_x(x.himu + NI_MAX * NI_MAX + p);
        sh.s_f[p] = ld_x(s_f + np + p);
        sh.g_f[p] = f_param_value(w, np + p, x.xp, x.xv, x.xb);
    }
    __syncthreads();
    double gmx = 0.0;
    for (int p = threadIdx.x; p < ni; p += BA_THREADS) {
        const double gg = Hs[NI_MAX * NI_MAX + p], cs = Hs[p * ni + p], sp = sh.s_f[p];
        gmx = fmax(gmx, grad_term(sh.g_f[p], gg));
        double d = cs * sp * sp;
        d = fmin(fmax(d, 1e-6), 1e32);
        sh.D_f[p] = sqrt(d / radius);
        sh.b[p] = sp * gg;
    }
    const double gmax = block_max(gmx, sh.redm);
    if (threadIdx.x == 0) st_x(rec, gmax);
    ph_arrive(sync + PS_G);
    double* S = sh.S;
    for (int e = threadIdx.x; e < ni6 * ni6; e += BA_THREADS) {
        const int r = e / ni6, c = e - ni6 * (e / ni6);
        double v = r == c ? 1.0 : 0.0;
        if (r < ni && c < ni) {
            v = Hs[r * ni + c] * sh.s_f[r] * sh.s_f[c];
            if (r == c) v += sh.D_f[r] * sh.D_f[r];
        }
        S[r * ls + c] = v;
    }
    for (int f = threadIdx.x; f < ni6; f += BA_THREADS) S[ni6 * ls + f] = f < ni ? sh.b[f] : 0.0;
    if (threadIdx.x == 0) sh.chol_bad = 0;
    __syncthreads();
    bool ok;
    if (P.chol_variant == 2 && chol_tile_rows(ni6) == 3)
        ok = chol_tile_solve2<3, 0>(S, ni6, S, 0, ls, sh.b, sh.b, sh.stage + 128, &sh.chol_bad);
    else
        ok = chol6_solve2<BA_THREADS>(S, ni6, S, 0, ls, sh.b, sh.b, sh.stage + 128, sh.stage + 128 + BA_NF_MAX,
                                      &sh.chol_bad);
    double sn = 0.0, xn = 0.0, fin = 0.0;
    if (ok) {
        for (int p = threadIdx.x; p < ni; p += BA_THREADS) {
            sh.D_f[p] = -sh.b[p] * sh.s_f[p];  // the IMU rows of the f-space step
            st_x(Dd + np + p, sh.D_f[p]);
            if (!isfinite(sh.b[p])) fin = 1.0;
        }
        __syncthreads();
        for (int e = threadIdx.x; e < 3 * K; e += BA_THREADS) {  // ph_solve_body's candidate loops
            const int vf = w.vel_f[e / 3];
            const double xx = x.xv[e];
            const double cnd = vf >= 0 ? xx + sh.D_f[vf - np + e % 3] : xx;
            st_x(x.cv + e, cnd);
            if (vf >= 0) { const double d = xx - cnd; sn += d * d; xn += cnd * cnd; }
        }
        for (int e = threadIdx.x; e < 6; e += BA_THREADS) {
            const int f = e < 3 ? w.bg_f + e : w.ba_f + e - 3;
            const bool a = e < 3 ? w.bg_f >= 0 : w.ba_f >= 0;
            const double xx = x.xb[e];
            const double cnd = a ? xx + sh.D_f[f - np] : xx;
            st_x(x.cb + e, cnd);
            if (a) { const double d = xx - cnd; sn += d * d; xn += cnd * cnd; }
        }
    }
    double rv[3] = {sn, xn, fin};
    block_reduce<2, 1>(rv, sh.redv);
    if (threadIdx.x == 0) {
        st_x(rec + 1, rv[0]);
        st_x(rec + 2, rv[1]);
        st_x(rec + 3, rv[2]);
        st_x(rec + 4, ok ? 0.0 : 1.0);
    }
    ph_arrive(sync + PS_I);
}

template <int TI>
__device__ __forceinline__ void ph_cluster_schur_t(const BaPools& P, const PhCtx& x, int wi, int gi, double radius,
                                                PhSchurSh& ss, double* dyn) {
    ph_schur_group<TI>(P, x, wi, gi, radius, ss, dyn);
}
__device__ __forceinline__ void ph_cluster_schur(const BaPools& P, const PhCtx& x, int wi, int gi, double radius, PhSchurSh& ss,
                                        double* dyn) {
    switch (ph_schur_t(x.c.w->T)) {
        case 1: ph_cluster_schur_t<1>(P, x, wi, gi, radius, ss, dyn); break;
        case 2: ph_cluster_schur_t<2>(P, x, wi, gi, radius, ss, dyn); break;
        case 3: ph_cluster_schur_t<3>(P, x, wi, gi, radius, ss, dyn); break;
        case 4: ph_cluster_schur_t<4>(P, x, wi, gi, radius, ss, dyn); break;
        case 5: ph_cluster_schur_t<5>(P, x, wi, gi, radius, ss, dyn); break;
        default: ph_cluster_schur_t<6>(P, x, wi, gi, radius, ss, dyn); break;
    }
}

// grid: 8 * C * ceil(n / 8) blocks; block b -> window (b / 8 / C) * 8 + b % 8, member (b / 8) % C.
// Members: 0 the leader, 1..C-2 the chunk members (chunk ci owned by member 1 + ci % (C - 2)), C-1 the
// IMU member (VI windows: the IMU part of the model change, the IMU factors at the candidate and their
// normal equations beside the walks; ph_imu_terms).  Schur partials: the owner of chunk ci writes group ci's
// partial; once every chunk member has written its groups (counter WB, the chunk members' own barrier), a
// reduce-scatter sums them -- member r the elements [r E / nm, (r + 1) E / nm) over all groups in group
// order (ph_reduce_groups) -- and the leader reads the one total: the same sums whatever C is.
#ifdef VIO_BA_CLUSTER_TU
__global__ void __launch_bounds__(BA_THREADS, 1) ph_cluster_kernel(BaPools P, int n, int C) {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    const int b = (int)blockIdx.x, row = b >> 3;
    const int m = row % C, wi = (row / C) * 8 + (b & 7);
    if (wi >= n || ph_skip(P, wi)) return;
    BaShared& bs = *reinterpret_cast<BaShared*>(smem_raw);
    PhShared& sh = *reinterpret_cast<PhShared*>(smem_raw);
    double* sU = reinterpret_cast<double*>(smem_raw + sizeof(PhShared));
    PhClusterSh& cs = *reinterpret_cast<PhClusterSh*>(smem_raw + sizeof(BaShared));
    PhSchurSh& ss = *reinterpret_cast<PhSchurSh*>(smem_raw);
    double* sdyn = reinterpret_cast<double*>(smem_raw + ((sizeof(PhSchurSh) + 15) & ~(size_t)15));
    // a chunk member's walk prelude (ph_back_pre: its lanes' Jacobians), past PhShared: free between the
    // member's Schur group and its walk
    double* wjl = reinterpret_cast<double*>(smem_raw + ((sizeof(PhShared) + 15) & ~(size_t)15));
    static_assert(((sizeof(PhShared) + 15) & ~(size_t)15) + sizeof(double) * 18 * BA_THREADS <= sizeof(BaShared),
                  "walk prelude LDS");
    int* sync = P.csync + (size_t)PH_SYNC_INTS * wi;
    int* err = sync + PS_ERR;
    const int nw = C - 1;  // workgroups that arrive at A / B every iteration (chunk members + IMU member)
    const int nm = C - 2;  // chunk members
    if (m == 0) {
        // ---------------- leader ----------------
        ph_setup_body<true>(P, wi, sh);
        ph_release_arrive(sync + PS_S, false);  // setup's outputs (tables, initial parameters) to the members
        {   // the LM state stays on chip from here to the end of the solve (ph_ctx<true>): the step control,
            // prep and solve read and write it in LDS instead of a global round trip each
            __syncthreads();
            const double* g = reinterpret_cast<const double*>(ph_ctx(P, wi, 0).gs);
            double* l = reinterpret_cast<double*>(ph_lds_state());
            static_assert(sizeof(PhState) % 8 == 0, "PhState copy");
            for (int e = threadIdx.x; e < (int)(sizeof(PhState) / 8); e += BA_THREADS) l[e] = g[e];
            __syncthreads();
        }
        const PhCtx x0 = ph_ctx<true>(P, wi, 0);
        int genA = nw;  // the first linearisation's arrivals
        // record R {done, cur, radius}: after the step control (the Schur groups need nothing of the rest
        // of ph_prep but the first slot's Jacobi scaling: the first slot publishes after its whole prep)
        auto publish_r = [&](int gen) {
            int rv[2] = {0, 0};
            double rad = 0.0;
            if (threadIdx.x == 0) {
                const PhState& g = *x0.gs;
                rv[0] = g.st.done;
                rv[1] = g.cur;
                rad = g.st.radius;
            }
            ph_publish(sync + PS_R, sync + PS_REC, gen, rv, 2, &rad, 1);
        };
        // diagnostic slots of the cluster route (leader): 8 wait for the walks, 9 wait for the Schur
        // groups; (member 1): 11 wait for R, 12 wait for F, 23 walk; (IMU member) 10 IMU candidate terms
        PhStamp lst(P.prof, wi);
        for (int it = 0;; ++it) {
            lst.reset();
            if (!ph_wait(sync + PS_A, genA, err, cs)) return;
            lst(8);
            const int cur = ph_prep_ctrl<true>(P, wi, sh);
            __syncthreads();
            if (it > 0) publish_r(it + 1);
            ph_prep_rest<true>(P, wi, sh, sU, cur, sync + PS_G, it + 1, err);
            __syncthreads();
            if (it == 0) publish_r(it + 1);
            if (threadIdx.x == 0) cs.rec[0] = x0.gs->st.done;
            __syncthreads();
            int fv[2] = {0, 0};
            if (cs.rec[0]) {  // done: by the step control (members stop at R) or by the finalisation (at F)
                fv[1] = 1;
                ph_publish(sync + PS_F, sync + PS_REC + 32, it + 1, fv, 2, nullptr, 0);
                break;
            }
            ph_solve_body<true>(P, wi, bs, 1);  // everything of the reduced system but the Schur partials
            lst.reset();
            if (!ph_wait(sync + PS_B, nw * (it + 1), err, cs)) return;
            lst(9);
            ph_solve_body<true>(P, wi, bs, 2, sync + PS_I, it + 1, err);
            __syncthreads();
            if (threadIdx.x == 0) fv[0] = x0.gs->step_valid;
            ph_publish(sync + PS_F, sync + PS_REC + 32, it + 1, fv, 2, nullptr, 0);
            genA += nw;
        }
        if (!ph_wait(sync + PS_E, nw, err, cs)) return;
        ph_acquire();
        ph_post_body<true>(P, wi, sh);
        return;
    }
    // ---------------- members ----------------
    const bool imu_member = m == C - 1;
    if (!ph_wait(sync + PS_S, 1, err, cs)) return;
    ph_acquire();
    const PhCtx x0 = ph_ctx(P, wi, 0);
    const int nch = x0.ph.nch;
    const int done0 = x0.gs->st.done;  // setup's (fenced)
    if (!done0 && !imu_member)
        for (int ci = m - 1; ci < nch; ci += nm) {
            ph_lin_body(P, wi, ci, sh);
            __syncthreads();
        }
    ph_arrive(sync + PS_A);
    PhStamp mst(m == 1 || imu_member ? P.prof : nullptr, wi);
    const int T = x0.c.w->T, NT = T * (T + 1) / 2;
    const bool is_vi = x0.c.w->is_vi != 0;
    const int64_t gstride = (int64_t)NT * 256 + 16 * T;
    for (int it = 0;; ++it) {
        // (an opaque copy of the window index per iteration: everything derived from it is recomputed in
        // the loop instead of being hoisted and kept live -- spilled -- across the whole persistent loop)
        int wil = wi;
        asm volatile("" : "+s"(wil));
        int* sync = P.csync + (size_t)PH_SYNC_INTS * wil;
        int* err = sync + PS_ERR;
        mst.reset();
        if (!ph_wait(sync + PS_R, it + 1, err, cs)) return;
        if (!imu_member) mst(11);
        ph_read_rec(sync + PS_REC, 2, cs, true);
        if (cs.rec[0]) break;  // done
        const int cur = cs.rec[1];
        const double radius = cs.radius;
        const PhCtx x = ph_ctx(P, wil, cur);
        if (!imu_member) {
            for (int ci = m - 1; ci < nch; ci += nm) {  // own groups (one landmark chunk each)
                ph_schur_inputs(ss, x, nullptr);
                __syncthreads();
                ph_cluster_schur(P, x, wil, ci, radius, ss, sdyn);
                __syncthreads();
            }
            // reduce-scatter: once every chunk member's partials are out, member r sums the elements
            // [r E / nm, (r + 1) E / nm) over all groups in group order into the total -- the same sums
            // whatever nm is; the leader then reads one total instead of every partial
            ph_arrive(sync + PS_WB);
            if (!ph_wait(sync + PS_WB, nm * (it + 1), err, cs)) return;
            ph_reduce_groups(x.pr + x.ph.spart, x.pr + x.ph.stot, gstride, nch, m - 1, nm);
            if (m == 1 && threadIdx.x == 0) {  // any group's landmark block not positive definite
                double bad = 0.0;
                for (int q = 0; q < nch; ++q) bad = fmax(bad, ld_x(x.pr + x.ph.bpart + 8 * q));
                st_x(x.pr + x.ph.stot + gstride, bad);
            }
        }
        ph_arrive(sync + PS_B);
        if (imu_member && is_vi) ph_imu_solve(P, wil, cur, radius, bs, sync);
        // while the leader solves the reduced system: the first own chunk's step-independent walk inputs
        if (!imu_member) ph_back_pre(P, sh, wil, m - 1, cur, wjl);
        mst.reset();
        if (!ph_wait(sync + PS_F, it + 1, err, cs)) return;
        if (!imu_member) mst(12);
        ph_read_rec(sync + PS_REC + 32, 2, cs, false);
        if (cs.rec[1]) break;  // done by the finalisation of this slot
        if (cs.rec[0]) {  // a valid step: the walks / the IMU candidate terms
            const PhView v{cur, 0, 1, radius, nullptr};
            if (imu_member) {
                mst.reset();
                ph_back_body<true>(P, sh, wil, nch, v);
                mst(10);
                ph_arrive(sync + PS_A);  // the step control needs the terms; the normal equations follow
                if (is_vi) {
                    ph_imu_spec_normal_eq(sh, ph_ctx(P, wil, cur), sh.buf);
                    mst(28);
                }
                ph_arrive(sync + PS_H);
                continue;
            } else {
                ph_back_body<false>(P, sh, wil, m - 1, v, wjl);  // (the first own chunk: its prelude)
                __syncthreads();
                for (int ci = m - 1 + nm; ci < nch; ci += nm) {
                    ph_back_body<false>(P, sh, wil, ci, v);
                    __syncthreads();
                }
                mst(23);
            }
        }
        ph_arrive(sync + PS_A);
        if (imu_member) ph_arrive(sync + PS_H);  // (no step: nothing to form, the count advances)
    }
    ph_release_arrive(sync + PS_E, true);  // the final landmark positions (and the rest) to the leader's post
}
#endif
// ------------------------------------------------------------------------------------------
#ifndef VIO_BA_CLUSTER_TU
size_t ba_phase_doubles(int K, int L, int N, int T) { return (size_t)ph_layout(K, L, N, T, PH_GS_MIN).total; }

static const char* ph_last_failed = "";
// per Schur instance (tile count) of a batch: the largest dynamic LDS in doubles of the unstaged kernel over
// all its windows (0: tile count unused) and of the staged kernel over the windows that fit it, and whether a
// launch over these windows takes the staged instance: where every one of them fits it
struct PhSchurPlan {
    int lds_u[7], lds_s[7];
    bool staged[7];
    size_t bytes(int t) const { return sizeof(double) * (size_t)(staged[t] ? lds_s[t] : lds_u[t]); }
};
// grid extents of a batch and its Schur plan
static void ph_extents(const BaWin* hw, int n, int& slots, int& nch_max, int& ng_max, PhSchurPlan& sp) {
    slots = 1; nch_max = 1; ng_max = 1;
    for (int t = 0; t <= 6; ++t) sp.lds_u[t] = sp.lds_s[t] = 0, sp.staged[t] = true;
    for (int i = 0; i < n; ++i) {
        const PhLayout pl = ph_layout(hw[i].K, hw[i].L, hw[i].N, hw[i].T, hw[i].gs);
        slots = std::max(slots, hw[i].max_iter + 1);
        nch_max = std::max(nch_max, pl.nch);
        ng_max = std::max(ng_max, pl.ng);
        if (!hw[i].is_pnp) {
            const int ti = ph_schur_t(hw[i].T);
            sp.lds_u[ti] = std::max(sp.lds_u[ti], ph_schur_lds_doubles(hw[i].T, pl.LC));
            const int sd = ph_schur_staged_doubles(hw[i].T, pl.LC, std::min(hw[i].gs, pl.nch));
            sp.lds_s[ti] = std::max(sp.lds_s[ti], sd);
            if (!sd) sp.staged[ti] = false;
        }
    }
    for (int t = 0; t <= 6; ++t) sp.staged[t] = sp.staged[t] && sp.lds_s[t] > 0;
}
// ph_schur's LDS for one window shape (tests): out = { dynamic bytes, static bytes, staged instance taken }
void ba_schur_lds_info(int K, int L, int T, int gs, int32_t out[3]) {
    BaWin w{};
    w.K = K; w.L = L; w.T = T; w.max_iter = 1;
    ba_win_set_geometry(w);
    ba_win_set_gs(w, gs);
    int slots, nch_max, ng_max;
    PhSchurPlan sp;
    ph_extents(&w, 1, slots, nch_max, ng_max, sp);
    const int ti = ph_schur_t(T);
    out[0] = (int32_t)sp.bytes(ti);
    out[1] = (int32_t)sizeof(PhSchurSh);
    out[2] = sp.staged[ti] ? 1 : 0;
}
// kernel attributes (dynamic LDS limits) for a batch: set outside any stream capture.  Both instances of a tile
// count get theirs -- the unstaged one for the batch's largest panel, the staged one for the largest staged
// size among the windows that fit it: a sub-batch of the batch (launch_ba_phases) decides for its own windows,
// and whichever instance it takes then needs no more than was set here
hipError_t ba_phases_prepare(const BaWin* hw, int n) {
    int slots, nch_max, ng_max;
    PhSchurPlan sp;
    ph_extents(hw, n, slots, nch_max, ng_max, sp);
    static bool attr_set[kMaxDevices] = {};
    static size_t schur_attr[kMaxDevices][7][2] = {};
    std::lock_guard<std::mutex> lock(g_attr_mutex);  // see launch_ba_windows
    const int dev = current_device();
    if (!attr_set[dev]) {
        hipError_t e = hipFuncSetAttribute((const void*)ph_solve_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)sizeof(BaShared));
        if (e != hipSuccess) return e;
        attr_set[dev] = true;
    }
    for (int t = 1; t <= 6; ++t)
        for (int st = 0; st < 2; ++st) {
            const size_t schur_lds = sizeof(double) * (size_t)(st ? sp.lds_s[t] : sp.lds_u[t]);
            if (schur_lds > schur_attr[dev][t][st]) {
                hipError_t e = hipFuncSetAttribute(ph_schur_fn(t, st != 0), hipFuncAttributeMaxDynamicSharedMemorySize, (int)schur_lds);
                if (e != hipSuccess) return e;
                schur_attr[dev][t][st] = schur_lds;
            }
        }
    return hipSuccess;
}
const char* ba_phases_failed_launch() { return ph_last_failed; }

#endif
#ifdef VIO_BA_CLUSTER_TU
// Cluster route geometry: members per window (1 leader + up to one member per landmark chunk), or 0 when
// the batch cannot have every member resident at once on this device (its workgroups wait for each
// other: a member that cannot be scheduled would stall the others until their bounded waits expire) or
// a window's Schur panel does not fit the kernel's LDS.  Call outside any stream capture.
int ba_cluster_members(const BaWin* hw, int n, int max_per_window) {
    static int cap[kMaxDevices] = {};
    std::lock_guard<std::mutex> lock(g_attr_mutex);
    const int dev = current_device();
    if (!cap[dev]) {
        if (hipFuncSetAttribute((const void*)ph_cluster_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)ph_cluster_lds_bytes()) != hipSuccess)
            return 0;
        int per_cu = 0, cus = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)ph_cluster_kernel, BA_THREADS,
                                                         ph_cluster_lds_bytes()) != hipSuccess ||
            hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
            return 0;
        // one fewer per CU than the API reports when near its edge (MICROARCH "Residency"): the kernel
        // is sized for one workgroup per CU; keep a margin of 8 CUs for anything else on the device
        cap[dev] = std::max(1, std::min(per_cu, 1) * cus - 8);
    }
    int nch_max = 1, live = 0;
    for (int i = 0; i < n; ++i) {
        if (hw[i].is_pnp) continue;
        ++live;
        const PhLayout pl = ph_layout(hw[i].K, hw[i].L, hw[i].N, hw[i].T, 1);
        nch_max = std::max(nch_max, pl.nch);
        if (sizeof(PhSchurSh) + 16 + sizeof(double) * (size_t)ph_schur_lds_doubles(hw[i].T, pl.LC) > sizeof(BaShared))
            return 0;
    }
    if (!live) return 0;

    int C = std::min(nch_max + 2, max_per_window > 0 ? max_per_window : nch_max + 2);  // + leader, IMU member
    C = std::min(C, cap[dev] / n);
    // without an explicit member count, a window needs at least half a member per landmark chunk: below
    // that the walks of a member's several chunks run back to back on one CU and the phase kernels (which
    // spread every chunk over its own workgroup) are faster (measured: 32 config-3 windows, 7 members per
    // window, 2.18 ms per 10 iterations against 1.65 on the phase route; 16 windows, 15 members, 1.47 / 1.53)
    if (max_per_window <= 0 && 2 * C < nch_max + 2) return 0;
    return C >= 3 ? C : 0;
}
// the hand-off words of a cluster launch, cleared before every run (outside the captured graph of a reusable
// batch, so that the test hook below applies to graph replays too)
hipError_t ba_cluster_prelaunch(const BaPools& P, int n, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(P.csync, 0, sizeof(int) * PH_SYNC_INTS * (size_t)n, stream);
    if (e != hipSuccess) return e;
    // (VIO_BA_TEST_CLUSTER_ERR=1: window 0's error word starts set, as after a timed-out wait -- every
    // member's next wait gives up; the host's device-error path, exercised by tests/test_ba_gpu.py)
    static std::atomic<int> test_err{[] {
        const char* v = std::getenv("VIO_BA_TEST_CLUSTER_ERR");
        return v && v[0] == '1' ? 1 : 0;
    }()};  // one-shot: the first cluster run of the process only (one-shot solve or batch replay)
    if (test_err.exchange(0) && (e = hipMemsetAsync(P.csync + PS_ERR, 1, 1, stream)) != hipSuccess) return e;
    return hipSuccess;
}
hipError_t launch_ba_cluster(const BaPools& P, int n, int C, hipStream_t stream) {
    const int groups = (n + 7) / 8;
    hipLaunchKernelGGL(ph_cluster_kernel, dim3(8 * C * groups), dim3(BA_THREADS), ph_cluster_lds_bytes(), stream, P, n, C);
    return hipGetLastError();  // (the caller names the kernel on failure)
}
#endif
#ifndef VIO_BA_CLUSTER_TU
// the phase sequence of the windows [P.win_base, P.win_base + n) on one stream; hw: host copy of the
// packed window descriptors of those windows (grid extents and LDS sizes come from them)
static dim3 ph_grid(int per, int n) {
    static const bool plain = [] {
        const char* v = std::getenv("VIO_BA_XCD_ROWS");  // experiment override: 0 = the plain (per, n) order
        return v && v[0] == '0';
    }();
    const int gx = !plain && n % 8 == 0 ? 8 : 1;
    return dim3(gx, per, n / gx);
}
static hipError_t launch_ba_phase_seq(const BaPools& P, const BaWin* hw, int n, hipStream_t stream) {
    int slots, nch_max, ng_max;
    PhSchurPlan sp;
    ph_extents(hw, n, slots, nch_max, ng_max, sp);
    hipError_t e;
#define PH_CHECK(what)                                                             \
    if ((e = hipGetLastError()) != hipSuccess) {                                   \
        ph_last_failed = what;                                                     \
        return e;                                                                  \
    }
    hipLaunchKernelGGL(ph_setup_kernel, dim3(n), dim3(BA_THREADS), 0, stream, P);
    PH_CHECK("ph_setup_kernel");
    for (int s = 0; s < slots; ++s) {
        // the last slot's finalisation ends every window (iteration == max_iterations, counted on every
        // slot, valid step or not): its step kernels would all return at once, so they are not enqueued
        // (measured and not kept: the step control as its own launch with ph_prep beside the Schur groups,
        // 305 -> 345 us per iteration at 256 windows -- the long Schur workgroups then wait for slots)
        if (s == 0) {  // later linearisations come from ph_back (the accepted candidate's)
            hipLaunchKernelGGL(ph_lin_kernel, ph_grid(nch_max, n), dim3(BA_THREADS), 0, stream, P);
            PH_CHECK("ph_lin_kernel");
        }
        hipLaunchKernelGGL(ph_prep_kernel, dim3(n), dim3(BA_THREADS), 0, stream, P);
        PH_CHECK("ph_prep_kernel");
        if (s + 1 == slots) break;
        for (int t = 1; t <= 6; ++t)  // one launch per tile count present (config batches: one)
            if (sp.lds_u[t]) ph_schur_launch(t, sp.staged[t], ph_grid(ng_max, n), sp.bytes(t), stream, P);
        PH_CHECK("ph_schur_kernel");
        hipLaunchKernelGGL(ph_solve_kernel, dim3(n), dim3(BA_THREADS), sizeof(BaShared), stream, P);
        PH_CHECK("ph_solve_kernel");
        if (P.imu_in_back) hipLaunchKernelGGL(ph_back_x_kernel, ph_grid(nch_max + 1, n), dim3(BA_THREADS), 0, stream, P);
        else hipLaunchKernelGGL(ph_back_kernel, ph_grid(nch_max, n), dim3(BA_THREADS), 0, stream, P);
        PH_CHECK("ph_back_kernel");

    }
    hipLaunchKernelGGL(ph_post_kernel, dim3(n), dim3(BA_THREADS), 0, stream, P);
    PH_CHECK("ph_post_kernel");
#undef PH_CHECK
    return hipGetLastError();
}
// The batch as L contiguous sub-batches, each running its own phase sequence on its own stream (lane 0
// on `stream`, lane l on side[l - 1], forked from and joined back into `stream` through ev[]): the
// windows are independent, so one sub-batch's single-workgroup phases (ph_prep, ph_solve: one workgroup
// per window, latency-bound) overlap another's chip-filling ones (ph_schur, ph_back).  Every window
// runs the same kernels on the same data either way: bitwise the single-stream results.
hipError_t launch_ba_phases(const BaPools& P, const BaWin* hw, int n, hipStream_t stream, int lanes,
                            hipStream_t* side, hipEvent_t* ev) {
    if (lanes <= 1 || n < 2) return launch_ba_phase_seq(P, hw, n, stream);
    lanes = std::min(lanes, n);
    hipError_t e;
    if ((e = hipEventRecord(ev[0], stream)) != hipSuccess) return e;  // fork
    for (int l = 0; l < lanes; ++l) {
        const int b = (int)((long long)n * l / lanes), m = (int)((long long)n * (l + 1) / lanes) - b;
        hipStream_t st = l == 0 ? stream : side[l - 1];
        if (l > 0 && (e = hipStreamWaitEvent(st, ev[0], 0)) != hipSuccess) return e;
        BaPools Pl = P;
        Pl.win_base = P.win_base + b;
        if ((e = launch_ba_phase_seq(Pl, hw + b, m, st)) != hipSuccess) return e;
        if (l > 0 && (e = hipEventRecord(ev[l], st)) != hipSuccess) return e;
    }
    for (int l = 1; l < lanes; ++l)  // join
        if ((e = hipStreamWaitEvent(stream, ev[l], 0)) != hipSuccess) return e;
    return hipSuccess;
}

#endif
}  // namespace vio360
