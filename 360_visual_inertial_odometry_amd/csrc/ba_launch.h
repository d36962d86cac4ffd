// ba_launch.h — the host functions that cross the BA translation units, declared once: included by the callers
// (ba_host.cpp, lie_host.cpp) and by every file that defines one.  Declarations only, nothing device-side.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "vio360.h"

namespace vio360 {

struct BaPools;  // ba_types.h
struct BaWin;

// ba_kernel.hip: the single-kernel solver, the record pack, the workspace the kernels add to ba_ws_layout
hipError_t launch_ba_windows(const BaPools& P, int n, hipStream_t stream);
hipError_t launch_ba_pack(const BaPools& P, int n, uint8_t* dst, int64_t rec_bytes, hipStream_t stream);
size_t ba_ws_extra_doubles();

// ba_phases.inc: the phase route
constexpr int kPhLanesMax = 4;  // sub-batches of the phase route, each on its own stream
hipError_t launch_ba_phases(const BaPools& P, const BaWin* hw, int n, hipStream_t stream, int lanes,
                            hipStream_t* side, hipEvent_t* ev);
size_t ba_phase_doubles(int K, int L, int N, int T);  // sized for the smallest group (most partials)
const char* ba_phases_failed_launch();
hipError_t ba_phases_prepare(const BaWin* hw, int n);
void ba_schur_lds_info(int K, int L, int T, int gs, int32_t out[3]);

// ba_phases.inc as compiled into ba_cluster.hip: the cluster route
int ba_cluster_members(const BaWin* hw, int n, int max_per_window);
hipError_t launch_ba_cluster(const BaPools& P, int n, int C, hipStream_t stream);
hipError_t ba_cluster_prelaunch(const BaPools& P, int n, hipStream_t stream);

// ba_global_host.cpp: problems beyond one workgroup's reduced system
bool global_ba_applicable(const vio_ba_problem& p);
int global_ba_solve(vio_ctx* ctx, const vio_ba_problem& p, vio_ba_output* out);

// ba_kernel.hip / imu_init.hip: the evaluation probes of lie_host.cpp
hipError_t launch_lie_ba(int op, const double* in, double* out, int n, hipStream_t stream);
hipError_t launch_lie_init(int op, const double* in, double* out, int n, hipStream_t stream);
hipError_t launch_imu_factor(const vio_preint* pre, const vio_pose* Ti, const vio_pose* Tj, const double* st,
                             double* out, int n, hipStream_t stream);

}  // namespace vio360
