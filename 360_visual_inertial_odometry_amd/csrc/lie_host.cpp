// lie_host.cpp — the two evaluation probes of the C-ABI: vio_lie_eval (the Lie maps of lie_dev.h on the device)
// and vio_imu_factor_eval (the BA inertial factor's residual and Jacobians), for the known-answer tests.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "ba_launch.h"
#include "ctx.h"

using namespace vio360;

extern "C" {

int vio_lie_eval(vio_ctx* ctx, int op, const double* in, int n, double* out) {
    static const int kIn[5] = {3, 6, 9, 3, 9}, kOut[5] = {9, 12, 3, 9, 3};
    if (!ctx || op < VIO_LIE_SO3_EXP || op > VIO_LIE_SO3D_LOG || n < 0 || (n > 0 && (!in || !out))) return VIO_EINVAL;
    if (n == 0) return VIO_OK;
    const size_t bi = sizeof(double) * kIn[op] * (size_t)n, bo = sizeof(double) * kOut[op] * (size_t)n;
    auto* d = static_cast<char*>(ctx_buffer(ctx, kSlotLie, bi + bo));
    if (!d) {
        set_error(ctx, "vio_lie_eval: device allocation failed");
        return VIO_ENOMEM;
    }
    VIO_DEVICE(ctx);
    double* din = reinterpret_cast<double*>(d);
    double* dout = reinterpret_cast<double*>(d + bi);
    VIO_HIP(ctx, hipMemcpyAsync(din, in, bi, hipMemcpyHostToDevice, ctx->stream));
    VIO_HIP(ctx, op <= VIO_LIE_IMU_LOG ? launch_lie_ba(op, din, dout, n, ctx->stream)
                                       : launch_lie_init(op, din, dout, n, ctx->stream));
    VIO_HIP(ctx, hipMemcpyAsync(out, dout, bo, hipMemcpyDeviceToHost, ctx->stream));
    VIO_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return VIO_OK;
}

int vio_imu_factor_eval(vio_ctx* ctx, int n, const vio_preint* preint, const double* gravity, const vio_pose* T_wb_i_init,
                        const vio_pose* T_wb_j_init, const double* delta_i, const double* v_i, const double* bg,
                        const double* ba, const double* delta_j, const double* v_j, double* out) {
    constexpr size_t kIn = 27, kOut = 315;
    if (!ctx || n < 0) return VIO_EINVAL;
    if (n > 0 && (!preint || !gravity || !T_wb_i_init || !T_wb_j_init || !delta_i || !v_i || !bg || !ba || !delta_j ||
                  !v_j || !out))
        return VIO_EINVAL;
    if (n == 0) return VIO_OK;
    const size_t N = (size_t)n, b_pre = sizeof(vio_preint) * N, b_pose = sizeof(vio_pose) * N,
                 b_st = sizeof(double) * kIn * N, b_in = b_pre + 2 * b_pose + b_st, b_out = sizeof(double) * kOut * N;
    static_assert(sizeof(vio_preint) % 8 == 0 && sizeof(vio_pose) % 8 == 0, "the packed inputs stay 8-byte aligned");
    auto* d = static_cast<char*>(ctx_buffer(ctx, kSlotLie, b_in + b_out));
    if (!d) {
        set_error(ctx, "vio_imu_factor_eval: device allocation failed");
        return VIO_ENOMEM;
    }
    std::vector<char> h(b_in);
    std::memcpy(h.data(), preint, b_pre);
    std::memcpy(h.data() + b_pre, T_wb_i_init, b_pose);
    std::memcpy(h.data() + b_pre + b_pose, T_wb_j_init, b_pose);
    double* st = reinterpret_cast<double*>(h.data() + b_pre + 2 * b_pose);
    for (size_t f = 0; f < N; ++f) {
        double* s = st + kIn * f;
        std::memcpy(s, gravity + 3 * f, sizeof(double) * 3);
        std::memcpy(s + 3, delta_i + 6 * f, sizeof(double) * 6);
        std::memcpy(s + 9, v_i + 3 * f, sizeof(double) * 3);
        std::memcpy(s + 12, bg + 3 * f, sizeof(double) * 3);
        std::memcpy(s + 15, ba + 3 * f, sizeof(double) * 3);
        std::memcpy(s + 18, delta_j + 6 * f, sizeof(double) * 6);
        std::memcpy(s + 24, v_j + 3 * f, sizeof(double) * 3);
    }
    VIO_DEVICE(ctx);
    VIO_HIP(ctx, hipMemcpyAsync(d, h.data(), b_in, hipMemcpyHostToDevice, ctx->stream));
    VIO_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (h is pageable: the copy has left it)
    VIO_HIP(ctx, launch_imu_factor(reinterpret_cast<const vio_preint*>(d), reinterpret_cast<const vio_pose*>(d + b_pre),
                                   reinterpret_cast<const vio_pose*>(d + b_pre + b_pose),
                                   reinterpret_cast<const double*>(d + b_pre + 2 * b_pose),
                                   reinterpret_cast<double*>(d + b_in), n, ctx->stream));
    VIO_HIP(ctx, hipMemcpyAsync(out, d + b_in, b_out, hipMemcpyDeviceToHost, ctx->stream));
    VIO_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return VIO_OK;
}

}  // extern "C"
