// ecgpu_inst_h2c.hip — instantiates the hash-to-curve kernels (ecgpu_h2c.h) for -DECGPU_CURVE=...; a translation unit of its own so
// that tools/ct_isa_check.py --unit h2c can look at exactly these kernels.  A parameter set without a suite (everything but k256,
// p256, p384) gets empty kernels that are never launched: the entry points return ECGPU_ERR_CURVE before they reach this file.
#include "ecgpu_h2c.h"
#include "ecgpu_launch.h"

namespace ecgpu {

using CurveT = ECGPU_CURVE;

namespace {
inline unsigned h2c_grid(size_t n) { return (unsigned)((n + BLOCK - 1) / BLOCK); }
}  // namespace

template <> bool h2c_supported<CurveT>() { return H2cSuite<CurveT>::SUPPORTED; }
template <> int h2c_digest<CurveT>() { return H2cSuite<CurveT>::D; }
template <> void launch_h2c_expand<CurveT>(hipStream_t s, const uint8_t* msgs, size_t msg_len, size_t n, const uint8_t* dstp,
                                           size_t dstp_len, int count, bool to_scalar, uint8_t* out) {
    hipLaunchKernelGGL(k_h2c_expand<CurveT>, dim3(h2c_grid(n)), dim3(BLOCK), 0, s, msgs, msg_len, n, dstp, dstp_len, count,
                       to_scalar ? 1 : 0, out);
}
template <> void launch_h2c_map<CurveT>(hipStream_t s, const uint8_t* u, int per_point, size_t n, uint32_t* proj_out, uint8_t* flags,
                                        int* status) {
    hipLaunchKernelGGL(k_h2c_map<CurveT>, dim3(h2c_grid(n)), dim3(BLOCK), 0, s, u, per_point, n, proj_out, flags);
    hipLaunchKernelGGL(k_h2c_flags, dim3(64), dim3(BLOCK), 0, s, (const uint8_t*)flags, n, status);
}
template <> int h2c_draw_bytes<CurveT>() { return H2cSuite<CurveT>::L; }
template <> void launch_selftest_h2c<CurveT>(hipStream_t s, int op, const uint8_t* in, size_t n, uint8_t* out) {
    hipLaunchKernelGGL(k_selftest_h2c<CurveT>, dim3(h2c_grid(n)), dim3(BLOCK), 0, s, op, in, n, out);
}

}  // namespace ecgpu
