// ecgpu_x448.hip — instantiates the X448 kernels (ecgpu_x448.h) and the fe448 self-test; built once, not per curve: a translation
// unit of its own so that tools/ct_isa_check.py --unit x448 looks at exactly these kernels
#include "ecgpu_x448.h"
#include "ecgpu_launch.h"

namespace ecgpu {

namespace {
inline unsigned x448_grid(size_t n) { return (unsigned)((n + X448_BLOCK - 1) / X448_BLOCK); }
}  // namespace

void launch_x448(hipStream_t s, int mode, const uint8_t* scalars, const uint8_t* points, size_t n, uint8_t* out, uint8_t* ok) {
    const dim3 grid(x448_grid(n)), block(X448_BLOCK);
    if (mode == X448_CHECKED)
        hipLaunchKernelGGL(k_x448_ladder<X448_CHECKED>, grid, block, 0, s, scalars, points, n, out, ok);
    else if (mode == X448_UNCHECKED)
        hipLaunchKernelGGL(k_x448_ladder<X448_UNCHECKED>, grid, block, 0, s, scalars, points, n, out, ok);
    else
        hipLaunchKernelGGL(k_x448_ladder<X448_BASE>, grid, block, 0, s, scalars, points, n, out, ok);
}

void launch_selftest_fe448(hipStream_t s, int op, const uint32_t* a, const uint32_t* b, size_t n, uint32_t* out) {
    hipLaunchKernelGGL(k_selftest_fe448<>, dim3(x448_grid(n)), dim3(X448_BLOCK), 0, s, op, a, b, n, out);
}

}  // namespace ecgpu
