// ecgpu_selftest_msm.h — device-side known-answer entry points for the cross-lane code behind the MSM's buckets (device only).
//
// The row-parallel k256 field (ecgpu_rows.h), the complete addition on the lanes of a quad, the quad tree and the Jacobian
// doubling shared by three lanes (ecgpu_msm.h) are built from DPP row shifts, quad permutes, ds_bpermute and __shfl: no CPU
// build can run them, and inside an MSM their operands are whatever the buckets sum to.  This kernel calls the very inline
// functions k_msm_reduce_windows / k_msm_window_sums / k_msm_combine call, on operands the caller chooses limb by limb.  A kernel
// of its own (ops 20 - 26 of ecgpu_selftest_point), so that the code objects of the other kernels stay what they are.
// Vectors and expectations: tests/msm_tail_vectors.py (model: tools/rows_field_model.py, group model: tests/pyec.py);
// tests/test_gpu_msm_tail.py.
//
// op = code | steps << 8.  n is a multiple of 64 (of BLOCK for the tree): the cross-lane steps need whole waves.
//   k256 only, RAW records: a 64-byte record is sixteen little-endian 32-bit words, words 0..8 are the nine limbs as they are (no
//   unpack, no from_canonical, no range check), and the result record holds the nine output limbs as they are (out_inf = 0):
//   20  RowsK256::mul: row r of a wave multiplies the p-record by the q-record of the wave's lane r; lane i gets the product of row
//       i mod 4
//   21  RowsK256::norm64: row r takes the per-position 64-bit values p-record word | q-record word << 32 of the wave's lane r;
//       lane i gets the result of row i mod 4
//   22  RowsDblK256: X, Y, Z = the p-records of the wave's lanes 0, 1, 2; enter, `steps` times step, leave; lane i gets
//       coordinate i mod 3 as leave produced it (Y: limbs below 2 LB)
//   k256 only, points (affine x || y + identity flag in, affine + flag out, one inversion per lane):
//   23  msm_hom_add_quad on the pair (P, Q) of each quad's first lane, P and Q affine-born or the identity; every lane returns
//       its own copy
//   24  the same on X = Group::add(P, Q) and Y = Group::dbl(Q) (generic Z on both sides): P + 3 Q
//   25  msm_block_sum over the points P of a workgroup's lanes: the sum in the workgroup's first record, the identity in the others
//   the sets whose k_msm_combine takes msm_jac_dbl_lanes (a = -3: every set but k256 and the any-a ones):
//   26  the wave's first point P (+ Q if given: a generic Z) -> (X Z : Y Z^2 : Z), `steps` times msm_jac_dbl_lanes, jac_to_proj —
//       the identity skipped as k_msm_combine skips it; every lane returns its own copy
#pragma once

#include "ecgpu_msm.h"

namespace ecgpu {

#if defined(__HIPCC__)

template <class C>
__device__ __forceinline__ Proj<C> selftest_point_of_lane(const Proj<C>& p, int src) {
    Proj<C> r;
#pragma unroll
    for (int l = 0; l < C::NL; l++) {
        r.x.v[l] = (uint32_t)__shfl((int)p.x.v[l], src, 64);
        r.y.v[l] = (uint32_t)__shfl((int)p.y.v[l], src, 64);
        r.z.v[l] = (uint32_t)__shfl((int)p.z.v[l], src, 64);
    }
    return r;
}

template <class C>
__global__ void __launch_bounds__(BLOCK) k_selftest_msm(int op, const uint8_t* __restrict__ pxy, const uint8_t* __restrict__ pinf,
                                                        const uint8_t* __restrict__ qxy, const uint8_t* __restrict__ qinf, size_t n,
                                                        uint8_t* __restrict__ out_xy, uint8_t* __restrict__ out_inf, int* status) {
    using G = Group<C>;
    using F = Field<C>;
    constexpr int N = C::N, WB = WireBytes<C>::value;
    constexpr bool K256 = C::A_IS_ZERO && C::REPR == REPR_U29_K256;
    const int code = op & 0xFF, steps = op >> 8;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;                                                 // (n is a multiple of 64: whole waves leave)
    const int lane = (int)(threadIdx.x & 63u);
    if constexpr (K256) {
        static_assert(2 * WB == 64, "a record is sixteen words");
        if (code >= 20 && code <= 22) {
            __shared__ uint32_t rows_lds[BLOCK / 64][48];
            const uint32_t* pa = (const uint32_t*)pxy + i * 16;
            const uint32_t* pb = (const uint32_t*)qxy + i * 16;
            uint32_t w[9];
            if (code == 22) {
                Fe<9> X, Y, Z;
#pragma unroll
                for (int t = 0; t < 9; t++) {
                    X.v[t] = (uint32_t)__shfl((int)pa[t], 0, 64);
                    Y.v[t] = (uint32_t)__shfl((int)pa[t], 1, 64);
                    Z.v[t] = (uint32_t)__shfl((int)pa[t], 2, 64);
                }
                RowsDblK256 rd;
                rd.init();
                uint32_t A, B, Q = 0;
                rd.enter(rows_lds[threadIdx.x / 64], X, Y, Z, A, B);
#pragma unroll 1
                for (int s = 0; s < steps; s++) Q = rd.step(A, B);
                rd.leave(Q, X, Y, Z);
                const int which = lane % 3;
#pragma unroll
                for (int t = 0; t < 9; t++) w[t] = which == 0 ? X.v[t] : which == 1 ? Y.v[t] : Z.v[t];
            } else {
                RowsK256 k;
                k.init();
                uint32_t a = 0, b = 0;
#pragma unroll
                for (int t = 0; t < 9; t++) {                           // row r takes the records of the wave's lane r
                    const uint32_t u = (uint32_t)__shfl((int)pa[t], (int)k.row, 64), v = (uint32_t)__shfl((int)pb[t], (int)k.row, 64);
                    a = k.pos == (uint32_t)t ? u : a;
                    b = k.pos == (uint32_t)t ? v : b;
                }
                const uint32_t r = code == 20 ? k.mul(a, b) : k.norm64((uint64_t)a | (uint64_t)b << 32);
                const uint32_t src = ((threadIdx.x & 3u) * 16u) * 4u;
#pragma unroll
                for (int t = 0; t < 9; t++) w[t] = lane_pull(src + 4u * t, r);
            }
            uint32_t* o = (uint32_t*)out_xy + i * 16;
#pragma unroll
            for (int t = 0; t < 16; t++) o[t] = t < 9 ? w[t] : 0u;
            out_inf[i] = 0;
            return;
        }
    }
    const Fe<C::NL> b = G::curve_b();
    Affine<C> pa, qa;
    const bool pf = load_affine<C>(&pa, pxy, pinf, i, b, status);
    const bool qf = qxy ? load_affine<C>(&qa, qxy, qinf, i, b, status) : false;
    const Proj<C> p = pf ? G::from_affine(pa) : G::identity(), q = qf ? G::from_affine(qa) : G::identity();
    Proj<C> r = G::identity();
    bool known = false;
    if constexpr (K256) {
        if (code == 23 || code == 24) {
            const Proj<C> p0 = selftest_point_of_lane<C>(p, lane & ~3), q0 = selftest_point_of_lane<C>(q, lane & ~3);
            const Proj<C> x = code == 23 ? p0 : G::add(p0, q0, b), y = code == 23 ? q0 : G::dbl(q0, b);
            auto X = G::m(x.x), Y = G::m(x.y), Z = G::m(x.z);
            msm_hom_add_quad<C>(X, Y, Z, y, lane & 3);
            r.x = X.e;
            r.y = Y.e;
            r.z = Z.e;
            known = true;
        } else if (code == 25) {
            __shared__ uint32_t tree_lds[BLOCK * 3 * C::NL];
            const Proj<C> sum = msm_block_sum<C>(p, tree_lds, b);
            if (threadIdx.x == 0) r = sum;
            known = true;
        }
    } else if constexpr (!GenericA<C>::value) {
        if (code == 26) {
            Proj<C> acc = selftest_point_of_lane<C>(qxy ? G::add(p, q, b) : p, 0);
            if (!G::is_identity(acc)) {
                Jac<C> j;
                {
                    auto X = G::m(acc.x), Y = G::m(acc.y), Z = G::m(acc.z);
                    j.x = F::mul(X, Z).e;
                    j.y = F::mul(Y, F::sqr(Z)).e;
                    j.z = acc.z;
                }
#pragma unroll 1
                for (int s = 0; s < steps; s++) j = msm_jac_dbl_lanes<C>(j, lane);
                acc = G::jac_to_proj(j);
            }
            r = acc;
            known = true;
        }
    }
    if (!known) atomicOr(status, ST_BAD_SCALAR);
    if (G::is_identity(r)) {
        zero_wire<C>(out_xy + i * (2 * WB), 2);
        out_inf[i] = 1;
    } else {
        auto zi = F::inv(G::m(r.z));
        uint32_t w[N];
        F::to_canonical(w, F::mul(G::m(r.x), zi));
        store_wire<C>(out_xy + i * (2 * WB), w);
        F::to_canonical(w, F::mul(G::m(r.y), zi));
        store_wire<C>(out_xy + i * (2 * WB) + WB, w);
        out_inf[i] = 0;
    }
}

template <class C>
void launch_selftest_msm(hipStream_t s, int op, const uint8_t* pxy, const uint8_t* pinf, const uint8_t* qxy, const uint8_t* qinf, size_t n,
                         uint8_t* out_xy, uint8_t* out_inf, int* status) {
    hipLaunchKernelGGL(k_selftest_msm<C>, dim3((unsigned)((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s, op, pxy, pinf, qxy, qinf, n, out_xy,
                       out_inf, status);
}

#endif  // __HIPCC__

}  // namespace ecgpu
