// ecgpu_xyz.h — projective records X || Y || Z into the variable-time path: the lane body of k_xyz_affine (ecgpu_kernels.h),
// written once for the kernel and for its CPU twin (tests/hostcheck_xyz_var).
//
// `ProjectivePoint::to_affine` (k256/src/arithmetic/projective.rs:64-69, primeorder/src/projective.rs:68-74) of every record,
// with one field inversion for all the records of a lane (Montgomery's trick, as `BatchNormalize::batch_normalize`,
// k256 projective.rs:367-391, primeorder projective.rs:452-478), and the verdict of the _ct_xyz forms (ct_xyz_point,
// ecgpu_ctmul.h): X, Y or Z >= p, or Z != 0 and the point off the curve, is a bad record; Z = 0 is the identity whatever
// X and Y are.  The kernel is variable-time and branches on the record: Z = 0 and Z = 1 (what `ProjectivePoint::from(AffinePoint)`
// gives) stay out of the product chain, and a Z = 1 record is its own affine point.
#pragma once

#include "ecgpu_point.h"

namespace ecgpu {

// the class of a record, kept by the product pass in the spare word of the record's prefix entry
enum : uint32_t { XYZ_FINITE = 0, XYZ_IDENT = 1, XYZ_Z_ONE = 2 };

template <int N>
ECGPU_HD bool mp_is_one(const uint32_t* a) {
    uint32_t r = a[0] ^ 1u;
#pragma unroll
    for (int i = 1; i < N; i++) r |= a[i];
    return r == 0;
}

// Lane t of nthreads owns records t, t + nthreads, t + 2 nthreads, ... (a wave touches 64 consecutive records).  Io:
//   load_z(j, cz)              Z of record j as N canonical words
//   load_xyz(j, cx, cy, cz)    the whole record
//   put_prefix(j, w) / get_prefix(j, w)   NS words: the running product before record j, its class in word NS - 1
//   put_affine(j, x, y, ident) the output record (x = y = 0 for the identity)
//   verdict(j, ok)             false: a bad record
// Each pass has ONE load site: the loads of record i + 1 are issued before record i is worked on (with one wave per SIMD nothing
// else hides their latency), and a p521 kernel keeps to one halfword load per record it reads (tools/wire_codec_isa_check.py).
template <class C, class Io>
ECGPU_HD void xyz_affine_lane(size_t t, size_t n, size_t nthreads, Io& io) {
    using F = Field<C>;
    using G = Group<C>;
    constexpr int N = C::N, NS = F::NS;
    static_assert(NS > C::NL, "raw form has no spare word");
    if (t >= n) return;
    const size_t K = (n - 1 - t) / nthreads + 1;              // records of this lane
    // pass 1, forward: the running product of the Z that are neither 0 nor 1
    typename F::M1 acc = F::one();
    uint32_t cz[N], cz_next[N];
    for (size_t it = 0; it <= K; it++) {
        if (it < K) io.load_z(t + it * nthreads, cz_next);
        if (it > 0) {
            const size_t j = t + (it - 1) * nthreads;
            // (a Z >= p fails the call in pass 2; it stays out of the chain so that it cannot zero the lane's product)
            const uint32_t cls = (mp_is_zero<N>(cz) || mp_geq<N>(cz, C::P)) ? XYZ_IDENT : mp_is_one<N>(cz) ? XYZ_Z_ONE : XYZ_FINITE;
            uint32_t w[NS];
#pragma unroll
            for (int i = 0; i < NS; i++) w[i] = i < C::NL ? acc.e.v[i] : 0u;
            w[NS - 1] = cls;
            io.put_prefix(j, w);
            if (cls == XYZ_FINITE) acc = F::mul(acc, F::from_canonical(cz));
        }
#pragma unroll
        for (int i = 0; i < N; i++) cz[i] = cz_next[i];
    }
    typename F::M1 inv = F::inv(acc);
    // pass 2, backward: zinv_j = prefix_j * inv, then inv *= Z_j
    const Fe<C::NL> b = G::curve_b();
    uint32_t cx[N], cy[N], pw[NS], cx_n[N], cy_n[N], cz_n[N], pw_n[NS];
    for (size_t it = 0; it <= K; it++) {
        if (it < K) {
            const size_t j = t + (K - 1 - it) * nthreads;
            io.load_xyz(j, cx_n, cy_n, cz_n);
            io.get_prefix(j, pw_n);
        }
        if (it > 0) {
            const size_t j = t + (K - it) * nthreads;
            bool ok = !mp_geq<N>(cx, C::P) && !mp_geq<N>(cy, C::P) && !mp_geq<N>(cz, C::P);
            uint32_t wx[N], wy[N];
            const uint32_t cls = pw[NS - 1];
            if (cls == XYZ_IDENT) {
#pragma unroll
                for (int i = 0; i < N; i++) wx[i] = wy[i] = 0u;
            } else {
                typename F::M1 x = F::from_canonical(cx), y = F::from_canonical(cy);
                if (cls == XYZ_FINITE) {
                    Fe<C::NL> pre;
#pragma unroll
                    for (int i = 0; i < C::NL; i++) pre.v[i] = pw[i];
                    const typename F::M1 zinv = F::mul(G::m(pre), inv);
                    inv = F::mul(inv, F::from_canonical(cz));
                    x = F::mul(x, zinv);
                    y = F::mul(y, zinv);
                }
                Affine<C> a;
                a.x = x.e;
                a.y = y.e;
                ok = ok && G::on_curve(a, b);
                F::to_canonical(wx, x);
                F::to_canonical(wy, y);
            }
            io.put_affine(j, wx, wy, cls == XYZ_IDENT);
            io.verdict(j, ok);
        }
#pragma unroll
        for (int i = 0; i < N; i++) { cx[i] = cx_n[i]; cy[i] = cy_n[i]; cz[i] = cz_n[i]; }
#pragma unroll
        for (int i = 0; i < NS; i++) pw[i] = pw_n[i];
    }
}

}  // namespace ecgpu
