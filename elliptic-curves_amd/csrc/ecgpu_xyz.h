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

#include "ecgpu_batchinv.h"

namespace ecgpu {

// the class of a record, kept by the product pass in the spare word of the record's prefix entry (0: in the lane's product)
enum : uint32_t { XYZ_FINITE = 0, XYZ_IDENT = 1, XYZ_Z_ONE = 2 };

template <int N>
ECGPU_HD bool mp_is_one(const uint32_t* a) {
    uint32_t r = a[0] ^ 1u;
#pragma unroll
    for (int i = 1; i < N; i++) r |= a[i];
    return r == 0;
}

// The chain of a lane — the product pass, the one inversion, the way back and their prefetch — is batch_inv_lane
// (ecgpu_batchinv.h) over FieldLane<XyzRec>; these are its records.  Io:
//   load_z(j, cz)              Z of record j as N canonical words
//   load_xyz(j, cx, cy, cz)    the whole record
//   put_prefix(j, w) / get_prefix(j, w)   NS words: the running product before record j, its class in word NS - 1
//   put_affine(j, x, y, ident) the output record (x = y = 0 for the identity)
//   verdict(j, ok)             false: a bad record
template <class C, class Io>
struct XyzRec {
    using F = Field<C>;
    using G = Group<C>;
    using El = typename F::M1;
    static constexpr int N = C::N, NL = C::NL, NS = F::NS;
    struct Fwd { uint32_t cz[N]; };
    struct Back { uint32_t cx[N], cy[N], cz[N], pw[NS]; };
    Io& io;
    ECGPU_HD void load_fwd(size_t j, Fwd& r) const { io.load_z(j, r.cz); }
    ECGPU_HD void load_back(size_t j, Back& r) const { io.load_xyz(j, r.cx, r.cy, r.cz); io.get_prefix(j, r.pw); }
    // (a Z >= p fails the call on the way back; it stays out of the chain so that it cannot zero the lane's product)
    ECGPU_HD uint32_t classify(size_t, const Fwd& r, El& f) const {
        if (mp_is_zero<N>(r.cz) || mp_geq<N>(r.cz, C::P)) return XYZ_IDENT;
        if (mp_is_one<N>(r.cz)) return XYZ_Z_ONE;
        f = F::from_canonical(r.cz);
        return XYZ_FINITE;
    }
    ECGPU_HD uint32_t classify(size_t, const Back& r, El& f) const {
        if (r.pw[NS - 1] == XYZ_FINITE) f = F::from_canonical(r.cz);
        return r.pw[NS - 1];
    }
    ECGPU_HD void emit(size_t j, const Back& r, uint32_t c, const El& zinv) const {
        bool ok = !mp_geq<N>(r.cx, C::P) && !mp_geq<N>(r.cy, C::P) && !mp_geq<N>(r.cz, C::P);
        uint32_t wx[N], wy[N];
        if (c == XYZ_IDENT) {
#pragma unroll
            for (int i = 0; i < N; i++) wx[i] = wy[i] = 0u;
        } else {
            El x = F::from_canonical(r.cx), y = F::from_canonical(r.cy);
            if (c == XYZ_FINITE) {
                x = F::mul(x, zinv);
                y = F::mul(y, zinv);
            }
            Affine<C> a;
            a.x = x.e;
            a.y = y.e;
            ok = ok && G::on_curve(a, G::curve_b());
            F::to_canonical(wx, x);
            F::to_canonical(wy, y);
        }
        io.put_affine(j, wx, wy, c == XYZ_IDENT);
        io.verdict(j, ok);
    }
};
template <class C, class Io>
ECGPU_HD void xyz_affine_lane(size_t t, size_t n, size_t nthreads, Io& io) {
    FieldLane<XyzRec<C, Io>> lane{{io}};
    batch_inv_lane(t, n, nthreads, lane);
}

}  // namespace ecgpu
