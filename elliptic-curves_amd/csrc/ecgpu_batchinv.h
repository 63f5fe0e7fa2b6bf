// ecgpu_batchinv.h — Montgomery's trick over the records of a lane: the lane body behind k_xyz_affine (ecgpu_kernels.h; its
// records in ecgpu_xyz.h) and k_scalar_batch_inv (ecgpu_ecdsa.h), and what k_normalize (ecgpu_kernels.h) does with a record,
// compiled for the kernels and for their CPU twins (tests/hostcheck).  k_normalize walks its lane's records itself, with the next
// record held in plain variables: under batch_inv_lane nine of its instantiations lost a wave per SIMD
// (profiles/batch_inv/isa_identity_all_three.txt); its CPU twin runs NormRec under batch_inv_lane.
//
// `BatchNormalize::batch_normalize` (k256 projective.rs:367-391 + field.rs:244-265; primeorder projective.rs:452-478) and, modulo
// the group order, `Scalar::invert` (k256/src/arithmetic/scalar.rs:139-143; primefield/src/monty.rs:373-375) for a whole batch.
// Lane t of nthreads owns records t, t + nthreads, t + 2 nthreads, ... so that a wave always touches consecutive records: a
// running product over that chain, ONE inversion, and a walk back that peels the inverses off.
#pragma once

#include "ecgpu_point.h"
#include "ecgpu_scalar.h"

namespace ecgpu {

// The records first, first + step, ... (step = -nthreads modulo 2^64 on the way back) as long as has_next(j) says there is one
// after record j — a bound the whole wave shares (j + nthreads < n; j >= nthreads), so that no lane keeps a count of its own.
// ONE load site: the loads of record i + 1 are issued before record i is worked on — with one wave per SIMD (the launches are
// sized that way: one inversion per lane) nothing else hides a load's ~2 us, and the loop-carried product keeps the compiler from
// hoisting the loads itself.  One site also keeps a p521 kernel to one halfword load per record it reads
// (tools/wire_codec_isa_check.py).
template <class R, class Load, class More, class Work>
ECGPU_HD void chain_walk(size_t first, size_t step, Load load, More has_next, Work work) {
    R cur, next;
    bool more = true;                                         // there is a record j to load
    for (size_t j = first, it = 0;; j += step, it++) {
        if (more) load(j, next);
        if (it) work(j - step, cur);
        if (!more) break;
        cur = next;
        more = has_next(j);
    }
}

// The policy P supplies the algebra and everything a record is:
//   El, one(), mul(a, b), inv(a)               the product's domain
//   Fwd, load_fwd(j, Fwd&)                     what the product pass reads of record j, one record ahead
//   Back, load_back(j, Back&)                  what the way back reads, one record ahead: the record and its prefix entry
//                                              (a policy with empty Fwd / Back opts out of the prefetch and reads in classify)
//   classify(j, Fwd / Back, El& factor)        the record's class: 0 = in the product, with its factor; any other value stays out
//                                              of the product on BOTH passes (a degenerate record: Z = 0, a scalar outside
//                                              [1, n - 1]) and means what the policy likes
//   put_prefix(j, acc, cls), prefix(j, Back)   the product of the lane's earlier factors, parked per record
//   emit(j, Back, cls, inverse)                the output record; `inverse` = 1 / factor for class 0, unspecified otherwise
template <class P>
ECGPU_HD void batch_inv_lane(size_t t, size_t n, size_t nthreads, P& p) {
    using El = typename P::El;
    using Fwd = typename P::Fwd;
    using Back = typename P::Back;
    if (t >= n) return;
    El acc = p.one();
    chain_walk<Fwd>(t, nthreads, [&](size_t j, Fwd& r) { p.load_fwd(j, r); }, [&](size_t j) { return j + nthreads < n; },
                    [&](size_t j, const Fwd& r) {
                        El f;
                        const uint32_t cls = p.classify(j, r, f);
                        p.put_prefix(j, acc, cls);
                        if (cls == 0) acc = p.mul(acc, f);
                    });
    El inv = p.inv(acc);
    chain_walk<Back>(t + (n - 1 - t) / nthreads * nthreads, (size_t)0 - nthreads, [&](size_t j, Back& r) { p.load_back(j, r); },
                     [&](size_t j) { return j >= nthreads; },
                     [&](size_t j, const Back& r) {
                         El f, own;
                         const uint32_t cls = p.classify(j, r, f);
                         if (cls == 0) {
                             own = p.mul(p.prefix(j, r), inv);   // (a_0 .. a_j)^-1 (a_0 .. a_(j-1)) = a_j^-1
                             inv = p.mul(inv, f);                // (a_0 .. a_(j-1))^-1
                         }
                         p.emit(j, r, cls, own);
                     });
}

// ---- the base field under the records Rec of a kernel (NormRec below, XyzRec in ecgpu_xyz.h): the algebra, and a prefix entry of
// NS words — the running product in the first NL, the class in the spare last one (Back::pw holds the entry read back)
template <class Rec>
struct FieldLane : Rec {
    using F = typename Rec::F;
    using El = typename Rec::El;
    static constexpr int NL = Rec::NL, NS = Rec::NS;
    static_assert(NS > NL, "raw form has no spare word");
    ECGPU_HD El one() const { return F::one(); }
    ECGPU_HD El mul(const El& a, const El& b) const { return F::mul(a, b); }
    ECGPU_HD El inv(const El& a) const { return F::inv(a); }
    ECGPU_HD void put_prefix(size_t j, const El& acc, uint32_t cls) const {
        uint32_t w[NS];
#pragma unroll
        for (int i = 0; i < NS; i++) w[i] = i < NL ? acc.e.v[i] : 0u;
        w[NS - 1] = cls;
        this->io.put_prefix(j, w);
    }
    ECGPU_HD El prefix(size_t, const typename Rec::Back& r) const {
        Fe<NL> e;
#pragma unroll
        for (int i = 0; i < NL; i++) e.v[i] = r.pw[i];
        return F::template wrap<1, 1>(e);
    }
};

// ---- normalisation: internal (X:Y:Z) -> (X/Z, Y/Z) -------------------------------------------------------------------------
// MODE NORM_WIRE      : big-endian canonical x||y records + identity flags (wire format)
// MODE NORM_PACKED    : [n][2] packed elements (table entries; identities not expected, and nothing is written for one)
// MODE NORM_COMPRESSED: SEC1 compressed form split in two arrays: x (L bytes) and the tag byte 0x02 / 0x03 (y even / odd), 0x00
//                       for the identity — `ToSec1Point::to_sec1_point(true)`, primeorder/src/affine.rs:387-401
enum : int { NORM_WIRE = 0, NORM_PACKED = 1, NORM_COMPRESSED = 2 };
// Io (it knows MODE: where a coordinate of record j goes):
//   load_z(j) -> Fe, load_point(j) -> Proj     Z alone / the whole record, raw
//   put_prefix(j, w) / get_prefix(j, w)        NS words
//   put_x(j, w), put_y(j, w), put_flag(j, v)   a coordinate as N words (packed for NORM_PACKED, canonical otherwise); the identity
//                                              flag or the tag
template <class C, int MODE, class Io>
struct NormRec {
    using F = Field<C>;
    using G = Group<C>;
    using El = typename F::M1;
    static constexpr int N = C::N, NL = C::NL, NS = F::NS;
    struct Fwd { Fe<NL> z; };
    struct Back { Proj<C> p; uint32_t pw[NS]; };
    Io& io;
    ECGPU_HD void load_fwd(size_t j, Fwd& r) const { r.z = io.load_z(j); }
    ECGPU_HD void load_back(size_t j, Back& r) const { r.p = io.load_point(j); io.get_prefix(j, r.pw); }
    ECGPU_HD uint32_t classify(size_t, const Fwd& r, El& f) const {
        f = G::m(r.z);
        return F::is_zero_short(f) ? 1u : 0u;        // (k256: no canonical words for a zero test)
    }
    ECGPU_HD uint32_t classify(size_t, const Back& r, El& f) const {
        f = G::m(r.p.z);
        return r.pw[NS - 1];
    }
    ECGPU_HD void coord(uint32_t* w, const El& v) const {
        if constexpr (MODE == NORM_PACKED) F::pack(w, v);
        else F::to_canonical(w, v);
    }
    ECGPU_HD void emit(size_t j, const Back& r, uint32_t cls, const El& zinv) const {
        uint32_t w[N];
        if (cls) {
            if (MODE == NORM_PACKED) return;
#pragma unroll
            for (int i = 0; i < N; i++) w[i] = 0u;
            io.put_x(j, w);
            if (MODE == NORM_WIRE) io.put_y(j, w);
            io.put_flag(j, MODE == NORM_WIRE ? 1 : 0);
            return;
        }
        const El x = F::mul(G::m(r.p.x), zinv), y = F::mul(G::m(r.p.y), zinv);
        coord(w, x);
        io.put_x(j, w);
        coord(w, y);
        if (MODE != NORM_COMPRESSED) io.put_y(j, w);
        if (MODE != NORM_PACKED) io.put_flag(j, MODE == NORM_WIRE ? 0 : (uint8_t)(2u + (w[0] & 1u)));
    }
};
template <class C, int MODE, class Io>
ECGPU_HD void normalize_lane(size_t t, size_t n, size_t nthreads, Io& io) {
    FieldLane<NormRec<C, MODE, Io>> lane{{io}};
    batch_inv_lane(t, n, nthreads, lane);
}

// ---- inverses modulo the group order ---------------------------------------------------------------------------------------
// Running products in the Montgomery domain (one multiplication per product); the prefix entry is the N words of the product alone,
// and the way back tells the record's class from the reloaded record.  An element outside [1, n - 1] gets 0 — the prepare kernels
// fail it on their range check and never use its inverse.  This policy OPTS OUT of the skeleton's prefetch, as the kernel
// always did: Fwd and Back are empty and the words are read where they are used — a record held ahead costs the k256-sized kernels
// their 72 registers (7 waves per SIMD).
// Io: load(j, a), put(j, w): N words of a wire record; put_prefix(j, w) / get_prefix(j, w): N words.
template <class C, class Io>
struct ScalarInvLane {
    using S = ScalarN<C>;
    static constexpr int N = C::N;
    struct El { uint32_t v[N]; };
    struct Fwd {};
    struct Back {};
    Io& io;
    ECGPU_HD El one() const {
        El r = {{1u}};
        S::to_mont(r.v, r.v);                                     // R mod n
        return r;
    }
    ECGPU_HD El mul(const El& a, const El& b) const {
        El r;
        S::mont_mul(r.v, a.v, b.v);
        return r;
    }
    // acc = P R as an integer; x = acc^-1 = P^-1 R^-1; x R2 / R = P^-1; P^-1 R2 / R = P^-1 R: the Montgomery form of P^-1
    ECGPU_HD El inv(const El& acc) const {
        El x;
        S::inv(x.v, acc.v);
        S::to_mont(x.v, x.v);
        S::to_mont(x.v, x.v);
        return x;
    }
    ECGPU_HD void load_fwd(size_t, Fwd&) const {}
    ECGPU_HD void load_back(size_t, Back&) const {}
    template <class R>
    ECGPU_HD uint32_t classify(size_t j, const R&, El& f) const {
        uint32_t a[N];
        io.load(j, a);
        if (S::is_zero(a) || !S::in_range(a)) return 1u;
        S::to_mont(f.v, a);
        return 0u;
    }
    ECGPU_HD void put_prefix(size_t j, const El& acc, uint32_t) const { io.put_prefix(j, acc.v); }
    ECGPU_HD El prefix(size_t j, const Back&) const {
        El e;
        io.get_prefix(j, e.v);
        return e;
    }
    ECGPU_HD void emit(size_t j, const Back&, uint32_t cls, const El& ainv) const {
        El w = {};
        if (!cls) S::from_mont(w.v, ainv.v);
        io.put(j, w.v);
    }
};
template <class C, class Io>
ECGPU_HD void scalar_batch_inv_lane(size_t t, size_t n, size_t nthreads, Io& io) {
    ScalarInvLane<C, Io> lane{io};
    batch_inv_lane(t, n, nthreads, lane);
}

}  // namespace ecgpu
