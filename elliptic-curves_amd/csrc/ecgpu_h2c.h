// ecgpu_h2c.h — batch hash-to-curve (RFC 9380) for the three tuned parameter sets: expand_message_xmd, hash_to_field, the
// simplified SWU map and (secp256k1) the 3-isogeny, as host + device lane bodies with the HIP kernels at the end.
//
// Reference counterparts.  `hash2curve::GroupDigest::{hash_from_bytes, encode_from_bytes}` and `hash2curve::hash_to_scalar`
// (hash2curve/src/group_digest.rs, hash2field.rs), `ExpandMsgXmd` (hash2curve/src/hash2field/expand_msg/xmd.rs), `OsswuMap::osswu`
// and `sqrt_ratio_3mod4` (primeorder/src/osswu.rs), the k256 specialisation with its isogeny (k256/src/arithmetic/hash2curve.rs),
// `MapToCurve::map_to_curve` and `Reduce<Array<u8, L>>` of p256 / p384 (…/src/arithmetic/hash2curve.rs).  Suites (RFC 9380):
//     secp256k1_XMD:SHA-256_SSWU_RO_ / _NU_   section 8.7   SHA-256, L = 48, Z = -11, SSWU on E' (A', B' = 1771) + Appendix E.1
//     P256_XMD:SHA-256_SSWU_RO_ / _NU_        section 8.2   SHA-256, L = 48, Z = -10, SSWU on the curve itself
//     P384_XMD:SHA-384_SSWU_RO_ / _NU_        section 8.3   SHA-384, L = 72, Z = -12, SSWU on the curve itself
// All three primes are 3 mod 4 (sqrt_ratio_3mod4, section F.2.1.2: c1 = (p - 3) / 4, c2 = sqrt(-Z)) and all three cofactors are 1
// (clear_cofactor is the identity map).  Every other parameter set has no suite here: H2cSuite<C>::SUPPORTED is false and its
// translation unit holds no kernel body.
//
// Where this departs from the reference's arithmetic, not from its results: the map keeps x as the fraction xn / xd and never
// inverts — the reference inverts tv4 (`x * tv4.invert().unwrap()`) and, for secp256k1, both isogeny denominators per element.
// Here the point leaves as (X : Y : Z) = (xn : y xd : xd), the four isogeny polynomials are evaluated homogenised in (xn, xd), two
// points of one element are added with the complete addition, and the ONE inversion per lane of k_normalize (Montgomery's trick)
// brings the batch to affine.  y comes from one fixed addition chain for (p - 3) / 4 per prime (`pow_vartime(c1)` in the reference:
// the same exponent, a fixed schedule either way).
// The isogeny's denominators: x_den has the double root x0 = -k_(2,1) / 2, which is also a root of y_den.  No point of E' has that
// x (g'(x0) is a non-square), so the map never gets there, but a caller of h2c_iso_k256 can forge it: the lane then returns the
// identity (Z = 0 selects (0 : 1 : 0)) where the reference panics in `invert().unwrap()`.
//
// Secrecy.  Hashed inputs may be secret (an OPRF input is a password), so the rule of the `_ct` entry points holds in
// k_h2c_expand and k_h2c_map: no branch and no address depends on message bytes, on a digest, on u or on a point
// (tools/ct_isa_check.py --unit h2c).  msg_len, the DST, count / per_point and n are public and uniform: the block count of the
// hash and the loops over elements follow them.  A u >= p is computed on like any other and its verdict goes to a flag byte.
#pragma once

#include <type_traits>

#include "ecgpu_ctmul.h"
#include "ecgpu_h2c_consts.h"
#include "ecgpu_hash.h"
#include "ecgpu_point.h"
#include "ecgpu_scalar.h"
#include "ecgpu_sign.h"

namespace ecgpu {

// the suite of a parameter set: digest, L = ceil((ceil(log2 p) + k) / 8) bytes per drawn element, the map constants
template <class C>
struct H2cSuite {
    ECGPU_CONST bool SUPPORTED = false;
    ECGPU_CONST int D = HASH_SHA256, L = 48;
    using K = consts::H2C_K256;
};
template <>
struct H2cSuite<K256Params> {
    ECGPU_CONST bool SUPPORTED = true;
    ECGPU_CONST int D = HASH_SHA256, L = 48;
    using K = consts::H2C_K256;
};
template <>
struct H2cSuite<P256Params> {
    ECGPU_CONST bool SUPPORTED = true;
    ECGPU_CONST int D = HASH_SHA256, L = 48;
    using K = consts::H2C_P256;
};
template <>
struct H2cSuite<P384Params> {
    ECGPU_CONST bool SUPPORTED = true;
    ECGPU_CONST int D = HASH_SHA384, L = 72;
    using K = consts::H2C_P384;
};

struct H2cConst {
    ECGPU_CONST uint8_t ZPAD[128] = {};     // Z_pad: one block of zeros (64 bytes for SHA-256, 128 for SHA-384)
};

// ---- expand_message_xmd (section 5.3.1) ------------------------------------------------------------------------------------
// out = the first count * L bytes of b_1 || ... || b_ell, ell = ceil(count L / D) (3 for count = 2, 2 for count = 1, with both
// digests).  dstp = DST' = DST || I2OSP(len(DST), 1), made on the host once per call.
//     b_0 = H(Z_pad || msg || I2OSP(count L, 2) || I2OSP(0, 1) || DST')
//     b_1 = H(b_0 || I2OSP(1, 1) || DST'),   b_i = H((b_0 ^ b_(i-1)) || I2OSP(i, 1) || DST')
// ONE loop over the ell + 1 hashes and ONE call of hash_pieces in it: the compression function keeps one call site per
// instantiation (ecgpu_hash.h:26-27).  Which pieces a pass has depends on the pass number alone.
template <class C>
ECGPU_HD void h2c_expand(uint8_t* out, const uint8_t* msg, size_t msg_len, const uint8_t* dstp, size_t dstp_len, int count) {
    using S = H2cSuite<C>;
    using H = SignHash<S::D>;
    using W = typename H::W;
    constexpr int D = S::D, L = S::L, WB = H::WB;
    const int len_in_bytes = count * L;
    const int ell = (len_in_bytes + D - 1) / D;
    uint8_t b0[D], x[D + 1], tail[3];
    tail[0] = (uint8_t)(len_in_bytes >> 8);
    tail[1] = (uint8_t)len_in_bytes;
    tail[2] = 0;
#pragma unroll
    for (int j = 0; j <= D; j++) x[j] = 0;
#pragma unroll 1
    for (int t = 0; t <= ell; t++) {
        HashPiece pc[4];
        if (t == 0) {
            pc[0] = HashPiece{H2cConst::ZPAD, (size_t)H::BB};
            pc[1] = HashPiece{msg, msg_len};
            pc[2] = HashPiece{tail, 3};
        } else {
            x[D] = (uint8_t)t;
            pc[0] = HashPiece{x, (size_t)(D + 1)};
            pc[1] = HashPiece{msg, 0};
            pc[2] = HashPiece{tail, 0};
        }
        pc[3] = HashPiece{dstp, dstp_len};
        W h[8];
        H::init(h);
        hash_pieces<typename H::Core, 4>(h, pc);
#pragma unroll
        for (int j = 0; j < D; j++) {
            const uint8_t byte = (uint8_t)(h[j / WB] >> (8 * (WB - 1 - j % WB)));
            if (t == 0) b0[j] = byte;                              // (the pass number: not data)
            else if ((t - 1) * D + j < len_in_bytes) out[(t - 1) * D + j] = byte;
            x[j] = t == 0 ? byte : (uint8_t)(b0[j] ^ byte);        // what the next pass hashes first
        }
    }
}

// 24 big-endian bytes -> N little-endian words (a value below 2^192, so below p and below n on all three sets)
template <int N>
ECGPU_HD void h2c_piece_words(uint32_t* w, const uint8_t* be) {
#pragma unroll
    for (int k = 0; k < N; k++) {
        w[k] = 0;
        if (k < 6) w[k] = ((uint32_t)be[20 - 4 * k] << 24) | ((uint32_t)be[21 - 4 * k] << 16) | ((uint32_t)be[22 - 4 * k] << 8) | be[23 - 4 * k];
    }
}

// hash_to_field's reduction: OS2IP(L bytes) mod p as canonical words.  `Reduce<Array<u8, U48>> for FieldElement` (k256, p256:
// d0 * 2^192 + d1) and its 72-byte counterpart of p384, as Horner steps over 24-byte pieces.
template <class C>
ECGPU_HD void h2c_reduce_field(uint32_t* out, const uint8_t* be) {
    using F = Field<C>;
    using S = H2cSuite<C>;
    constexpr int N = C::N, PIECES = S::L / 24;
    static_assert(S::L % 24 == 0, "L is a whole number of 24-byte pieces");
    typename F::E f192e;
#pragma unroll
    for (int i = 0; i < C::NL; i++) f192e.v[i] = S::K::F192[i];
    const typename F::M1 f192 = F::template wrap<1, 1>(f192e);
    uint32_t w[N];
    h2c_piece_words<N>(w, be);
    typename F::M1 acc = F::from_canonical(w);
#pragma unroll
    for (int j = 1; j < PIECES; j++) {
        h2c_piece_words<N>(w, be + 24 * j);
        const typename F::M1 one = F::one();
        acc = F::mul2(acc, f192, F::from_canonical(w), one);
    }
    F::to_canonical(out, acc);
}

// hash_to_scalar's reduction: OS2IP(L bytes) mod n (`Reduce<Array<u8, L>> for Scalar`); zero is a legal result
template <class C>
ECGPU_HD void h2c_reduce_scalar(uint32_t* out, const uint8_t* be) {
    using SN = ScalarN<C>;
    using S = H2cSuite<C>;
    constexpr int N = C::N, PIECES = S::L / 24;
    uint32_t f192[N], acc[N], w[N], t[N];
#pragma unroll
    for (int i = 0; i < N; i++) f192[i] = i == 6 ? 1u : 0u;
    h2c_piece_words<N>(acc, be);
#pragma unroll
    for (int j = 1; j < PIECES; j++) {
        h2c_piece_words<N>(w, be + 24 * j);
        SN::mul(t, acc, f192);
        SignScalar<C>::add(acc, t, w);
    }
#pragma unroll
    for (int i = 0; i < N; i++) out[i] = acc[i];
}

// ---- the map ------------------------------------------------------------------------------------------------------------------
template <class C>
struct H2cMap {
    using F = Field<C>;
    using G = Group<C>;
    using S = H2cSuite<C>;
    using K = typename S::K;
    using M1 = typename F::M1;
    using E = Fe<C::NL>;

    static ECGPU_HD M1 konst(const uint32_t* limbs) {
        E e;
#pragma unroll
        for (int i = 0; i < C::NL; i++) e.v[i] = limbs[i];
        return F::template wrap<1, 1>(e);
    }
    // flag ? a : b under an opaque mask; both of magnitude (L, V) at most
    template <int L, int V>
    static ECGPU_HD Mag<C, L, V> pick(bool flag, const E& a, const E& b) {
        return F::template wrap<L, V>(ct_sel_fe<C>(ct_mask(flag), a, b));
    }

    // a^((p - 3) / 4) by one fixed addition chain per prime (x_k = a^(2^k - 1): k ones)
    static ECGPU_HD M1 pow_c1(const M1& a) {
        const M1 x2 = F::mul(F::sqr(a), a);
        const M1 x3 = F::mul(F::sqr(x2), a);
        if constexpr (C::ID == CURVE_K256) {
            // (p - 3) / 4 = 2^254 - 2^30 - 245: 223 ones, 0, 22 ones, 0000, 1011
            const M1 x6 = F::mul(F::sqr_n(x3, 3), x3);
            const M1 x9 = F::mul(F::sqr_n(x6, 3), x3);
            const M1 x11 = F::mul(F::sqr_n(x9, 2), x2);
            const M1 x22 = F::mul(F::sqr_n(x11, 11), x11);
            const M1 x44 = F::mul(F::sqr_n(x22, 22), x22);
            const M1 x88 = F::mul(F::sqr_n(x44, 44), x44);
            const M1 x176 = F::mul(F::sqr_n(x88, 88), x88);
            const M1 x220 = F::mul(F::sqr_n(x176, 44), x44);
            const M1 x223 = F::mul(F::sqr_n(x220, 3), x3);
            M1 r = F::mul(F::sqr_n(x223, 23), x22);
            r = F::mul(F::sqr_n(r, 5), a);
            return F::mul(F::sqr_n(r, 3), x2);
        } else if constexpr (C::ID == CURVE_P256) {
            // (p - 3) / 4 = 2^254 - 2^222 + 2^190 + 2^94 - 1: 32 ones, 31 zeros, 1, 96 zeros, 94 ones
            const M1 x6 = F::mul(F::sqr_n(x3, 3), x3);
            const M1 x12 = F::mul(F::sqr_n(x6, 6), x6);
            const M1 x15 = F::mul(F::sqr_n(x12, 3), x3);
            const M1 x30 = F::mul(F::sqr_n(x15, 15), x15);
            const M1 x32 = F::mul(F::sqr_n(x30, 2), x2);
            const M1 x64 = F::mul(F::sqr_n(x32, 32), x32);
            const M1 x94 = F::mul(F::sqr_n(x64, 30), x30);
            M1 r = F::mul(F::sqr_n(x32, 32), a);
            return F::mul(F::sqr_n(r, 96 + 94), x94);
        } else {
            static_assert(C::ID == CURVE_P384, "an addition chain per supported prime");
            // (p - 3) / 4 = 2^382 - 2^126 - 2^94 + 2^30 - 1: 255 ones, 0, 32 ones, 64 zeros, 30 ones
            const M1 x6 = F::mul(F::sqr_n(x3, 3), x3);
            const M1 x12 = F::mul(F::sqr_n(x6, 6), x6);
            const M1 x15 = F::mul(F::sqr_n(x12, 3), x3);
            const M1 x30 = F::mul(F::sqr_n(x15, 15), x15);
            const M1 x32 = F::mul(F::sqr_n(x30, 2), x2);
            const M1 x60 = F::mul(F::sqr_n(x30, 30), x30);
            const M1 x120 = F::mul(F::sqr_n(x60, 60), x60);
            const M1 x240 = F::mul(F::sqr_n(x120, 120), x120);
            const M1 x255 = F::mul(F::sqr_n(x240, 15), x15);
            M1 r = F::mul(F::sqr_n(x255, 33), x32);
            return F::mul(F::sqr_n(r, 64 + 30), x30);
        }
    }

    // map_to_curve_simple_swu in its straight-line form (section F.2, `OsswuMap::osswu`) without step 25: the point of the curve
    // the map runs on as xn / xd and y.  cu: the canonical words of u (its parity is sgn0(u)).  xd is never zero: it is A Z or
    // -A (Z^2 u^4 + Z u^2) with the second factor non-zero.
    static ECGPU_HD void sswu(E* xn_out, E* xd_out, E* y_out, const uint32_t* cu) {
        const M1 Zc = konst(K::Z), A = konst(K::A), B = konst(K::B), C2 = konst(K::C2), one = F::one();
        const M1 u = F::from_canonical(cu);
        const M1 tv1 = F::mul(Zc, F::sqr(u));                                 // 1, 2
        const auto tv2 = F::add(F::sqr(tv1), tv1);                            // 3, 4
        const M1 tv3 = F::mul(B, F::add(tv2, one));                           // 5, 6
        const bool tv2_zero = F::is_zero(tv2);
        const auto ntv2 = F::neg(tv2);
        using NT = typename std::remove_const<decltype(ntv2)>::type;
        NT tv4s;
        tv4s.e = ct_sel_fe<C>(ct_mask(tv2_zero), Zc.e, ntv2.e);               // 7: Z where tv2 = 0, else -tv2
        const M1 tv4 = F::mul(A, tv4s);                                       // 8: xd
        const M1 tv6a = F::sqr(tv4);                                          // 10
        const auto t9 = F::add(F::sqr(tv3), F::mul(A, tv6a));                 // 9, 11, 12
        const M1 tv6 = F::mul(tv6a, tv4);                                     // 14: gxd = xd^3
        const M1 gxn = F::mul2(t9, tv3, B, tv6);                              // 13, 15, 16: gx1 = gxn / gxd
        const M1 x2n = F::mul(tv1, tv3);                                      // 17
        // 18: sqrt_ratio_3mod4(gxn, gxd)
        const M1 s2 = F::mul(gxn, tv6);
        const M1 s1 = F::mul(F::sqr(tv6), s2);
        const M1 y1 = F::mul(pow_c1(s1), s2);
        const M1 y2 = F::mul(y1, C2);
        const bool is_qr = F::eq(F::mul(F::sqr(y1), tv6), gxn);
        const M1 yr = pick<1, 1>(is_qr, y1.e, y2.e);
        const M1 yx2 = F::mul(F::mul(tv1, u), yr);                            // 19, 20
        const M1 xn = pick<1, 1>(is_qr, tv3.e, x2n.e);                        // 21
        const M1 y = pick<1, 1>(is_qr, yr.e, yx2.e);                          // 22
        uint32_t cy[C::N];
        F::to_canonical(cy, y);
        const bool e1 = ((cu[0] ^ cy[0]) & 1u) == 0u;                         // 23: sgn0(u) == sgn0(y)
        const auto ny = F::neg(y);
        using NY = typename std::remove_const<decltype(ny)>::type;
        NY ys;
        ys.e = ct_sel_fe<C>(ct_mask(e1), y.e, ny.e);                          // 24
        *xn_out = xn.e;
        *xd_out = tv4.e;
        *y_out = F::mul(ys, one).e;                                           // magnitude (1, 1) again
    }

    // The 3-isogeny E' -> secp256k1 (Appendix E.1, `isogeny` of k256/src/arithmetic/hash2curve.rs) on x' = xn / xd, y' = y with
    // the four polynomials homogenised in (xn, xd):
    //     x = XN / (XD xd),  y = y' YN / YD   ->   (X : Y : Z) = (XN YD : y' YN XD xd : XD xd YD).
    // Z = 0 (a forged x', see the head of this file) gives the identity.
    static ECGPU_HD Proj<C> iso_k256(const E& xn_e, const E& xd_e, const E& y_e) {
        static_assert(C::ID == CURVE_K256, "the isogeny belongs to secp256k1");
        const M1 xn = G::m(xn_e), xd = G::m(xd_e), y = G::m(y_e);
        const M1 xn2 = F::sqr(xn), xd2 = F::sqr(xd), xnxd = F::mul(xn, xd);
        const M1 xn3 = F::mul(xn2, xn), xd3 = F::mul(xd2, xd), xn2xd = F::mul(xn2, xd), xnxd2 = F::mul(xn, xd2);
        const M1 XN = F::norm(F::add(F::mul2(konst(K::XNUM[3]), xn3, konst(K::XNUM[2]), xn2xd),
                                     F::mul2(konst(K::XNUM[1]), xnxd2, konst(K::XNUM[0]), xd3)));
        const M1 XD = F::norm(F::add(xn2, F::mul2(konst(K::XDEN[1]), xnxd, konst(K::XDEN[0]), xd2)));       // k_(2,2) = 1
        const M1 YN = F::norm(F::add(F::mul2(konst(K::YNUM[3]), xn3, konst(K::YNUM[2]), xn2xd),
                                     F::mul2(konst(K::YNUM[1]), xnxd2, konst(K::YNUM[0]), xd3)));
        const M1 YD = F::norm(F::add(F::mul2(xn3, F::one(), konst(K::YDEN[2]), xn2xd),                       // k_(4,3) = 1
                                     F::mul2(konst(K::YDEN[1]), xnxd2, konst(K::YDEN[0]), xd3)));
        const M1 t = F::mul(XD, xd);
        Proj<C> q;
        q.x = F::mul(XN, YD).e;
        q.y = F::mul(F::mul(y, YN), t).e;
        q.z = F::mul(t, YD).e;
        return ct_sel_proj<C>(F::is_zero(G::m(q.z)), G::identity(), q);
    }

    // `MapToCurve::map_to_curve(u)` as a projective point; never the identity for a canonical u
    static ECGPU_HD Proj<C> map(const uint32_t* cu) {
        E xn, xd, y;
        sswu(&xn, &xd, &y, cu);
        if constexpr (C::ID == CURVE_K256) {
            return iso_k256(xn, xd, y);
        } else {
            Proj<C> q;
            q.x = xn;
            q.y = F::mul(G::m(y), G::m(xd)).e;
            q.z = xd;
            return q;
        }
    }
};

}  // namespace ecgpu

// =============================================================================================================================
#if defined(__HIPCC__)

#include "ecgpu_kernels.h"
#include "ecgpu_launch.h"

namespace ecgpu {

// count elements per message: u_0 [, u_1] mod p (to_scalar == 0) or the scalar mod n (to_scalar != 0), as wire records at
// out[(i * count + j) * WB]
template <class C>
__global__ void __launch_bounds__(BLOCK)
k_h2c_expand(const uint8_t* __restrict__ msgs, size_t msg_len, size_t n, const uint8_t* __restrict__ dstp, size_t dstp_len, int count,
             int to_scalar, uint8_t* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if constexpr (H2cSuite<C>::SUPPORTED) {
        constexpr int N = C::N, WB = WireBytes<C>::value, L = H2cSuite<C>::L;
        uint8_t ub[2 * L];
        h2c_expand<C>(ub, msgs + i * msg_len, msg_len, dstp, dstp_len, count);
#pragma unroll 1
        for (int j = 0; j < count; j++) {
            uint32_t w[N];
            if (to_scalar) h2c_reduce_scalar<C>(w, ub + j * L);           // (an argument of the call, not data)
            else h2c_reduce_field<C>(w, ub + j * L);
            store_wire<C>(out + (i * (size_t)count + j) * WB, w);
        }
    }
}

// proj_out[i] = map(u[i * per_point]) [+ map(u[i * per_point + 1])]; flags[i] = ST_BAD_POINT when a u is not below p.  One call
// site of the map and one of the complete addition: the sum starts from the identity.
template <class C>
__global__ void __launch_bounds__(BLOCK)
k_h2c_map(const uint8_t* __restrict__ u, int per_point, size_t n, uint32_t* __restrict__ proj_out, uint8_t* __restrict__ flags) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if constexpr (H2cSuite<C>::SUPPORTED) {
        using G = Group<C>;
        constexpr int N = C::N, WB = WireBytes<C>::value;
        const Fe<C::NL> b = G::curve_b();
        Proj<C> acc = G::identity();
        uint32_t bad = 0;
#pragma unroll 1
        for (int j = 0; j < per_point; j++) {
            uint32_t cu[N];
            load_wire<C>(cu, u + (i * (size_t)per_point + j) * WB);
            bad |= mp_geq<N>(cu, C::P) ? (uint32_t)ST_BAD_POINT : 0u;
            acc = G::add(acc, H2cMap<C>::map(cu), b);
        }
        flags[i] = (uint8_t)bad;
        store_proj<C>(proj_out, i, acc);
    }
}

// status |= OR of the n flag bytes (the k_ct_flags of ecgpu_ct.h: a kernel of its own, so that the map has no path that depends
// on a verdict)
static __global__ void __launch_bounds__(BLOCK) k_h2c_flags(const uint8_t* __restrict__ flags, size_t n, int* status) {
    uint32_t f = 0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) f |= flags[i];
    if (f) atomicOr(status, (int)f);
}

// ---- ecgpu_selftest_h2c: one lane body of this file on records the caller supplies (test infrastructure: tests/h2c_vectors.py) ----
// A kernel of its own: k_h2c_expand and k_h2c_map stay as they are, and this one calls the same functions on what no digest and no
// map produces.  op (H2C_ST_*, ecgpu_launch.h; an argument of the call, uniform):
//     0  h2c_reduce_field    L bytes (OKM, big-endian)        ->  the residue mod p as a wire record
//     1  h2c_reduce_scalar   L bytes                          ->  the residue mod n as a wire record
//     2  H2cMap::sswu        u, a wire record below p         ->  xn || xd || y, canonical wire records
//     3  H2cMap::iso_k256    xn || xd || y, wire records      ->  X || Y || Z, canonical wire records (secp256k1 only)
// Nothing is range-checked: the entry point says what each op accepts.
template <class C>
__global__ void __launch_bounds__(BLOCK)
k_selftest_h2c(int op, const uint8_t* __restrict__ in, size_t n, uint8_t* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if constexpr (H2cSuite<C>::SUPPORTED) {
        using F = Field<C>;
        using G = Group<C>;
        using M = H2cMap<C>;
        constexpr int N = C::N, WB = WireBytes<C>::value, L = H2cSuite<C>::L;
        uint32_t w[N];
        if (op == H2C_ST_REDUCE_P || op == H2C_ST_REDUCE_N) {
            // the record goes to a private array first, as k_h2c_expand holds its OKM: handed the global pointer, the compiler
            // merged h2c_piece_words' byte loads into wide ones and its byte extraction left bits of a neighbouring byte in a
            // word (k256 mod p on gfx950: bits 24, 25 of word 1 came out as byte 40 | byte 42), the defect ecgpu_kernels.h
            // describes at load_wire
            uint8_t ub[L];
#pragma unroll
            for (int k = 0; k < L; k++) ub[k] = in[i * L + k];
            if (op == H2C_ST_REDUCE_N) h2c_reduce_scalar<C>(w, ub);
            else h2c_reduce_field<C>(w, ub);
            store_wire<C>(out + i * WB, w);
        } else if (op == H2C_ST_SSWU) {
            typename M::E e[3];
            load_wire<C>(w, in + i * WB);
            M::sswu(&e[0], &e[1], &e[2], w);
#pragma unroll
            for (int j = 0; j < 3; j++) {
                F::to_canonical(w, G::m(e[j]));
                store_wire<C>(out + (3 * i + j) * WB, w);
            }
        } else if (op == H2C_ST_ISO) {
            if constexpr (C::ID == CURVE_K256) {
                typename M::E e[3];
#pragma unroll
                for (int j = 0; j < 3; j++) {
                    load_wire<C>(w, in + (3 * i + j) * WB);
                    e[j] = F::from_canonical(w).e;
                }
                const Proj<C> q = M::iso_k256(e[0], e[1], e[2]);
                F::to_canonical(w, G::m(q.x)); store_wire<C>(out + (3 * i) * WB, w);
                F::to_canonical(w, G::m(q.y)); store_wire<C>(out + (3 * i + 1) * WB, w);
                F::to_canonical(w, G::m(q.z)); store_wire<C>(out + (3 * i + 2) * WB, w);
            }
        }
    }
}

}  // namespace ecgpu

#endif  // __HIPCC__
