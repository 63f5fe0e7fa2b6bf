// ecgpu_fe448.h — arithmetic modulo the Goldilocks prime p = 2^448 - 2^224 - 1 (Curve448, Ed448), host + device.
//
// Reference counterpart: `ed448_goldilocks::field::FieldElement` (ed448-goldilocks/src/field/element.rs): `from_bytes` accepts any
// 56 bytes and reduces (:370-372), `to_bytes` is canonical, `invert` maps 0 to 0 (:319-321).
//
// Representation: 16 limbs of 28 bits in 32-bit words, plain residues (no Montgomery form).  224 = 8 * 28, so with phi = 2^224 the
// identity phi^2 = phi + 1 (mod p) lands on limb boundaries: a = a0 + a1 phi (eight limbs each), and
//     a b = (a0 b0 + a1 b1) + (a0 b1 + a1 b0 + a1 b1) phi = L + H phi.
// L and H are 8 x 8 products with columns 0..14; column 8 + j of L belongs to phi's column j, column 8 + j of H to phi^2's column j,
// that is to the low column j AND the high column j.  So
//     low column j  = L[j] + H[8 + j],     high column j = H[j] + L[8 + j] + H[8 + j]          (j = 0..7; column 15 is empty).
// H is computed as a0 b1 + a1 (b0 + b1): 4 * 64 = 256 multiply-adds for a product.  A square shares a1^2 between L and H and uses
// the symmetry of a0^2 and a1^2: 36 + 36 + 64 = 136 multiply-adds.
//
// ---- bounds (DESIGN.md section 3 has the long form) ----
// T = 2^28 + 2^8 is the limb bound of a TIGHT element (magnitude 1).  Gf<M> promises limbs <= M * T.
//   * carry (one parallel pass, no chain): limb i keeps its low 28 bits and receives limb (i - 1) >> 28; the top limb's carry goes
//     to limbs 0 and 8.  Any 32-bit limbs in: carries <= 15, limb 8 receives two, so limbs <= 2^28 - 1 + 30 <= T out.
//   * add: Gf<A> + Gf<B> = Gf<A + B>, no carry.  sub: a + 2B p - b limb-wise (every limb of 2B p is >= 2B (2^28 - 2) >= B T), then
//     the carry pass: tight out.  A T + 2B 2^28 must stay below 2^32: A + 2B <= 15.
//   * mul, sqr: counting L's products once and H's as they are (a1 (b0 + b1) doubles the limbs of one factor), high column j holds
//     3 (j + 1) + 2 (7 - j) + 3 (7 - j) = 38 - 2 j products of limbs <= A T and <= B T, low column j holds 23 - j.  The widest
//     column is <= 38 A B T^2.  A B <= 4 is accepted: 152 T^2 < 2^63.25.  The columns are then carried in 64 bits from column 0
//     up (a carry is < 2^36: no overflow), the carry out of column 15 (< 2^36) is added to limbs 0 and 8 and those two are
//     carried once more into limbs 1 and 9 (< 2^8 + 1): limbs <= 2^28 - 1 + 2^8 <= T out.
//   * mul_small(c), c < 2^16: limbs <= 2 T times c is < 2^46; the same 64-bit carry.  Tight out.
//   * canon: the carry pass (value < 2^448 + 2^428 < 2 p), then p is subtracted with a signed chain and added back under the
//     borrow's mask.
// Every bound that is not carried by the type is a static_assert below; -DECGPU_BOUNDS_CHECK (host only) checks the limbs of every
// Gf<M> against M * T where an operation reads them.
#pragma once

#include <stdint.h>

#include "ecgpu_params.h"

#if defined(ECGPU_BOUNDS_CHECK) && !defined(__HIP_DEVICE_COMPILE__)
#define ECGPU_FE448_CHECK(cond) do { if (!(cond)) __builtin_trap(); } while (0)
#else
#define ECGPU_FE448_CHECK(cond) do { } while (0)
#endif

namespace ecgpu {
namespace fe448 {

ECGPU_CONST int NL = 16;                                   // limbs
ECGPU_CONST int LB = 28;                                   // bits per limb
ECGPU_CONST uint32_t MASK = (1u << LB) - 1u;
ECGPU_CONST uint64_t T = ((uint64_t)1 << LB) + 256u;      // limb bound of a tight element
ECGPU_CONST int NW = 14;                                   // 32-bit words of a 56-byte record

// limb i of p: 2^28 - 1, except limb 8 (the -2^224): 2^28 - 2
ECGPU_HD constexpr uint32_t p_limb(int i) { return i == 8 ? MASK - 1u : MASK; }

template <int M>
struct Gf {
    static_assert(M >= 1 && (uint64_t)M * T < ((uint64_t)1 << 32), "limbs are 32-bit words");
    uint32_t v[NL];
    ECGPU_HD void check() const {
#pragma unroll
        for (int i = 0; i < NL; i++) ECGPU_FE448_CHECK((uint64_t)v[i] <= (uint64_t)M * T);
    }
};
using Gf1 = Gf<1>;

// raw limbs as a claim of magnitude M (checked in the bounds build)
template <int M>
ECGPU_HD Gf<M> wrap(const uint32_t* w) {
    Gf<M> r;
#pragma unroll
    for (int i = 0; i < NL; i++) r.v[i] = w[i];
    r.check();
    return r;
}

ECGPU_HD Gf1 zero() {
    Gf1 r;
#pragma unroll
    for (int i = 0; i < NL; i++) r.v[i] = 0u;
    return r;
}
ECGPU_HD Gf1 small(uint32_t c) {                           // c < 2^28
    Gf1 r = zero();
    r.v[0] = c;
    return r;
}

// the carry pass on any 32-bit limbs
ECGPU_HD Gf1 carry_words(const uint32_t* a) {
    Gf1 r;
    const uint32_t top = a[NL - 1] >> LB;
#pragma unroll
    for (int i = NL - 1; i >= 1; i--) r.v[i] = (a[i] & MASK) + (a[i - 1] >> LB);
    r.v[0] = (a[0] & MASK) + top;
    r.v[8] += top;
    r.check();
    return r;
}
template <int M>
ECGPU_HD Gf1 carry(const Gf<M>& a) {
    a.check();
    return carry_words(a.v);
}

template <int A, int B>
ECGPU_HD Gf<A + B> add(const Gf<A>& a, const Gf<B>& b) {
    a.check();
    b.check();
    Gf<A + B> r;
#pragma unroll
    for (int i = 0; i < NL; i++) r.v[i] = a.v[i] + b.v[i];
    return r;
}

template <int A, int B>
ECGPU_HD Gf1 sub(const Gf<A>& a, const Gf<B>& b) {
    static_assert(A + 2 * B <= 15, "a + 2B p - b must fit 32-bit limbs");
    static_assert((uint64_t)2 * B * (MASK - 1u) >= (uint64_t)B * T, "every limb of 2B p covers a limb of b");
    a.check();
    b.check();
    uint32_t t[NL];
#pragma unroll
    for (int i = 0; i < NL; i++) t[i] = a.v[i] + (uint32_t)(2 * B) * p_limb(i) - b.v[i];
    return carry_words(t);
}

template <int B>
ECGPU_HD Gf1 neg(const Gf<B>& b) {
    return sub(zero(), b);
}

// 16 columns (c[j] + a carry < 2^36 must not overflow) -> tight limbs
ECGPU_HD Gf1 reduce_columns(const uint64_t* c) {
    Gf1 r;
    uint64_t acc = 0;
#pragma unroll
    for (int j = 0; j < NL; j++) {
        ECGPU_FE448_CHECK(c[j] <= ~(uint64_t)0 - acc);
        acc += c[j];
        r.v[j] = (uint32_t)acc & MASK;
        acc >>= LB;
    }
    ECGPU_FE448_CHECK(acc < ((uint64_t)1 << 36));
    const uint64_t lo = (uint64_t)r.v[0] + acc, hi = (uint64_t)r.v[8] + acc;       // 2^448 = 2^224 + 1
    r.v[0] = (uint32_t)lo & MASK;
    r.v[1] += (uint32_t)(lo >> LB);
    r.v[8] = (uint32_t)hi & MASK;
    r.v[9] += (uint32_t)(hi >> LB);
    r.check();
    return r;
}

ECGPU_HD uint64_t mul32(uint32_t a, uint32_t b) { return (uint64_t)a * b; }

template <int A, int B>
ECGPU_HD Gf1 mul(const Gf<A>& a, const Gf<B>& b) {
    static_assert(A * B <= 4, "38 A B T^2 must fit a 64-bit column with room for the carry");
    static_assert(T * T < (~(uint64_t)0 - ((uint64_t)1 << 36)) / (38 * 4), "the column bound, with room for a carry");
    static_assert((uint64_t)2 * B * T < ((uint64_t)1 << 32), "b0 + b1 fits a word");
    a.check();
    b.check();
    const uint32_t *a0 = a.v, *a1 = a.v + 8, *b0 = b.v, *b1 = b.v + 8;
    uint32_t bs[8];
#pragma unroll
    for (int i = 0; i < 8; i++) bs[i] = b0[i] + b1[i];
    uint64_t c[NL];
#pragma unroll
    for (int j = 0; j < 8; j++) {
        uint64_t l = 0, h = 0, x = 0;                      // L[j];  H[j] + L[8 + j];  H[8 + j]
#pragma unroll
        for (int i = 0; i <= j; i++) {
            l += mul32(a0[i], b0[j - i]) + mul32(a1[i], b1[j - i]);
            h += mul32(a0[i], b1[j - i]) + mul32(a1[i], bs[j - i]);
        }
#pragma unroll
        for (int i = j + 1; i < 8; i++) {
            h += mul32(a0[i], b0[8 + j - i]) + mul32(a1[i], b1[8 + j - i]);
            x += mul32(a0[i], b1[8 + j - i]) + mul32(a1[i], bs[8 + j - i]);
        }
        c[j] = l + x;
        c[8 + j] = h + x;
    }
    return reduce_columns(c);
}

template <int A>
ECGPU_HD Gf1 sqr(const Gf<A>& a) {
    static_assert(A * A <= 4, "38 A^2 T^2 must fit a 64-bit column with room for the carry");
    static_assert((uint64_t)2 * A * T < ((uint64_t)1 << 32), "a doubled limb fits a word");
    a.check();
    const uint32_t *a0 = a.v, *a1 = a.v + 8;
    uint32_t d0[8], d1[8];
#pragma unroll
    for (int i = 0; i < 8; i++) {
        d0[i] = 2u * a0[i];
        d1[i] = 2u * a1[i];
    }
    // column k of a0^2, a1^2 and 2 a0 a1 (k = 0..14)
    uint64_t c[NL];
#pragma unroll
    for (int j = 0; j < 8; j++) {
        uint64_t s0[2] = {0, 0}, s1[2] = {0, 0}, m[2] = {0, 0};
#pragma unroll
        for (int half = 0; half < 2; half++) {
            const int k = j + 8 * half;
            if (k <= 14) {
#pragma unroll
                for (int i = 0; i < 8; i++) {
                    const int l = k - i;
                    if (l < 0 || l > 7) continue;
                    m[half] += mul32(d0[i], a1[l]);
                    if (i < l) {
                        s0[half] += mul32(d0[i], a0[l]);
                        s1[half] += mul32(d1[i], a1[l]);
                    } else if (i == l) {
                        s0[half] += mul32(a0[i], a0[i]);
                        s1[half] += mul32(a1[i], a1[i]);
                    }
                }
            }
        }
        // L = a0^2 + a1^2, H = 2 a0 a1 + a1^2:  low = L[j] + H[8 + j],  high = H[j] + L[8 + j] + H[8 + j]
        const uint64_t x = m[1] + s1[1];
        c[j] = s0[0] + s1[0] + x;
        c[8 + j] = m[0] + s1[0] + s0[1] + s1[1] + x;
    }
    return reduce_columns(c);
}

template <uint32_t C, int A>
ECGPU_HD Gf1 mul_small(const Gf<A>& a) {
    static_assert(C < (1u << 16) && A <= 2, "limb * c stays far below 2^64");
    a.check();
    uint64_t c[NL];
#pragma unroll
    for (int i = 0; i < NL; i++) c[i] = mul32(a.v[i], C);
    return reduce_columns(c);
}

// the unique representative in [0, p), limbs < 2^28
template <int M>
ECGPU_HD Gf1 canon(const Gf<M>& a) {
    Gf1 r = carry(a);                                      // value < 2^448 + 2^428 < 2 p
    int32_t sc = 0;
#pragma unroll
    for (int i = 0; i < NL; i++) {                         // r - p, signed chain
        sc += (int32_t)r.v[i] - (int32_t)p_limb(i);
        r.v[i] = (uint32_t)sc & MASK;
        sc >>= LB;
    }
    ECGPU_FE448_CHECK(sc == 0 || sc == -1);
    const uint32_t back = (uint32_t)sc;                    // all ones when r < p: add p back
    uint32_t cy = 0;
#pragma unroll
    for (int i = 0; i < NL; i++) {
        cy += r.v[i] + (p_limb(i) & back);
        r.v[i] = cy & MASK;
        cy >>= LB;
    }
    return r;
}

// 14 little-endian words (the 56-byte record as it lies) -> limbs < 2^28; any value below 2^448 is taken as it is (a lazy
// representative: [p, 2^448) is reduced by whatever canon comes last)
ECGPU_HD Gf1 from_words(const uint32_t* w) {
    Gf1 r;
#pragma unroll
    for (int i = 0; i < NL; i++) {
        const int bit = LB * i, q = bit / 32, s = bit % 32;
        uint32_t x = w[q] >> s;
        if (s > 32 - LB && q + 1 < NW) x |= w[q + 1] << (32 - s);
        r.v[i] = x & MASK;
    }
    return r;
}

// canonical limbs -> 14 little-endian words
ECGPU_HD void to_words(uint32_t* w, const Gf1& c) {
#pragma unroll
    for (int q = 0; q < NW; q++) {
        uint32_t x = 0;
#pragma unroll
        for (int i = 0; i < NL; i++) {
            const int lo = LB * i - 32 * q;                // where limb i starts, relative to word q
            if (lo >= 32 || lo + LB <= 0) continue;
            x |= lo >= 0 ? c.v[i] << lo : c.v[i] >> -lo;
        }
        w[q] = x;
    }
}

// mask: all ones or zero
ECGPU_HD Gf1 select(uint32_t mask, const Gf1& a, const Gf1& b) {          // mask ? a : b
    Gf1 r;
#pragma unroll
    for (int i = 0; i < NL; i++) r.v[i] = b.v[i] ^ (mask & (a.v[i] ^ b.v[i]));
    return r;
}
ECGPU_HD void cswap(uint32_t mask, Gf1& a, Gf1& b) {
#pragma unroll
    for (int i = 0; i < NL; i++) {
        const uint32_t t = mask & (a.v[i] ^ b.v[i]);
        a.v[i] ^= t;
        b.v[i] ^= t;
    }
}

ECGPU_HD Gf1 sqr_n(Gf1 a, int n) {
#pragma unroll 1
    for (int i = 0; i < n; i++) a = sqr(a);
    return a;
}

// a^(p - 2): p - 2 is 223 ones, a zero, 222 ones, a zero, a one.  447 squarings and 13 products, fixed; 0 -> 0.
ECGPU_HD Gf1 invert(const Gf1& a) {
    const Gf1 x2 = mul(sqr(a), a);                         // a^(2^2 - 1)
    const Gf1 x3 = mul(sqr(x2), a);
    const Gf1 x6 = mul(sqr_n(x3, 3), x3);
    const Gf1 x12 = mul(sqr_n(x6, 6), x6);
    const Gf1 x24 = mul(sqr_n(x12, 12), x12);
    const Gf1 x27 = mul(sqr_n(x24, 3), x3);
    const Gf1 x54 = mul(sqr_n(x27, 27), x27);
    const Gf1 x108 = mul(sqr_n(x54, 54), x54);
    const Gf1 x111 = mul(sqr_n(x108, 3), x3);
    const Gf1 x222 = mul(sqr_n(x111, 111), x111);          // a^(2^222 - 1)
    const Gf1 x223 = mul(sqr(x222), a);
    const Gf1 t = mul(sqr_n(x223, 223), x222);             // (2^223 - 1) 2^223 + 2^222 - 1
    return mul(sqr_n(t, 2), a);
}

}  // namespace fe448
}  // namespace ecgpu
