// ecgpu_selftest_raw.h — the raw-domain field operations and the mod-n scalar operations of the self-tests (host + device).
//
// One statement of the operations for both compilers: tests/hostcheck (g++) and k_selftest_field_raw (gfx950,
// ecgpu_selftest.h) call the functions below, and tests/field_vectors.py holds the expected values as Python integers.
// "Raw domain": the operands enter through Field::unpack — no conversion into the Montgomery domain, no canonical check — so
// the limbs a test writes are the limbs the reduction sees: all ones, a single set limb, a value in [p, 2p) (the second
// representative every magnitude-1 element may have).  Operands are then scaled by repeated Field::add up to the magnitude
// limits of the parameter set (MAXPROD, MAXMAG, SQLIM), so the types carry the magnitudes and every static_assert of
// ecgpu_field.h is part of the test.
#pragma once

#include "ecgpu_field.h"
#include "ecgpu_scalar.h"

namespace ecgpu {

// m * x as x + x + ... + x: limb and value magnitude (m, m)
template <class C, int M>
ECGPU_HD auto selftest_times(const typename Field<C>::M1& x) {
    if constexpr (M == 1) return x;
    else return Field<C>::add(selftest_times<C, M - 1>(x), x);
}

// Operations 30 - 39, 46 and 47 on the words wa, wb (N little-endian words each, any value below 2^(32 N) whose limbs fit: below 2p or
// 2^(8 WireBytes)); with MP = MAXPROD, MM = MAXMAG, A1 = min(MP, MM), B1 = MP / A1, A2 = 5 / 4 / 3 / 2 for MP >= 25 / 16 / 9 /
// else, B2 = MP / A2, SQ = SQLIM (Ri = R^-1, or 1 for k256):
//   30 mul(A1 x, B1 y)                       31 mul(A2 x, B2 y)              32 sqr(SQ x)             33 mul(x, y)
//   34 norm(mul_sub(A2 x, B2 y, 6 y))        35 norm(sqr_sub(SQ x, 6 y))     (the fused forms, on every parameter set)
//   36 mul2(A2 x, floor(B2 / 2) y, A2 y, ceil(B2 / 2) x)
//   37 norm(sub(s x, s y)), s = 3 for k256 and 6 otherwise
//   38 to_canonical(x)                       39 is_zero(x) as 0 / 1 in the first word
//   46 inv(x)                                47 inv<true>(x)  (the variable-time division steps)
// 46 and 47 (45 stays unknown: the op-range tests pin it): F::inv packs its operand and inverts the words, so x < p is EXACTLY the
// integer ModInv::invert receives, and x in [p, 2p), p itself included, reaches it through pack's reduction — ModInv::invert wants
// x < p (invert(p) is 1, not 0: tools/modinv_model.py), and pack is what guarantees it.  The result is x^-1 mod p for k256 and
// x^-1 R^2 mod p for the Montgomery sets (0 for x = 0 mod p).
// 30 - 37, 46 and 47 come back through Field::pack (the internal-domain value in [0, p)).  False for an unknown operation.
template <class C>
ECGPU_HD bool selftest_field_raw(int op, const uint32_t* wa, const uint32_t* wb, uint32_t* wr) {
    using F = Field<C>;
    constexpr int MP = F::MAXPROD, MM = F::MAXMAG;
    constexpr int A1 = MP <= MM ? MP : MM, B1 = MP / A1;
    constexpr int A2 = MP >= 25 ? 5 : (MP >= 16 ? 4 : (MP >= 9 ? 3 : 2)), B2 = MP / A2;
    constexpr int SQ = F::SQLIM, S = C::REPR == REPR_U29_K256 ? 3 : 6;
    const auto x = F::unpack(wa), y = F::unpack(wb);
    switch (op) {
    case 30: F::pack(wr, F::mul(selftest_times<C, A1>(x), selftest_times<C, B1>(y))); break;
    case 31: F::pack(wr, F::mul(selftest_times<C, A2>(x), selftest_times<C, B2>(y))); break;
    case 32: F::pack(wr, F::sqr(selftest_times<C, SQ>(x))); break;
    case 33: F::pack(wr, F::mul(x, y)); break;
    case 34: F::pack(wr, F::norm(F::mul_sub(selftest_times<C, A2>(x), selftest_times<C, B2>(y), selftest_times<C, 6>(y)))); break;
    case 35: F::pack(wr, F::norm(F::sqr_sub(selftest_times<C, SQ>(x), selftest_times<C, 6>(y)))); break;
    case 36:
        F::pack(wr, F::mul2(selftest_times<C, A2>(x), selftest_times<C, B2 / 2>(y), selftest_times<C, A2>(y),
                            selftest_times<C, B2 - B2 / 2>(x)));
        break;
    case 37: F::pack(wr, F::norm(F::sub(selftest_times<C, S>(x), selftest_times<C, S>(y)))); break;
    case 38: F::to_canonical(wr, x); break;
    case 39:
        wr[0] = F::is_zero(x) ? 1u : 0u;
#pragma unroll
        for (int t = 1; t < C::N; t++) wr[t] = 0;
        break;
    case 46: F::pack(wr, F::inv(x)); break;
    case 47: F::pack(wr, F::template inv<true>(x)); break;
    default: return false;
    }
    return true;
}

// ScalarN<C>: 0 a * b mod n, 1 1 / a mod n (0 -> 0), 2 reduce_wire(a) (a < 2^(8 WireBytes)), 3 is_high(a) as 0 / 1 in the
// first word, 4 a through to_mont and from_mont.  a, b < n except for 2.  False for an unknown operation.
template <class C>
ECGPU_HD bool selftest_scalar(int op, const uint32_t* x, const uint32_t* y, uint32_t* r) {
    using S = ScalarN<C>;
#pragma unroll
    for (int t = 0; t < C::N; t++) r[t] = 0;
    switch (op) {
    case 0: S::mul(r, x, y); break;
    case 1: S::inv(r, x); break;
    case 2: S::reduce_wire(r, x); break;
    case 3: r[0] = S::is_high(x) ? 1u : 0u; break;
    case 4: {
        uint32_t m[C::N];
        S::to_mont(m, x);
        S::from_mont(r, m);
        break;
    }
    default: return false;
    }
    return true;
}

}  // namespace ecgpu
