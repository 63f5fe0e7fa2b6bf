// ecgpu_x448.h — batch X448 (RFC 7748 over Curve448): the Montgomery ladder with secret scalars, one element per lane (host +
// device lane body, HIP kernels at the end).
//
// Reference counterparts: `x448::x448` / `x448_unchecked` (x448/src/lib.rs:152-163), `PublicKey::from(&EphemeralSecret)`
// (:25-31), `&MontgomeryPoint * &EdwardsScalar` (ed448-goldilocks/src/montgomery.rs:83-110) and its ladder step
// `differential_add_and_double` (:168-204).  All records are 56 bytes, little-endian.
//     k = the scalar's bytes with bytes[0] &= 252, bytes[55] |= 128 (lib.rs:122-126), used as the 448-bit integer it is: never
//         reduced modulo the group order.  Bit 0 is therefore 0, and the reference's ladder has no final swap: neither has this one.
//     u = any 56 bytes, taken modulo p (`FieldElement::from_bytes`): [p, 2^448) is legal input.
//     x0 = (1 : 0), x1 = (u : 1); 448 steps from bit 447 down; the result is U W^-1 of x0 with 0^-1 = 0, canonical: a result at
//         infinity is the record of 56 zero bytes, not an error.
//     The checked form refuses a point whose BYTES are LOW_A (0), LOW_B (1) or LOW_C (p - 1) (montgomery.rs:23-42,137-139): ok = 0
//     and a zero record.  The aliases p and p + 1 are not refused; their product is the zero record with ok = 1.
//
// Secrecy: scalars, ladder state and results are secret.  No branch and no address depends on them (tools/ct_isa_check.py --unit
// x448): the scalar sits in fourteen registers that are shifted left by one bit per step, the conditional swap is a per-limb select
// under the mask of swap ^ bit, the inversion is the fixed chain of ecgpu_fe448.h, and the low-order verdict — of a public point —
// is computed without a branch all the same, so that the analysis has nothing to excuse.  A refused element runs the ladder on
// u = 5 in place of its point and has its result masked away: it never changes what its neighbours do.
//
// Per step: 5 products + 4 squares + one product by 39082 (the base form: 4 + 4 + products by 39082 and by 5).  The kernel keeps
// nothing in memory between its load and its store: there is no parked state to wipe; the staged scalars and results are the
// host-pointer calls' to mark.
#pragma once

#include "ecgpu_fe448.h"

namespace ecgpu {

enum : int { X448_CHECKED = 0, X448_UNCHECKED = 1, X448_BASE = 2 };
ECGPU_CONST uint32_t X448_A24 = 39082;                     // (A + 2) / 4 for A = 156326: `A_PLUS_TWO_OVER_FOUR`
ECGPU_CONST uint32_t X448_BASE_U = 5;                      // `MontgomeryPoint::GENERATOR`

// all ones when x == 0
ECGPU_HD uint32_t x448_mask_zero(uint32_t x) { return ((x | (0u - x)) >> 31) - 1u; }

// all ones when the 14 words are LOW_A, LOW_B or LOW_C; the comparison is on the record as it lies
ECGPU_HD uint32_t x448_low_order_words(const uint32_t* u) {
    uint32_t rest = 0, rest_c = 0;                         // words 1..13 against 0, and against the words of p - 1
#pragma unroll
    for (int j = 1; j < fe448::NW; j++) {
        rest |= u[j];
        rest_c |= u[j] ^ (j == 7 ? 0xFFFFFFFEu : 0xFFFFFFFFu);
    }
    const uint32_t a = rest | u[0], b = rest | (u[0] ^ 1u), c = rest_c | (u[0] ^ 0xFFFFFFFEu);
    return x448_mask_zero(a) | x448_mask_zero(b) | x448_mask_zero(c);
}

struct X448Point {
    fe448::Gf1 U, W;
};

// `differential_add_and_double`: P <- 2 P, Q <- P + Q, for P - Q = (u : 1)
template <bool BASE>
ECGPU_HD void x448_step(X448Point& P, X448Point& Q, const fe448::Gf1& u) {
    using namespace fe448;
    const Gf<2> t0 = add(P.U, P.W);
    const Gf1 t1 = sub(P.U, P.W);
    const Gf<2> t2 = add(Q.U, Q.W);
    const Gf1 t3 = sub(Q.U, Q.W);
    const Gf1 t4 = sqr(t0);
    const Gf1 t5 = sqr(t1);
    const Gf1 t6 = sub(t4, t5);
    const Gf1 t7 = mul(t0, t3);
    const Gf1 t8 = mul(t1, t2);
    const Gf<2> t9 = add(t7, t8);
    const Gf1 t10 = sub(t7, t8);
    const Gf1 t12 = sqr(t10);
    const Gf1 t13 = mul_small<X448_A24>(t6);
    const Gf<2> t15 = add(t13, t5);
    P.U = mul(t4, t5);
    P.W = mul(t6, t15);
    Q.U = sqr(t9);
    if constexpr (BASE)
        Q.W = mul_small<X448_BASE_U>(t12);
    else
        Q.W = mul(u, t12);
}

// One element.  k_in, u_in: the records as they lie (u_in is not read in the base form).  Returns the verdict as a mask (all ones:
// accepted; only the checked form refuses) and writes the result, zero where refused.
template <int MODE>
ECGPU_HD uint32_t x448_lane_words(uint32_t* out, const uint32_t* k_in, const uint32_t* u_in) {
    using namespace fe448;
    uint32_t k[NW], uw[NW];
#pragma unroll
    for (int j = 0; j < NW; j++) k[j] = k_in[j];
    k[0] &= 0xFFFFFFFCu;                                   // the clamp
    k[NW - 1] |= 0x80000000u;
    uint32_t refused = 0;
    if constexpr (MODE == X448_CHECKED) refused = x448_low_order_words(u_in);
#pragma unroll
    for (int j = 0; j < NW; j++) {
        const uint32_t base = j == 0 ? X448_BASE_U : 0u;
        if constexpr (MODE == X448_BASE)
            uw[j] = base;
        else
            uw[j] = base ^ (~refused & (u_in[j] ^ base));
    }
    const Gf1 u = from_words(uw);
    X448Point x0{small(1), zero()}, x1{u, small(1)};
    uint32_t swap = 0;
#pragma unroll 1
    for (int s = 0; s < 448; s++) {                        // the counter is public; the scalar is a shift register
        const uint32_t bit = k[NW - 1] >> 31;
#pragma unroll
        for (int j = NW - 1; j >= 1; j--) k[j] = (k[j] << 1) | (k[j - 1] >> 31);
        k[0] <<= 1;
        const uint32_t m = 0u - (swap ^ bit);
        cswap(m, x0.U, x1.U);
        cswap(m, x0.W, x1.W);
        x448_step<MODE == X448_BASE>(x0, x1, u);
        swap = bit;
    }
    const Gf1 r = canon(mul(x0.U, invert(x0.W)));
    to_words(out, r);
#pragma unroll
    for (int j = 0; j < NW; j++) out[j] &= ~refused;
    return ~refused;
}

// ---- ecgpu_selftest_fe448: one op of ecgpu_fe448.h on raw limbs (16 words per element), the same body on the device and in
// the g++ twin.  The magnitude each op claims for what it is handed is the widest it accepts. ----
enum : int {
    FE448_OP_MUL = 0,        // Gf<2> x Gf<2>
    FE448_OP_SQR = 1,        // Gf<2>
    FE448_OP_ADD = 2,        // Gf<1> + Gf<1>, limbs as the lazy sum leaves them
    FE448_OP_SUB = 3,        // Gf<2> - Gf<2>
    FE448_OP_MUL_SMALL = 4,  // 39082 x Gf<2>
    FE448_OP_CARRY = 5,      // any 32-bit limbs
    FE448_OP_CANON = 6,      // Gf<15>: limbs up to 15 T
    FE448_OP_INVERT = 7,     // Gf<1>
    FE448_OP_BYTES = 8,      // words 0..13 of a: the 56-byte record -> from_bytes -> to_bytes (words 14, 15 of out: zero)
    FE448_OPS = 9
};

ECGPU_HD void fe448_selftest_op(int op, uint32_t* out, const uint32_t* a, const uint32_t* b) {
    using namespace fe448;
    Gf1 r = zero();
    uint32_t raw[NL];
    bool is_raw = false;
    switch (op) {
    case FE448_OP_MUL: r = mul(wrap<2>(a), wrap<2>(b)); break;
    case FE448_OP_SQR: r = sqr(wrap<2>(a)); break;
    case FE448_OP_ADD: {
        const Gf<2> s = add(wrap<1>(a), wrap<1>(b));
        for (int i = 0; i < NL; i++) raw[i] = s.v[i];
        is_raw = true;
        break;
    }
    case FE448_OP_SUB: r = sub(wrap<2>(a), wrap<2>(b)); break;
    case FE448_OP_MUL_SMALL: r = mul_small<X448_A24>(wrap<2>(a)); break;
    case FE448_OP_CARRY: r = carry_words(a); break;
    case FE448_OP_CANON: r = canon(wrap<15>(a)); break;
    case FE448_OP_INVERT: r = invert(wrap<1>(a)); break;
    case FE448_OP_BYTES: {
        to_words(raw, canon(from_words(a)));
        raw[14] = raw[15] = 0u;
        is_raw = true;
        break;
    }
    default: break;
    }
    for (int i = 0; i < NL; i++) out[i] = is_raw ? raw[i] : r.v[i];
}

}  // namespace ecgpu

// =============================================================================================================================
#if defined(__HIPCC__)

namespace ecgpu {

ECGPU_CONST int X448_BLOCK = 64;                          // one wave per block: a short batch spreads over the CUs

// scalars, points, out: n records of 56 bytes (points: unused in the base form); ok: n verdict bytes (the checked form only)
template <int MODE>
__global__ void __launch_bounds__(X448_BLOCK)
k_x448_ladder(const uint8_t* __restrict__ scalars, const uint8_t* __restrict__ points, size_t n, uint8_t* __restrict__ out,
              uint8_t* __restrict__ ok) {
    constexpr int NW = fe448::NW;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t k[NW], u[NW], r[NW];
    const uint32_t* kp = reinterpret_cast<const uint32_t*>(scalars + i * 56);
#pragma unroll
    for (int j = 0; j < NW; j++) k[j] = kp[j];
    if constexpr (MODE != X448_BASE) {
        const uint32_t* up = reinterpret_cast<const uint32_t*>(points + i * 56);
#pragma unroll
        for (int j = 0; j < NW; j++) u[j] = up[j];
    }
    const uint32_t accepted = x448_lane_words<MODE>(r, k, u);
    uint32_t* op = reinterpret_cast<uint32_t*>(out + i * 56);
#pragma unroll
    for (int j = 0; j < NW; j++) op[j] = r[j];
    if constexpr (MODE == X448_CHECKED) ok[i] = (uint8_t)(accepted & 1u);
}

// (a template like every kernel of these headers: more than one translation unit includes the file)
template <class Unused = void>
__global__ void __launch_bounds__(X448_BLOCK)
k_selftest_fe448(int op, const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, size_t n, uint32_t* __restrict__ out) {
    constexpr int NL = fe448::NL;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t x[NL], y[NL], r[NL];
#pragma unroll
    for (int j = 0; j < NL; j++) {
        x[j] = a[i * NL + j];
        y[j] = b ? b[i * NL + j] : 0u;
    }
    fe448_selftest_op(op, r, x, y);
#pragma unroll
    for (int j = 0; j < NL; j++) out[i * NL + j] = r[j];
}

}  // namespace ecgpu

#endif  // __HIPCC__
