// ecgpu_bignsign.h — batch bign signing (STB 34.101.45-2013 §7.1, l = 128): the caller's nonce, the belt-based nonce generator of
// §6.3.3, and messages (host + device algorithms, HIP kernels at the end).
//
// Reference counterparts: `bignp256::ecdsa::SigningKey` — `PrehashSigner::sign_prehash` (bignp256/src/ecdsa/signing.rs:110-161) and
// `Signer::try_sign` (:164-176: H = belt-hash(message)).
//     h = prehash mod q (`Scalar::reduce`),  k from the generator below,  R = k G,
//     S0 = belt-hash(OID(h) || <x(R)>_256 || RAW prehash)[..16],  S1 = k - h - (S0 + 2^128) d mod q;
//     no signature when S0 = 0 or S1 = 0 (`Signature::from_bytes`, bignp256/src/ecdsa.rs:85-87).
// The generator is the un-vendored `bign_genk::KGenerator<BeltBlock>`; the standard's algorithm is restated here (t empty: no
// additional data) and pinned by the reference's own signature vector (bignp256/tests/ecdsa.rs:20-33), which is the deterministic
// signature of its key and message.  All byte strings as they lie, integers little-endian:
//     theta = belt-hash(OID(h) || <d>_256 || t),   r1 || r2 = <h>_256  — the prehash REDUCED mod q,
//     for i = 1, 2, ...:  s = r1;  r1 = belt-block(s, theta) xor r2 xor <i>_128;  r2 = s;
//                         if i mod 4 == 0 and 0 < (r1 || r2) < q:  k = r1 || r2, stop.
// The form with the caller's nonce is the standard's steps 3-7 and is OURS: the reference has no such entry point.
//
// R = k G is k_fixed_base_ct (ecgpu_ct.h).  The rule of ecgpu_sign.h holds for k_bign_genk and k_bign_sign_finish (and for
// k_sign_nonce_load, which loads the caller's nonce): no branch and no address depends on d, k, the prehash or anything derived
// from them (tools/ct_isa_check.py --unit bignsign).  belt's S-box is a table, and the generator looks it up at SECRET indices —
// every byte of a + K under the key theta — so these kernels use Belt::CtSbox (ecgpu_belt.h): byte permutes and bitwise selects over
// constants, no memory access.
// Two kernels are NOT on the checked list, each on purpose:
//   * k_bign_genk_retry — variable time like k_rfc6979_retry: it runs the generator on for the elements whose candidate of round
//     4 was rejected, so its trip count follows the REJECTED candidates.  With the real q that is one element in 2^130.  Its lookups
//     are the constant-address ones all the same: the state it continues leads to the nonce that is used.
//   * k_bign_sign_s0 — S0 hashes x(R) and the prehash.  Both are public: R = (S1 + H) G + (S0 + 2^128) Q can be recomputed from the
//     finished signature, the prehash and the public key (it is what verification does).  So it stages the S-box in LDS and indexes
//     it by data, exactly as k_bign_finish does for verification.  (Only the refused elements' R stays unpublished: an R computed
//     from k = 1 in place of an unusable nonce, which is G.)
#pragma once

#include "ecgpu_belt.h"
#include "ecgpu_sign.h"

namespace ecgpu {

// the curve bign signing exists over (ecgpu_inst_sign.hip asks this instead of comparing ids)
template <class C>
struct BignSign {
    ECGPU_CONST bool value = C::ID == CURVE_BIGN256;
};

// the generator's acceptance bound as a kernel argument: q in the signing calls, the caller's value in ecgpu_selftest_bign_genk
// (no input makes a candidate >= q with the real q, so the retry path is reached on hardware with a smaller bound)
struct BignBound {
    uint32_t w[8];
};

// the generator between two candidates; parked word-major in context scratch (word j of element i at [j * n + i])
struct BignGenkState {
    uint32_t theta[8], r1[4], r2[4], i;
};
ECGPU_CONST int BIGN_GENK_STATE_WORDS = 17;

// theta = belt-hash(OID(h) || <d>_256): d = the key's eight words as read (an out-of-range key hashes as it is: its element ends with
// ok = 0 whatever the nonce).  The 43 message bytes are put together from the words by shifts: the eleven bytes of the OID move d
// by three bytes.
template <class SB>
ECGPU_HD void bign_theta_words(SB sb, uint32_t* theta, const uint32_t* d) {
    constexpr int NO = (int)sizeof(Belt::OID);
    static_assert(NO == 11, "the shifts below place d behind eleven bytes");
    uint32_t m[16];
#pragma unroll
    for (int j = 0; j < 16; j++) m[j] = 0;
#pragma unroll
    for (int j = 0; j < NO; j++) m[j / 4] |= (uint32_t)Belt::OID[j] << (8 * (j % 4));
    m[2] |= d[0] << 24;
#pragma unroll
    for (int w = 3; w < 11; w++) m[w] = (d[w - 3] >> 8) | (w - 2 < 8 ? d[w - 2] << 24 : 0u);
    Belt::hash_two_blocks(sb, theta, m, (uint32_t)NO + 32u);
}

// rounds st.i + 1 .. st.i + 4, then the candidate r1 || r2 and whether it is in (0, bound).  `i` is a counter, never data.
template <class SB>
ECGPU_HD bool bign_genk_candidate(SB sb, BignGenkState& st, const uint32_t* bound, uint32_t* k) {
#pragma unroll 1
    for (int r = 0; r < 4; r++) {
        uint32_t y[4];
        st.i++;
        Belt::block(sb, y, st.r1, st.theta);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint32_t s = st.r1[j];
            st.r1[j] = y[j] ^ st.r2[j] ^ (j == 0 ? st.i : 0u);
            st.r2[j] = s;
        }
    }
#pragma unroll
    for (int j = 0; j < 4; j++) {
        k[j] = st.r1[j];
        k[4 + j] = st.r2[j];
    }
    return (bool)((int)!mp_is_zero<8>(k) & (int)!mp_geq<8>(k, bound));
}

// the generator up to its first candidate (round 4).  h_in: the prehash as read; it is reduced here, and the REDUCED value is what
// the generator is given (signing.rs:117-123).  Writes the candidate, or 1 in place of a rejected one; returns its verdict.
template <class C, class SB>
ECGPU_HD bool bign_genk_first_words(SB sb, const uint32_t* d_in, const uint32_t* h_in, const uint32_t* bound, uint32_t* k_out,
                                    BignGenkState& st) {
    constexpr int N = C::N;
    static_assert(N == 8, "bign signatures are defined here for l = 128 (bign-curve256v1)");
    uint32_t h[N], k[N], one[N];
    ScalarN<C>::reduce_once(h, h_in);                                 // q > 2^255: one subtraction
    bign_theta_words(sb, st.theta, d_in);
#pragma unroll
    for (int j = 0; j < 4; j++) {
        st.r1[j] = h[j];
        st.r2[j] = h[4 + j];
    }
    st.i = 0;
    const bool ok = bign_genk_candidate(sb, st, bound, k);
    sg_one<N>(one);
    sg_sel<N>(k_out, ok, k, one);
    return ok;
}

// the generator run on from a parked state until a candidate is accepted or `cap` candidates (the first one counted) were rejected:
// VARIABLE TIME in the rejected candidates, on purpose.  k_out is written only when a candidate was accepted.
template <class SB>
ECGPU_HD bool bign_genk_retry_words(SB sb, BignGenkState& st, const uint32_t* bound, int cap, uint32_t* k_out) {
    uint32_t k[8];
    bool ok = false;
#pragma unroll 1
    for (int tried = 1; tried < cap && !ok; tried++) ok = bign_genk_candidate(sb, st, bound, k);
    if (ok) {
#pragma unroll
        for (int j = 0; j < 8; j++) k_out[j] = k[j];
    }
    return ok;
}

// S0 = belt-hash(OID(h) || <x(R)>_256 || RAW prehash)[..16] (signing.rs:141-147): public inputs, the table form of the S-box
ECGPU_HD void bign_sign_s0_words(const uint8_t* sb, uint32_t* s0, const uint8_t* rx_bytes, const uint8_t* h_bytes) {
    uint32_t t[8];
    const HashPiece pc[3] = {{Belt::OID, sizeof(Belt::OID)}, {rx_bytes, (size_t)32}, {h_bytes, (size_t)32}};
    Belt::hash_pieces<3>(sb, t, pc);
#pragma unroll
    for (int j = 0; j < 4; j++) s0[j] = t[j];
}

// a - b mod q for a, b < q
template <class C>
ECGPU_HD void bign_sub_mod(uint32_t* r, const uint32_t* a, const uint32_t* b) {
    constexpr int N = C::N;
    uint32_t t[N], u[N];
    const uint32_t borrow = mp_sub<N>(t, a, b);
    (void)mp_add<N>(u, t, C::ORDER);
    sg_sel<N>(r, borrow != 0, u, t);
}

// ---- bign: everything after S0 ------------------------------------------------------------------------------------------------
// d_in, k_in: the key and the nonce as read (any value); k_ok: the nonce's verdict (the load kernel's, or the generator's) — an
// invalid k was replaced by 1 before the multiplication and is replaced here the same way; h_in: the prehash as read (reduced here,
// once: q > 2^255); s0: four words, any value; r_inf: the identity flag of R (never set for 1 <= k < q).
// Writes S0 || S1 as 4 + 8 words (a zero record when not ok).
template <class C>
ECGPU_HD bool bign_sign_finish_words(const uint32_t* d_in, const uint32_t* k_in, bool k_ok, const uint32_t* h_in, const uint32_t* s0,
                                     bool r_inf, uint32_t* s0_out, uint32_t* s1_out) {
    using S = ScalarN<C>;
    using SS = SignScalar<C>;
    constexpr int N = C::N;
    static_assert(N == 8, "bign signatures are defined here for l = 128 (bign-curve256v1)");
    uint32_t one[N], d[N], k[N], h[N], t[N], td[N], kh[N], s1[N];
    sg_one<N>(one);
    const bool d_ok = SS::valid(d_in);
    sg_sel<N>(d, d_ok, d_in, one);
    k_ok = (bool)((int)k_ok & (int)SS::valid(k_in));
    sg_sel<N>(k, k_ok, k_in, one);
    S::reduce_once(h, h_in);
#pragma unroll
    for (int j = 0; j < 4; j++) {
        t[j] = s0[j];
        t[4 + j] = j == 0 ? 1u : 0u;                                  // S0 + 2^128 < 2^129 < q
    }
    S::mul(td, t, d);
    bign_sub_mod<C>(kh, k, h);
    bign_sub_mod<C>(s1, kh, td);
    const bool s0_nz = (s0[0] | s0[1] | s0[2] | s0[3]) != 0u;
    const bool ok = (bool)((int)d_ok & (int)k_ok & (int)!r_inf & (int)s0_nz & (int)!S::is_zero(s1));
    const uint32_t keep = sn_mask(ok);
#pragma unroll
    for (int j = 0; j < 4; j++) s0_out[j] = s0[j] & keep;
#pragma unroll
    for (int j = 0; j < N; j++) s1_out[j] = s1[j] & keep;
    return ok;
}

}  // namespace ecgpu

// =============================================================================================================================
#if defined(__HIPCC__)

#include "ecgpu_kernels.h"

namespace ecgpu {

// theta and rounds 1-4 of the generator with the constant-address S-box.  Writes the candidate (1 in place of a rejected one), its
// verdict, and the state (theta, r1, r2, i = 4) for k_bign_genk_retry.
template <class C>
__global__ void __launch_bounds__(BLOCK)
k_bign_genk(const uint8_t* __restrict__ d_in, const uint8_t* __restrict__ h_in, BignBound bound, size_t n, uint8_t* __restrict__ k_out,
            uint8_t* __restrict__ flag, uint32_t* __restrict__ state) {
    constexpr int N = C::N;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t d[N], h[N], k[N];
    load_wire<C>(d, d_in + i * 32);
    load_wire<C>(h, h_in + i * 32);
    BignGenkState st;
    const bool ok = bign_genk_first_words<C>(Belt::CtSbox(), d, h, bound.w, k, st);
    store_wire<C>(k_out + i * 32, k);
    flag[i] = ok ? 1 : 0;
#pragma unroll
    for (int j = 0; j < 8; j++) state[(size_t)j * n + i] = st.theta[j];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        state[(size_t)(8 + j) * n + i] = st.r1[j];
        state[(size_t)(12 + j) * n + i] = st.r2[j];
    }
    state[(size_t)16 * n + i] = st.i;
}

// VARIABLE TIME ON PURPOSE (see the head of this file): the generator run on for the elements whose flag is clear.  Launched once
// per call, by the rule of k_rfc6979_retry; lanes whose first candidate was accepted leave at once.  The round count is written
// back to the parked state (ecgpu_selftest_bign_genk reads it).
template <class C>
__global__ void __launch_bounds__(BLOCK)
k_bign_genk_retry(BignBound bound, size_t n, int cap, uint8_t* __restrict__ k_out, uint8_t* __restrict__ flag,
                  uint32_t* __restrict__ state) {
    constexpr int N = C::N;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (flag[i]) return;
    BignGenkState st;
#pragma unroll
    for (int j = 0; j < 8; j++) st.theta[j] = state[(size_t)j * n + i];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        st.r1[j] = state[(size_t)(8 + j) * n + i];
        st.r2[j] = state[(size_t)(12 + j) * n + i];
    }
    st.i = state[(size_t)16 * n + i];
    uint32_t k[N];
    const bool ok = bign_genk_retry_words(Belt::CtSbox(), st, bound.w, cap, k);
    state[(size_t)16 * n + i] = st.i;
    if (ok) {
        store_wire<C>(k_out + i * 32, k);
        flag[i] = 1;
    }
}

// S0 of element i from the affine R of k_normalize and the RAW prehash, 16 bytes per element.  NOT on the checked list: its inputs
// are public (see the head of this file), so the S-box is the LDS table of k_bign_finish.
template <class C>
__global__ void __launch_bounds__(BLOCK)
k_bign_sign_s0(const uint8_t* __restrict__ h_in, const uint8_t* __restrict__ r_xy, size_t n, uint8_t* __restrict__ s0_out) {
    static_assert(BLOCK == 256, "the 256-byte S-box is staged with one byte per lane");
    __shared__ uint8_t sbox[256];
    sbox[threadIdx.x] = Belt::H[threadIdx.x];
    __syncthreads();
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t s0[4];
    bign_sign_s0_words(sbox, s0, r_xy + i * 64, h_in + i * 32);
    store_words_vec<4>(reinterpret_cast<uint32_t*>(s0_out + i * 16), s0);
}

// S1 and ok; sig = S0 || S1 (48 bytes).  s0_in: S0 of element i at s0_in + i * s0_stride (16 in the pipeline; the self-test hands
// them in at the head of 64-byte records)
template <class C>
__global__ void __launch_bounds__(BLOCK)
k_bign_sign_finish(const uint8_t* __restrict__ d_in, const uint8_t* __restrict__ k_in, const uint8_t* __restrict__ k_flag,
                   const uint8_t* __restrict__ h_in, const uint8_t* __restrict__ s0_in, size_t s0_stride,
                   const uint8_t* __restrict__ r_inf, size_t n, uint8_t* __restrict__ sig_out, uint8_t* __restrict__ ok_out) {
    constexpr int N = C::N;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t d[N], k[N], h[N], s0[4], o0[4], o1[N];
    load_wire<C>(d, d_in + i * 32);
    load_wire<C>(k, k_in + i * 32);
    load_wire<C>(h, h_in + i * 32);
    load_words_vec<4>(s0, reinterpret_cast<const uint32_t*>(s0_in + i * s0_stride));
    const bool ok = bign_sign_finish_words<C>(d, k, k_flag[i] != 0, h, s0, r_inf[i] != 0, o0, o1);
    store_words_vec<4>(reinterpret_cast<uint32_t*>(sig_out + i * 48), o0);
    store_wire<C>(sig_out + i * 48 + 16, o1);
    ok_out[i] = ok ? 1 : 0;
}

}  // namespace ecgpu

#endif  // __HIPCC__
