// ecgpu_pke.h — batch SM2 public-key encryption and decryption (GB/T 32918.4): everything around the two multiplications
// (host + device algorithms, HIP kernels at the end).
//
// Reference counterparts: `sm2::pke` — `encrypt` (sm2/src/pke/encrypting.rs:166-230, the hazmat shape: the caller's nonce),
// `Cipher::from_slice`'s point checks (sm2/src/pke.rs:131-143), `decrypt` (sm2/src/pke/decrypting.rs:174-222) and `kdf`
// (sm2/src/pke.rs:349-381).  The reference's functions are generic but instantiated for Sm2 with Sm3 only; so is this file.
//     encrypt   C1 = k G,  (x2, y2) = k P_B,  t = KDF(x2 || y2, len M),  C2 = M ^ t,  C3 = SM3(x2 || M || y2)
//     decrypt   (x2, y2) = d C1,  M' = C2 ^ KDF(x2 || y2, len C2),  ok = (SM3(x2 || M' || y2) == C3)
//     KDF       block j (32 bytes) of t = SM3(x2 || y2 || I2OSP(j + 1, 4))
// The multiplications are k_fixed_base_ct and k_var_base_ct (ecgpu_ct.h).  What this file adds follows their rule — SECRECY: in
// k_pke_load, k_pke_seal and k_pke_open no branch and no address depends on k, d, x2, y2, t, a message byte or the outcome of the
// C3 comparison (tools/ct_isa_check.py --unit pke); msg_len and n are kernel arguments and every loop count follows them alone.  A
// scalar outside [1, n) is replaced by 1 under a mask and its element gets ok = 0.  k_pke_point checks the PUBLIC point (P_B, or
// the C1 of an untrusted ciphertext) and may branch on it: it is a kernel of its own so that the scalar half passes the checker
// as a whole.
//
// The hashing is ONE loop over passes with ONE call site of the compression function (ecgpu_hash.h:26-27); what a pass is — the
// block x2 || y2, KDF block j, block m of the C3 input — is a function of the loop counter.  x2 || y2 is exactly one SM3 block, so
// its chaining value is computed once and every KDF block costs one compression (the counter, the padding and the length 544 fit
// the second block): the digest is the same.
#pragma once

#include "ecgpu_hash.h"
#include "ecgpu_scalar.h"
#include "ecgpu_sign.h"
#include "ecgpu_sm3.h"
#include "ecgpu_verify.h"

namespace ecgpu {

// byte `idx` of 16 big-endian words (idx is a position, never data)
ECGPU_HD uint32_t pke_xy_byte(const uint32_t* xy, size_t idx) { return (xy[idx >> 2] >> (8 * (3 - (idx & 3)))) & 0xffu; }

// The KDF, the XOR and C3 of one element.  xy: x2 || y2 as 16 big-endian words; in: msg_len bytes (M when sealing, C2 when
// opening); out: msg_len bytes (C2 resp. M', written in full: the caller masks it once the verdict is known); c3: the digest
// SM3(x2 || M || y2) as 8 big-endian words, M being `in` when sealing and `out` when opening.  Returns the OR of the keystream
// bytes used (0: t was all zero).  words: `in` and `out` are both 4-byte aligned, so whole words of message may be moved as words
// (a kernel derives it from its arguments — the array bases and msg_len — so that it is the same for every lane of the launch).
template <bool OPEN>
ECGPU_HD uint32_t pke_stream(const uint32_t* xy, const uint8_t* in, size_t msg_len, uint8_t* out, uint32_t* c3, bool words) {
    const size_t kb = (msg_len + 31) / 32;               // KDF blocks
    const size_t total = 64 + msg_len;                    // bytes of x2 || M || y2
    const size_t nb3 = (total + 1 + 8 + 63) / 64;         // its padded blocks
    const uint8_t* hs = OPEN ? out : in;                  // the message C3 is taken over
    uint32_t mid[8], tnz = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) mid[j] = 0;
    Sm3::init(c3);
#pragma unroll 1
    for (size_t pass = 0; pass < 1 + kb + nb3; pass++) {
        const bool is_mid = pass == 0, is_kdf = pass != 0 && pass <= kb;      // (the loop counter's properties)
        uint32_t w[16], s[8];
        if (is_mid) {
#pragma unroll
            for (int j = 0; j < 16; j++) w[j] = xy[j];
            Sm3::init(s);
        } else if (is_kdf) {
#pragma unroll
            for (int j = 0; j < 16; j++) w[j] = 0;
            w[0] = (uint32_t)pass;                        // I2OSP(j + 1, 4)
            w[1] = 0x80000000u;
            w[15] = 68u * 8u;
#pragma unroll
            for (int j = 0; j < 8; j++) s[j] = mid[j];
        } else {
            const size_t base = (pass - 1 - kb) * 64;
#pragma unroll
            for (int j = 0; j < 16; j++) {
                const size_t o = base + 4 * (size_t)j;    // the word's first byte in x2 || M || y2 || padding
                uint32_t word = 0;
                if (o + 4 <= 32) {
                    word = xy[o >> 2];
                } else if (words && o >= 32 && o + 4 <= 32 + msg_len) {
                    word = bswap32(*reinterpret_cast<const uint32_t*>(hs + (o - 32)));
                } else {
#pragma unroll 1
                    for (int q = 0; q < 4; q++) {
                        const size_t p = o + q;
                        uint32_t byte = 0;
                        if (p < 32 + msg_len) byte = hs[p - 32];          // (p >= 32 here: the first 32 bytes are whole words)
                        else if (p < total) byte = pke_xy_byte(xy, p - msg_len);
                        else if (p == total) byte = 0x80u;
                        else if (p >= nb3 * 64 - 8) byte = (uint32_t)(((uint64_t)total * 8) >> (8 * (nb3 * 64 - 1 - p))) & 0xffu;
                        word = (word << 8) | byte;
                    }
                }
                w[j] = word;
            }
#pragma unroll
            for (int j = 0; j < 8; j++) s[j] = c3[j];
        }
        Sm3::compress(s, w);
        if (is_mid) {
#pragma unroll
            for (int j = 0; j < 8; j++) mid[j] = s[j];
        } else if (is_kdf) {
            const size_t base = (pass - 1) * 32;
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const size_t o = base + 4 * (size_t)j;
                if (o + 4 <= msg_len && words) {
                    const uint32_t t = bswap32(s[j]);
                    *reinterpret_cast<uint32_t*>(out + o) = *reinterpret_cast<const uint32_t*>(in + o) ^ t;
                    tnz |= t;
                } else {
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        if (o + q < msg_len) {
                            const uint32_t t = (s[j] >> (8 * (3 - q))) & 0xffu;
                            out[o + q] = (uint8_t)(in[o + q] ^ t);
                            tnz |= t;
                        }
                    }
                }
            }
        } else {
#pragma unroll
            for (int j = 0; j < 8; j++) c3[j] = s[j];
        }
    }
    return tnz;
}

// out[0 .. len) &= mask (all ones or all zeros): the record of an element without a verdict is zero
ECGPU_HD void pke_mask_bytes(uint8_t* out, size_t len, uint32_t mask, bool words) {
    if (words) {
        size_t o = 0;
#pragma unroll 1
        for (; o + 4 <= len; o += 4) *reinterpret_cast<uint32_t*>(out + o) &= mask;
#pragma unroll 1
        for (; o < len; o++) out[o] = (uint8_t)(out[o] & mask);
    } else {
#pragma unroll 1
        for (size_t o = 0; o < len; o++) out[o] = (uint8_t)(out[o] & mask);
    }
}

// every element's records 4-byte aligned: the bases are and msg_len is a multiple of 4
ECGPU_HD bool pke_word_aligned(const uint8_t* a, const uint8_t* b, size_t msg_len) {
    return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | (uintptr_t)msg_len) & 3u) == 0;
}

// ---- the lane bodies of the kernels, on wire bytes (tests/hostcheck_pke runs exactly these on the CPU) -------------------------
template <int NW>
ECGPU_HD void pke_load_words_be(uint32_t* w, const uint8_t* bytes) {          // big-endian words as SM3 reads them
    const uint32_t* p = reinterpret_cast<const uint32_t*>(bytes);
#pragma unroll
    for (int j = 0; j < NW; j++) w[j] = bswap32(p[j]);
}
template <int NW>
ECGPU_HD void pke_store_words_be(uint8_t* bytes, const uint32_t* w) {
    uint32_t* p = reinterpret_cast<uint32_t*>(bytes);
#pragma unroll
    for (int j = 0; j < NW; j++) p[j] = bswap32(w[j]);
}

// k_pke_load: the secret scalar (k or d) as read -> itself or, outside [1, n), 1; returns the verdict.  No short circuit.
template <class C>
ECGPU_HD bool pke_load_scalar(uint8_t* s_out, const uint8_t* s_in) {
    constexpr int N = C::N;
    uint32_t k[N], one[N];
    load_be<N>(k, s_in);
    sg_one<N>(one);
    const bool ok = SignScalar<C>::valid(k);
    sg_sel<N>(k, ok, k, one);
    store_be<N>(s_out, k);
    return ok;
}
// k_pke_point: the public point (P_B or C1) as read -> itself or, off the curve or with a coordinate >= p, G; returns the verdict
template <class C>
ECGPU_HD bool pke_load_point(uint8_t* xy_out, const uint8_t* xy_in) {
    constexpr int N = C::N;
    uint32_t cx[N], cy[N];
    load_be<N>(cx, xy_in);
    load_be<N>(cy, xy_in + 4 * N);
    const bool ok = verify_point_ok<C>(cx, cy);
#pragma unroll
    for (int j = 0; j < N; j++) {
        cx[j] = ok ? cx[j] : C::GX[j];
        cy[j] = ok ? cy[j] : C::GY[j];
    }
    store_be<N>(xy_out, cx);
    store_be<N>(xy_out + 4 * N, cy);
    return ok;
}
// k_pke_seal: x2y2 = the 64 wire bytes of k P_B; flag = the verdict of the load kernels; c1 = the 64 wire bytes of k G (zeroed
// in place without a verdict).  Writes C2 (msg_len bytes) and C3 (32 bytes); returns ok.
ECGPU_HD bool pke_seal_lane(const uint8_t* x2y2, uint32_t flag, const uint8_t* msg, size_t msg_len, uint8_t* c1, uint8_t* c2,
                            uint8_t* c3_out, bool words) {
    uint32_t xy[16], c3[8], p1[16];
    pke_load_words_be<16>(xy, x2y2);
    const uint32_t tnz = pke_stream<false>(xy, msg, msg_len, c2, c3, words);
    const bool ok = (bool)((int)(flag != 0) & (int)(tnz != 0));
    const uint32_t keep = sn_mask(ok);
    pke_load_words_be<16>(p1, c1);
#pragma unroll
    for (int j = 0; j < 16; j++) p1[j] &= keep;
    pke_store_words_be<16>(c1, p1);
#pragma unroll
    for (int j = 0; j < 8; j++) c3[j] &= keep;
    pke_store_words_be<8>(c3_out, c3);
    pke_mask_bytes(c2, msg_len, keep, words);
    return ok;
}
// k_pke_open: x2y2 = the 64 wire bytes of d C1; c3_in = the ciphertext's 32 bytes.  Writes M' (zero without a verdict: an
// unauthenticated plaintext is not released); returns ok.  The comparison is an OR of XORs.
ECGPU_HD bool pke_open_lane(const uint8_t* x2y2, uint32_t flag, const uint8_t* c2, size_t msg_len, const uint8_t* c3_in,
                            uint8_t* msg_out, bool words) {
    uint32_t xy[16], u[8], c3[8];
    pke_load_words_be<16>(xy, x2y2);
    pke_load_words_be<8>(c3, c3_in);
    (void)pke_stream<true>(xy, c2, msg_len, msg_out, u, words);
    uint32_t diff = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) diff |= u[j] ^ c3[j];
    const bool ok = (bool)((int)(flag != 0) & (int)(diff == 0));
    pke_mask_bytes(msg_out, msg_len, sn_mask(ok), words);
    return ok;
}

}  // namespace ecgpu

// =============================================================================================================================
#if defined(__HIPCC__)

#include "ecgpu_kernels.h"

namespace ecgpu {

// the secret scalar: sanitised copy and one flag byte
template <class C>
__global__ void __launch_bounds__(BLOCK)
k_pke_load(const uint8_t* __restrict__ s_in, size_t n, uint8_t* __restrict__ s_out, uint8_t* __restrict__ flag) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    flag[i] = pke_load_scalar<C>(s_out + i * 32, s_in + i * 32) ? 1 : 0;
}

// the public point: sanitised copy, its verdict ANDed into the flag byte k_pke_load wrote (branches on the point on purpose)
template <class C>
__global__ void __launch_bounds__(BLOCK)
k_pke_point(const uint8_t* __restrict__ xy_in, size_t n, uint8_t* __restrict__ xy_out, uint8_t* __restrict__ flag) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const bool ok = pke_load_point<C>(xy_out + i * 64, xy_in + i * 64);
    flag[i] = (uint8_t)(flag[i] & (ok ? 1 : 0));
}

template <class C>
__global__ void __launch_bounds__(BLOCK)
k_pke_seal(const uint8_t* __restrict__ x2y2, const uint8_t* __restrict__ flag, const uint8_t* __restrict__ msgs, size_t msg_len,
           size_t n, uint8_t* __restrict__ c1, uint8_t* __restrict__ c2, uint8_t* __restrict__ c3, uint8_t* __restrict__ ok) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    ok[i] = pke_seal_lane(x2y2 + i * 64, flag[i], msgs + i * msg_len, msg_len, c1 + i * 64, c2 + i * msg_len, c3 + i * 32,
                          pke_word_aligned(msgs, c2, msg_len)) ? 1 : 0;
}

template <class C>
__global__ void __launch_bounds__(BLOCK)
k_pke_open(const uint8_t* __restrict__ x2y2, const uint8_t* __restrict__ flag, const uint8_t* __restrict__ c2, size_t msg_len,
           const uint8_t* __restrict__ c3, size_t n, uint8_t* __restrict__ msgs_out, uint8_t* __restrict__ ok) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    ok[i] = pke_open_lane(x2y2 + i * 64, flag[i], c2 + i * msg_len, msg_len, c3 + i * 32, msgs_out + i * msg_len,
                          pke_word_aligned(c2, msgs_out, msg_len)) ? 1 : 0;
}

}  // namespace ecgpu

#endif  // __HIPCC__
