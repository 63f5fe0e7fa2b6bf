// ecgpu_sign.h — batch signing: ECDSA with the caller's nonce or the RFC 6979 nonce, and BIP340 Schnorr (host + device
// algorithms, HIP kernels at the end).
//
// Reference counterparts.  ECDSA: `ecdsa::hazmat::sign_prehashed` (the un-vendored `ecdsa` crate 0.17.0, Cargo.lock) as
// instantiated by `ecdsa::SigningKey<C>` in k256 / p256 / p384 / p224 / p521 / bp256 / bp384 — `new_signing_test!` at
// p256/src/ecdsa.rs:156-159 is the form with the caller's nonce, `PrehashSigner::sign_prehash` and `Signer::sign` take the nonce
// from RFC 6979 §3.2 (crate `rfc6979`, HMAC-DRBG over the curve's `DigestAlgorithm`), `NORMALIZE_S` is k256/src/ecdsa.rs:104-106:
//     R = k G,  r = x(R) mod n,  s = k^-1 (z + r d) mod n,  recovery id = (y(R) odd) | (x(R) >= n) << 1,
//     s > (n - 1) / 2 and NORMALIZE_S: s <- n - s and bit 0 of the recovery id flips.
// Schnorr: `SigningKey::sign_raw` (k256/src/schnorr/signing.rs:97-137) with the key fix-up of `From<NonZeroScalar>` (:146-167).
//
// Both multiplications by the generator are the uniform-schedule kernel k_fixed_base_ct (ecgpu_ct.h); what this file adds around
// it follows the rule of the `_ct` entry points: in k_rfc6979_first, k_schnorr_nonce, k_ecdsa_sign_finish, k_schnorr_sign_finish
// and k_sign_nonce_load no branch and no address depends on the bytes of a key, a nonce, a digest or anything derived from them
// (tools/ct_isa_check.py --unit sign); a value outside its range is replaced under a mask and its element gets ok = 0.
// (k_sign_hash_msg digests the MESSAGES of `Signer::sign`, which are public, with the producer of ecgpu_hash.h.)
// k^-1 is one branch-free division-step inversion per element (ModInv::invert -> divsteps_30, never divsteps_30_var): 21.5 k
// instructions beside the ~43 mixed additions of k G.  k_scalar_batch_inv (ecgpu_ecdsa.h) is NOT used: it skips elements by branch
// and was written for public s.
//
// The ONE deliberately variable-time piece is k_rfc6979_retry: it runs the HMAC-DRBG on for the elements whose first candidate was
// not in [1, n), so its trip count depends on the REJECTED candidates — which are never used, and which is exactly what the
// `loop` of the reference's `generate_k` reveals.  (The other variable-time piece of the path is the one every entry point has:
// `to_affine` of the public R in k_normalize.)
#pragma once

#include <type_traits>

#include "ecgpu_hash.h"
#include "ecgpu_scalar.h"
#include "ecgpu_sha256.h"

namespace ecgpu {

// candidates the RFC 6979 loop tries per element before it gives up (ok = 0); a conforming generator practically never gets
// past a handful (brainpool: 35-45 % of the elements reject once or more, twelve times at most in 2,000)
ECGPU_CONST int RFC6979_MAX_CANDIDATES = 128;

// ---- small helpers on N little-endian words ------------------------------------------------------------------------------
template <int N>
ECGPU_HD void sg_sel(uint32_t* r, bool c, const uint32_t* a, const uint32_t* b) {        // r = c ? a : b under an opaque mask (sn_mask)
    const uint32_t m = sn_mask(c);
#pragma unroll
    for (int i = 0; i < N; i++) r[i] = (a[i] & m) | (b[i] & ~m);
}
template <int N>
ECGPU_HD void sg_one(uint32_t* r) {
#pragma unroll
    for (int i = 0; i < N; i++) r[i] = i == 0 ? 1u : 0u;
}
// byte j (0 = most significant) of the L-byte big-endian encoding of a
template <int L>
ECGPU_HD uint32_t sg_be_byte(const uint32_t* a, int j) {
    const int pos = L - 1 - j;
    return (a[pos / 4] >> (8 * (pos % 4))) & 0xffu;
}

template <class C>
struct SignScalar {
    using S = ScalarN<C>;
    ECGPU_CONST int N = C::N;
    // 1 <= a < n, without a short circuit
    static ECGPU_HD bool valid(const uint32_t* a) { return (bool)((int)!S::is_zero(a) & (int)S::in_range(a)); }
    // a + b mod n for a, b < n
    static ECGPU_HD void add(uint32_t* r, const uint32_t* a, const uint32_t* b) {
        uint32_t t[N], d[N];
        const uint32_t carry = mp_add<N>(t, a, b);
        const uint32_t borrow = mp_sub<N>(d, t, C::ORDER);
        const bool use_d = (bool)((int)(carry != 0) | (int)(borrow == 0));
        sg_sel<N>(r, use_d, d, t);
    }
    // n - a for 1 <= a < n  (0 -> n, which no caller keeps)
    static ECGPU_HD void neg(uint32_t* r, const uint32_t* a) { (void)mp_sub<N>(r, C::ORDER, a); }
};

// ---- SHA-2 by digest size, as the HMAC below needs it ---------------------------------------------------------------------
template <int D>
struct SignHash {
    ECGPU_CONST bool WIDE = D == HASH_SHA384 || D == HASH_SHA512;
    using Core = typename std::conditional<WIDE, Sha512Core, Sha256Core>::type;
    using W = typename Core::word_t;
    ECGPU_CONST int WB = (int)sizeof(W), BB = Core::BLOCK_BYTES, LB = Core::LEN_BYTES;
    ECGPU_CONST int HW = D / WB;                         // digest words (28 / 4, 32 / 4, 48 / 8, 64 / 8: all whole)
    static ECGPU_HD void init(W* h) {
        if constexpr (D == HASH_SHA224) Core::init224(h);
        else if constexpr (D == HASH_SHA256) Core::init256(h);
        else if constexpr (D == HASH_SHA384) Core::init384(h);
        else Core::init512(h);
    }
    // byte `pos` of a message held as big-endian words
    static ECGPU_HD void put(W* w, int pos, uint32_t byte) { w[pos / WB] |= (W)byte << (8 * (WB - 1 - pos % WB)); }
    static ECGPU_HD uint32_t get(const W* w, int pos) { return (uint32_t)(w[pos / WB] >> (8 * (WB - 1 - pos % WB))) & 0xffu; }
};

// ---- HMAC-DRBG of RFC 6979 §3.2 -------------------------------------------------------------------------------------------
// State: K and V, HW digest words each.  One `step` is one HMAC under K:
//     DRBG_K_LONG   K <- HMAC_K(V || sep || x || h1)        (steps d and f; x = int2octets(d), h1 = bits2octets(digest))
//     DRBG_K_SHORT  K <- HMAC_K(V || 0x00)                  (step h.3, after a rejected candidate)
//     DRBG_V        V <- HMAC_K(V)
// Every message fits two blocks behind the key block (197 bytes at most: p521 with SHA-512), so an HMAC is at most five
// compressions — key ^ ipad, one or two message blocks, key ^ opad, the inner digest — issued by ONE loop with ONE call site of
// the compression function (ecgpu_hash.h:26-27), and the callers below drive `step` from a loop of their own: the function is
// inlined once per kernel.  Which blocks a step has depends on `kind`, which is a loop counter, never on data.
enum : int { DRBG_K_LONG = 0, DRBG_K_SHORT = 1, DRBG_V = 2 };

// HT: the hash as the HMAC sees it (SignHash<D>; SignHashSm3 of ecgpu_sm2sign.h for SM2DSA, whose digest is D = 32 bytes too)
template <class C, int D = EcdsaDigest<C>::value, class HT = SignHash<D>>
struct Rfc6979 {
    using H = HT;
    using W = typename H::W;
    ECGPU_CONST int N = C::N, L = WireBytes<C>::value, HW = H::HW, BB = H::BB, WB = H::WB;
    ECGPU_CONST int NV = (L + D - 1) / D;                // HMAC outputs per candidate: 2 for p521 (64 < 66), else 1
    ECGPU_CONST int SHIFT = C::ID == CURVE_P521 ? 7 : 0; // 8 L - bitlen(n): bits2int drops the low bits of the L bytes taken
    static_assert(D + 1 + 2 * L + 1 + H::LB <= 2 * BB, "an HMAC-DRBG message is at most two blocks");
    static_assert(D + 1 + 1 + H::LB <= BB, "V || 0x00 fits one block");
    static_assert(NV <= 2, "a candidate is at most two HMAC outputs");

    struct State {
        W k[HW], v[HW];
    };

    template <int LEN>
    static ECGPU_HD int close(W* m) {                    // padding of a LEN-byte message behind the 1-block key prefix
        constexpr int NB = (LEN + 1 + H::LB + BB - 1) / BB;
        H::put(m, LEN, 0x80u);
        m[16 * NB - 1] |= (W)((BB + LEN) * 8);
        return NB;
    }

    static ECGPU_HD void step(State& st, int kind, uint32_t sep, const uint32_t* x, const uint32_t* h1) {
        W m[32];
#pragma unroll
        for (int j = 0; j < 32; j++) m[j] = 0;
#pragma unroll
        for (int j = 0; j < HW; j++) m[j] = st.v[j];
        int nb;
        if (kind == DRBG_V) {
            nb = close<D>(m);
        } else if (kind == DRBG_K_SHORT) {
            nb = close<D + 1>(m);                        // (the separator 0x00 is already there)
        } else {
            H::put(m, D, sep);
#pragma unroll
            for (int j = 0; j < L; j++) {
                H::put(m, D + 1 + j, sg_be_byte<L>(x, j));
                H::put(m, D + 1 + L + j, sg_be_byte<L>(h1, j));
            }
            nb = close<D + 1 + 2 * L>(m);
        }
        W s[8], inner[HW];
#pragma unroll
        for (int j = 0; j < HW; j++) inner[j] = 0;
#pragma unroll 1
        for (int t = 0; t < 5; t++) {                    // 0: key ^ ipad, 1 / 2: message, 3: key ^ opad, 4: inner digest
            if (t == 2 && nb == 1) continue;
            W w[16];
            if (t == 0 || t == 3) {
                const W pad = (W)(t == 0 ? 0x3636363636363636ull : 0x5c5c5c5c5c5c5c5cull);
#pragma unroll
                for (int j = 0; j < 16; j++) w[j] = (j < HW ? st.k[j] : (W)0) ^ pad;
                H::init(s);
            } else if (t == 4) {
#pragma unroll
                for (int j = 0; j < 16; j++) w[j] = j < HW ? inner[j] : (W)0;
                w[HW] = (W)0x80u << (8 * (WB - 1));
                w[15] = (W)((BB + D) * 8);
            } else {
#pragma unroll
                for (int j = 0; j < 16; j++) w[j] = t == 1 ? m[j] : m[16 + j];
            }
            H::Core::compress(s, w);
#pragma unroll
            for (int j = 0; j < HW; j++) inner[j] = t < 3 ? s[j] : inner[j];      // the inner digest, kept across the opad block
        }
        const bool to_k = kind != DRBG_V;                // (a loop counter's property, not data)
#pragma unroll
        for (int j = 0; j < HW; j++) {
            st.k[j] = to_k ? s[j] : st.k[j];
            st.v[j] = to_k ? st.v[j] : s[j];
        }
    }

    // bits2int of the candidate bytes T = t[0 .. L) (big-endian words of NV HMAC outputs): the L bytes as an integer, shifted right
    static ECGPU_HD void candidate(uint32_t* k, const W* t) {
        uint32_t c[N + 1];
#pragma unroll
        for (int i = 0; i <= N; i++) c[i] = 0;
#pragma unroll
        for (int j = 0; j < L; j++) {
            const int pos = L - 1 - j;
            c[pos / 4] |= H::get(t, j) << (8 * (pos % 4));
        }
#pragma unroll
        for (int i = 0; i < N; i++) {
            if constexpr (SHIFT != 0) k[i] = (c[i] >> SHIFT) | (c[i + 1] << (32 - SHIFT));
            else k[i] = c[i];
        }
    }

    // steps b-g and the first pass of h: the state after it, the first candidate and whether it is in [1, n).  Branch-free in
    // the data: the loop below runs 4 + NV steps whatever x and h1 are.
    static ECGPU_HD bool first(State& st, uint32_t* k, const uint32_t* x, const uint32_t* h1) {
#pragma unroll
        for (int j = 0; j < HW; j++) {
            st.k[j] = 0;
            st.v[j] = (W)0x0101010101010101ull;
        }
        W t[2 * HW];
#pragma unroll
        for (int j = 0; j < 2 * HW; j++) t[j] = 0;
#pragma unroll 1
        for (int op = 0; op < 4 + NV; op++) {
            const int kind = op < 4 && (op & 1) == 0 ? DRBG_K_LONG : DRBG_V;
            step(st, kind, op == 2 ? 1u : 0u, x, h1);
            const bool second = op == 5;                  // the second output of a two-output candidate (NV == 2: p521)
#pragma unroll
            for (int j = 0; j < HW; j++) {                // (the last NV outputs are the candidate; earlier ones are overwritten)
                t[HW + j] = second ? st.v[j] : t[HW + j];
                t[j] = second ? t[j] : st.v[j];
            }
        }
        candidate(k, t);
        return SignScalar<C>::valid(k);
    }

    // the next candidate after a rejected one (step h.3 and h again); called by the retry loop only
    static ECGPU_HD bool next(State& st, uint32_t* k, const uint32_t* x, const uint32_t* h1) {
        W t[2 * HW];
#pragma unroll
        for (int j = 0; j < 2 * HW; j++) t[j] = 0;
#pragma unroll 1
        for (int op = 0; op < 2 + NV; op++) {
            step(st, op == 0 ? DRBG_K_SHORT : DRBG_V, 0u, x, h1);
            const bool second = op == 3;                  // (NV == 2)
#pragma unroll
            for (int j = 0; j < HW; j++) {
                t[HW + j] = second ? st.v[j] : t[HW + j];
                t[j] = second ? t[j] : st.v[j];
            }
        }
        candidate(k, t);
        return SignScalar<C>::valid(k);
    }

    // the whole of `generate_k` for one element (the host twin and the tests; the device splits it over two kernels): candidates
    // tried (the accepted one included) or 0 when `cap` candidates were all rejected
    static ECGPU_HD int generate(uint32_t* k, const uint32_t* x, const uint32_t* h1, int cap) {
        State st;
        bool ok = first(st, k, x, h1);
        int tried = 1;
        while (!ok && tried < cap) {
            ok = next(st, k, x, h1);
            tried++;
        }
        return ok ? tried : 0;
    }
};

// ---- ECDSA: everything after R = k G ----------------------------------------------------------------------------------------
// d, k: the key and the nonce as read (any value); k_ok: the nonce's verdict (1 <= k < n, or the generator's accepted flag) — an
// invalid k was replaced by 1 before the multiplication and is replaced here the same way; z: the prehash as read (reduced here);
// (rx, ry): affine R, r_inf its identity flag (never set for 1 <= k < n).  Writes r, s, the recovery id; returns ok.
template <class C>
ECGPU_HD bool ecdsa_sign_finish_words(const uint32_t* d_in, const uint32_t* k_in, bool k_ok, const uint32_t* z_in, const uint32_t* rx,
                                      const uint32_t* ry, bool r_inf, int normalize_s, uint32_t* r_out, uint32_t* s_out,
                                      uint32_t* recid_out) {
    using S = ScalarN<C>;
    using SS = SignScalar<C>;
    constexpr int N = C::N;
    uint32_t one[N], d[N], k[N], z[N], r[N];
    sg_one<N>(one);
    const bool d_ok = SS::valid(d_in);
    k_ok = (bool)((int)k_ok & (int)SS::valid(k_in));
    sg_sel<N>(d, d_ok, d_in, one);
    sg_sel<N>(k, k_ok, k_in, one);
    S::reduce_wire(z, z_in);
    const bool x_high = mp_geq<N>(rx, C::ORDER);                      // x(R) >= n: p < 2n, one subtraction reduces it
    S::reduce_once(r, rx);
    uint32_t rd[N], sum[N], kinv[N], s[N], sneg[N];
    S::mul(rd, r, d);
    SS::add(sum, z, rd);
    S::inv(kinv, k);                                                  // branch-free division steps
    S::mul(s, kinv, sum);
    const bool flip = (bool)((int)(normalize_s != 0) & (int)S::is_high(s));
    SS::neg(sneg, s);
    sg_sel<N>(s, flip, sneg, s);
    const uint32_t recid = ((ry[0] & 1u) ^ (uint32_t)flip) | ((uint32_t)x_high << 1);
    const bool ok = (bool)((int)d_ok & (int)k_ok & (int)!r_inf & (int)!S::is_zero(r) & (int)!S::is_zero(s));
    const uint32_t keep = sn_mask(ok);
#pragma unroll
    for (int i = 0; i < N; i++) {
        r_out[i] = r[i] & keep;
        s_out[i] = s[i] & keep;
    }
    *recid_out = recid & keep;
    return ok;
}

// z = bits2field(digest): the leftmost min(D, L) bytes of the digest as an integer of L bytes (ecdsa `hazmat::bits2field`)
template <class C, int D>
ECGPU_HD void bits2field_words(uint32_t* z, const uint8_t* digest) {
    constexpr int N = C::N, L = WireBytes<C>::value, TAKE = D < L ? D : L;
#pragma unroll
    for (int j = 0; j < N; j++) z[j] = 0;
#pragma unroll
    for (int j = 0; j < TAKE; j++) {
        const int pos = TAKE - 1 - j;
        z[pos / 4] |= (uint32_t)digest[j] << (8 * (pos % 4));
    }
}

// ---- BIP340 ---------------------------------------------------------------------------------------------------------------
struct Bip340 {
    // states after the block SHA256(tag) || SHA256(tag)   (tests/sign_model.py recomputes them)
    ECGPU_CONST uint32_t AUX_MIDSTATE[8] = {0x24DD3219u, 0x4EBA7E70u, 0xCA0FABB9u, 0x0FA3166Du,
                                            0x3AFBE4B1u, 0x4C44DF97u, 0x4AAC2739u, 0x249E850Au};
    ECGPU_CONST uint32_t NONCE_MIDSTATE[8] = {0x46615B35u, 0xF4BFBFF7u, 0x9F8DC671u, 0x83627AB3u,
                                              0x60217180u, 0x57358661u, 0x21A29E54u, 0x68B07B4Cu};

    // SHA256(tag block || a [|| b] || m) from the tag's midstate: a, b are 256-bit values as 8 little-endian words each (hashed
    // big-endian), m is msg_len bytes.  NPRE = 1: a and no message (the aux hash); 2: a || b || m (the nonce hash t || x(P) || m
    // and the challenge x(R) || x(P) || m).  Result as 8 little-endian words of the big-endian integer.  One call site of the
    // compression function; the block count depends on msg_len alone.
    template <int NPRE>
    static ECGPU_HD void tagged(uint32_t* out, const uint32_t* midstate, const uint32_t* a, const uint32_t* b, const uint8_t* m,
                                size_t msg_len) {
        uint32_t h[8];
#pragma unroll
        for (int i = 0; i < 8; i++) h[i] = midstate[i];
        constexpr size_t PRE = 32 * NPRE;
        const size_t total = PRE + msg_len;                       // bytes behind the tag block
        const uint64_t bitlen = (uint64_t)(64 + total) * 8;
        const size_t nblocks = (total + 9 + 63) / 64;
#pragma unroll 1
        for (size_t blk = 0; blk < nblocks; blk++) {
            uint32_t w[16];
#pragma unroll
            for (int j = 0; j < 16; j++) {
                const size_t o = blk * 64 + (size_t)j * 4;        // the word's first byte
                uint32_t word = 0;
                if (o + 4 <= PRE) {                               // (a position, not data)
                    uint32_t wb = 0;
                    if constexpr (NPRE >= 2) wb = b[7 - (j & 7)];
                    word = o < 32 ? a[7 - (j & 7)] : wb;
                } else {
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        const size_t p = o + q;
                        uint32_t byte = 0;
                        if (p < total) byte = m[p - PRE];
                        else if (p == total) byte = 0x80u;
                        else if (p >= nblocks * 64 - 8) byte = (uint32_t)(bitlen >> (8 * (nblocks * 64 - 1 - p))) & 0xffu;
                        word = (word << 8) | byte;
                    }
                }
                w[j] = word;
            }
            Sha256::compress(h, w);
        }
#pragma unroll
        for (int i = 0; i < 8; i++) out[i] = h[7 - i];
    }
};

// the key fix-up and the nonce of `sign_raw`: d_in the secret key as read, (px, py) = d G (of the sanitised d), aux 32 bytes as 8
// little-endian words of the big-endian value.  Writes d' (n - d when y(P) is odd) and the nonce k (1 in place of an unusable
// one); returns whether both are usable (1 <= d < n and k != 0).
template <class C>
ECGPU_HD bool schnorr_nonce_words(const uint32_t* d_in, const uint32_t* px, const uint32_t* py, const uint32_t* aux,
                                  const uint8_t* msg, size_t msg_len, uint32_t* d_out, uint32_t* k_out) {
    using S = ScalarN<C>;
    using SS = SignScalar<C>;
    constexpr int N = C::N;
    static_assert(N == 8 && C::A_IS_ZERO, "BIP340 is defined over secp256k1");
    uint32_t one[N], d[N], dn[N], t[N], k[N];
    sg_one<N>(one);
    const bool d_ok = SS::valid(d_in);
    sg_sel<N>(d, d_ok, d_in, one);
    SS::neg(dn, d);
    sg_sel<N>(d, (py[0] & 1u) != 0u, dn, d);
    Bip340::tagged<1>(t, Bip340::AUX_MIDSTATE, aux, nullptr, nullptr, 0);
#pragma unroll
    for (int i = 0; i < N; i++) t[i] ^= d[i];
    Bip340::tagged<2>(k, Bip340::NONCE_MIDSTATE, t, px, msg, msg_len);
    S::reduce_once(k, k);
    const bool k_ok = !S::is_zero(k);
    sg_sel<N>(k_out, k_ok, k, one);
#pragma unroll
    for (int i = 0; i < N; i++) d_out[i] = d[i];
    return (bool)((int)d_ok & (int)k_ok);
}
// everything after R = k G: the parity fix of k, the challenge, s = k + e d.  d, k: the outputs of schnorr_nonce_words; usable
// its verdict.  Writes x(R) and s (a zero record when not ok).
template <class C>
ECGPU_HD bool schnorr_sign_finish_words(const uint32_t* d, const uint32_t* k_in, bool usable, const uint32_t* px, const uint32_t* rx,
                                        const uint32_t* ry, bool r_inf, const uint8_t* msg, size_t msg_len, uint32_t* r_out,
                                        uint32_t* s_out) {
    using S = ScalarN<C>;
    using SS = SignScalar<C>;
    constexpr int N = C::N;
    uint32_t k[N], kn[N], e[N], ed[N], s[N];
    SS::neg(kn, k_in);
    sg_sel<N>(k, (ry[0] & 1u) != 0u, kn, k_in);
    Bip340::tagged<2>(e, Sha256::BIP340_CHALLENGE_MIDSTATE, rx, px, msg, msg_len);
    S::reduce_once(e, e);
    S::mul(ed, e, d);
    SS::add(s, k, ed);
    const bool ok = (bool)((int)usable & (int)!r_inf & (int)!S::is_zero(s));
    const uint32_t keep = sn_mask(ok);
#pragma unroll
    for (int i = 0; i < N; i++) {
        r_out[i] = rx[i] & keep;
        s_out[i] = s[i] & keep;
    }
    return ok;
}

}  // namespace ecgpu

// =============================================================================================================================
#if defined(__HIPCC__)

#include "ecgpu_kernels.h"

namespace ecgpu {

// the caller's nonce (and the Schnorr key before d G): k as read -> k or, outside [1, n), 1; flag = its verdict
template <class C>
__global__ void __launch_bounds__(BLOCK)
k_sign_nonce_load(const uint8_t* __restrict__ k_in, size_t n, uint8_t* __restrict__ k_out, uint8_t* __restrict__ flag) {
    constexpr int N = C::N, WB = WireBytes<C>::value;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t k[N], one[N];
    load_wire<C>(k, k_in + i * WB);
    sg_one<N>(one);
    const bool ok = SignScalar<C>::valid(k);
    sg_sel<N>(k, ok, k, one);
    store_wire<C>(k_out + i * WB, k);
    flag[i] = ok ? 1 : 0;
}

// z = bits2field(digest of message i) for `Signer::sign(msg)`
template <class C>
__global__ void __launch_bounds__(BLOCK)
k_sign_hash_msg(const uint8_t* __restrict__ msgs, size_t msg_len, size_t n, uint8_t* __restrict__ z_out) {
    constexpr int N = C::N, WB = WireBytes<C>::value, D = EcdsaDigest<C>::value;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if constexpr (D != 0) {
        uint8_t digest[D];
        const HashPiece one[1] = {{msgs + i * msg_len, msg_len}};
        sha2_pieces<D, 1>(digest, one);
        uint32_t zw[N];
        bits2field_words<C, D>(zw, digest);
        store_wire<C>(z_out + i * WB, zw);
    }
}

// The generator's state between k_rfc6979_first and k_rfc6979_retry: K then V, HW digest words each (32-bit words for SHA-224 / 256,
// 64-bit ones for SHA-384 / 512), word-major — word j of element i at [j * n + i] — so that a wave's loads and stores of one word
// are contiguous.
template <class C>
constexpr size_t rfc6979_state_bytes_of() {
    if constexpr (EcdsaDigest<C>::value != 0) return 2 * Rfc6979<C>::HW * sizeof(typename Rfc6979<C>::W);
    else return 0;
}

// RFC 6979 §3.2 up to the first candidate.  x = the key as read (an out-of-range key hashes as it is: its element ends with
// ok = 0 whatever the nonce), h1 = z mod n.  Writes the candidate (1 in place of a rejected one), the accepted flag and the
// generator's state.
template <class C>
__global__ void __launch_bounds__(BLOCK)
k_rfc6979_first(const uint8_t* __restrict__ d_in, const uint8_t* __restrict__ z_in, size_t n, uint8_t* __restrict__ k_out,
                uint8_t* __restrict__ flag, void* __restrict__ state) {
    constexpr int N = C::N, WB = WireBytes<C>::value;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if constexpr (EcdsaDigest<C>::value != 0) {
        using G = Rfc6979<C>;
        uint32_t x[N], z[N], h1[N], k[N], one[N];
        load_wire<C>(x, d_in + i * WB);
        load_wire<C>(z, z_in + i * WB);
        ScalarN<C>::reduce_wire(h1, z);
        typename G::State st;
        const bool ok = G::first(st, k, x, h1);
        sg_one<N>(one);
        sg_sel<N>(k, ok, k, one);
        store_wire<C>(k_out + i * WB, k);
        flag[i] = ok ? 1 : 0;
        typename G::W* sp = static_cast<typename G::W*>(state);
#pragma unroll
        for (int j = 0; j < G::HW; j++) {
            sp[(size_t)j * n + i] = st.k[j];
            sp[(size_t)(G::HW + j) * n + i] = st.v[j];
        }
    }
}

// VARIABLE TIME ON PURPOSE (see the head of this file): the generator run on for the elements whose flag is clear, until a
// candidate is in [1, n) or `cap` candidates (the first one counted) were rejected.  Launched once per call; lanes whose first
// candidate was accepted leave at once.
template <class C>
__global__ void __launch_bounds__(BLOCK)
k_rfc6979_retry(const uint8_t* __restrict__ d_in, const uint8_t* __restrict__ z_in, size_t n, int cap, uint8_t* __restrict__ k_out,
                uint8_t* __restrict__ flag, const void* __restrict__ state) {
    constexpr int N = C::N, WB = WireBytes<C>::value;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if constexpr (EcdsaDigest<C>::value != 0) {
        using G = Rfc6979<C>;
        using W = typename G::W;
        if (flag[i]) return;
        uint32_t x[N], z[N], h1[N], k[N];
        load_wire<C>(x, d_in + i * WB);
        load_wire<C>(z, z_in + i * WB);
        ScalarN<C>::reduce_wire(h1, z);
        typename G::State st;
        const W* sp = static_cast<const W*>(state);
#pragma unroll
        for (int j = 0; j < G::HW; j++) {
            st.k[j] = sp[(size_t)j * n + i];
            st.v[j] = sp[(size_t)(G::HW + j) * n + i];
        }
        bool ok = false;
#pragma unroll 1
        for (int tried = 1; tried < cap && !ok; tried++) ok = G::next(st, k, x, h1);
        if (ok) {
            store_wire<C>(k_out + i * WB, k);
            flag[i] = 1;
        }
    }
}

// r, s, recovery id and ok from the affine R of k_normalize; sig = r || s
template <class C>
__global__ void __launch_bounds__(BLOCK)
k_ecdsa_sign_finish(const uint8_t* __restrict__ d_in, const uint8_t* __restrict__ k_in, const uint8_t* __restrict__ k_flag,
                    const uint8_t* __restrict__ z_in, const uint8_t* __restrict__ r_xy, const uint8_t* __restrict__ r_inf, size_t n,
                    int normalize_s, uint8_t* __restrict__ sig_out, uint8_t* __restrict__ recid_out, uint8_t* __restrict__ ok_out) {
    constexpr int N = C::N, WB = WireBytes<C>::value;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t d[N], k[N], z[N], rx[N], ry[N], r[N], s[N], recid;
    load_wire<C>(d, d_in + i * WB);
    load_wire<C>(k, k_in + i * WB);
    load_wire<C>(z, z_in + i * WB);
    load_wire<C>(rx, r_xy + i * (2 * WB));
    load_wire<C>(ry, r_xy + i * (2 * WB) + WB);
    const bool ok = ecdsa_sign_finish_words<C>(d, k, k_flag[i] != 0, z, rx, ry, r_inf[i] != 0, normalize_s, r, s, &recid);
    store_wire<C>(sig_out + i * (2 * WB), r);
    store_wire<C>(sig_out + i * (2 * WB) + WB, s);
    recid_out[i] = (uint8_t)recid;
    ok_out[i] = ok ? 1 : 0;
}

// BIP340: d' || x(P) into dp_out (64 bytes per element), the nonce into k_out, the verdict so far into flag
template <class C>
__global__ void __launch_bounds__(BLOCK)
k_schnorr_nonce(const uint8_t* __restrict__ sk, const uint8_t* __restrict__ p_xy, const uint8_t* __restrict__ aux,
                const uint8_t* __restrict__ msgs, size_t msg_len, size_t n, uint8_t* __restrict__ dp_out, uint8_t* __restrict__ k_out,
                uint8_t* __restrict__ flag) {
    constexpr int N = C::N;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t d[N], px[N], py[N], a[N], dd[N], k[N];
    load_be_vec<N>(d, sk + i * 32);
    load_be_vec<N>(px, p_xy + i * 64);
    load_be_vec<N>(py, p_xy + i * 64 + 32);
    load_be_vec<N>(a, aux + i * 32);
    const bool ok = schnorr_nonce_words<C>(d, px, py, a, msgs + i * msg_len, msg_len, dd, k);
    store_be_vec<N>(dp_out + i * 64, dd);
    store_be_vec<N>(dp_out + i * 64 + 32, px);
    store_be_vec<N>(k_out + i * 32, k);
    flag[i] = ok ? 1 : 0;
}

template <class C>
__global__ void __launch_bounds__(BLOCK)
k_schnorr_sign_finish(const uint8_t* __restrict__ dp, const uint8_t* __restrict__ k_in, const uint8_t* __restrict__ flag,
                      const uint8_t* __restrict__ r_xy, const uint8_t* __restrict__ r_inf, const uint8_t* __restrict__ msgs,
                      size_t msg_len, size_t n, uint8_t* __restrict__ sig_out, uint8_t* __restrict__ ok_out) {
    constexpr int N = C::N;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t d[N], px[N], k[N], rx[N], ry[N], r[N], s[N];
    load_be_vec<N>(d, dp + i * 64);
    load_be_vec<N>(px, dp + i * 64 + 32);
    load_be_vec<N>(k, k_in + i * 32);
    load_be_vec<N>(rx, r_xy + i * 64);
    load_be_vec<N>(ry, r_xy + i * 64 + 32);
    const bool ok = schnorr_sign_finish_words<C>(d, k, flag[i] != 0, px, rx, ry, r_inf[i] != 0, msgs + i * msg_len, msg_len, r, s);
    store_be_vec<N>(sig_out + i * 64, r);
    store_be_vec<N>(sig_out + i * 64 + 32, s);
    ok_out[i] = ok ? 1 : 0;
}

}  // namespace ecgpu

#endif  // __HIPCC__
