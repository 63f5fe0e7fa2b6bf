// ecgpu_sm2sign.h — batch SM2DSA signing (GB/T 32918.2 §6.1): the caller's nonce, the RFC 6979 nonce over HMAC-SM3, and messages
// (host + device algorithms, HIP kernels at the end).
//
// Reference counterparts: `sm2::dsa::SigningKey` — `sign_prehash_rfc6979` (sm2/src/dsa/signing.rs:213-258), `PrehashSigner::
// sign_prehash` (:122-126), `Signer::sign` (:162-174: e = SM3(Z || M), Z = `hash_z(distid, PA)`, PA = d G).
//     e = prehash mod n (`bytes2scalar`),  k = ONE candidate of RFC 6979 §3.2 over HMAC-SM3 (x = d, h1 = e, no additional data),
//     R = k G,  r = e + x(R) mod n,  s = (1 + d)^-1 (k - r d) mod n;  no signature when r = 0, r + k = 0, 1 + d = 0 or s = 0.
// There is no retry: the reference calls `fill_next_k` once and a candidate >= n is an `Error` (its source carries a TODO for the
// loop), so an element whose first candidate is outside [1, n) gets ok = 0.  (k = 0 is refused here; the reference's `from_repr`
// would take it.  Probability 2^-256 either way.)  The form with the caller's nonce is the standard's steps A3-A7 and is OURS: the
// reference has no such entry point.
//
// Both multiplications by the generator are k_fixed_base_ct (ecgpu_ct.h).  The rule of ecgpu_sign.h holds for the three kernels of
// this file: in k_sm2_sign_e, k_sm2_rfc6979 and k_sm2dsa_sign_finish no branch and no address depends on d, k, e or anything derived
// from them (tools/ct_isa_check.py --unit sm2sign); a value outside its range is replaced under a mask and its element gets ok = 0.
// (1 + d)^-1 is one branch-free division-step inversion per element, as k^-1 is for ECDSA.
#pragma once

#include "ecgpu_sign.h"
#include "ecgpu_sm3.h"

namespace ecgpu {

// the curve SM2DSA exists over (ecgpu_inst_sign.hip asks this instead of comparing ids)
template <class C>
struct Sm2Sign {
    ECGPU_CONST bool value = C::ID == CURVE_SM2;
};

// SM3 as the HMAC of Rfc6979 sees it: a 64-byte block, eight big-endian 32-bit words of state — the shape of SHA-256
struct SignHashSm3 {
    using Core = Sm3;
    using W = uint32_t;
    ECGPU_CONST int WB = 4, BB = Sm3::BLOCK_BYTES, LB = Sm3::LEN_BYTES, HW = 8;
    static ECGPU_HD void init(W* h) { Sm3::init(h); }
    static ECGPU_HD void put(W* w, int pos, uint32_t byte) { w[pos / WB] |= (W)byte << (8 * (WB - 1 - pos % WB)); }
    static ECGPU_HD uint32_t get(const W* w, int pos) { return (uint32_t)(w[pos / WB] >> (8 * (WB - 1 - pos % WB))) & 0xffu; }
};
template <class C>
using Sm2Rfc6979 = Rfc6979<C, 32, SignHashSm3>;

// the generator's one candidate: x = d as read, e_in the prehash as read (h1 = e mod n).  Writes the candidate, or 1 in place of one
// outside [1, n); returns its verdict.  No generator state is kept: there is no retry.
template <class C>
ECGPU_HD bool sm2_rfc6979_words(const uint32_t* x, const uint32_t* e_in, uint32_t* k_out) {
    constexpr int N = C::N;
    using G = Sm2Rfc6979<C>;
    uint32_t h1[N], k[N], one[N];
    ScalarN<C>::reduce_wire(h1, e_in);
    typename G::State st;
    const bool ok = G::first(st, k, x, h1);
    sg_one<N>(one);
    sg_sel<N>(k_out, ok, k, one);
    return ok;
}

// a - b mod n for a, b < n
template <class C>
ECGPU_HD void sm2_sub_mod(uint32_t* r, const uint32_t* a, const uint32_t* b) {
    constexpr int N = C::N;
    uint32_t t[N], u[N];
    const uint32_t borrow = mp_sub<N>(t, a, b);
    (void)mp_add<N>(u, t, C::ORDER);
    sg_sel<N>(r, borrow != 0, u, t);
}

// ---- SM2DSA: everything after R = k G ---------------------------------------------------------------------------------------
// d_in, k_in: the key and the nonce as read (any value); k_ok: the nonce's verdict (the load kernel's, or the generator's) — an
// invalid k was replaced by 1 before the multiplication and is replaced here the same way; e_in: the prehash as read (reduced
// here); rx: x(R), r_inf the identity flag of R (never set for 1 <= k < n).  Writes r and s (a zero record when not ok).
template <class C>
ECGPU_HD bool sm2dsa_sign_finish_words(const uint32_t* d_in, const uint32_t* k_in, bool k_ok, const uint32_t* e_in, const uint32_t* rx,
                                       bool r_inf, uint32_t* r_out, uint32_t* s_out) {
    using S = ScalarN<C>;
    using SS = SignScalar<C>;
    constexpr int N = C::N;
    uint32_t one[N], d[N], k[N], e[N], x[N], dp1[N];
    sg_one<N>(one);
    bool d_ok = SS::valid(d_in);
    sg_sel<N>(d, d_ok, d_in, one);
    SS::add(dp1, d, one);
    d_ok = (bool)((int)d_ok & (int)!S::is_zero(dp1));                 // d = n - 1: 1 + d has no inverse
    sg_sel<N>(d, d_ok, d, one);
    SS::add(dp1, d, one);
    k_ok = (bool)((int)k_ok & (int)SS::valid(k_in));
    sg_sel<N>(k, k_ok, k_in, one);
    S::reduce_wire(e, e_in);
    S::reduce_once(x, rx);                                            // x(R) in [n, p): p < 2n, one subtraction reduces it
    uint32_t r[N], rk[N], rd[N], num[N], inv[N], s[N];
    SS::add(r, e, x);
    SS::add(rk, r, k);
    S::mul(rd, r, d);
    sm2_sub_mod<C>(num, k, rd);
    S::inv(inv, dp1);                                                 // branch-free division steps
    S::mul(s, inv, num);
    const bool ok = (bool)((int)d_ok & (int)k_ok & (int)!r_inf & (int)!S::is_zero(r) & (int)!S::is_zero(rk) & (int)!S::is_zero(s));
    const uint32_t keep = sn_mask(ok);
#pragma unroll
    for (int i = 0; i < N; i++) {
        r_out[i] = r[i] & keep;
        s_out[i] = s[i] & keep;
    }
    return ok;
}

}  // namespace ecgpu

// =============================================================================================================================
#if defined(__HIPCC__)

#include "ecgpu_kernels.h"

namespace ecgpu {

// e = SM3(Z || M) of `Signer::sign(msg)`: pa_xy = the affine PA = d G that k_normalize wrote (of the sanitised d: an unusable key
// hashes G's and its element ends with ok = 0 in the finish kernel)
template <class C>
__global__ void __launch_bounds__(BLOCK)
k_sm2_sign_e(const uint8_t* __restrict__ distid, size_t distid_len, const uint8_t* __restrict__ pa_xy, const uint8_t* __restrict__ msgs,
             size_t msg_len, size_t n, uint8_t* __restrict__ e_out) {
    constexpr int N = C::N;
    static_assert(N == 8, "SM2DSA is defined over the 256-bit sm2 curve");
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t ew[N];
    Sm3::sm2_message_hash<C>(ew, distid, distid_len, pa_xy + i * 64, msgs + i * msg_len, msg_len);
    store_be_vec<N>(e_out + i * 32, ew);
}

// RFC 6979 §3.2 over HMAC-SM3 up to the first candidate, which is the only one.  x = the key as read (an out-of-range key hashes
// as it is: its element ends with ok = 0 whatever the nonce), h1 = e mod n.  Writes the candidate (1 in place of a rejected one)
// and the accepted flag.
template <class C>
__global__ void __launch_bounds__(BLOCK)
k_sm2_rfc6979(const uint8_t* __restrict__ d_in, const uint8_t* __restrict__ e_in, size_t n, uint8_t* __restrict__ k_out,
              uint8_t* __restrict__ flag) {
    constexpr int N = C::N;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t x[N], e[N], k[N];
    load_be_vec<N>(x, d_in + i * 32);
    load_be_vec<N>(e, e_in + i * 32);
    const bool ok = sm2_rfc6979_words<C>(x, e, k);
    store_be_vec<N>(k_out + i * 32, k);
    flag[i] = ok ? 1 : 0;
}

// r, s and ok from the affine R of k_normalize; sig = r || s
template <class C>
__global__ void __launch_bounds__(BLOCK)
k_sm2dsa_sign_finish(const uint8_t* __restrict__ d_in, const uint8_t* __restrict__ k_in, const uint8_t* __restrict__ k_flag,
                     const uint8_t* __restrict__ e_in, const uint8_t* __restrict__ r_xy, const uint8_t* __restrict__ r_inf, size_t n,
                     uint8_t* __restrict__ sig_out, uint8_t* __restrict__ ok_out) {
    constexpr int N = C::N;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t d[N], k[N], e[N], rx[N], r[N], s[N];
    load_be_vec<N>(d, d_in + i * 32);
    load_be_vec<N>(k, k_in + i * 32);
    load_be_vec<N>(e, e_in + i * 32);
    load_be_vec<N>(rx, r_xy + i * 64);
    const bool ok = sm2dsa_sign_finish_words<C>(d, k, k_flag[i] != 0, e, rx, r_inf[i] != 0, r, s);
    store_be_vec<N>(sig_out + i * 64, r);
    store_be_vec<N>(sig_out + i * 64 + 32, s);
    ok_out[i] = ok ? 1 : 0;
}

}  // namespace ecgpu

#endif  // __HIPCC__
