// ecgpu_inst_sign.hip — instantiates the signing kernels (ecgpu_sign.h) for -DECGPU_CURVE=...; a translation unit of its own so
// that tools/ct_isa_check.py --unit sign can look at exactly these kernels, and so that the HMAC bodies build beside the rest
#include "ecgpu_sign.h"
#include "ecgpu_pke.h"
#include "ecgpu_sm2sign.h"
#include "ecgpu_bignsign.h"
#include "ecgpu_launch.h"

namespace ecgpu {

using CurveT = ECGPU_CURVE;

namespace {
inline unsigned sign_grid(size_t n) { return (unsigned)((n + BLOCK - 1) / BLOCK); }

// BIP340 exists over secp256k1 only: the other curves' translation units hold no Schnorr kernel
template <class C>
void schnorr_nonce_impl(hipStream_t s, const uint8_t* sk, const uint8_t* p_xy, const uint8_t* aux, const uint8_t* msgs, size_t msg_len,
                        size_t n, uint8_t* dp_out, uint8_t* k_out, uint8_t* flag) {
    if constexpr (C::ID == CURVE_K256)
        hipLaunchKernelGGL(k_schnorr_nonce<C>, dim3(sign_grid(n)), dim3(BLOCK), 0, s, sk, p_xy, aux, msgs, msg_len, n, dp_out, k_out, flag);
}
template <class C>
void schnorr_finish_impl(hipStream_t s, const uint8_t* dp, const uint8_t* k, const uint8_t* flag, const uint8_t* r_xy,
                         const uint8_t* r_inf, const uint8_t* msgs, size_t msg_len, size_t n, uint8_t* sig, uint8_t* ok) {
    if constexpr (C::ID == CURVE_K256)
        hipLaunchKernelGGL(k_schnorr_sign_finish<C>, dim3(sign_grid(n)), dim3(BLOCK), 0, s, dp, k, flag, r_xy, r_inf, msgs, msg_len, n,
                           sig, ok);
}

// SM2 public-key encryption exists over the sm2 curve with SM3 only (ecgpu_pke.h): the other curves' translation units hold none of
// its kernels
template <class C>
void pke_load_impl(hipStream_t s, const uint8_t* s_in, const uint8_t* xy_in, size_t n, uint8_t* s_out, uint8_t* xy_out, uint8_t* flag) {
    if constexpr (C::ID == CURVE_SM2) {
        hipLaunchKernelGGL(k_pke_load<C>, dim3(sign_grid(n)), dim3(BLOCK), 0, s, s_in, n, s_out, flag);
        hipLaunchKernelGGL(k_pke_point<C>, dim3(sign_grid(n)), dim3(BLOCK), 0, s, xy_in, n, xy_out, flag);
    }
}
template <class C>
void pke_seal_impl(hipStream_t s, const uint8_t* x2y2, const uint8_t* flag, const uint8_t* msgs, size_t msg_len, size_t n, uint8_t* c1,
                   uint8_t* c2, uint8_t* c3, uint8_t* ok) {
    if constexpr (C::ID == CURVE_SM2)
        hipLaunchKernelGGL(k_pke_seal<C>, dim3(sign_grid(n)), dim3(BLOCK), 0, s, x2y2, flag, msgs, msg_len, n, c1, c2, c3, ok);
}
template <class C>
void pke_open_impl(hipStream_t s, const uint8_t* x2y2, const uint8_t* flag, const uint8_t* c2, size_t msg_len, const uint8_t* c3,
                   size_t n, uint8_t* msgs_out, uint8_t* ok) {
    if constexpr (C::ID == CURVE_SM2)
        hipLaunchKernelGGL(k_pke_open<C>, dim3(sign_grid(n)), dim3(BLOCK), 0, s, x2y2, flag, c2, msg_len, c3, n, msgs_out, ok);
}

// SM2DSA signing exists over the sm2 curve with SM3 only (ecgpu_sm2sign.h): the other curves' translation units hold none of its
// kernels
template <class C>
void sm2_sign_e_impl(hipStream_t s, const uint8_t* distid, size_t distid_len, const uint8_t* pa_xy, const uint8_t* msgs, size_t msg_len,
                     size_t n, uint8_t* e_out) {
    if constexpr (Sm2Sign<C>::value)
        hipLaunchKernelGGL(k_sm2_sign_e<C>, dim3(sign_grid(n)), dim3(BLOCK), 0, s, distid, distid_len, pa_xy, msgs, msg_len, n, e_out);
}
template <class C>
void sm2_rfc6979_impl(hipStream_t s, const uint8_t* d, const uint8_t* e, size_t n, uint8_t* k_out, uint8_t* flag) {
    if constexpr (Sm2Sign<C>::value) hipLaunchKernelGGL(k_sm2_rfc6979<C>, dim3(sign_grid(n)), dim3(BLOCK), 0, s, d, e, n, k_out, flag);
}
template <class C>
void sm2dsa_sign_finish_impl(hipStream_t s, const uint8_t* d, const uint8_t* k, const uint8_t* k_flag, const uint8_t* e,
                             const uint8_t* r_xy, const uint8_t* r_inf, size_t n, uint8_t* sig, uint8_t* ok) {
    if constexpr (Sm2Sign<C>::value)
        hipLaunchKernelGGL(k_sm2dsa_sign_finish<C>, dim3(sign_grid(n)), dim3(BLOCK), 0, s, d, k, k_flag, e, r_xy, r_inf, n, sig, ok);
}

// bign signing exists over bign-curve256v1 with belt only (ecgpu_bignsign.h): the other curves' translation units hold none of its
// kernels
template <class C>
void bign_genk_impl(hipStream_t s, const uint8_t* d, const uint8_t* h, const uint32_t* bound, size_t n, int cap, uint8_t* k_out,
                    uint8_t* flag, uint32_t* state) {
    if constexpr (BignSign<C>::value) {
        BignBound b;
        for (int j = 0; j < 8; j++) b.w[j] = bound[j];
        hipLaunchKernelGGL(k_bign_genk<C>, dim3(sign_grid(n)), dim3(BLOCK), 0, s, d, h, b, n, k_out, flag, state);
        hipLaunchKernelGGL(k_bign_genk_retry<C>, dim3(sign_grid(n)), dim3(BLOCK), 0, s, b, n, cap, k_out, flag, state);
    }
}
template <class C>
void bign_sign_s0_impl(hipStream_t s, const uint8_t* h, const uint8_t* r_xy, size_t n, uint8_t* s0_out) {
    if constexpr (BignSign<C>::value) hipLaunchKernelGGL(k_bign_sign_s0<C>, dim3(sign_grid(n)), dim3(BLOCK), 0, s, h, r_xy, n, s0_out);
}
template <class C>
void bign_sign_finish_impl(hipStream_t s, const uint8_t* d, const uint8_t* k, const uint8_t* k_flag, const uint8_t* h, const uint8_t* s0,
                           size_t s0_stride, const uint8_t* r_inf, size_t n, uint8_t* sig, uint8_t* ok) {
    if constexpr (BignSign<C>::value)
        hipLaunchKernelGGL(k_bign_sign_finish<C>, dim3(sign_grid(n)), dim3(BLOCK), 0, s, d, k, k_flag, h, s0, s0_stride, r_inf, n, sig, ok);
}
}  // namespace

template <> void launch_sign_nonce_load<CurveT>(hipStream_t s, const uint8_t* k_in, size_t n, uint8_t* k_out, uint8_t* flag) {
    hipLaunchKernelGGL(k_sign_nonce_load<CurveT>, dim3(sign_grid(n)), dim3(BLOCK), 0, s, k_in, n, k_out, flag);
}
template <> void launch_sign_hash_msg<CurveT>(hipStream_t s, const uint8_t* msgs, size_t msg_len, size_t n, uint8_t* z_out) {
    hipLaunchKernelGGL(k_sign_hash_msg<CurveT>, dim3(sign_grid(n)), dim3(BLOCK), 0, s, msgs, msg_len, n, z_out);
}
template <> size_t rfc6979_state_bytes<CurveT>() { return rfc6979_state_bytes_of<CurveT>(); }
template <> void launch_rfc6979<CurveT>(hipStream_t s, const uint8_t* d, const uint8_t* z, size_t n, int cap, uint8_t* k_out,
                                        uint8_t* flag, void* state) {
    hipLaunchKernelGGL(k_rfc6979_first<CurveT>, dim3(sign_grid(n)), dim3(BLOCK), 0, s, d, z, n, k_out, flag, state);
    hipLaunchKernelGGL(k_rfc6979_retry<CurveT>, dim3(sign_grid(n)), dim3(BLOCK), 0, s, d, z, n, cap, k_out, flag,
                       (const void*)state);
}
template <> void launch_ecdsa_sign_finish<CurveT>(hipStream_t s, const uint8_t* d, const uint8_t* k, const uint8_t* k_flag,
                                                  const uint8_t* z, const uint8_t* r_xy, const uint8_t* r_inf, size_t n,
                                                  int normalize_s, uint8_t* sig, uint8_t* recid, uint8_t* ok) {
    hipLaunchKernelGGL(k_ecdsa_sign_finish<CurveT>, dim3(sign_grid(n)), dim3(BLOCK), 0, s, d, k, k_flag, z, r_xy, r_inf, n, normalize_s,
                       sig, recid, ok);
}
template <> void launch_schnorr_nonce<CurveT>(hipStream_t s, const uint8_t* sk, const uint8_t* p_xy, const uint8_t* aux,
                                              const uint8_t* msgs, size_t msg_len, size_t n, uint8_t* dp_out, uint8_t* k_out,
                                              uint8_t* flag) {
    schnorr_nonce_impl<CurveT>(s, sk, p_xy, aux, msgs, msg_len, n, dp_out, k_out, flag);
}
template <> void launch_schnorr_sign_finish<CurveT>(hipStream_t s, const uint8_t* dp, const uint8_t* k, const uint8_t* flag,
                                                    const uint8_t* r_xy, const uint8_t* r_inf, const uint8_t* msgs, size_t msg_len,
                                                    size_t n, uint8_t* sig, uint8_t* ok) {
    schnorr_finish_impl<CurveT>(s, dp, k, flag, r_xy, r_inf, msgs, msg_len, n, sig, ok);
}
template <> void launch_pke_load<CurveT>(hipStream_t s, const uint8_t* s_in, const uint8_t* xy_in, size_t n, uint8_t* s_out,
                                         uint8_t* xy_out, uint8_t* flag) {
    pke_load_impl<CurveT>(s, s_in, xy_in, n, s_out, xy_out, flag);
}
template <> void launch_pke_seal<CurveT>(hipStream_t s, const uint8_t* x2y2, const uint8_t* flag, const uint8_t* msgs, size_t msg_len,
                                         size_t n, uint8_t* c1, uint8_t* c2, uint8_t* c3, uint8_t* ok) {
    pke_seal_impl<CurveT>(s, x2y2, flag, msgs, msg_len, n, c1, c2, c3, ok);
}
template <> void launch_pke_open<CurveT>(hipStream_t s, const uint8_t* x2y2, const uint8_t* flag, const uint8_t* c2, size_t msg_len,
                                         const uint8_t* c3, size_t n, uint8_t* msgs_out, uint8_t* ok) {
    pke_open_impl<CurveT>(s, x2y2, flag, c2, msg_len, c3, n, msgs_out, ok);
}
template <> void launch_sm2_sign_e<CurveT>(hipStream_t s, const uint8_t* distid, size_t distid_len, const uint8_t* pa_xy,
                                          const uint8_t* msgs, size_t msg_len, size_t n, uint8_t* e_out) {
    sm2_sign_e_impl<CurveT>(s, distid, distid_len, pa_xy, msgs, msg_len, n, e_out);
}
template <> void launch_sm2_rfc6979<CurveT>(hipStream_t s, const uint8_t* d, const uint8_t* e, size_t n, uint8_t* k_out, uint8_t* flag) {
    sm2_rfc6979_impl<CurveT>(s, d, e, n, k_out, flag);
}
template <> void launch_sm2dsa_sign_finish<CurveT>(hipStream_t s, const uint8_t* d, const uint8_t* k, const uint8_t* k_flag,
                                                   const uint8_t* e, const uint8_t* r_xy, const uint8_t* r_inf, size_t n, uint8_t* sig,
                                                   uint8_t* ok) {
    sm2dsa_sign_finish_impl<CurveT>(s, d, k, k_flag, e, r_xy, r_inf, n, sig, ok);
}
template <> size_t bign_genk_state_bytes<CurveT>() { return BignSign<CurveT>::value ? BIGN_GENK_STATE_WORDS * sizeof(uint32_t) : 0; }
template <> void launch_bign_genk<CurveT>(hipStream_t s, const uint8_t* d, const uint8_t* h, const uint32_t* bound, size_t n, int cap,
                                          uint8_t* k_out, uint8_t* flag, uint32_t* state) {
    bign_genk_impl<CurveT>(s, d, h, bound, n, cap, k_out, flag, state);
}
template <> void launch_bign_sign_s0<CurveT>(hipStream_t s, const uint8_t* h, const uint8_t* r_xy, size_t n, uint8_t* s0_out) {
    bign_sign_s0_impl<CurveT>(s, h, r_xy, n, s0_out);
}
template <> void launch_bign_sign_finish<CurveT>(hipStream_t s, const uint8_t* d, const uint8_t* k, const uint8_t* k_flag,
                                                 const uint8_t* h, const uint8_t* s0, size_t s0_stride, const uint8_t* r_inf, size_t n,
                                                 uint8_t* sig, uint8_t* ok) {
    bign_sign_finish_impl<CurveT>(s, d, k, k_flag, h, s0, s0_stride, r_inf, n, sig, ok);
}

}  // namespace ecgpu
