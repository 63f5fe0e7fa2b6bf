// hostcheck_sign.cpp — TEST INFRASTRUCTURE.  The per-element algorithms of the signing kernels (csrc/ecgpu_sign.h: the RFC 6979
// generator, the ECDSA and BIP340 finish steps, the nonce and message hashing) compiled with g++ and run element by element with the
// kernels' record layout, so that they can be checked against tests/sign_model.py without a GPU.  The multiplications by the
// generator between the steps are not here: the test takes them from tests/hostcheck (fixed_base_mul_ct on the CPU).
// Nothing here is linked into libecgpu.so.
#include <cstring>

#include "../../elliptic-curves_amd/csrc/ecgpu_sign.h"

using namespace ecgpu;

namespace {

template <class F>
int dispatch(int curve, F&& f) {
    switch (curve) {
    case CURVE_K256: return f(K256Params{});
    case CURVE_P256: return f(P256Params{});
    case CURVE_P384: return f(P384Params{});
    case CURVE_P224: return f(P224Params{});
    case CURVE_P192: return f(P192Params{});
    case CURVE_P521: return f(P521Params{});
    case CURVE_BP256: return f(Bp256Params{});
    case CURVE_BP384: return f(Bp384Params{});
    case CURVE_BP256T1: return f(Bp256t1Params{});
    case CURVE_BP384T1: return f(Bp384t1Params{});
    default: return -1;
    }
}

}  // namespace

extern "C" {

// k_rfc6979_first + k_rfc6979_retry: k_out[i] = the nonce (1 where none was accepted), tried[i] = candidates tried, 0 = cap reached
int hs_rfc6979(int curve, const uint8_t* d, const uint8_t* z, size_t n, int cap, uint8_t* k_out, int* tried) {
    return dispatch(curve, [&](auto c) -> int {
        using C = decltype(c);
        constexpr int N = C::N, WB = WireBytes<C>::value;
        if constexpr (EcdsaDigest<C>::value == 0) {
            return -2;
        } else {
            for (size_t i = 0; i < n; i++) {
                uint32_t x[N], zw[N], h1[N], k[N], one[N];
                load_be_wire<C>(x, d + i * WB);
                load_be_wire<C>(zw, z + i * WB);
                ScalarN<C>::reduce_wire(h1, zw);
                tried[i] = Rfc6979<C>::generate(k, x, h1, cap);
                sg_one<N>(one);
                sg_sel<N>(k, tried[i] != 0, k, one);
                store_be_wire<C>(k_out + i * WB, k);
            }
            return 0;
        }
    });
}

// k_sign_nonce_load
int hs_nonce_load(int curve, const uint8_t* k_in, size_t n, uint8_t* k_out, uint8_t* flag) {
    return dispatch(curve, [&](auto c) -> int {
        using C = decltype(c);
        constexpr int N = C::N, WB = WireBytes<C>::value;
        for (size_t i = 0; i < n; i++) {
            uint32_t k[N], one[N];
            load_be_wire<C>(k, k_in + i * WB);
            sg_one<N>(one);
            const bool ok = SignScalar<C>::valid(k);
            sg_sel<N>(k, ok, k, one);
            store_be_wire<C>(k_out + i * WB, k);
            flag[i] = ok ? 1 : 0;
        }
        return 0;
    });
}

// k_ecdsa_sign_finish
int hs_ecdsa_sign_finish(int curve, const uint8_t* d, const uint8_t* k, const uint8_t* k_flag, const uint8_t* z, const uint8_t* r_xy,
                         const uint8_t* r_inf, size_t n, int normalize_s, uint8_t* sig, uint8_t* recid, uint8_t* ok) {
    return dispatch(curve, [&](auto c) -> int {
        using C = decltype(c);
        constexpr int N = C::N, WB = WireBytes<C>::value;
        for (size_t i = 0; i < n; i++) {
            uint32_t dw[N], kw[N], zw[N], rx[N], ry[N], r[N], s[N], id;
            load_be_wire<C>(dw, d + i * WB);
            load_be_wire<C>(kw, k + i * WB);
            load_be_wire<C>(zw, z + i * WB);
            load_be_wire<C>(rx, r_xy + i * 2 * WB);
            load_be_wire<C>(ry, r_xy + i * 2 * WB + WB);
            ok[i] = ecdsa_sign_finish_words<C>(dw, kw, k_flag[i] != 0, zw, rx, ry, r_inf[i] != 0, normalize_s, r, s, &id) ? 1 : 0;
            store_be_wire<C>(sig + i * 2 * WB, r);
            store_be_wire<C>(sig + i * 2 * WB + WB, s);
            recid[i] = (uint8_t)id;
        }
        return 0;
    });
}

// k_sign_hash_msg
int hs_hash_msg(int curve, const uint8_t* msgs, size_t msg_len, size_t n, uint8_t* z_out) {
    return dispatch(curve, [&](auto c) -> int {
        using C = decltype(c);
        constexpr int N = C::N, WB = WireBytes<C>::value, D = EcdsaDigest<C>::value;
        if constexpr (D == 0) {
            return -2;
        } else {
            for (size_t i = 0; i < n; i++) {
                uint8_t digest[D];
                const HashPiece one[1] = {{msgs + i * msg_len, msg_len}};
                sha2_pieces<D, 1>(digest, one);
                uint32_t zw[N];
                bits2field_words<C, D>(zw, digest);
                store_be_wire<C>(z_out + i * WB, zw);
            }
            return 0;
        }
    });
}

// k_schnorr_nonce: p_xy = (sanitised d) G
int hs_schnorr_nonce(const uint8_t* sk, const uint8_t* p_xy, const uint8_t* aux, const uint8_t* msgs, size_t msg_len, size_t n,
                     uint8_t* dp_out, uint8_t* k_out, uint8_t* flag) {
    using C = K256Params;
    for (size_t i = 0; i < n; i++) {
        uint32_t d[8], px[8], py[8], a[8], dd[8], k[8];
        load_be<8>(d, sk + i * 32);
        load_be<8>(px, p_xy + i * 64);
        load_be<8>(py, p_xy + i * 64 + 32);
        load_be<8>(a, aux + i * 32);
        flag[i] = schnorr_nonce_words<C>(d, px, py, a, msgs + i * msg_len, msg_len, dd, k) ? 1 : 0;
        store_be<8>(dp_out + i * 64, dd);
        store_be<8>(dp_out + i * 64 + 32, px);
        store_be<8>(k_out + i * 32, k);
    }
    return 0;
}

// k_schnorr_sign_finish
int hs_schnorr_sign_finish(const uint8_t* dp, const uint8_t* k_in, const uint8_t* flag, const uint8_t* r_xy, const uint8_t* r_inf,
                           const uint8_t* msgs, size_t msg_len, size_t n, uint8_t* sig, uint8_t* ok) {
    using C = K256Params;
    for (size_t i = 0; i < n; i++) {
        uint32_t d[8], px[8], k[8], rx[8], ry[8], r[8], s[8];
        load_be<8>(d, dp + i * 64);
        load_be<8>(px, dp + i * 64 + 32);
        load_be<8>(k, k_in + i * 32);
        load_be<8>(rx, r_xy + i * 64);
        load_be<8>(ry, r_xy + i * 64 + 32);
        ok[i] = schnorr_sign_finish_words<C>(d, k, flag[i] != 0, px, rx, ry, r_inf[i] != 0, msgs + i * msg_len, msg_len, r, s) ? 1 : 0;
        store_be<8>(sig + i * 64, r);
        store_be<8>(sig + i * 64 + 32, s);
    }
    return 0;
}

}  // extern "C"
