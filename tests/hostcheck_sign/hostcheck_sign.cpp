// hostcheck_sign.cpp — TEST INFRASTRUCTURE.  The per-element algorithms of the signing kernels (csrc/ecgpu_sign.h: the RFC 6979
// generator, the ECDSA and BIP340 finish steps, the nonce and message hashing) compiled with g++ and run element by element with the
// kernels' record layout, so that they can be checked against tests/sign_model.py without a GPU.  The multiplications by the
// generator between the steps are not here: the test takes them from tests/hostcheck (fixed_base_mul_ct on the CPU).
// Nothing here is linked into libecgpu.so.
//
// With -DHOSTCHECK_SIGN_MAIN the same source is a stand-alone program (built with -fsanitize=address,undefined by
// tests/test_sign_vectors.py): it reads one finish-step record per line, all values in hex —
//     E <curve id> <normalize_s> <d> <k> <flag> <z> <x(R) || y(R)> <r_inf>         the ECDSA finish step
//     S <d' || x(P)> <k> <flag> <x(R) || y(R)> <r_inf> <message, "-" when empty>   the BIP340 finish step
// — runs the step on heap buffers of exactly the record's size and prints what it wrote.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

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

#ifdef HOSTCHECK_SIGN_MAIN
namespace {
std::vector<uint8_t> unhex(const std::string& s) {
    std::vector<uint8_t> out;
    if (s == "-") return out;
    for (size_t i = 0; i + 1 < s.size(); i += 2) out.push_back((uint8_t)std::stoi(s.substr(i, 2), nullptr, 16));
    return out;
}
void put(const char* name, const std::vector<uint8_t>& v) {
    std::printf(" %s=", name);
    for (uint8_t b : v) std::printf("%02x", b);
}
// exactly `v`'s bytes on the heap (one byte for an empty string: never a null data pointer)
std::vector<uint8_t> exact(const std::vector<uint8_t>& v) { return v.empty() ? std::vector<uint8_t>(1) : v; }
}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    static char kind[4], a[300], b[300], c[300], d[300], m[4096];
    int curve = 0, norm = 0, kf = 0, ri = 0;
    while (std::fscanf(f, "%3s", kind) == 1) {
        if (kind[0] == 'E') {
            if (std::fscanf(f, "%d %d %299s %299s %d %299s %299s %d", &curve, &norm, a, b, &kf, c, d, &ri) != 8) return 3;
            size_t L = 0;
            dispatch(curve, [&](auto cv) -> int { L = WireBytes<decltype(cv)>::value; return 0; });
            const std::vector<uint8_t> dd = unhex(a), kk = unhex(b), zz = unhex(c), rxy = unhex(d);
            if (!L || dd.size() != L || kk.size() != L || zz.size() != L || rxy.size() != 2 * L) return 3;
            const std::vector<uint8_t> kflag(1, (uint8_t)kf), rinf(1, (uint8_t)ri);
            std::vector<uint8_t> sig(2 * L), recid(1), ok(1);
            if (hs_ecdsa_sign_finish(curve, dd.data(), kk.data(), kflag.data(), zz.data(), rxy.data(), rinf.data(), 1, norm, sig.data(),
                                     recid.data(), ok.data()) != 0)
                return 4;
            put("sig", sig); put("recid", recid); put("ok", ok);
        } else if (kind[0] == 'S') {
            if (std::fscanf(f, "%299s %299s %d %299s %d %4095s", a, b, &kf, c, &ri, m) != 6) return 3;
            const std::vector<uint8_t> dp = unhex(a), kk = unhex(b), rxy = unhex(c), msg = unhex(m), mb = exact(msg);
            if (dp.size() != 64 || kk.size() != 32 || rxy.size() != 64) return 3;
            const std::vector<uint8_t> kflag(1, (uint8_t)kf), rinf(1, (uint8_t)ri);
            std::vector<uint8_t> sig(64), ok(1);
            hs_schnorr_sign_finish(dp.data(), kk.data(), kflag.data(), rxy.data(), rinf.data(), mb.data(), msg.size(), 1, sig.data(), ok.data());
            put("sig", sig); put("ok", ok);
        } else {
            return 3;
        }
        std::printf("\n");
    }
    std::fclose(f);
    return 0;
}
#endif
