// hostcheck_h2c.cpp — TEST INFRASTRUCTURE.  The lane bodies of the hash-to-curve kernels (csrc/ecgpu_h2c.h: expand_message_xmd with
// the reductions of hash_to_field / hash_to_scalar, the simplified SWU map, the secp256k1 isogeny, the sum of two maps) compiled with
// g++ and run element by element with the kernels' record layout, so that they can be checked against tests/h2c_model.py without a
// GPU.  Points leave in projective form (X || Y || Z, canonical): the normalisation is not part of these lanes.
// Nothing here is linked into libecgpu.so.
#include <cstring>

#include "../../elliptic-curves_amd/csrc/ecgpu_h2c.h"

using namespace ecgpu;

namespace {

template <class F>
int dispatch(int curve, F&& f) {
    switch (curve) {
    case CURVE_K256: return f(K256Params{});
    case CURVE_P256: return f(P256Params{});
    case CURVE_P384: return f(P384Params{});
    default: return -1;
    }
}

template <class C>
void put_proj(uint8_t* out, const Proj<C>& p) {
    using F = Field<C>;
    using G = Group<C>;
    constexpr int WB = WireBytes<C>::value;
    uint32_t w[C::N];
    F::to_canonical(w, G::m(p.x)); store_be_wire<C>(out, w);
    F::to_canonical(w, G::m(p.y)); store_be_wire<C>(out + WB, w);
    F::to_canonical(w, G::m(p.z)); store_be_wire<C>(out + 2 * WB, w);
}

}  // namespace

extern "C" {

// k_h2c_expand: count wire records per message
int hh_expand(int curve, const uint8_t* msgs, size_t msg_len, size_t n, const uint8_t* dstp, size_t dstp_len, int count, int to_scalar,
              uint8_t* out) {
    return dispatch(curve, [&](auto c) -> int {
        using C = decltype(c);
        constexpr int N = C::N, WB = WireBytes<C>::value, L = H2cSuite<C>::L;
        for (size_t i = 0; i < n; i++) {
            uint8_t ub[2 * L];
            h2c_expand<C>(ub, msgs + i * msg_len, msg_len, dstp, dstp_len, count);
            for (int j = 0; j < count; j++) {
                uint32_t w[N];
                if (to_scalar) h2c_reduce_scalar<C>(w, ub + j * L);
                else h2c_reduce_field<C>(w, ub + j * L);
                store_be_wire<C>(out + (i * (size_t)count + j) * WB, w);
            }
        }
        return 0;
    });
}

// the two reductions alone on n records of L bytes the caller chose (hh_expand reaches them only behind the hash): out[i] = the
// residue mod p (to_scalar == 0) or mod n as a wire record — op 0 / 1 of ecgpu_selftest_h2c
int hh_reduce(int curve, int to_scalar, const uint8_t* okm, size_t n, uint8_t* out) {
    return dispatch(curve, [&](auto c) -> int {
        using C = decltype(c);
        constexpr int N = C::N, WB = WireBytes<C>::value, L = H2cSuite<C>::L;
        for (size_t i = 0; i < n; i++) {
            uint32_t w[N];
            if (to_scalar) h2c_reduce_scalar<C>(w, okm + i * L);
            else h2c_reduce_field<C>(w, okm + i * L);
            store_be_wire<C>(out + i * WB, w);
        }
        return 0;
    });
}

// the map without the isogeny and without the projective hand-over: out[i] = xn || xd || y, canonical, of the curve SSWU runs on
// (E' for secp256k1) — op 2 of ecgpu_selftest_h2c
int hh_sswu(int curve, const uint8_t* u, size_t n, uint8_t* out) {
    return dispatch(curve, [&](auto c) -> int {
        using C = decltype(c);
        using F = Field<C>;
        using G = Group<C>;
        constexpr int N = C::N, WB = WireBytes<C>::value;
        for (size_t i = 0; i < n; i++) {
            uint32_t w[N];
            Fe<C::NL> e[3];
            load_be_wire<C>(w, u + i * WB);
            H2cMap<C>::sswu(&e[0], &e[1], &e[2], w);
            for (int j = 0; j < 3; j++) {
                F::to_canonical(w, G::m(e[j]));
                store_be_wire<C>(out + (3 * i + j) * WB, w);
            }
        }
        return 0;
    });
}

// k_h2c_map: out_xyz[i] = the sum of the maps of per_point consecutive u records, flags[i] != 0 when a u is not below p
int hh_map(int curve, const uint8_t* u, int per_point, size_t n, uint8_t* out_xyz, uint8_t* flags) {
    return dispatch(curve, [&](auto c) -> int {
        using C = decltype(c);
        using G = Group<C>;
        constexpr int N = C::N, WB = WireBytes<C>::value;
        const Fe<C::NL> b = G::curve_b();
        for (size_t i = 0; i < n; i++) {
            Proj<C> acc = G::identity();
            uint32_t bad = 0;
            for (int j = 0; j < per_point; j++) {
                uint32_t cu[N];
                load_be_wire<C>(cu, u + (i * (size_t)per_point + j) * WB);
                bad |= mp_geq<N>(cu, C::P) ? 1u : 0u;
                acc = G::add(acc, H2cMap<C>::map(cu), b);
            }
            flags[i] = (uint8_t)bad;
            put_proj<C>(out_xyz + i * 3 * WB, acc);
        }
        return 0;
    });
}

// the secp256k1 isogeny alone on x' = xn / xd, y' (canonical records), so that a test can feed it an x' the map never produces
int hh_iso_k256(const uint8_t* xn, const uint8_t* xd, const uint8_t* y, size_t n, uint8_t* out_xyz) {
    using C = K256Params;
    using F = Field<C>;
    for (size_t i = 0; i < n; i++) {
        uint32_t a[C::N], b[C::N], c[C::N];
        load_be_wire<C>(a, xn + i * 32);
        load_be_wire<C>(b, xd + i * 32);
        load_be_wire<C>(c, y + i * 32);
        put_proj<C>(out_xyz + i * 96, H2cMap<C>::iso_k256(F::from_canonical(a).e, F::from_canonical(b).e, F::from_canonical(c).e));
    }
    return 0;
}

}  // extern "C"
