// hostcheck_xyz.cpp — TEST INFRASTRUCTURE.  The lane body of the projective-input uniform-schedule kernel (k_xyz_mul_ct,
// csrc/ecgpu_ct.h: the record verdict of ct_xyz_point, then var_base_mul_ct from (X : Y : Z)) compiled with g++ so that it
// can be checked against the oracle without a GPU.  One CPU thread, the kernel's control flow; nothing here is linked into
// libecgpu.so.
#include <cstring>
#include <vector>

#include "../../elliptic-curves_amd/csrc/ecgpu_point.h"
#include "../../elliptic-curves_amd/csrc/ecgpu_recode.h"
#include "../../elliptic-curves_amd/csrc/ecgpu_ctmul.h"

using namespace ecgpu;

namespace {

template <class C>
struct TabLocal {
    Fe<C::NL> t[8][3];
    void put_el(int e, int k, const Fe<C::NL>& v) { t[e][k] = v; }
    Fe<C::NL> get_el(int e, int k) const { return t[e][k]; }
};

template <class C>
void store_affine(const Proj<C>& p, uint8_t* xy, uint8_t* inf) {
    using F = Field<C>;
    using G = Group<C>;
    if (F::is_zero(G::m(p.z))) {
        std::memset(xy, 0, 2 * WireBytes<C>::value);
        *inf = 1;
        return;
    }
    auto zi = F::inv(G::m(p.z));
    F::to_bytes(xy, F::mul(G::m(p.x), zi));
    F::to_bytes(xy + WireBytes<C>::value, F::mul(G::m(p.y), zi));
    *inf = 0;
}

// per record: the verdict flags (CT_FLAG_*) the kernel writes, and the product k P (or P itself for mode 1) as affine bytes
template <class C>
int mul_ct_xyz(int mode, const uint8_t* scalars, const uint8_t* xyz, size_t n, uint8_t* out_xy, uint8_t* out_inf, uint8_t* flags) {
    using G = Group<C>;
    constexpr int N = C::N, WB = WireBytes<C>::value;
    const auto b = G::curve_b();
    for (size_t i = 0; i < n; i++) {
        uint32_t k[N], cx[N], cy[N], cz[N];
        load_be_wire<C>(k, scalars + i * WB);
        uint32_t f = mp_geq<N>(k, C::ORDER) ? CT_FLAG_BAD_SCALAR : 0u;
        load_be_wire<C>(cx, xyz + i * 3 * WB);
        load_be_wire<C>(cy, xyz + i * 3 * WB + WB);
        load_be_wire<C>(cz, xyz + i * 3 * WB + 2 * WB);
        Proj<C> p;
        f |= ct_xyz_point<C>(&p, cx, cy, cz, b);
        flags[i] = (uint8_t)f;
        TabLocal<C> tab;
        const Proj<C> r = mode == 1 ? p : var_base_mul_ct<C>(p, k, b, tab);
        store_affine<C>(r, out_xy + i * 2 * WB, out_inf + i);
    }
    return 0;
}

#define DISPATCH(curve, fn, args)                                                                                   \
    switch (curve) { case 0: return fn<K256Params> args; case 1: return fn<P256Params> args; case 2: return fn<P384Params> args; \
                     case 3: return fn<Sm2Params> args; case 4: return fn<P224Params> args; case 5: return fn<P192Params> args; case 6: return fn<P521Params> args; case 7: return fn<Bp256Params> args; case 8: return fn<Bp384Params> args; case 9: return fn<Bp256t1Params> args; case 10: return fn<Bp384t1Params> args; case 11: return fn<Bign256Params> args; default: return -1; }

}  // namespace

extern "C" {

// mode 0: out = k_i (X_i : Y_i : Z_i); mode 1: out = the point the record decodes to (the loader alone)
int hx_mul_ct_xyz(int curve, int mode, const uint8_t* s, const uint8_t* xyz, size_t n, uint8_t* o, uint8_t* oi, uint8_t* flags) {
    DISPATCH(curve, mul_ct_xyz, (mode, s, xyz, n, o, oi, flags))
}

}  // extern "C"
