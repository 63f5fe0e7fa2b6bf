// ecgpu_selftest_point_raw.h — the point formulas on coordinates taken limb by limb (host + device).
//
// One statement of the operations for both compilers: tests/hostcheck (g++) and k_selftest_point_raw (gfx950, ecgpu_selftest.h)
// call the function below, and tests/point_vectors.py holds the model: a coordinate is the integer sum limb_i 2^(B i) (times
// R^-1 on the Montgomery sets), results are compared as projective classes.  "Raw": a record is four coordinate slots of NL
// 32-bit words each and the words ARE the limbs — no unpack, no from_canonical, no range or curve check — so a test can write
// what the types allow and Field::unpack cannot produce: limbs at LB (above 2^B), a top limb at its bound, the limbs of p
// itself, value magnitude JV on the Jacobian and XYZZ inputs.  The formulas wrap the coordinates themselves, as they do for
// their production callers (m for Proj and Affine, mj for Jac and Xyzz), so in a -DECGPU_BOUNDS_CHECK build every claim is
// checked against what the test wrote.  The result comes back in the same layout, limbs as the formula left them.
//
// Slots:  homogeneous X Y Z -     Jacobian X Y Z -     XYZZ X Y ZZ ZZZ     affine x y - -     (an unused slot: ignored / zero)
// Ops (op & 0xFF; the chains take their step count from op >> 8):
//    0 add(P, Q)               1 add(P, Q, negq)            2 add_mixed(P, q)        3 add_mixed(P, q, negq)
//    4 dbl(P)                  5 neg(P)                     6 ct_dbl4(P)
//    7 jac_dbl(J)              8 jac_madd(J, q)             9 jac_madd(J, q, negq)   10 jac_to_proj(J)
//   11 xyzz_madd(S, q)        12 xyzz_madd(S, q, negq)     13 xyzz_mmadd(p, q)       14 xyzz_to_proj(S)
//   15 acc = dbl(add(acc, Q)), steps times, acc = P (homogeneous in and out)
//   16 acc = jac_madd(jac_dbl^4(acc), q), steps times, acc = J: the ladder step of ecgpu_varmul.h (Jacobian in and out)
//   17 is_identity(P) as 0 / 1 in the first word of the result
//   19 the identity test of k_normalize's forward pass on the limbs of Z as they are (NormRec::classify, ecgpu_batchinv.h):
//      Field::is_zero_short(m(Z)) as 0 / 1 in the first word and Field::is_zero(m(Z)) in the second (18 stays unknown: the
//      op-range tests pin it)
// False for an unknown operation.
#pragma once

#include "ecgpu_point.h"
#include "ecgpu_ctmul.h"

namespace ecgpu {

ECGPU_CONST int SELFTEST_POINT_RAW_MAX_STEPS = 64;

template <class C>
ECGPU_HD bool selftest_point_raw(int op, const uint32_t* p, const uint32_t* q, uint32_t* r) {
    using G = Group<C>;
    constexpr int NL = C::NL;
    const int code = op & 0xFF, steps = op >> 8;
    Fe<NL> a[4], b[4], o[4];
#pragma unroll
    for (int k = 0; k < 4; k++)
#pragma unroll
        for (int t = 0; t < NL; t++) {
            a[k].v[t] = p[k * NL + t];
            b[k].v[t] = q[k * NL + t];
            o[k].v[t] = 0;
        }
    const Fe<NL> cb = G::curve_b();
    Proj<C> P, Q;
    P.x = a[0]; P.y = a[1]; P.z = a[2];
    Q.x = b[0]; Q.y = b[1]; Q.z = b[2];
    Jac<C> J;
    J.x = a[0]; J.y = a[1]; J.z = a[2];
    Xyzz<C> S;
    S.x = a[0]; S.y = a[1]; S.zz = a[2]; S.zzz = a[3];
    Affine<C> pa, qa;
    pa.x = a[0]; pa.y = a[1];
    qa.x = b[0]; qa.y = b[1];
    auto put_p = [&](const Proj<C>& v) { o[0] = v.x; o[1] = v.y; o[2] = v.z; };
    auto put_j = [&](const Jac<C>& v) { o[0] = v.x; o[1] = v.y; o[2] = v.z; };
    auto put_s = [&](const Xyzz<C>& v) { o[0] = v.x; o[1] = v.y; o[2] = v.zz; o[3] = v.zzz; };
    bool known = steps == 0 || ((code == 15 || code == 16) && steps <= SELFTEST_POINT_RAW_MAX_STEPS);
    if (known) {
        switch (code) {
        case 0: put_p(G::add(P, Q, cb)); break;
        case 1: put_p(G::add(P, Q, cb, true)); break;
        case 2: put_p(G::add_mixed(P, qa, cb)); break;
        case 3: put_p(G::add_mixed(P, qa, cb, true)); break;
        case 4: put_p(G::dbl(P, cb)); break;
        case 5: put_p(G::neg(P)); break;
        case 6: put_p(ct_dbl4<C>(P, cb)); break;
        case 7: put_j(G::jac_dbl(J)); break;
        case 8: put_j(G::jac_madd(J, qa, false)); break;
        case 9: put_j(G::jac_madd(J, qa, true)); break;
        case 10: put_p(G::jac_to_proj(J)); break;
        case 11: put_s(G::xyzz_madd(S, qa, false)); break;
        case 12: put_s(G::xyzz_madd(S, qa, true)); break;
        case 13: put_s(G::xyzz_mmadd(pa, qa, false)); break;
        case 14: put_p(G::xyzz_to_proj(S)); break;
        case 15:
#pragma unroll 1
            for (int s = 0; s < steps; s++) P = G::dbl(G::add(P, Q, cb), cb);
            put_p(P);
            break;
        case 16:
#pragma unroll 1
            for (int s = 0; s < steps; s++) {
#pragma unroll 1
                for (int d = 0; d < 4; d++) J = G::jac_dbl(J);
                J = G::jac_madd(J, qa, false);
            }
            put_j(J);
            break;
        case 17: o[0].v[0] = G::is_identity(P) ? 1u : 0u; break;
        case 19:
            o[0].v[0] = Field<C>::is_zero_short(G::m(P.z)) ? 1u : 0u;
            o[0].v[1] = Field<C>::is_zero(G::m(P.z)) ? 1u : 0u;
            break;
        default: known = false;
        }
    }
#pragma unroll
    for (int k = 0; k < 4; k++)
#pragma unroll
        for (int t = 0; t < NL; t++) r[k * NL + t] = o[k].v[t];
    return known;
}

}  // namespace ecgpu
