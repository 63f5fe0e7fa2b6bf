// batchinv_host.h — TEST INFRASTRUCTURE.  Host Io structs for the three policies of batch_inv_lane (csrc/ecgpu_batchinv.h,
// csrc/ecgpu_xyz.h) and drivers that run every lane of a launch in turn with the kernels' record stride: the CPU twins of
// k_normalize, k_xyz_affine and k_scalar_batch_inv.  Shared by hostcheck.cpp, hostcheck_xyz_var.cpp and batchinv_san.cpp.
#pragma once

#include <cstring>
#include <vector>

#include "../../elliptic-curves_amd/csrc/ecgpu_xyz.h"

namespace ecgpu_host {

using namespace ecgpu;

// k_normalize over internal projective records
template <class C, int MODE>
struct NormIoHost {
    static constexpr int N = C::N, WB = WireBytes<C>::value, NS = Field<C>::NS;
    const Proj<C>* proj;
    uint32_t* prefix;
    uint8_t* out_xy;          // NORM_COMPRESSED: x alone
    uint8_t* out_inf;         // NORM_COMPRESSED: the tags
    uint32_t* out_packed;
    Fe<C::NL> load_z(size_t j) const { return proj[j].z; }
    Proj<C> load_point(size_t j) const { return proj[j]; }
    void put_prefix(size_t j, const uint32_t* w) const { std::memcpy(prefix + j * NS, w, NS * 4); }
    void get_prefix(size_t j, uint32_t* w) const { std::memcpy(w, prefix + j * NS, NS * 4); }
    void put_x(size_t j, const uint32_t* w) const {
        if (MODE == NORM_PACKED) std::memcpy(out_packed + j * 2 * N, w, N * 4);
        else store_be_wire<C>(out_xy + j * (MODE == NORM_WIRE ? 2 * WB : WB), w);
    }
    void put_y(size_t j, const uint32_t* w) const {
        if (MODE == NORM_PACKED) std::memcpy(out_packed + j * 2 * N + N, w, N * 4);
        else store_be_wire<C>(out_xy + j * 2 * WB + WB, w);
    }
    void put_flag(size_t j, uint8_t v) const {
        if (out_inf) out_inf[j] = v;
    }
};
template <class C, int MODE>
void normalize(const std::vector<Proj<C>>& proj, size_t nthreads, uint8_t* out_xy, uint8_t* out_inf, uint32_t* out_packed = nullptr) {
    const size_t n = proj.size();
    std::vector<uint32_t> prefix(n * Field<C>::NS);
    NormIoHost<C, MODE> io{proj.data(), prefix.data(), out_xy, out_inf, out_packed};
    for (size_t t = 0; t < nthreads; t++) normalize_lane<C, MODE>(t, n, nthreads, io);
}

// k_xyz_affine over wire records X || Y || Z; ok[j] = 0 for a bad record
template <class C>
struct XyzIoHost {
    static constexpr int WB = WireBytes<C>::value, NS = Field<C>::NS;
    const uint8_t* xyz;
    uint32_t* prefix;
    uint8_t* out_xy;
    uint8_t* out_inf;
    uint8_t* ok;
    void load_z(size_t j, uint32_t* cz) const { load_be_wire<C>(cz, xyz + j * 3 * WB + 2 * WB); }
    void load_xyz(size_t j, uint32_t* cx, uint32_t* cy, uint32_t* cz) const {
        load_be_wire<C>(cx, xyz + j * 3 * WB);
        load_be_wire<C>(cy, xyz + j * 3 * WB + WB);
        load_be_wire<C>(cz, xyz + j * 3 * WB + 2 * WB);
    }
    void put_prefix(size_t j, const uint32_t* w) const { std::memcpy(prefix + j * NS, w, NS * 4); }
    void get_prefix(size_t j, uint32_t* w) const { std::memcpy(w, prefix + j * NS, NS * 4); }
    void put_affine(size_t j, const uint32_t* x, const uint32_t* y, bool ident) const {
        store_be_wire<C>(out_xy + j * 2 * WB, x);
        store_be_wire<C>(out_xy + j * 2 * WB + WB, y);
        out_inf[j] = ident ? 1 : 0;
    }
    void verdict(size_t j, bool good) { ok[j] = good ? 1 : 0; }
};
template <class C>
void xyz_affine(const uint8_t* xyz, size_t n, size_t nthreads, uint8_t* out_xy, uint8_t* out_inf, uint8_t* ok) {
    std::vector<uint32_t> prefix(n * Field<C>::NS);
    XyzIoHost<C> io{xyz, prefix.data(), out_xy, out_inf, ok};
    for (size_t t = 0; t < nthreads; t++) xyz_affine_lane<C>(t, n, nthreads, io);
}

// k_scalar_batch_inv over wire records
template <class C>
struct ScalarIoHost {
    static constexpr int N = C::N, WB = WireBytes<C>::value;
    const uint8_t* in;
    uint32_t* prefix;
    uint8_t* out;
    void load(size_t j, uint32_t* a) const { load_be_wire<C>(a, in + j * WB); }
    void put(size_t j, const uint32_t* w) const { store_be_wire<C>(out + j * WB, w); }
    void put_prefix(size_t j, const uint32_t* w) const { std::memcpy(prefix + j * N, w, N * 4); }
    void get_prefix(size_t j, uint32_t* w) const { std::memcpy(w, prefix + j * N, N * 4); }
};
template <class C>
int scalar_batch_inv(const uint8_t* in, size_t n, size_t nthreads, uint8_t* out) {
    std::vector<uint32_t> prefix(n * C::N);
    ScalarIoHost<C> io{in, prefix.data(), out};
    for (size_t t = 0; t < nthreads; t++) scalar_batch_inv_lane<C>(t, n, nthreads, io);
    return 0;
}

// the normalisation of wire records X || Y || Z taken as they are (no curve check): MODE NORM_WIRE -> x || y and identity flags,
// NORM_COMPRESSED -> x and tags
template <class C>
int normalize_xyz(int mode, const uint8_t* xyz, size_t n, size_t nthreads, uint8_t* out, uint8_t* flags) {
    using F = Field<C>;
    constexpr int WB = WireBytes<C>::value;
    std::vector<Proj<C>> proj(n);
    for (size_t i = 0; i < n; i++) {
        bool okx, oky, okz;
        proj[i].x = F::from_bytes(xyz + i * 3 * WB, &okx).e;
        proj[i].y = F::from_bytes(xyz + i * 3 * WB + WB, &oky).e;
        proj[i].z = F::from_bytes(xyz + i * 3 * WB + 2 * WB, &okz).e;
        if (!(okx && oky && okz)) return -3;
    }
    if (mode == NORM_WIRE) normalize<C, NORM_WIRE>(proj, nthreads, out, flags);
    else if (mode == NORM_COMPRESSED) normalize<C, NORM_COMPRESSED>(proj, nthreads, out, flags);
    else return -1;
    return 0;
}

#define ECGPU_HOST_DISPATCH(curve, fn, args)                                                                        \
    switch (curve) { case 0: return fn<K256Params> args; case 1: return fn<P256Params> args; case 2: return fn<P384Params> args; \
                     case 3: return fn<Sm2Params> args; case 4: return fn<P224Params> args; case 5: return fn<P192Params> args; case 6: return fn<P521Params> args; case 7: return fn<Bp256Params> args; case 8: return fn<Bp384Params> args; case 9: return fn<Bp256t1Params> args; case 10: return fn<Bp384t1Params> args; case 11: return fn<Bign256Params> args; default: return -1; }

}  // namespace ecgpu_host
