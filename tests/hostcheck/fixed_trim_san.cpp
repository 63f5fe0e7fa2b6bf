// fixed_trim_san.cpp — TEST INFRASTRUCTURE.  A stand-alone program for AddressSanitizer + UBSan: fixed_base_mul
// (csrc/ecgpu_fixedmul.h — both forms of the comb walk; on the host a lane is its own wave) over a table built here, followed by
// k_normalize's lane body, compared with the affine points passed in.  Built and run by tests/test_hostcheck_fixed_trim.py.
//
// argv[1]: a file of cases.  A case is three little-endian u32 (curve, w, n), n scalars (wire records), n expected x || y records
// and n identity flags (one byte each).
// Exit status 0: every case equal; 1: a case differs (named on stderr); 2: malformed input or an unknown curve.
#include <cstdio>
#include <vector>

#include "../../elliptic-curves_amd/csrc/ecgpu_fixedmul.h"
#include "batchinv_host.h"

using namespace ecgpu;

namespace {

// entry (index + 1) * 2^(w * window) * G in the packed storage form, in a heap array that is exactly as large as the table
template <class C>
struct Table {
    int w, nwin;
    std::vector<uint32_t> e;
    void load(PackedPoint<2 * C::N>& p, int window, uint32_t index) const {
        const size_t at = ((size_t)window * ((size_t)1 << (w - 1)) + index) * (2 * C::N);
        for (int i = 0; i < 2 * C::N; i++) p.w[i] = e.at(at + i);
    }
};

template <class C>
Table<C> build(int w) {
    using G = Group<C>;
    using F = Field<C>;
    Table<C> t{w, signed_window_count(32 * C::N - 1, w), {}};
    const size_t half = (size_t)1 << (w - 1);
    t.e.resize(half * t.nwin * 2 * C::N);
    const auto b = G::curve_b();
    Affine<C> g;
    g.x = F::from_canonical(C::GX).e;
    g.y = F::from_canonical(C::GY).e;
    Proj<C> base = G::from_affine(g);
    for (int j = 0; j < t.nwin; j++) {
        Proj<C> cur = base;
        for (size_t i = 0; i < half; i++) {
            const auto zi = F::inv(G::m(cur.z));
            F::pack(&t.e[(j * half + i) * 2 * C::N], F::mul(G::m(cur.x), zi));
            F::pack(&t.e[(j * half + i) * 2 * C::N + C::N], F::mul(G::m(cur.y), zi));
            cur = G::add(cur, base, b);
        }
        for (int s = 0; s < w; s++) base = G::dbl(base, b);
    }
    return t;
}

template <class C>
int run_case(int w, size_t n, const uint8_t* scalars, const uint8_t* want_xy, const uint8_t* want_inf) {
    constexpr size_t WB = WireBytes<C>::value;
    if (w < 2 || w > 12) return 2;
    const Table<C> t = build<C>(w);
    std::vector<Proj<C>> proj(n);
    for (size_t i = 0; i < n; i++) {
        std::vector<uint8_t> rec(scalars + i * WB, scalars + (i + 1) * WB);      // one record, exactly as large as it is
        std::vector<uint32_t> k(C::N);
        load_be_wire<C>(k.data(), rec.data());
        if (mp_geq<C::N>(k.data(), C::ORDER)) return 2;
        proj[i] = fixed_base_mul<C>(k.data(), t, t.w, t.nwin, Group<C>::curve_b());
    }
    std::vector<uint8_t> xy(n * 2 * WB, 0xEE), inf(n, 0xEE);
    ecgpu_host::normalize<C, NORM_WIRE>(proj, 3, xy.data(), inf.data());
    for (size_t i = 0; i < n; i++) {
        if (inf[i] != want_inf[i] || std::memcmp(&xy[i * 2 * WB], want_xy + i * 2 * WB, 2 * WB) != 0) {
            std::fprintf(stderr, "scalar %zu differs\n", i);
            return 1;
        }
    }
    return 0;
}
template <class C>
int wire_bytes(int) { return WireBytes<C>::value; }
int wire_bytes_of(uint32_t curve) {
    switch (curve) { case 0: return wire_bytes<K256Params>(0); case 1: return wire_bytes<P256Params>(0); case 2: return wire_bytes<P384Params>(0);
                     case 7: return wire_bytes<Bp256Params>(0); default: return -1; }
}
int run(uint32_t curve, int w, size_t n, const uint8_t* s, const uint8_t* xy, const uint8_t* inf) {
    switch (curve) { case 0: return run_case<K256Params>(w, n, s, xy, inf); case 1: return run_case<P256Params>(w, n, s, xy, inf);
                     case 2: return run_case<P384Params>(w, n, s, xy, inf); case 7: return run_case<Bp256Params>(w, n, s, xy, inf); default: return 2; }
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t h[3];
    int cases = 0, rc = 0;
    while (rc == 0 && std::fread(h, 4, 3, f) == 3) {
        const int wb = wire_bytes_of(h[0]);
        if (wb <= 0 || h[2] == 0 || h[2] > 4096) { rc = 2; break; }
        const size_t n = h[2];
        std::vector<uint8_t> s(n * wb), xy(n * 2 * wb), inf(n);
        if (std::fread(s.data(), 1, s.size(), f) != s.size() || std::fread(xy.data(), 1, xy.size(), f) != xy.size() ||
            std::fread(inf.data(), 1, n, f) != n) {
            rc = 2;
            break;
        }
        rc = run(h[0], (int)h[1], n, s.data(), xy.data(), inf.data());
        if (rc == 1) std::fprintf(stderr, "case %d (curve %u w %u n %u)\n", cases, h[0], h[1], h[2]);
        cases++;
    }
    std::fclose(f);
    if (rc == 0) std::printf("%d cases equal\n", cases);
    return rc;
}
