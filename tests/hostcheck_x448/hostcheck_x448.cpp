// hostcheck_x448.cpp — TEST INFRASTRUCTURE.  csrc/ecgpu_fe448.h and the lane body of k_x448_ladder (csrc/ecgpu_x448.h) compiled
// with g++ and run element by element with the kernels' record layout, so that they can be checked against Python integers and
// tests/x448_model.py without a GPU.  Built twice by tests/test_hostcheck_x448.py: plain, and with -DECGPU_BOUNDS_CHECK, where every
// Gf<M> is checked against its magnitude where an operation reads it (a trap is a failure of the bound analysis).  Nothing here is
// linked into libecgpu.so.
//
// With -DHOSTCHECK_X448_MAIN the same source is a stand-alone program (built with -fsanitize=address,undefined): it reads one
// element per line — mode, scalar, point in hex — runs the lane body on buffers of exactly the records' sizes and prints the
// result and the verdict.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../elliptic-curves_amd/csrc/ecgpu_x448.h"

using namespace ecgpu;

namespace {
void load_le(uint32_t* w, const uint8_t* b, int nw) {
    for (int j = 0; j < nw; j++) w[j] = (uint32_t)b[4 * j] | (uint32_t)b[4 * j + 1] << 8 | (uint32_t)b[4 * j + 2] << 16 | (uint32_t)b[4 * j + 3] << 24;
}
void store_le(uint8_t* b, const uint32_t* w, int nw) {
    for (int j = 0; j < nw; j++)
        for (int t = 0; t < 4; t++) b[4 * j + t] = (uint8_t)(w[j] >> (8 * t));
}

// what k_x448_ladder<MODE> does for element i
int lane(int mode, const uint8_t* scalar, const uint8_t* point, uint8_t* out, uint8_t* ok) {
    uint32_t k[fe448::NW], u[fe448::NW] = {}, r[fe448::NW];
    load_le(k, scalar, fe448::NW);
    if (mode != X448_BASE) load_le(u, point, fe448::NW);
    uint32_t accepted;
    if (mode == X448_CHECKED) accepted = x448_lane_words<X448_CHECKED>(r, k, u);
    else if (mode == X448_UNCHECKED) accepted = x448_lane_words<X448_UNCHECKED>(r, k, u);
    else if (mode == X448_BASE) accepted = x448_lane_words<X448_BASE>(r, k, u);
    else return 1;
    store_le(out, r, fe448::NW);
    *ok = (uint8_t)(accepted & 1u);
    return 0;
}
}  // namespace

extern "C" {

// one op of ecgpu_selftest_fe448 on n records of 16 raw limbs (b may be null)
int hx_fe448(int op, const uint32_t* a, const uint32_t* b, size_t n, uint32_t* out) {
    if (op < 0 || op >= FE448_OPS) return 1;
    const uint32_t zero[fe448::NL] = {};
    for (size_t i = 0; i < n; i++) fe448_selftest_op(op, out + 16 * i, a + 16 * i, b ? b + 16 * i : zero);
    return 0;
}

// n elements through the lane body: 56-byte records; ok: n bytes (1 for every element of the unchecked and base forms)
int hx_x448(int mode, const uint8_t* scalars, const uint8_t* points, size_t n, uint8_t* out, uint8_t* ok) {
    for (size_t i = 0; i < n; i++)
        if (lane(mode, scalars + 56 * i, points ? points + 56 * i : nullptr, out + 56 * i, ok + i)) return 1;
    return 0;
}

// `iters` rounds of the iterated vector of RFC 7748 section 5.2 from k = u = start, through the checked form
int hx_x448_iterate(const uint8_t* start, int iters, uint8_t* out) {
    uint8_t k[56], u[56], r[56], ok;
    memcpy(k, start, 56);
    memcpy(u, start, 56);
    memset(r, 0, 56);
    for (int i = 0; i < iters; i++) {
        if (lane(X448_CHECKED, k, u, r, &ok) || !ok) return 1;
        memcpy(u, k, 56);
        memcpy(k, r, 56);
    }
    memcpy(out, r, 56);
    return 0;
}

}  // extern "C"

#ifdef HOSTCHECK_X448_MAIN
namespace {
bool unhex(const std::string& s, std::vector<uint8_t>& out) {
    if (s.size() % 2) return false;
    out.clear();
    for (size_t i = 0; i < s.size(); i += 2) {
        unsigned v;
        if (sscanf(s.c_str() + i, "%2x", &v) != 1) return false;
        out.push_back((uint8_t)v);
    }
    return true;
}
}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    char ks[256], us[256];
    int mode;
    while (fscanf(f, "%d %255s %255s", &mode, ks, us) == 3) {
        std::vector<uint8_t> k, u;
        if (!unhex(ks, k) || !unhex(us, u) || k.size() != 56 || u.size() != 56) return 3;
        std::vector<uint8_t> out(56), ok(1);                      // exactly the records' sizes
        if (lane(mode, k.data(), u.data(), out.data(), ok.data())) return 4;
        for (uint8_t b : out) printf("%02x", b);
        printf(" %d\n", ok[0]);
    }
    fclose(f);
    return 0;
}
#endif
