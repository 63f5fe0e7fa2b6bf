// point_raw_san.cpp — TEST INFRASTRUCTURE.  A stand-alone program for AddressSanitizer + UBSan: selftest_point_raw
// (csrc/ecgpu_selftest_point_raw.h — Group<C>'s formulas and ct_dbl4 on raw limbs) over heap buffers that are exactly as large as
// the records they hold, compared with the results passed in.  Built and run by tests/test_point_vectors.py.
//
// argv[1]: a file of cases.  A case is four little-endian u32 (curve, op, n, has_q), n p records, n q records if has_q, and the n
// expected result records; a record is 4 NL u32.
// Exit status 0: every case equal; 1: a case differs (named on stderr); 2: malformed input or an unknown op.
#include <cstdio>
#include <vector>

#include "../../elliptic-curves_amd/csrc/ecgpu_selftest_point_raw.h"
#include "batchinv_host.h"

using namespace ecgpu;

namespace {

template <class C>
int run_case(int op, size_t n, const uint32_t* p, const uint32_t* q, uint32_t* out) {
    constexpr size_t W = 4 * C::NL;
    const std::vector<uint32_t> zero(W, 0);
    for (size_t i = 0; i < n; i++) {
        // one record at a time through buffers of exactly one record: a read or write past a record is a heap overflow
        std::vector<uint32_t> a(p + i * W, p + (i + 1) * W), b(q ? q + i * W : zero.data(), q ? q + (i + 1) * W : zero.data() + W), r(W, 0xEEEEEEEEu);
        if (!selftest_point_raw<C>(op, a.data(), b.data(), r.data())) return 2;
        for (size_t t = 0; t < W; t++) out[i * W + t] = r[t];
    }
    return 0;
}
template <class C>
int words(int) { return 4 * C::NL; }
int words_of(uint32_t curve) { ECGPU_HOST_DISPATCH(curve, words, (0)) }
int run(uint32_t curve, int op, size_t n, const uint32_t* p, const uint32_t* q, uint32_t* out) {
    ECGPU_HOST_DISPATCH(curve, run_case, (op, n, p, q, out))
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t h[4];
    int cases = 0, rc = 0;
    while (rc == 0 && std::fread(h, 4, 4, f) == 4) {
        const int w = words_of(h[0]);
        if (w <= 0 || h[2] == 0) { rc = 2; break; }
        const size_t len = (size_t)h[2] * (size_t)w;
        std::vector<uint32_t> p(len), q(h[3] ? len : 0), want(len), got(len);
        if (std::fread(p.data(), 4, len, f) != len || (h[3] && std::fread(q.data(), 4, len, f) != len) || std::fread(want.data(), 4, len, f) != len) {
            rc = 2;
            break;
        }
        rc = run(h[0], (int)h[1], h[2], p.data(), h[3] ? q.data() : nullptr, got.data());
        if (rc == 0 && got != want) {
            std::fprintf(stderr, "case %d (curve %u op %u n %u) differs\n", cases, h[0], h[1], h[2]);
            rc = 1;
        }
        cases++;
    }
    std::fclose(f);
    if (rc == 0) std::printf("%d cases equal\n", cases);
    return rc;
}
