// batchinv_san.cpp — TEST INFRASTRUCTURE.  A stand-alone program for AddressSanitizer + UBSan: the three policies of
// batch_inv_lane (k_normalize, k_xyz_affine, k_scalar_batch_inv) over host buffers that are exactly as large as the records they
// hold, compared with the outputs passed in.  Built and run by tests/test_lane_chains.py.
//
// stdin: cases of seven little-endian u32 (kind, curve, mode, n, lanes, input bytes, output bytes), the input, the expected output.
//   kind 0: k_normalize, input X || Y || Z records, output x || y records + n flags (mode 0) or x records + n tags (mode 2)
//   kind 1: k_xyz_affine, input X || Y || Z records, output x || y records + n identity flags + n verdicts
//   kind 2: k_scalar_batch_inv, input and output n scalars
// Exit status 0: every case equal; 1: a case differs (named on stderr); 2: malformed input.
#include <cstdio>

#include "batchinv_host.h"

using namespace ecgpu_host;

namespace {

template <class C>
int run_case(uint32_t kind, uint32_t mode, size_t n, size_t lanes, const std::vector<uint8_t>& in, std::vector<uint8_t>& out) {
    constexpr size_t WB = WireBytes<C>::value;
    const size_t rec = kind == 2 ? WB : kind == 0 && mode == NORM_COMPRESSED ? WB : 2 * WB;
    if (in.size() != n * (kind == 2 ? WB : 3 * WB) || out.size() != n * (rec + (kind == 2 ? 0 : kind == 1 ? 2 : 1))) return -2;
    if (kind == 0) return normalize_xyz<C>((int)mode, in.data(), n, lanes, out.data(), out.data() + n * rec);
    if (kind == 1) { xyz_affine<C>(in.data(), n, lanes, out.data(), out.data() + n * rec, out.data() + n * rec + n); return 0; }
    if (kind == 2) return scalar_batch_inv<C>(in.data(), n, lanes, out.data());
    return -2;
}
int run(uint32_t curve, uint32_t kind, uint32_t mode, size_t n, size_t lanes, const std::vector<uint8_t>& in, std::vector<uint8_t>& out) {
    ECGPU_HOST_DISPATCH(curve, run_case, (kind, mode, n, lanes, in, out))
}

}  // namespace

int main() {
    uint32_t h[7];
    int cases = 0;
    while (std::fread(h, 4, 7, stdin) == 7) {
        std::vector<uint8_t> in(h[5]), want(h[6]), got(h[6], 0xEE);
        if (std::fread(in.data(), 1, in.size(), stdin) != in.size() || std::fread(want.data(), 1, want.size(), stdin) != want.size()) return 2;
        if (h[3] == 0 || h[4] == 0 || run(h[1], h[0], h[2], h[3], h[4], in, got) != 0) return 2;
        if (got != want) {
            std::fprintf(stderr, "case %d (kind %u curve %u mode %u n %u lanes %u) differs\n", cases, h[0], h[1], h[2], h[3], h[4]);
            return 1;
        }
        cases++;
    }
    std::printf("%d cases equal\n", cases);
    return 0;
}
