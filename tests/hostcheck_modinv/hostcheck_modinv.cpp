// hostcheck_modinv.cpp — TEST INFRASTRUCTURE.  The inversions of csrc/ecgpu_modinv.h as a stand-alone host program, for a build with
// AddressSanitizer + UBSan (tests/test_modinv_vectors.py): the same functions tests/hostcheck runs as field ops 4 and 17, scalar op 1
// and the raw-domain ops 46 and 47, on the vectors of a file.
//
//   hostcheck_modinv FILE        FILE: one "<curve id> <op> <hex of the operand's wire bytes>" per line; op 4 / 17: F::inv / F::inv<true>
//                                on a canonical operand, 1: ScalarN::inv, 46 / 47: the raw-domain inversions.
// Prints the hex of the result's wire bytes, one line per input line.  Exit status 2 for a malformed line or a non-canonical operand.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../elliptic-curves_amd/csrc/ecgpu_field.h"
#include "../../elliptic-curves_amd/csrc/ecgpu_scalar.h"
#include "../../elliptic-curves_amd/csrc/ecgpu_selftest_raw.h"

using namespace ecgpu;

namespace {

template <class C>
int run(int op, const std::vector<uint8_t>& in, std::vector<uint8_t>& out) {
    using F = Field<C>;
    constexpr size_t WB = WireBytes<C>::value;
    if (in.size() != WB) return 2;
    out.assign(WB, 0);
    uint32_t w[C::N], zero[C::N] = {0}, r[C::N];
    if (op == 4 || op == 17) {
        bool ok;
        const auto x = F::from_bytes(in.data(), &ok);
        if (!ok) return 2;
        if (op == 4) F::to_bytes(out.data(), F::inv(x));
        else F::to_bytes(out.data(), F::template inv<true>(x));
        return 0;
    }
    load_be_wire<C>(w, in.data());
    if (op == 1) {
        if (!selftest_scalar<C>(1, w, zero, r)) return 2;
    } else if (!selftest_field_raw<C>(op, w, zero, r)) {
        return 2;
    }
    store_be_wire<C>(out.data(), r);
    return 0;
}

int dispatch(int curve, int op, const std::vector<uint8_t>& in, std::vector<uint8_t>& out) {
    switch (curve) {
    case 0: return run<K256Params>(op, in, out);
    case 1: return run<P256Params>(op, in, out);
    case 2: return run<P384Params>(op, in, out);
    case 3: return run<Sm2Params>(op, in, out);
    case 4: return run<P224Params>(op, in, out);
    case 5: return run<P192Params>(op, in, out);
    case 6: return run<P521Params>(op, in, out);
    case 7: return run<Bp256Params>(op, in, out);
    case 8: return run<Bp384Params>(op, in, out);
    case 9: return run<Bp256t1Params>(op, in, out);
    case 10: return run<Bp384t1Params>(op, in, out);
    case 11: return run<Bign256Params>(op, in, out);
    default: return 2;
    }
}

int nibble(char ch) {
    if (ch >= '0' && ch <= '9') return ch - '0';
    if (ch >= 'a' && ch <= 'f') return ch - 'a' + 10;
    return -1;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    char line[512];
    int rc = 0;
    while (rc == 0 && std::fgets(line, sizeof line, f)) {
        int curve, op, used = 0;
        if (std::sscanf(line, "%d %d %n", &curve, &op, &used) != 2) { rc = 2; break; }
        std::vector<uint8_t> in, out;
        const char* h = line + used;
        while (nibble(h[0]) >= 0 && nibble(h[1]) >= 0) {
            in.push_back((uint8_t)(nibble(h[0]) * 16 + nibble(h[1])));
            h += 2;
        }
        rc = dispatch(curve, op, in, out);
        if (rc != 0) break;
        std::string s;
        for (uint8_t b : out) {
            s += "0123456789abcdef"[b >> 4];
            s += "0123456789abcdef"[b & 15];
        }
        std::puts(s.c_str());
    }
    std::fclose(f);
    return rc;
}
