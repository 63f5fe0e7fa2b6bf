// hostcheck_pke.cpp — TEST INFRASTRUCTURE.  The lane bodies of the SM2 public-key encryption kernels (csrc/ecgpu_pke.h: k_pke_load,
// k_pke_point, k_pke_seal, k_pke_open) compiled with g++ and run element by element with the kernels' record layout, so that they
// can be checked against tests/pke_model.py without a GPU.  The two multiplications between the steps are not here: the test takes
// them from tests/hostcheck (the CPU build of the `_ct` kernels' algorithms).  Nothing here is linked into libecgpu.so.
//
// With -DHOSTCHECK_PKE_MAIN the same source is a stand-alone program (built with -fsanitize=address,undefined by
// tests/test_hostcheck_pke.py): it reads one element per line — scalar, point, x2 || y2 and message in hex, "-" for an empty
// message — runs load, seal and open on buffers of exactly the records' sizes and prints what they wrote.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../elliptic-curves_amd/csrc/ecgpu_pke.h"

using namespace ecgpu;
using C = Sm2Params;

extern "C" {

// k_pke_load + k_pke_point
int hp_load(const uint8_t* s_in, const uint8_t* xy_in, size_t n, uint8_t* s_out, uint8_t* xy_out, uint8_t* flag) {
    for (size_t i = 0; i < n; i++) {
        flag[i] = pke_load_scalar<C>(s_out + i * 32, s_in + i * 32) ? 1 : 0;
        const bool ok = pke_load_point<C>(xy_out + i * 64, xy_in + i * 64);
        flag[i] = (uint8_t)(flag[i] & (ok ? 1 : 0));
    }
    return 0;
}

// k_pke_seal
int hp_seal(const uint8_t* x2y2, const uint8_t* flag, const uint8_t* msgs, size_t msg_len, size_t n, uint8_t* c1, uint8_t* c2, uint8_t* c3,
            uint8_t* ok) {
    const bool words = pke_word_aligned(msgs, c2, msg_len);
    for (size_t i = 0; i < n; i++)
        ok[i] = pke_seal_lane(x2y2 + i * 64, flag[i], msgs + i * msg_len, msg_len, c1 + i * 64, c2 + i * msg_len, c3 + i * 32, words) ? 1 : 0;
    return 0;
}

// k_pke_open
int hp_open(const uint8_t* x2y2, const uint8_t* flag, const uint8_t* c2, size_t msg_len, const uint8_t* c3, size_t n, uint8_t* msgs_out,
            uint8_t* ok) {
    const bool words = pke_word_aligned(c2, msgs_out, msg_len);
    for (size_t i = 0; i < n; i++)
        ok[i] = pke_open_lane(x2y2 + i * 64, flag[i], c2 + i * msg_len, msg_len, c3 + i * 32, msgs_out + i * msg_len, words) ? 1 : 0;
    return 0;
}

}  // extern "C"

#ifdef HOSTCHECK_PKE_MAIN
namespace {
std::vector<uint8_t> unhex(const std::string& s) {
    std::vector<uint8_t> out;
    if (s == "-") return out;
    for (size_t i = 0; i + 1 < s.size(); i += 2) out.push_back((uint8_t)std::stoi(s.substr(i, 2), nullptr, 16));
    return out;
}
void put(const char* name, const std::vector<uint8_t>& v) {
    std::printf(" %s=", name);
    if (v.empty()) std::printf("-");
    for (uint8_t b : v) std::printf("%02x", b);
}
}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    char a[128], b[256], c[256], d[4096];
    while (std::fscanf(f, "%127s %255s %255s %4095s", a, b, c, d) == 4) {
        const std::vector<uint8_t> s_in = unhex(a), p_in = unhex(b), x2y2 = unhex(c), msg = unhex(d);
        if (s_in.size() != 32 || p_in.size() != 64 || x2y2.size() != 64) return 3;
        // (every buffer its record's exact size, so that the sanitizer sees one byte too many; never a null data pointer)
        const size_t len = msg.size(), cap = len ? len : 1;
        std::vector<uint8_t> s_out(32), p_out(64), flag(1), c1(p_in), m_in(cap), c2(cap), c3(32), ok(1), m_out(cap), ok2(1);
        if (len) std::memcpy(m_in.data(), msg.data(), len);
        hp_load(s_in.data(), p_in.data(), 1, s_out.data(), p_out.data(), flag.data());
        hp_seal(x2y2.data(), flag.data(), m_in.data(), len, 1, c1.data(), c2.data(), c3.data(), ok.data());
        // open what seal wrote (the zero records of an element without a verdict do not open)
        hp_open(x2y2.data(), flag.data(), c2.data(), len, c3.data(), 1, m_out.data(), ok2.data());
        c2.resize(len);
        m_out.resize(len);
        put("s", s_out); put("p", p_out); put("flag", flag); put("c1", c1); put("c2", c2); put("c3", c3); put("ok", ok);
        put("m", m_out); put("ok2", ok2);
        std::printf("\n");
    }
    std::fclose(f);
    return 0;
}
#endif
