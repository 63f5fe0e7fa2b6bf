// hostcheck_bignsign.cpp — TEST INFRASTRUCTURE.  The lane bodies of the bign signing kernels (csrc/ecgpu_bignsign.h: k_bign_genk,
// k_bign_genk_retry, k_bign_sign_s0, k_bign_sign_finish) and both S-box access policies of csrc/ecgpu_belt.h compiled with g++ and
// run element by element with the kernels' record layout, so that they can be checked against tests/bignsign_model.py without a
// GPU — and with values no real input reaches (S0 = 0, a smaller acceptance bound, a cleared flag).  The multiplication R = k G is
// not here.  Nothing here is linked into libecgpu.so.
//
// With -DHOSTCHECK_BIGNSIGN_MAIN the same source is a stand-alone program (built with -fsanitize=address,undefined by
// tests/test_hostcheck_bignsign.py): it reads one element per line — d, the prehash, the bound, k, the nonce's flag, x(R), S0 in
// hex and a message ("-" for an empty one) — runs the bodies on buffers of exactly the records' sizes and prints what they wrote.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../elliptic-curves_amd/csrc/ecgpu_bignsign.h"

using namespace ecgpu;
using C = Bign256Params;

namespace {
void load_le8(uint32_t* w, const uint8_t* b, int nw = 8) {
    for (int j = 0; j < nw; j++) w[j] = (uint32_t)b[4 * j] | (uint32_t)b[4 * j + 1] << 8 | (uint32_t)b[4 * j + 2] << 16 | (uint32_t)b[4 * j + 3] << 24;
}
void store_le8(uint8_t* b, const uint32_t* w, int nw = 8) {
    for (int j = 0; j < nw; j++)
        for (int t = 0; t < 4; t++) b[4 * j + t] = (uint8_t)(w[j] >> (8 * t));
}
}  // namespace

extern "C" {

// the four lookups of one word under each policy (no rotation)
uint32_t hb_sub_table(uint32_t u) { return Belt::sub(Belt::H, u); }
uint32_t hb_sub_ct(uint32_t u) { return Belt::sub(Belt::CtSbox(), u); }

// belt-block under either policy: x 16 bytes, key 32 bytes
void hb_block(int ct, const uint8_t* x, const uint8_t* key, uint8_t* y) {
    uint32_t xw[4], kw[8], yw[4];
    load_le8(xw, x, 4);
    load_le8(kw, key, 8);
    if (ct) Belt::block(Belt::CtSbox(), yw, xw, kw);
    else Belt::block(Belt::H, yw, xw, kw);
    store_le8(y, yw, 4);
}

// belt-hash under either policy
void hb_hash(int ct, const uint8_t* msg, size_t len, uint8_t* out) {
    uint32_t hw[8];
    const HashPiece pc[1] = {{msg, len}};
    if (ct) Belt::hash_pieces<1>(Belt::CtSbox(), hw, pc);
    else Belt::hash_pieces<1>(Belt::H, hw, pc);
    store_le8(out, hw);
}

// k_bign_genk followed by k_bign_genk_retry: bound 32 bytes little-endian, cap candidates; rounds = the state's counter afterwards
int hb_genk(const uint8_t* d_in, const uint8_t* h_in, const uint8_t* bound, size_t n, int cap, uint8_t* k_out, uint8_t* flag,
            uint32_t* rounds) {
    uint32_t bw[8];
    load_le8(bw, bound);
    for (size_t i = 0; i < n; i++) {
        uint32_t d[8], h[8], k[8];
        load_le8(d, d_in + i * 32);
        load_le8(h, h_in + i * 32);
        BignGenkState st;
        bool ok = bign_genk_first_words<C>(Belt::CtSbox(), d, h, bw, k, st);
        if (!ok) ok = bign_genk_retry_words(Belt::CtSbox(), st, bw, cap, k);
        flag[i] = ok ? 1 : 0;
        rounds[i] = st.i;
        store_le8(k_out + i * 32, k);
    }
    return 0;
}

// k_bign_sign_s0; rx: x(R) alone, 32 bytes per element
int hb_s0(const uint8_t* h_in, const uint8_t* rx_in, size_t n, uint8_t* s0_out) {
    for (size_t i = 0; i < n; i++) {
        uint32_t s0[4];
        bign_sign_s0_words(Belt::H, s0, rx_in + i * 32, h_in + i * 32);
        store_le8(s0_out + i * 16, s0, 4);
    }
    return 0;
}

// k_bign_sign_finish
int hb_finish(const uint8_t* d_in, const uint8_t* k_in, const uint8_t* k_flag, const uint8_t* h_in, const uint8_t* s0_in,
              const uint8_t* r_inf, size_t n, uint8_t* sig, uint8_t* ok) {
    for (size_t i = 0; i < n; i++) {
        uint32_t d[8], k[8], h[8], s0[4], o0[4], o1[8];
        load_le8(d, d_in + i * 32);
        load_le8(k, k_in + i * 32);
        load_le8(h, h_in + i * 32);
        load_le8(s0, s0_in + i * 16, 4);
        ok[i] = bign_sign_finish_words<C>(d, k, k_flag[i] != 0, h, s0, r_inf[i] != 0, o0, o1) ? 1 : 0;
        store_le8(sig + i * 48, o0, 4);
        store_le8(sig + i * 48 + 16, o1);
    }
    return 0;
}

}  // extern "C"

#ifdef HOSTCHECK_BIGNSIGN_MAIN
namespace {
std::vector<uint8_t> unhex(const std::string& s) {
    std::vector<uint8_t> out;
    if (s == "-") return out;
    for (size_t i = 0; i + 1 < s.size(); i += 2) out.push_back((uint8_t)std::stoi(s.substr(i, 2), nullptr, 16));
    return out;
}
void put(const char* name, const std::vector<uint8_t>& v) {
    std::printf(" %s=", name);
    for (uint8_t b : v) std::printf("%02x", b);
}
}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    static char a[80], b[80], c[80], d[80], e[80], g[40], m[4096];
    int kf = 0;
    while (std::fscanf(f, "%79s %79s %79s %79s %d %79s %39s %4095s", a, b, c, d, &kf, e, g, m) == 8) {
        const std::vector<uint8_t> dd = unhex(a), hh = unhex(b), bound = unhex(c), kk = unhex(d), rx = unhex(e), s0in = unhex(g), msg = unhex(m);
        if (dd.size() != 32 || hh.size() != 32 || bound.size() != 32 || kk.size() != 32 || rx.size() != 32 || s0in.size() != 16) return 3;
        // exactly the message's bytes on the heap (one byte for an empty one: never a null data pointer)
        const std::vector<uint8_t> mb = msg.empty() ? std::vector<uint8_t>(1) : msg;
        const std::vector<uint8_t> kflag(1, (uint8_t)kf), rinf(1, 0);
        std::vector<uint8_t> cand(32), cflag(1), s0(16), sig(48), ok(1), sig2(48), ok2(1), hm(32), hm2(32);
        std::vector<uint32_t> rounds(1);
        hb_genk(dd.data(), hh.data(), bound.data(), 1, 128, cand.data(), cflag.data(), rounds.data());
        hb_s0(hh.data(), rx.data(), 1, s0.data());
        hb_finish(dd.data(), kk.data(), kflag.data(), hh.data(), s0.data(), rinf.data(), 1, sig.data(), ok.data());
        hb_finish(dd.data(), kk.data(), kflag.data(), hh.data(), s0in.data(), rinf.data(), 1, sig2.data(), ok2.data());
        hb_hash(1, mb.data(), msg.size(), hm.data());
        hb_hash(0, mb.data(), msg.size(), hm2.data());
        if (hm != hm2) return 4;
        put("cand", cand); put("cflag", cflag);
        std::printf(" rounds=%u", rounds[0]);
        put("s0", s0); put("sig", sig); put("ok", ok); put("sig2", sig2); put("ok2", ok2); put("hash", hm);
        std::printf("\n");
    }
    std::fclose(f);
    return 0;
}
#endif
