// hostcheck_xyz_var.cpp — TEST INFRASTRUCTURE.  The lane body of the projective-to-affine conversion kernel of the
// variable-time _xyz forms (k_xyz_affine, csrc/ecgpu_kernels.h; its body xyz_affine_lane, csrc/ecgpu_xyz.h) compiled with g++,
// every lane of a launch run in turn with the kernel's record stride (../hostcheck/batchinv_host.h), so that it can be checked
// against the oracle without a GPU.  Also the GPU tests' record generator: affine points rescaled by random z (X = x z, Y = y z, Z = z), on CPU threads.
// Nothing here is linked into libecgpu.so.
#include <cstring>
#include <thread>
#include <vector>

#include "../hostcheck/batchinv_host.h"

using namespace ecgpu;

namespace {

template <class C>
int xyz_affine(const uint8_t* xyz, size_t n, size_t nthreads, uint8_t* out_xy, uint8_t* out_inf, uint8_t* ok) {
    if (n == 0 || nthreads == 0) return n == 0 ? 0 : -1;
    ecgpu_host::xyz_affine<C>(xyz, n, nthreads, out_xy, out_inf, ok);
    return 0;
}

uint64_t splitmix(uint64_t* s) {
    uint64_t z = (*s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// out[i] = (x z : y z : z) for a random z in [2, p) of record i's own (Z = 0, Y = z for an identity); `shared` != 0: one z for all
template <class C>
int rescale(const uint8_t* xy, const uint8_t* inf, size_t n, uint64_t seed, int shared, uint8_t* out) {
    using F = Field<C>;
    constexpr int N = C::N, WB = WireBytes<C>::value;
    auto body = [&](size_t lo, size_t hi) {
        for (size_t i = lo; i < hi; i++) {
            uint64_t s = seed * 0x2545F4914F6CDD1Dull + (shared ? 0 : i);
            uint32_t cz[N], cx[N], cy[N], w[N];
            for (int k = 0; k < N; k++) cz[k] = (uint32_t)splitmix(&s);
            cz[N - 1] %= C::P[N - 1];                      // below p's top word: below p
            if (mp_is_zero<N>(cz) || mp_is_one<N>(cz)) cz[0] = 2;
            uint8_t* o = out + i * 3 * WB;
            if (inf && inf[i]) {
                for (int k = 0; k < N; k++) w[k] = 0;
                store_be_wire<C>(o, w);
                store_be_wire<C>(o + WB, cz);
                store_be_wire<C>(o + 2 * WB, w);
                continue;
            }
            load_be_wire<C>(cx, xy + i * 2 * WB);
            load_be_wire<C>(cy, xy + i * 2 * WB + WB);
            const auto z = F::from_canonical(cz);
            F::to_canonical(w, F::mul(F::from_canonical(cx), z));
            store_be_wire<C>(o, w);
            F::to_canonical(w, F::mul(F::from_canonical(cy), z));
            store_be_wire<C>(o + WB, w);
            store_be_wire<C>(o + 2 * WB, cz);
        }
    };
    const size_t nt = n < 4096 ? 1 : 16;
    std::vector<std::thread> th;
    for (size_t t = 0; t < nt; t++) th.emplace_back(body, n * t / nt, n * (t + 1) / nt);
    for (auto& t : th) t.join();
    return 0;
}

#define DISPATCH ECGPU_HOST_DISPATCH

}  // namespace

extern "C" {

// the conversion of n records by `nthreads` lanes; ok[i] = 0 for a bad record
int hx_xyz_affine(int curve, const uint8_t* xyz, size_t n, size_t nthreads, uint8_t* out_xy, uint8_t* out_inf, uint8_t* ok) {
    DISPATCH(curve, xyz_affine, (xyz, n, nthreads, out_xy, out_inf, ok))
}

int hx_rescale(int curve, const uint8_t* xy, const uint8_t* inf, size_t n, uint64_t seed, int shared, uint8_t* out_xyz) {
    DISPATCH(curve, rescale, (xy, inf, n, seed, shared, out_xyz))
}

}  // extern "C"
