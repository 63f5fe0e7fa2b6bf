// ecgpu_api.hip — the C ABI of include/ecgpu.h on top of the gfx950 kernels.
// No torch, no CPU compute path: every entry point either runs HIP kernels or returns an error.

#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <atomic>
#include <chrono>
#include <map>
#include <set>
#include <mutex>
#include <string>
#include <thread>
#include <tuple>
#include <vector>

#include "../../include/ecgpu.h"
#include "ecgpu_launch.h"
#include "ecgpu_hash.h"
#include "ecgpu_knobs.h"
#include "ecgpu_recode.h"
#include "ecgpu_x448.h"

using namespace ecgpu;

namespace {

constexpr int BLOCK = 256;
enum : int { ST_BAD_SCALAR = 1, ST_BAD_POINT = 2 };

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    size_t dirty = 0;         // bytes from the start that calls have asked for since the buffer was last wiped (wipe_scratch zeroes these, not cap)
    size_t used = 0;          // the most any call has asked for (never reset): beyond it the allocation was never written by this context
};

// A context's view of a basepoint comb table.  The table itself is owned by the per-device registry below and shared by
// every context of the process on that device (the analogue of the reference's process-wide `LazyLock<BasepointTable>`,
// k256/src/arithmetic/tables.rs:18): the 21.5 GB k256 table is built and held once per GPU however many contexts exist.
struct Table {
    uint32_t* d = nullptr;
    int w = 0, nwin = 0;      // the width actually in use (may be narrower than asked for after an out-of-memory fallback)
    int asked = 0;            // the width this view was made for (ctx->want_w at that time)
};

struct SharedTable {
    uint32_t* d = nullptr;
    int nwin = 0, refs = 0;
    size_t bytes = 0;         // device memory of the table
    double build_ms = 0;      // host wall time of its construction (allocation, kernels, the wait for them)
};
struct TableRegistry {
    std::mutex mu;                                               // held while a table is built: a second context of the device waits
    std::map<std::tuple<int, int, int>, SharedTable> tabs;       // (device, curve id, comb width)
    // widths whose allocation was refused -> calls left before the width is tried again: later contexts go straight to the
    // width that worked, but a refusal is not for ever (the memory may have been another process's or torch's cache);
    // forgotten at once when a table of the device is freed or enough memory shows as free
    std::map<std::tuple<int, int, int>, int> nofit;
    uint64_t seen[12] = {};                                      // generator multiplications asked of this device so far, per curve
};
constexpr int NOFIT_RETRY_CALLS = 64;
// adaptive policy: generator multiplications (log2) after which a device moves from the 16-bit table to the 22-bit one and from
// there to the context's widest (table_tier below)
constexpr int TABLE_TIER1_LOG2 = 26, TABLE_TIER2_LOG2 = 29;
// test-only fault injection (tests/test_gpu_multidevice.py through the exported ecgpu_testhook_table_max_mb; no environment
// variable: the production path cannot be steered from outside the process): comb tables above this many MiB are refused
std::atomic<size_t> g_test_table_max_mb{0};
TableRegistry& table_registry(int device) {                      // one per device: the GPUs of a group build in parallel
    static TableRegistry* r = new TableRegistry[64];             // never destroyed: contexts may outlive static destructors
    return r[device & 63];
}

}  // namespace

struct ecgpu_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr, stream = nullptr;
    hipStream_t up_stream = nullptr, down_stream = nullptr;   // host <-> device legs of the pipelined host-pointer calls
    std::string err;
    int* d_status = nullptr;
    int* h_status = nullptr;
    Table table[12];
    uint32_t* ct_lut[12] = {};   // uniform-schedule generator LUTs (shared per device like the comb tables; registry width key -1)
    // fixed-base comb width: every addition removed is worth 8 % and HBM keeps up with the gathers, so the tables are
    // sized for 288 GB, not for a cache.  k256: W = 26, 10 windows = 9 additions per scalar, 21.5 GB, built in 65 ms;
    // p256 and sm2: W = 24, 11 windows, 5.9 GB; p384: W = 20, 1.0 GB.  ecgpu_set_base_window trades memory for speed.
    int want_w[12] = {26, 24, 20, 24, 24, 24, 20, 24, 20, 24, 20, 24};
    // Footprint policy (ecgpu_set_table_policy / ecgpu_set_table_budget / ecgpu_set_base_window): want_w is the WIDEST table a
    // context will use; unless the width is pinned or the policy is eager, the table grows with the number of generator
    // multiplications the device has been asked for (table_tier) — the reference builds its 30-60 KB tables lazily and prices
    // a table half the size at 3 % (k256/src/arithmetic/mul.rs:191-192, primeorder/src/tables/basepoint.rs:29-76)
    bool w_pinned[12] = {};
    int table_policy = 0;        // ECGPU_TABLE_ADAPTIVE
    size_t table_budget = 0;     // bytes one comb table may take; 0 = no limit
    int msm_c = 0;   // 0 = choose from n
    DevBuf proj, prefix, vtab, bases, in0, in1, in2, in3, out0, out1, msm_ws;
    DevBuf ec_u1, ec_u2, ec_q, ec_valid, ec_xy, ec_inf, ec_r, ec_e, ec_s, ec_id;   // signature verification scratch
    DevBuf ec_winv;                    // the batch's s^-1 / r^-1 modulo the group order (k_scalar_batch_inv; its prefix products use `prefix`)
    DevBuf ct_flags;             // one verdict byte per element of a uniform-schedule batch
    DevBuf sg_k, sg_flag, sg_state, sg_dp;   // signing: the nonces handed to k_fixed_base_ct, their verdicts, the RFC 6979 generator's
                                 // K / V state between its two kernels, the fixed-up Schnorr key d' || x(P) — all wiped behind the call
    DevBuf out2;                 // a third staged output (the recovery ids of the host-pointer signing calls)
    DevBuf out3;                 // a fourth (ecgpu_sm2_pke_encrypt_batch: C1, C2, C3 and ok)
    int rfc6979_cap = 128;       // candidates the RFC 6979 generator tries per element; lowered by the tests only
                                 // (ecgpu_testhook_rfc6979_max_candidates, this context alone)
    DevBuf cx_xy, cx_inf;        // x || y + flag records decoded from compressed input (ecgpu_msm_compressed, ecgpu_batch_mul_compressed)
                                 // or converted from projective input (the variable-time _xyz forms; their product chain uses `prefix`)
    bool keep_status = false;    // the status word already holds the verdicts of a first stage of the call: do not clear it
    hipEvent_t ev[9] = {};       // 0..2 call spans, 3..4 the MSM's sort / accumulate marks, 5 spare, 6..8 MsmPlan::detail
    std::map<std::string, double> timing;
    std::vector<std::pair<std::string, std::pair<int, int>>> spans;   // event pairs of the last call not yet turned into `timing`
    // asynchronous mode (ecgpu_set_async): device-pointer calls return once their work is queued; the status word
    // accumulates on the device until ecgpu_synchronize (or a host-pointer call) collects it into `deferred`
    bool async = false, pending = false;
    bool timing_on = true;       // ecgpu_set_timing: per-call HIP events (ecgpu_last_timing)
    int deferred = 0;
    // MSM lanes (ecgpu_set_msm_lanes): in asynchronous mode consecutive MSMs alternate between two internal streams, each with
    // a workspace of its own, so that the sort and the reduction tail of one MSM (bandwidth- and latency-bound) run beside the
    // accumulation of the other (issue-bound)
    struct MsmLane {
        hipStream_t s = nullptr;
        DevBuf ws, proj, prefix;
        DevBuf cx_xy, cx_inf;              // x || y + flag records converted from X || Y || Z input on this lane (ecgpu_msm_xyz_dev)
        hipEvent_t ev_in = nullptr, ev_a = nullptr, ev_b = nullptr, ev_done = nullptr;
        const void* parts_out = nullptr;   // the parts record an ecgpu_msm_parts_dev on this lane wrote last (ecgpu_msm_parts_join_dev)
    };
    bool lanes_pending = false;  // an MSM was queued on a lane since the last other call: that call first waits for the lanes (ev_done)
    int msm_lanes = 1;
    unsigned msm_seq = 0;
    MsmLane lane[4];
    int lane_last = -1;          // the lane of the last MSM queued on one (ecgpu_last_timing "accumulate" reads its events)
};

namespace {

#define HIP_TRY(ctx, expr)                                                                      \
    do {                                                                                        \
        hipError_t e_ = (expr);                                                                 \
        if (e_ != hipSuccess) {                                                                 \
            (ctx)->err = std::string(#expr) + ": " + hipGetErrorString(e_);                     \
            return e_ == hipErrorOutOfMemory ? ECGPU_ERR_OOM : ECGPU_ERR_HIP;                   \
        }                                                                                       \
    } while (0)

// grows a scratch buffer to `bytes`; a buffer that has to move is freed behind the work of `stream`, the stream of the context
// it is used on (the context's own, or an MSM lane's)
int ensure_on(ecgpu_ctx* ctx, hipStream_t stream, DevBuf& b, size_t bytes) {
    if (bytes > b.dirty) b.dirty = bytes;
    if (bytes > b.used) b.used = bytes;
    if (bytes <= b.cap) return ECGPU_OK;
    if (b.p) {
        HIP_TRY(ctx, hipStreamSynchronize(stream));
        HIP_TRY(ctx, hipFree(b.p));
        b.p = nullptr;
        b.cap = 0;
    }
    size_t want = bytes + bytes / 8 + 4096;
    HIP_TRY(ctx, hipMalloc(&b.p, want));
    b.cap = want;
    return ECGPU_OK;
}
inline int ensure(ecgpu_ctx* ctx, DevBuf& b, size_t bytes) { return ensure_on(ctx, ctx->stream, b, bytes); }

template <class F>
int dispatch(int curve, F&& f) {
    switch (curve) {
    case ECGPU_K256: return f(K256Params{});
    case ECGPU_P256: return f(P256Params{});
    case ECGPU_P384: return f(P384Params{});
    case ECGPU_SM2: return f(Sm2Params{});
    case ECGPU_P224: return f(P224Params{});
    case ECGPU_P192: return f(P192Params{});
    case ECGPU_P521: return f(P521Params{});
    case ECGPU_BP256: return f(Bp256Params{});
    case ECGPU_BP384: return f(Bp384Params{});
    case ECGPU_BP256T1: return f(Bp256t1Params{});
    case ECGPU_BP384T1: return f(Bp384t1Params{});
    case ECGPU_BIGN256: return f(Bign256Params{});
    default: return ECGPU_ERR_CURVE;
    }
}

inline unsigned grid_for(size_t n) { return (unsigned)((n + BLOCK - 1) / BLOCK); }

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// MSMs in flight on the lanes: whatever the context does next on its own stream is ordered after them
int join_lanes(ecgpu_ctx* ctx) {
    if (!ctx->lanes_pending) return ECGPU_OK;
    for (auto& l : ctx->lane)
        if (l.s && l.ev_done) HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, l.ev_done, 0));
    ctx->lanes_pending = false;
    return ECGPU_OK;
}

int reset_status(ecgpu_ctx* ctx) {
    int rc = join_lanes(ctx);
    if (rc != ECGPU_OK) return rc;
    if (ctx->async || ctx->keep_status) return ECGPU_OK;          // flags accumulate until ecgpu_synchronize / the call's end
    HIP_TRY(ctx, hipMemsetAsync(ctx->d_status, 0, sizeof(int), ctx->stream));
    return ECGPU_OK;
}

int status_error(ecgpu_ctx* ctx, int st) {
    if (st & ST_BAD_SCALAR) { ctx->err = "scalar not in [0, n)"; return ECGPU_ERR_SCALAR_RANGE; }
    if (st & ST_BAD_POINT) { ctx->err = "point coordinate >= p or not on curve"; return ECGPU_ERR_POINT; }
    return ECGPU_OK;
}

// reads the status word back (synchronises the stream) and maps it to an error code; asynchronous mode: returns at once,
// the word is read by drain()
int finish(ecgpu_ctx* ctx) {
    HIP_TRY(ctx, hipGetLastError());
    if (ctx->async) {
        ctx->pending = true;
        return ECGPU_OK;
    }
    HIP_TRY(ctx, hipMemcpyAsync(ctx->h_status, ctx->d_status, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return status_error(ctx, *ctx->h_status);
}

// asynchronous mode: wait for the queued work, move its status flags into ctx->deferred, clear the device word
int drain(ecgpu_ctx* ctx) {
    for (auto& l : ctx->lane)                  // queued MSMs on the lanes: their status flags land in the same word
        if (l.s) HIP_TRY(ctx, hipStreamSynchronize(l.s));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->h_status, ctx->d_status, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(ctx->d_status, 0, sizeof(int), ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->deferred |= *ctx->h_status;
    ctx->pending = false;
    return ECGPU_OK;
}

// A host-pointer call on an asynchronous context runs synchronously: it first waits for the queued work (whose errors stay
// deferred for ecgpu_synchronize), and reports its own errors itself.
struct SyncScope {
    ecgpu_ctx* ctx;
    bool was;
    int rc = ECGPU_OK;      // a failed drain (sticky device fault of the queued work, failed copy): the entry point returns it
    explicit SyncScope(ecgpu_ctx* c) : ctx(c), was(c && c->async) {        // (no context: nothing to do, HostCall reports it)
        if (was) {
            rc = drain(ctx);
            ctx->async = false;
        }
    }
    ~SyncScope() {
        if (was) {
            (void)hipMemsetAsync(ctx->d_status, 0, sizeof(int), ctx->stream);
            ctx->async = true;
        }
    }
};

// The uniform-schedule entry points are meant for secret scalars, and the reference keeps such values in zeroize-on-drop
// types (`NonZeroScalar`, `SharedSecret`).  Whatever path such a call leaves by, the context's scratch that held values derived
// from its secrets — k P in projective form, the running products of the batch inversion, the affine products of an ECDH —
// is zeroed behind its last kernel (stream-ordered), and `staging` also clears the copies a host-pointer call made of the
// caller's scalars and results.  The caller's own buffers are the caller's to wipe; ecgpu_wipe does the same on request.
enum : int { WIPE_SCRATCH = 1, WIPE_EC = 2, WIPE_STAGING = 4, WIPE_SIGN = 8, WIPE_PREHASH = 16 };
void wipe_bufs(ecgpu_ctx* ctx, std::initializer_list<DevBuf*> bufs) {
    // what has been asked of a buffer since its last wipe, not its capacity: after one 2^20-term batch the scratch holds
    // ~170 MB, and zeroing all of it behind every later 1,024-scalar `_ct` call (or every chunk of a pipelined one) cost tens
    // of microseconds per call
    for (DevBuf* b : bufs) {
        if (b->p && b->dirty) (void)hipMemsetAsync(b->p, 0, b->dirty < b->cap ? b->dirty : b->cap, ctx->stream);
        b->dirty = 0;
    }
}
void wipe_scratch(ecgpu_ctx* ctx, int what) {
    if (what & WIPE_SCRATCH) wipe_bufs(ctx, {&ctx->proj, &ctx->prefix});
    if (what & WIPE_EC) wipe_bufs(ctx, {&ctx->ec_xy, &ctx->ec_inf});
    if (what & WIPE_STAGING) wipe_bufs(ctx, {&ctx->in0, &ctx->in3, &ctx->out0, &ctx->out1});
    if (what & WIPE_SIGN) wipe_bufs(ctx, {&ctx->sg_k, &ctx->sg_flag, &ctx->sg_state, &ctx->sg_dp, &ctx->ct_flags});
    // SM2DSA signing keeps e = SM3(Z || M) in ec_e.  Z hashes PA = d G, a PUBLIC value, so e is no more secret than the z that
    // ecdsa_sign_dev leaves in the same buffer; it is zeroed all the same because the contract of these calls lists the e buffer
    // among what is wiped behind them (include/ecgpu.h)
    if (what & WIPE_PREHASH) wipe_bufs(ctx, {&ctx->ec_e});
}
struct CtWipe {
    ecgpu_ctx* ctx;
    int what;
    CtWipe(ecgpu_ctx* c, int what_) : ctx(c), what(what_) {}
    ~CtWipe() {
        if (what) wipe_scratch(ctx, what);
    }
};

void record(ecgpu_ctx* ctx, int i) {
    if (ctx->timing_on) (void)hipEventRecord(ctx->ev[i], ctx->stream);
}

void resolve_timing(ecgpu_ctx* ctx) {
    if (ctx->spans.empty()) return;
    ctx->timing.clear();
    for (auto& s : ctx->spans) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, ctx->ev[s.second.first], ctx->ev[s.second.second]) == hipSuccess)
            ctx->timing[s.first] = ms;
        else
            (void)hipGetLastError();         // a mark the call never recorded (an MSM of no terms): no span, and no error left behind
    }
    ctx->spans.clear();
}

// The spans of a call: stage name -> the pair of event marks around it (record).  The three-span default, and the variants of the
// MSM (with and without the detail marks of MsmPlan), of ecgpu_lincomb_ct, of the verifiers ("recode" = their prepare kernel) and
// of the calls without a normalisation of their own (ecgpu_msm_parts_dev, ecgpu_batch_decompress_dev).
// "accumulate" is the accumulation kernel alone; "reduce" = everything after it = "finish" (bucket finish + running sums) +
// "tree" (over the segment sums) + "combine" (window sums, Horner chain, conversion to affine); "sort" = "prepare" + the sort
struct Span { const char* name; int from, to; };
struct SpanList {
    const Span* p;
    size_t n;
    template <size_t N> constexpr SpanList(const Span (&a)[N]) : p(a), n(N) {}
};
constexpr Span SPANS_DEFAULT[] = {{"main", 0, 1}, {"normalize", 1, 2}, {"total", 0, 2}};
constexpr Span SPANS_MSM[] = {{"main", 0, 1}, {"normalize", 1, 2}, {"total", 0, 2}, {"sort", 0, 3}, {"accumulate", 3, 4}, {"reduce", 4, 1}};
constexpr Span SPANS_MSM_DETAIL[] = {{"main", 0, 1}, {"normalize", 1, 2}, {"total", 0, 2}, {"sort", 0, 3}, {"accumulate", 3, 4},
                                     {"reduce", 4, 1}, {"prepare", 0, 6}, {"finish", 4, 7}, {"tree", 7, 8}, {"combine", 8, 1}};
constexpr Span SPANS_LINCOMB_CT[] = {{"main", 0, 1}, {"normalize", 1, 2}, {"total", 0, 2}, {"accumulate", 0, 3}, {"reduce", 3, 1}};
constexpr Span SPANS_VERIFY[] = {{"recode", 0, 3}, {"main", 3, 1}, {"normalize", 1, 2}, {"total", 0, 2}};
constexpr Span SPANS_MSM_PARTS[] = {{"main", 0, 1}, {"total", 0, 1}, {"sort", 0, 3}, {"accumulate", 3, 4}, {"reduce", 4, 1}};
constexpr Span SPANS_NO_NORMALIZE[] = {{"main", 0, 1}, {"total", 0, 1}};
constexpr Span SPANS_H2C[] = {{"main", 0, 1}, {"normalize", 1, 2}, {"total", 0, 2}, {"expand", 0, 3}, {"map", 3, 1}};

// the spans of the call just made; turned into milliseconds now, or (asynchronous mode: the events have not happened
// yet) when ecgpu_last_timing asks
void collect_timing(ecgpu_ctx* ctx, SpanList spans) {
    ctx->spans.clear();
    ctx->lane_last = -1;
    if (!ctx->timing_on) {                     // no events were recorded for this call: ecgpu_last_timing has nothing to report
        ctx->timing.clear();
        return;
    }
    for (size_t i = 0; i < spans.n; i++) ctx->spans.emplace_back(spans.p[i].name, std::make_pair(spans.p[i].from, spans.p[i].to));
    if (!ctx->async) resolve_timing(ctx);
}

// ---- basepoint table ---------------------------------------------------------------------------------

// drops this context's reference to its table of curve `id`; the last reference frees the device memory
void release_table(ecgpu_ctx* ctx, int id) {
    Table& t = ctx->table[id];
    if (!t.d) return;
    TableRegistry& reg = table_registry(ctx->device);
    std::lock_guard<std::mutex> lock(reg.mu);
    auto it = reg.tabs.find(std::make_tuple(ctx->device, id, t.w));
    if (it != reg.tabs.end() && it->second.d == t.d && --it->second.refs == 0) {
        (void)hipFree(it->second.d);
        reg.tabs.erase(it);
        reg.nofit.clear();                    // memory came back: widths refused earlier may fit now
    }
    t = Table();
}

// builds the comb table of width w into freshly allocated device memory; ECGPU_ERR_OOM when the table (or its build
// scratch) does not fit
template <class C>
int build_table(ecgpu_ctx* ctx, int w, SharedTable* out) {
    constexpr int N = C::N, NS = Field<C>::NS;
    const int bits = 32 * N;
    const int nwin = signed_window_count(bits - 1, w);       // scalars are folded to bits - 1 bits (fold_scalar)
    const size_t half = (size_t)1 << (w - 1);
    const size_t entries = half * nwin;
    int rc;
    // windows are built in slabs so that the projective scratch (192 B per entry, 3x the table) stays below ~2 GB
    size_t slab = ((size_t)2 << 30) / (half * (4 * NS) * 4);
    if (slab < 1) slab = 1;
    if (slab > (size_t)nwin) slab = nwin;
    if ((rc = ensure(ctx, ctx->bases, (size_t)nwin * 3 * NS * 4)) != ECGPU_OK) return rc;
    if ((rc = ensure(ctx, ctx->proj, slab * half * 3 * NS * 4)) != ECGPU_OK) return rc;
    if ((rc = ensure(ctx, ctx->prefix, slab * half * NS * 4)) != ECGPU_OK) return rc;
    uint32_t* d = nullptr;
    const auto t_build0 = std::chrono::steady_clock::now();
    if (const size_t cap_mb = g_test_table_max_mb.load()) {     // fault injection for the fallback path (ecgpu_testhook_table_max_mb)
        if (entries * 2 * N * 4 > cap_mb << 20) {
            ctx->err = "basepoint table: allocation refused by the test hook";
            return ECGPU_ERR_OOM;
        }
    }
    HIP_TRY(ctx, hipMalloc(reinterpret_cast<void**>(&d), entries * 2 * N * 4));
    launch_window_bases<C>(ctx->stream, (uint32_t*)ctx->bases.p, w, nwin);
    for (size_t j0 = 0; j0 < (size_t)nwin; j0 += slab) {
        const size_t ws = j0 + slab <= (size_t)nwin ? slab : (size_t)nwin - j0;
        launch_table_entries<C>(ctx->stream, (const uint32_t*)ctx->bases.p + j0 * (3 * NS), (uint32_t*)ctx->proj.p, w, (int)ws);
        launch_normalize<C>(ctx->stream, true, (const uint32_t*)ctx->proj.p, (uint32_t*)ctx->prefix.p, ws * half, nullptr,
                            nullptr, d + j0 * half * (2 * N));
    }
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);     // visible to every stream of the device from here on
    if (e != hipSuccess) {
        (void)hipFree(d);
        ctx->err = std::string("basepoint table build: ") + hipGetErrorString(e);
        return e == hipErrorOutOfMemory ? ECGPU_ERR_OOM : ECGPU_ERR_HIP;
    }
    out->d = d;
    out->nwin = nwin;
    out->bytes = entries * 2 * N * 4;
    out->build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_build0).count();
    return ECGPU_OK;
}

// the build scratch is larger than most batches need: give it back
int drop_build_scratch(ecgpu_ctx* ctx) {
    for (DevBuf* b : {&ctx->proj, &ctx->prefix}) {
        if (b->cap > ((size_t)64 << 20)) {
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            HIP_TRY(ctx, hipFree(b->p));
            b->p = nullptr;
            b->cap = 0;
        }
    }
    return ECGPU_OK;
}

// bytes of the comb table of width w for curve C
template <class C>
size_t comb_table_bytes(int w) {
    return ((size_t)1 << (w - 1)) * (size_t)signed_window_count(32 * C::N - 1, w) * 2 * C::N * 4;
}

// The width the adaptive policy gives a device that has been asked for `seen` generator multiplications of a curve so far (the
// call being served included), capped by `wmax`.  Every step up is taken where the time the narrower table has cost so far equals
// the time the next table takes to build (a rent-or-buy rule: never more than twice the time of the best fixed choice, whatever
// the caller goes on to do) — measured on MI355X for k256, profiles/r05/table_tiers.txt: 16 bits = 34 MB built in 1 ms, 9
// windows more per scalar than at 26; 22 bits = 1.6 GB in 5 ms; 26 bits = 21.5 GB in 65 ms.
inline int table_tier(uint64_t seen, int wmax) {
    int w = seen < ((uint64_t)1 << TABLE_TIER1_LOG2) ? 16 : seen < ((uint64_t)1 << TABLE_TIER2_LOG2) ? 22 : wmax;
    return w < wmax ? w : wmax;
}

// Makes ctx->table[C::ID] point at the device's shared comb table for a call with n scalars: the width is the context's pinned
// width (ecgpu_set_base_window), the widest allowed one (eager policy) or the tier the device's history asks for (adaptive, the
// default), never above the budget (ecgpu_set_table_budget) — and a wider table another context of the device has already built
// is taken as it is.  The table is built if no context of this process has yet.  When it does not fit — the k256 maximum is
// 21.5 GB — the width is lowered two bits at a time (a quarter of the memory, one or two more additions per scalar; results
// do not depend on it) down to 16 bits (36 MB) before ECGPU_ERR_OOM is returned.
template <class C>
int ensure_table(ecgpu_ctx* ctx, size_t n = 0) {
    Table& t = ctx->table[C::ID];
    TableRegistry& reg = table_registry(ctx->device);
    std::unique_lock<std::mutex> lock(reg.mu);
    const int wmax = ctx->want_w[C::ID];
    uint64_t& seen = reg.seen[C::ID];
    seen = seen + n < seen ? ~(uint64_t)0 : seen + n;
    // the width this call should get, from the registry as it is NOW (called again whenever the lock was dropped)
    const auto choose = [&]() -> int {
        int want = wmax;
        if (ctx->w_pinned[C::ID]) return want;
        if (ctx->table_policy == ECGPU_TABLE_ADAPTIVE) want = table_tier(seen, wmax);
        if (ctx->table_budget)
            while (want > 4 && comb_table_bytes<C>(want) > ctx->table_budget) want--;
        for (int w = wmax; w > want; w--) {                      // somebody has paid for a wider one already
            auto it = reg.tabs.find(std::make_tuple(ctx->device, (int)C::ID, w));
            if (it != reg.tabs.end() && it->second.d && (!ctx->table_budget || it->second.bytes <= ctx->table_budget)) return w;
        }
        return want;
    };
    // a refusal of `w` on this device is on record: has it expired (memory back, or NOFIT_RETRY_CALLS calls old)?  Erases it if so.
    const auto refusal_over = [&](int w) -> bool {
        auto nf = reg.nofit.find(std::make_tuple(ctx->device, (int)C::ID, w));
        if (nf == reg.nofit.end()) return true;
        size_t free_b = 0, total_b = 0;
        const bool roomy = hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b > comb_table_bytes<C>(w) + ((size_t)3 << 30) &&
                           !g_test_table_max_mb.load();
        if (!roomy && --nf->second > 0) return false;
        reg.nofit.erase(nf);
        return true;
    };
    int want = choose();
    if (t.d && t.asked == want) {
        if (t.w >= want) return ECGPU_OK;
        // The context sits on a NARROWER table than it asked for (the wide one did not fit when it was built).  That refusal is not
        // for ever (include/ecgpu.h): when it has expired the wide table is tried again — before the narrow one is let go, so that
        // a second refusal costs one failed allocation and nothing else.
        if (!refusal_over(want)) return ECGPU_OK;
        const auto key = std::make_tuple(ctx->device, (int)C::ID, want);
        SharedTable& st = reg.tabs[key];
        if (!st.d) {
            const int rc = build_table<C>(ctx, want, &st);
            if (rc != ECGPU_OK) {
                reg.tabs.erase(key);
                (void)hipGetLastError();
                (void)drop_build_scratch(ctx);
                if (rc != ECGPU_ERR_OOM) return rc;
                reg.nofit[key] = NOFIT_RETRY_CALLS;              // still no room: stay on the narrow table for another stretch of calls
                return ECGPU_OK;
            }
        }
        st.refs++;                                               // ours from here on: it cannot go away while the lock is dropped
        const Table fresh{st.d, want, st.nwin, want};
        lock.unlock();
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));         // queued kernels may still read the narrow table
        release_table(ctx, C::ID);
        t = fresh;
        return drop_build_scratch(ctx);
    }
    if (t.d) {
        lock.unlock();
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));      // queued kernels may still read the old table
        release_table(ctx, C::ID);
        lock.lock();
        want = choose();      // the registry may have changed meanwhile: a wider table this call meant to share can be gone with its last owner
    }
    int rc = ECGPU_ERR_OOM;
    for (int w = want;; w -= 2) {
        const auto key = std::make_tuple(ctx->device, (int)C::ID, w);
        if (w - 2 >= 16 && !refusal_over(w)) continue;           // an earlier context of the device was refused this width
        reg.nofit.erase(key);
        SharedTable& st = reg.tabs[key];
        if (!st.d) {
            rc = build_table<C>(ctx, w, &st);
            if (rc != ECGPU_OK) {
                reg.tabs.erase(key);
                (void)hipGetLastError();                         // an out-of-memory error is not sticky
                int rc2 = drop_build_scratch(ctx);
                if (rc == ECGPU_ERR_OOM) reg.nofit[key] = NOFIT_RETRY_CALLS;
                if (rc == ECGPU_ERR_OOM && rc2 == ECGPU_OK && w - 2 >= 16) continue;
                if (rc == ECGPU_ERR_OOM) ctx->err = "basepoint comb table does not fit in device memory (even at 16-bit windows)";
                return rc;
            }
        }
        st.refs++;
        t.d = st.d;
        t.w = w;
        t.nwin = st.nwin;
        t.asked = want;
        break;
    }
    return drop_build_scratch(ctx);
}

// ---- generator LUTs of the uniform-schedule fixed-base kernel (ecgpu_ctmul.h) ----------------------------------------
// [CT_BASE_LUTS][CT_BASE_ENTRIES][2] packed elements: lut i = {e * 2^(W i) * G, e = 1..2^(W-1)}, W = CT_BASE_W — `BasepointTable::new`
// (primeorder/src/tables/basepoint.rs:41-76) with affine entries.  43 LUTs of 32 entries = 88 KB for k256: built with the
// comb-table kernels (bases 2^(6 i) G, 32 multiples each, one normalisation), shared per device under the registry key width -1.
void release_ct_lut(ecgpu_ctx* ctx, int id) {
    if (!ctx->ct_lut[id]) return;
    TableRegistry& reg = table_registry(ctx->device);
    std::lock_guard<std::mutex> lock(reg.mu);
    auto it = reg.tabs.find(std::make_tuple(ctx->device, id, -1));
    if (it != reg.tabs.end() && it->second.d == ctx->ct_lut[id] && --it->second.refs == 0) {
        (void)hipFree(it->second.d);
        reg.tabs.erase(it);
    }
    ctx->ct_lut[id] = nullptr;
}

template <class C>
int ensure_ct_lut(ecgpu_ctx* ctx) {
    if (ctx->ct_lut[C::ID]) return ECGPU_OK;
    constexpr int N = C::N, NS = Field<C>::NS;
    const int nlut = ct_base_luts<C>();
    const size_t entries = (size_t)nlut * CT_BASE_ENTRIES;
    TableRegistry& reg = table_registry(ctx->device);
    std::lock_guard<std::mutex> lock(reg.mu);
    SharedTable& st = reg.tabs[std::make_tuple(ctx->device, (int)C::ID, -1)];
    if (!st.d) {
        int rc;
        auto fail = [&](int code) {
            reg.tabs.erase(std::make_tuple(ctx->device, (int)C::ID, -1));
            return code;
        };
        if ((rc = ensure(ctx, ctx->bases, (size_t)nlut * 3 * NS * 4)) != ECGPU_OK) return fail(rc);
        if ((rc = ensure(ctx, ctx->proj, entries * 3 * NS * 4)) != ECGPU_OK) return fail(rc);
        if ((rc = ensure(ctx, ctx->prefix, entries * NS * 4)) != ECGPU_OK) return fail(rc);
        uint32_t* d = nullptr;
        if (hipMalloc(reinterpret_cast<void**>(&d), entries * 2 * N * 4) != hipSuccess) {
            (void)hipGetLastError();
            ctx->err = "generator LUTs: hipMalloc failed";
            return fail(ECGPU_ERR_OOM);
        }
        launch_window_bases<C>(ctx->stream, (uint32_t*)ctx->bases.p, CT_BASE_W, nlut);                  // 2^(W i) G
        launch_table_entries<C>(ctx->stream, (const uint32_t*)ctx->bases.p, (uint32_t*)ctx->proj.p, CT_BASE_W, nlut);   // e = 1..32
        launch_normalize<C>(ctx->stream, true, (const uint32_t*)ctx->proj.p, (uint32_t*)ctx->prefix.p, entries, nullptr, nullptr, d);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) {
            (void)hipFree(d);
            ctx->err = std::string("generator LUT build: ") + hipGetErrorString(e);
            return fail(ECGPU_ERR_HIP);
        }
        st.d = d;
        st.nwin = nlut;
    }
    st.refs++;
    ctx->ct_lut[C::ID] = st.d;
    return ECGPU_OK;
}

// launches the normalisation of n projective points in ctx->proj to wire-format output
template <class C>
int normalize_out(ecgpu_ctx* ctx, size_t n, void* d_out_xy, void* d_out_inf, bool soa = false) {
    int rc;
    if ((rc = ensure(ctx, ctx->prefix, n * Field<C>::NS * 4)) != ECGPU_OK) return rc;
    launch_normalize<C>(ctx->stream, false, (const uint32_t*)ctx->proj.p, (uint32_t*)ctx->prefix.p, n, (uint8_t*)d_out_xy,
                        (uint8_t*)d_out_inf, nullptr, soa);
    return ECGPU_OK;
}

// ---- device-pointer implementations --------------------------------------------------------------------

// The one call frame of the device-pointer pipelines (the counterpart of HostCall / staged below).  An implementation states
//   what it does for an empty call, before the frame: a call that uses the comb table or the generator LUTs builds them for
//       n == 0 too (ensure_table / ensure_ct_lut come first), a reducing call writes the identity, every other returns at once;
//   what it reserves: {buffer, bytes[, wanted]} in order (a shared pipeline's list, then its caller's) — grown before anything is queued;
//   its wipe set: WIPE_* flags (0 for the variable-time forms), zeroed behind the call's last kernel on EVERY path out, early error
//       returns included (CtWipe);
//   its launches between marks: the constructor has joined the MSM lanes and cleared the status word (reset_status) before the
//       first of them; mark(i) records event i; `normalized` is the usual tail (mark 1, normalize_out of ctx->proj, mark 2), `done`
//       reads the status back (finish);
//   its span table (collect_timing): SPANS_DEFAULT unless it says otherwise.
struct Reserve { DevBuf& buf; size_t bytes; bool wanted = true; };
struct DevCall {
    ecgpu_ctx* ctx;
    CtWipe wipe;
    int rc = ECGPU_OK;         // not ECGPU_OK after the constructor: nothing was queued, the implementation returns it
    DevCall(ecgpu_ctx* c, int wipe_set, std::initializer_list<Reserve> bufs, std::initializer_list<Reserve> more = {})
        : ctx(c), wipe(c, wipe_set) {
        for (const auto& list : {bufs, more})
            for (const Reserve& r : list)
                if (r.wanted && (rc = ensure(ctx, r.buf, r.bytes)) != ECGPU_OK) return;
        rc = reset_status(ctx);
    }
    void mark(int i) { record(ctx, i); }
    int done(SpanList spans = SPANS_DEFAULT) {
        rc = finish(ctx);
        collect_timing(ctx, spans);
        return rc;
    }
    int done_unmarked() { return rc = finish(ctx); }      // a call that recorded no marks leaves the spans of the call before alone
    template <class C>
    int normalized(size_t n, void* d_out_xy, void* d_out_inf, SpanList spans = SPANS_DEFAULT, bool soa = false) {
        mark(1);
        if ((rc = normalize_out<C>(ctx, n, d_out_xy, d_out_inf, soa)) != ECGPU_OK) return rc;
        mark(2);
        return done(spans);
    }
};

template <class C>
int mul_base_dev(ecgpu_ctx* ctx, const void* d_scalars, size_t n, void* d_out_xy, void* d_out_inf, bool compressed = false) {
    constexpr int NS = Field<C>::NS;
    int rc;
    if ((rc = ensure_table<C>(ctx, n)) != ECGPU_OK) return rc;
    if (n == 0) return ECGPU_OK;
    DevCall call(ctx, 0, {{ctx->proj, n * 3 * NS * 4}});
    if (call.rc != ECGPU_OK) return call.rc;
    const Table& t = ctx->table[C::ID];
    // The hand-over between k_fixed_base and k_normalize is quad-major (store_proj_soa, ecgpu_kernels.h: a wave's load or store is
    // 1,024 contiguous bytes instead of 64 pieces 144 bytes apart; profiles/r06/fixed_soa_handover_ab.txt); the compressed form's
    // own normalisation reads the record-major one.
    const bool soa = !compressed;
    call.mark(0);
    launch_fixed_base<C>(ctx->stream, (const uint8_t*)d_scalars, n, (const uint32_t*)t.d, t.w, t.nwin, (uint32_t*)ctx->proj.p,
                         ctx->d_status, soa);
    if (!compressed) return call.normalized<C>(n, d_out_xy, d_out_inf, SPANS_DEFAULT, soa);
    call.mark(1);
    if ((rc = ensure(ctx, ctx->prefix, n * NS * 4)) != ECGPU_OK) return rc;
    launch_normalize_compressed<C>(ctx->stream, (const uint32_t*)ctx->proj.p, (uint32_t*)ctx->prefix.p, n, (uint8_t*)d_out_xy,
                                   (uint8_t*)d_out_inf);
    call.mark(2);
    return call.done();
}

template <class C>
int mul_var_dev(ecgpu_ctx* ctx, const void* d_scalars, const void* d_points_xy, const void* d_points_inf, size_t n,
                void* d_out_xy, void* d_out_inf) {
    constexpr int NS = Field<C>::NS;
    if (n == 0) return ECGPU_OK;
    const size_t tstride = var_base_slots<C>(n);
    DevCall call(ctx, 0, {{ctx->proj, n * 3 * NS * 4}, {ctx->vtab, tstride * var_base_tab_words<C>() * 4}});
    if (call.rc != ECGPU_OK) return call.rc;
    call.mark(0);
    launch_var_base<C>(ctx->stream, (const uint8_t*)d_scalars, (const uint8_t*)d_points_xy, (const uint8_t*)d_points_inf, n,
                       (uint32_t*)ctx->vtab.p, tstride, (uint32_t*)ctx->proj.p, ctx->d_status);
    return call.normalized<C>(n, d_out_xy, d_out_inf);
}

// ---- uniform-schedule variants (ecgpu_ct.h): the reference's constant-time drivers as they are ---------------------------
// k G for n scalars on the uniform-schedule fixed-base kernel, into ctx->proj (the caller has reserved proj and ct_flags)
template <class C>
void generator_mul_ct(ecgpu_ctx* ctx, const void* d_k, size_t n) {
    launch_fixed_base_ct<C>(ctx->stream, (const uint8_t*)d_k, n, (const uint32_t*)ctx->ct_lut[C::ID], (uint32_t*)ctx->proj.p,
                            (uint8_t*)ctx->ct_flags.p, ctx->d_status);
}

template <class C>
int mul_base_ct_dev(ecgpu_ctx* ctx, const void* d_scalars, size_t n, void* d_out_xy, void* d_out_inf) {
    constexpr int NS = Field<C>::NS;
    int rc;
    if ((rc = ensure_ct_lut<C>(ctx)) != ECGPU_OK) return rc;
    if (n == 0) return ECGPU_OK;
    DevCall call(ctx, WIPE_SCRATCH, {{ctx->proj, n * 3 * NS * 4}, {ctx->ct_flags, n + 16}});
    if (call.rc != ECGPU_OK) return call.rc;
    call.mark(0);
    generator_mul_ct<C>(ctx, d_scalars, n);
    return call.normalized<C>(n, d_out_xy, d_out_inf);
}

// ---- signing (ecgpu_sign.h, ecgpu_sm2sign.h, ecgpu_bignsign.h) ------------------------------------------------------------------
// The one pipeline of the four schemes: mark 0, the scheme's nonce stage, k G (generator_mul_ct), mark 1, affine R (normalize_out),
// the scheme's finish stage, mark 2.  A scheme that derives its nonce from P = d G (BIP340 always, SM2DSA from messages) runs
// sign_key_leg inside its nonce stage, so "main" covers that leg too.  Common scratch: proj, ct_flags, sg_k, sg_flag, ec_xy, ec_inf,
// handed to the stages by name (read after the reservations: the buffers may have grown).  A scheme (below) states its own beside it:
// sg_state (the parked state of a retrying nonce generator), ec_e (the prehash of a call from messages), sg_dp (d' || x(P) for BIP340,
// S0 for bign; the sanitised point for sm2_pke_dev).  All of it is in the wipe set — WIPE_SCRATCH | WIPE_EC | WIPE_SIGN, and
// WIPE_PREHASH (ec_e) for SM2DSA alone — which CtWipe zeroes behind the last kernel on EVERY path out, early error returns included.
// SM2DSA and bign have no public `_dev` form yet: the host-pointer entry points have checked every argument before a chunk gets here.
struct SignScratch {
    uint8_t *k, *flag;                 // the nonce stage writes: the sanitised nonce, the verdict so far
    uint8_t *xy, *inf;                 // the finish stage reads: R = k G as x || y records and their identity flags
};
// the key leg: P = d G into s.xy (d, or 1 in place of an unusable key, passes through s.k)
template <class C>
int sign_key_leg(ecgpu_ctx* ctx, const SignScratch& s, const void* d_key, size_t n) {
    launch_sign_nonce_load<C>(ctx->stream, (const uint8_t*)d_key, n, s.k, s.flag);
    generator_mul_ct<C>(ctx, s.k, n);
    return normalize_out<C>(ctx, n, s.xy, s.inf);
}
template <class C, class Nonce, class Finish>
int sign_pipeline(ecgpu_ctx* ctx, size_t n, std::initializer_list<Reserve> extra, int extra_wipe, Nonce&& nonce, Finish&& finish) {
    constexpr int NS = Field<C>::NS;
    constexpr size_t L = WireBytes<C>::value;
    int rc;
    if ((rc = ensure_ct_lut<C>(ctx)) != ECGPU_OK) return rc;
    if (n == 0) return ECGPU_OK;
    DevCall call(ctx, WIPE_SCRATCH | WIPE_EC | WIPE_SIGN | extra_wipe,
                 {{ctx->proj, n * 3 * NS * 4}, {ctx->ct_flags, n + 16}, {ctx->sg_k, n * L + 16}, {ctx->sg_flag, n + 16},
                  {ctx->ec_xy, n * 2 * L + 16}, {ctx->ec_inf, n + 16}}, extra);
    if (call.rc != ECGPU_OK) return call.rc;
    const SignScratch s{(uint8_t*)ctx->sg_k.p, (uint8_t*)ctx->sg_flag.p, (uint8_t*)ctx->ec_xy.p, (uint8_t*)ctx->ec_inf.p};
    call.mark(0);
    if ((rc = nonce(s)) != ECGPU_OK) return rc;
    generator_mul_ct<C>(ctx, s.k, n);
    call.mark(1);
    if ((rc = normalize_out<C>(ctx, n, s.xy, s.inf)) != ECGPU_OK) return rc;
    finish(s);
    call.mark(2);
    return call.done();
}

// d_k == nullptr: the nonce of RFC 6979 (k_rfc6979_first, k_rfc6979_retry; its parked state lives in sg_state).  from_msg: d_z holds
// n messages of msg_len bytes instead of prehashes; z = bits2field(digest) goes to ec_e first (k_sign_hash_msg).
template <class C>
int ecdsa_sign_dev(ecgpu_ctx* ctx, const void* d_d, const void* d_k, const void* d_z, size_t n, int normalize_s, void* d_sig,
                   void* d_recid, void* d_ok, bool from_msg = false, size_t msg_len = 0) {
    return sign_pipeline<C>(
        ctx, n, {{ctx->sg_state, n * rfc6979_state_bytes<C>() + 16, !d_k}, {ctx->ec_e, n * WireBytes<C>::value + 16, from_msg}}, 0,
        [&](const SignScratch& s) {
            if (from_msg) {
                launch_sign_hash_msg<C>(ctx->stream, (const uint8_t*)d_z, msg_len, n, (uint8_t*)ctx->ec_e.p);
                d_z = ctx->ec_e.p;
            }
            if (d_k)
                launch_sign_nonce_load<C>(ctx->stream, (const uint8_t*)d_k, n, s.k, s.flag);
            else
                launch_rfc6979<C>(ctx->stream, (const uint8_t*)d_d, (const uint8_t*)d_z, n, ctx->rfc6979_cap, s.k, s.flag, ctx->sg_state.p);
            return ECGPU_OK;
        },
        [&](const SignScratch& s) {
            launch_ecdsa_sign_finish<C>(ctx->stream, (const uint8_t*)d_d, s.k, s.flag, (const uint8_t*)d_z, s.xy, s.inf, n, normalize_s,
                                        (uint8_t*)d_sig, (uint8_t*)d_recid, (uint8_t*)d_ok);
        });
}

// BIP340 (k256): the fixed-base kernel runs twice, for the key's P = d G and for R = k G; k_schnorr_nonce leaves d' || x(P) in sg_dp
int schnorr_sign_dev(ecgpu_ctx* ctx, const void* d_sk, const void* d_msgs, size_t msg_len, const void* d_aux_rand, size_t n, void* d_out_sig,
                     void* d_ok) {
    using C = K256Params;
    return sign_pipeline<C>(
        ctx, n, {{ctx->sg_dp, n * 64 + 16}}, 0,
        [&](const SignScratch& s) {
            if (int rc = sign_key_leg<C>(ctx, s, d_sk, n); rc != ECGPU_OK) return rc;
            launch_schnorr_nonce<C>(ctx->stream, (const uint8_t*)d_sk, s.xy, (const uint8_t*)d_aux_rand, (const uint8_t*)d_msgs, msg_len, n,
                                    (uint8_t*)ctx->sg_dp.p, s.k, s.flag);
            return (int)ECGPU_OK;
        },
        [&](const SignScratch& s) {
            launch_schnorr_sign_finish<C>(ctx->stream, (const uint8_t*)ctx->sg_dp.p, s.k, s.flag, s.xy, s.inf, (const uint8_t*)d_msgs, msg_len,
                                          n, (uint8_t*)d_out_sig, (uint8_t*)d_ok);
        });
}

// SM2DSA.  d_k: the caller's nonce (the standard's A3-A7); d_k == nullptr: the ONE candidate of RFC 6979 over HMAC-SM3 (k_sm2_rfc6979;
// no retry kernel, so no sg_state).  from_msg: d_e holds n messages of msg_len bytes, and e = SM3(Z || M) goes to ec_e (k_sm2_sign_e)
// after the key leg, because Z hashes PA = d G; d_e is otherwise the prehash array.  ec_e is wiped behind this scheme (WIPE_PREHASH).
int sm2dsa_sign_dev(ecgpu_ctx* ctx, const void* d_d, const void* d_k, const void* d_e, size_t n, void* d_sig, void* d_ok,
                    bool from_msg = false, const void* d_distid = nullptr, size_t distid_len = 0, size_t msg_len = 0) {
    using C = Sm2Params;
    return sign_pipeline<C>(
        ctx, n, {{ctx->ec_e, n * 32 + 16, from_msg}}, WIPE_PREHASH,
        [&](const SignScratch& s) {
            if (from_msg) {
                if (int rc = sign_key_leg<C>(ctx, s, d_d, n); rc != ECGPU_OK) return rc;
                launch_sm2_sign_e<C>(ctx->stream, (const uint8_t*)d_distid, distid_len, s.xy, (const uint8_t*)d_e, msg_len, n,
                                     (uint8_t*)ctx->ec_e.p);
                d_e = ctx->ec_e.p;
            }
            if (d_k)
                launch_sign_nonce_load<C>(ctx->stream, (const uint8_t*)d_k, n, s.k, s.flag);
            else
                launch_sm2_rfc6979<C>(ctx->stream, (const uint8_t*)d_d, (const uint8_t*)d_e, n, s.k, s.flag);
            return (int)ECGPU_OK;
        },
        [&](const SignScratch& s) {
            launch_sm2dsa_sign_finish<C>(ctx->stream, (const uint8_t*)d_d, s.k, s.flag, (const uint8_t*)d_e, s.xy, s.inf, n, (uint8_t*)d_sig,
                                         (uint8_t*)d_ok);
        });
}

// bign.  d_k: the caller's nonce (the standard's steps 3-7); d_k == nullptr: the belt-based generator (k_bign_genk, then
// k_bign_genk_retry once, by the rule of launch_rfc6979; its parked state lives in sg_state).  from_msg: d_h holds n messages of
// msg_len bytes and H = belt-hash(message) goes to ec_e first (k_bign_hash_msg: messages are public).  S0 is staged in sg_dp.
int bign_sign_dev(ecgpu_ctx* ctx, const void* d_d, const void* d_k, const void* d_h, size_t n, void* d_sig, void* d_ok,
                  bool from_msg = false, size_t msg_len = 0) {
    using C = Bign256Params;
    return sign_pipeline<C>(
        ctx, n, {{ctx->sg_dp, n * 16 + 16}, {ctx->sg_state, n * bign_genk_state_bytes<C>() + 16, !d_k}, {ctx->ec_e, n * 32 + 16, from_msg}}, 0,
        [&](const SignScratch& s) {
            if (from_msg) {
                launch_bign_hash_msg(ctx->stream, (const uint8_t*)d_h, msg_len, n, (uint8_t*)ctx->ec_e.p);
                d_h = ctx->ec_e.p;
            }
            if (d_k)
                launch_sign_nonce_load<C>(ctx->stream, (const uint8_t*)d_k, n, s.k, s.flag);
            else
                launch_bign_genk<C>(ctx->stream, (const uint8_t*)d_d, (const uint8_t*)d_h, C::ORDER, n, ctx->rfc6979_cap, s.k, s.flag,
                                    (uint32_t*)ctx->sg_state.p);
            return ECGPU_OK;
        },
        [&](const SignScratch& s) {
            launch_bign_sign_s0<C>(ctx->stream, (const uint8_t*)d_h, s.xy, n, (uint8_t*)ctx->sg_dp.p);
            launch_bign_sign_finish<C>(ctx->stream, (const uint8_t*)d_d, s.k, s.flag, (const uint8_t*)d_h, (const uint8_t*)ctx->sg_dp.p, 16,
                                       s.inf, n, (uint8_t*)d_sig, (uint8_t*)d_ok);
        });
}

// ---- X448 (ecgpu_x448.h): one kernel from the records to the records; mode: X448_CHECKED / X448_UNCHECKED / X448_BASE ----------
// The ladder state never leaves the registers, so there is no scratch to reserve and none to wipe: what is secret outside the kernel
// are the staged scalars and the staged results, which the host-pointer entry points mark.  There is no public `_dev` form yet.
int x448_dev(ecgpu_ctx* ctx, int mode, const void* d_k, const void* d_u, size_t n, void* d_out, void* d_ok) {
    if (n == 0) return ECGPU_OK;
    DevCall call(ctx, 0, {});
    if (call.rc != ECGPU_OK) return call.rc;
    call.mark(0);
    launch_x448(ctx->stream, mode, (const uint8_t*)d_k, (const uint8_t*)d_u, n, (uint8_t*)d_out, (uint8_t*)d_ok);
    call.mark(1);
    return call.done(SPANS_NO_NORMALIZE);
}

// ---- SM2 public-key encryption (ecgpu_pke.h): a frame of its own — a variable-base leg, and no fixed-base leg on open ------------
// seal (encrypt): d_scalar = k, d_point = P_B, d_in = M; C1 = k G is normalised straight into the caller's array (a public point),
// (x2, y2) = k P_B into ec_xy, k_pke_seal writes C2 = d_out, C3 = d_c3 and ok (and zeroes the C1 of an element without a verdict).
// open (decrypt): d_scalar = d, d_point = C1, d_in = C2, d_c3 = the ciphertext's C3, M' = d_out.
// It reserves proj, vtab and ct_flags for the two multiplications, sg_k for the sanitised scalar, sg_dp for the sanitised point,
// sg_flag for the verdict bytes, ec_xy / ec_inf for x2 || y2: every buffer that holds k, d, x2 || y2 or anything derived from them is
// wiped (WIPE_SCRATCH | WIPE_EC | WIPE_SIGN) in stream order whatever way the call leaves; the staged copies of k, d and the messages
// are the host-pointer entry points' to mark.  No public `_dev` form: every chunk of a host-pointer call gets here through `staged`.
int sm2_pke_dev(ecgpu_ctx* ctx, bool open, const void* d_scalar, const void* d_point, const void* d_in, size_t msg_len, size_t n,
                void* d_c1, void* d_out, void* d_c3, void* d_ok) {
    using C = Sm2Params;
    constexpr int NS = Field<C>::NS;
    int rc;
    if (!open && (rc = ensure_ct_lut<C>(ctx)) != ECGPU_OK) return rc;
    if (n == 0) return ECGPU_OK;
    const size_t tstride = var_base_slots<C>(n);
    DevCall call(ctx, WIPE_SCRATCH | WIPE_EC | WIPE_SIGN,
                 {{ctx->proj, n * 3 * NS * 4}, {ctx->vtab, tstride * var_base_tab_words<C>() * 4}, {ctx->ct_flags, n + 16},
                  {ctx->sg_k, n * 32 + 16}, {ctx->sg_flag, n + 16}, {ctx->sg_dp, n * 64 + 16}, {ctx->ec_xy, n * 64 + 16},
                  {ctx->ec_inf, n + 16}});
    if (call.rc != ECGPU_OK) return call.rc;
    uint8_t *k = (uint8_t*)ctx->sg_k.p, *flag = (uint8_t*)ctx->sg_flag.p, *pt = (uint8_t*)ctx->sg_dp.p;
    uint8_t *xy = (uint8_t*)ctx->ec_xy.p, *inf = (uint8_t*)ctx->ec_inf.p;
    call.mark(0);
    launch_pke_load<C>(ctx->stream, (const uint8_t*)d_scalar, (const uint8_t*)d_point, n, k, pt, flag);
    if (!open) {
        generator_mul_ct<C>(ctx, k, n);
        if ((rc = normalize_out<C>(ctx, n, d_c1, inf)) != ECGPU_OK) return rc;                   // C1 = k G
    }
    launch_var_base_ct<C>(ctx->stream, k, pt, nullptr, n, (uint32_t*)ctx->vtab.p, tstride, (uint32_t*)ctx->proj.p,
                          (uint8_t*)ctx->ct_flags.p, ctx->d_status);
    call.mark(1);
    if ((rc = normalize_out<C>(ctx, n, xy, inf)) != ECGPU_OK) return rc;                         // (x2, y2) = k P_B resp. d C1
    if (open)
        launch_pke_open<C>(ctx->stream, xy, flag, (const uint8_t*)d_in, msg_len, (const uint8_t*)d_c3, n, (uint8_t*)d_out, (uint8_t*)d_ok);
    else
        launch_pke_seal<C>(ctx->stream, xy, flag, (const uint8_t*)d_in, msg_len, n, (uint8_t*)d_c1, (uint8_t*)d_out, (uint8_t*)d_c3,
                           (uint8_t*)d_ok);
    call.mark(2);
    return call.done();
}

// xyz: d_points_xy holds projective records X || Y || Z (k_xyz_mul_ct) and d_points_inf is unused
template <class C>
int mul_var_ct_dev(ecgpu_ctx* ctx, const void* d_scalars, const void* d_points_xy, const void* d_points_inf, size_t n,
                   void* d_out_xy, void* d_out_inf, bool xyz = false) {
    constexpr int NS = Field<C>::NS;
    if (n == 0) return ECGPU_OK;
    const size_t tstride = var_base_slots<C>(n);
    DevCall call(ctx, WIPE_SCRATCH,
                 {{ctx->proj, n * 3 * NS * 4}, {ctx->vtab, tstride * var_base_tab_words<C>() * 4}, {ctx->ct_flags, n + 16}});
    if (call.rc != ECGPU_OK) return call.rc;
    call.mark(0);
    if (xyz)
        launch_xyz_mul_ct<C>(ctx->stream, (const uint8_t*)d_scalars, (const uint8_t*)d_points_xy, n, (uint32_t*)ctx->vtab.p, tstride,
                             (uint32_t*)ctx->proj.p, (uint8_t*)ctx->ct_flags.p, ctx->d_status);
    else
        launch_var_base_ct<C>(ctx->stream, (const uint8_t*)d_scalars, (const uint8_t*)d_points_xy, (const uint8_t*)d_points_inf, n,
                              (uint32_t*)ctx->vtab.p, tstride, (uint32_t*)ctx->proj.p, (uint8_t*)ctx->ct_flags.p, ctx->d_status);
    return call.normalized<C>(n, d_out_xy, d_out_inf);
}

template <class C>
int normalize_dev(ecgpu_ctx* ctx, const void* d_xyz, size_t n, void* d_out_xy, void* d_out_inf) {
    if (n == 0) return ECGPU_OK;
    DevCall call(ctx, 0, {{ctx->proj, n * 3 * Field<C>::NS * 4}});
    if (call.rc != ECGPU_OK) return call.rc;
    call.mark(0);
    launch_load_proj<C>(ctx->stream, (const uint8_t*)d_xyz, n, (uint32_t*)ctx->proj.p, ctx->d_status);
    return call.normalized<C>(n, d_out_xy, d_out_inf);
}

// (a reducing call: the sum of no points is the identity, written by the same kernels)
template <class C>
int point_sum_dev(ecgpu_ctx* ctx, const void* d_xy, const void* d_inf, size_t n, void* d_out_xy, void* d_out_inf) {
    DevCall call(ctx, 0, {{ctx->proj, 3 * Field<C>::NS * 4}});
    if (call.rc != ECGPU_OK) return call.rc;
    call.mark(0);
    launch_point_sum<C>(ctx->stream, (const uint8_t*)d_xy, (const uint8_t*)d_inf, n, (uint32_t*)ctx->proj.p, ctx->d_status);
    return call.normalized<C>(1, d_out_xy, d_out_inf);
}

// ---- projective points into the variable-time path: X || Y || Z records are normalised on the device (k_xyz_affine: one
// inversion per lane of records, the verdicts of the _ct_xyz forms) into x || y + identity flag records on stream s, in the
// buffers given (the context's own, or an MSM lane's); the affine pipeline then runs unchanged on them.  A bad record sets
// ST_BAD_POINT like an off-curve x || y record would.
template <class C>
int xyz_stage(ecgpu_ctx* ctx, hipStream_t s, const void* d_xyz, size_t n, DevBuf& xy, DevBuf& inf, DevBuf& prefix) {
    constexpr int WB = WireBytes<C>::value, NS = Field<C>::NS;
    int rc;
    if ((rc = ensure_on(ctx, s, xy, n * 2 * WB + 16)) != ECGPU_OK) return rc;
    if ((rc = ensure_on(ctx, s, inf, n + 16)) != ECGPU_OK) return rc;
    if ((rc = ensure_on(ctx, s, prefix, n * NS * 4 + 16)) != ECGPU_OK) return rc;
    launch_xyz_affine<C>(s, (const uint8_t*)d_xyz, n, (uint32_t*)prefix.p, (uint8_t*)xy.p, (uint8_t*)inf.p, ctx->d_status);
    return ECGPU_OK;
}

// ---- the one decoded-points front stage -------------------------------------------------------------------------------------
// Points that arrive in another record than x || y + flag are decoded on the context's stream into ctx->cx_xy / ctx->cx_inf by a first
// stage — decode_xyz (projective records, xyz_stage) or decode_compressed (x + SEC1 tag records, k_decompress_tagged: one square
// root per point) —, and the ordinary pipeline `then(d_xy, d_inf)` runs on the result as the second stage of the same call: under
// KeepStatus, so that it does not clear the first stage's verdicts.  A record that decodes to no point ends the call with
// ECGPU_ERR_POINT like an off-curve x || y record would.  Both decoders open the call's frame themselves (the lanes are joined and
// the status word cleared before the decoding kernel); what an empty call does is the caller's business.
struct KeepStatus {            // the second stage of a two-stage call must not clear the first stage's verdicts
    ecgpu_ctx* ctx;
    explicit KeepStatus(ecgpu_ctx* c) : ctx(c) { ctx->keep_status = true; }
    ~KeepStatus() { ctx->keep_status = false; }
};
template <class C>
int decode_xyz(ecgpu_ctx* ctx, const void* d_xyz, const void* /* no tags */, size_t n) {
    DevCall front(ctx, 0, {});
    if (front.rc != ECGPU_OK) return front.rc;
    return xyz_stage<C>(ctx, ctx->stream, d_xyz, n, ctx->cx_xy, ctx->cx_inf, ctx->prefix);
}
template <class C>
int decode_compressed(ecgpu_ctx* ctx, const void* d_x, const void* d_tag, size_t n) {
    constexpr int WB = WireBytes<C>::value;
    DevCall front(ctx, 0, {{ctx->cx_xy, n * 2 * WB + 16}, {ctx->cx_inf, n + 16}});
    if (front.rc != ECGPU_OK) return front.rc;
    if (n)
        launch_decompress_tagged<C>(ctx->stream, (const uint8_t*)d_x, (const uint8_t*)d_tag, n, (uint8_t*)ctx->cx_xy.p,
                                    (uint8_t*)ctx->cx_inf.p, ctx->d_status);
    return ECGPU_OK;
}
template <class Then>
int decoded(ecgpu_ctx* ctx, int (*decode)(ecgpu_ctx*, const void*, const void*, size_t), const void* d_points, const void* d_tag,
            size_t n, Then&& then) {
    const int rc = decode(ctx, d_points, d_tag, n);
    if (rc != ECGPU_OK) return rc;
    KeepStatus keep(ctx);
    return then(ctx->cx_xy.p, ctx->cx_inf.p);
}

// The lane the next MSM (or local half of a sharded MSM) of an asynchronous context with ecgpu_set_msm_lanes > 1 goes to: lanes take
// turns; a lane's stream, events and workspace exist from its first use on.
int next_lane(ecgpu_ctx* ctx, size_t workspace_bytes, ecgpu_ctx::MsmLane** out) {
    ctx->lane_last = (int)(ctx->msm_seq % (unsigned)ctx->msm_lanes);
    ecgpu_ctx::MsmLane& l = ctx->lane[ctx->msm_seq++ % (unsigned)ctx->msm_lanes];
    ctx->spans.clear();
    ctx->timing.clear();
    if (!l.s) {
        HIP_TRY(ctx, hipStreamCreateWithFlags(&l.s, hipStreamNonBlocking));
        HIP_TRY(ctx, hipEventCreateWithFlags(&l.ev_in, hipEventDisableTiming));
        HIP_TRY(ctx, hipEventCreate(&l.ev_a));
        HIP_TRY(ctx, hipEventCreate(&l.ev_b));
        HIP_TRY(ctx, hipEventCreateWithFlags(&l.ev_done, hipEventDisableTiming));
    }
    int rc = ensure_on(ctx, l.s, l.ws, workspace_bytes);
    if (rc != ECGPU_OK) return rc;
    *out = &l;
    return ECGPU_OK;
}

// The one way onto a lane.  Everything of this MSM (or local half) runs on the lane's stream and in the lane's buffers, ordered after
// what the context's stream holds now (the inputs: ev_in) — the conversion of X || Y || Z records too (xyz: into the lane's buffers,
// beside the previous MSM).  `claim(lane)` is what the caller does to the lane before anything is queued on it, `launch(lane, d_xy,
// d_inf)` queues its kernels.  Any OTHER entry point called later on this context waits for ev_done first (reset_status): it may
// read the output or reuse the inputs.  Further MSMs do not — they go to the next lane — and neither does work the caller queues on
// the stream itself: for that, inputs and outputs belong to the lane until ecgpu_synchronize.  The call's timing marks are the
// lane's own (ev_a, ev_b: ecgpu_last_timing "accumulate").
template <class C, class Claim, class Launch>
int on_lane(ecgpu_ctx* ctx, size_t workspace_bytes, bool xyz, const void* d_xy, const void* d_inf, size_t n, Claim&& claim,
            Launch&& launch) {
    int rc;
    ecgpu_ctx::MsmLane* lp = nullptr;
    if ((rc = next_lane(ctx, workspace_bytes, &lp)) != ECGPU_OK) return rc;
    ecgpu_ctx::MsmLane& l = *lp;
    if ((rc = claim(l)) != ECGPU_OK) return rc;
    HIP_TRY(ctx, hipEventRecord(l.ev_in, ctx->stream));
    HIP_TRY(ctx, hipStreamWaitEvent(l.s, l.ev_in, 0));
    if (xyz) {
        if ((rc = xyz_stage<C>(ctx, l.s, d_xy, n, l.cx_xy, l.cx_inf, l.prefix)) != ECGPU_OK) return rc;
        d_xy = l.cx_xy.p;
        d_inf = l.cx_inf.p;
    }
    launch(l, d_xy, d_inf);
    HIP_TRY(ctx, hipEventRecord(l.ev_done, l.s));
    ctx->lanes_pending = true;
    return finish(ctx);
}

// largest term count for which the per-term multiplication + tree sum replaces the bucket method (0: never);
// ECGPU_MSM_SMALL_LOG2 overrides the measured default (tuning knob, -1 disables)
template <class C>
size_t msm_small_max() {
    // measured (round 1, tools/gpu_msm_sweep.py is today's form of the sweep): k256 0.75-0.91 ms against 1.21-1.36 ms up to 2^16 terms (1.51 against 1.39 at 2^17),
    // p256 1.23-1.44 against 1.39-1.59 ms, p384 3.3-3.4 against 3.7-4.1 ms up to 2^10 and level beyond
    int lg = C::N > 8 ? 10 : 16;
    if (const char* e = knob("ECGPU_MSM_SMALL_LOG2")) lg = atoi(e);
    return lg <= 0 ? 0 : (size_t)1 << (lg > 24 ? 24 : lg);
}

// xyz: d_xy holds projective records X || Y || Z and d_inf is unused — converted on the MSM's lane when it goes to one, on the
// context's stream otherwise.  (A reducing call: an MSM of no terms goes down the bucket path, which writes the identity.)
template <class C>
int msm_dev(ecgpu_ctx* ctx, const void* d_scalars, const void* d_xy, const void* d_inf, size_t n, void* d_out_xy,
            void* d_out_inf, bool xyz = false) {
    constexpr int NS = Field<C>::NS;
    if (n > msm_max_terms<C>()) {           // sorted entries are sub-term index | sign << 31
        ctx->err = "MSM of 2^31 (k256: 2^30) or more terms: split it and add the partial sums (ecgpu_point_sum)";
        return ECGPU_ERR_ARG;
    }
    const bool small = n >= 1 && n <= msm_small_max<C>() && ctx->msm_c == 0;
    const bool lanes = ctx->async && ctx->msm_lanes > 1;
    if (xyz && (small || !lanes))
        return decoded(ctx, decode_xyz<C>, d_xy, nullptr, n, [&](const void* xy, const void* inf) {
            return msm_dev<C>(ctx, d_scalars, xy, inf, n, d_out_xy, d_out_inf);
        });
    if (small) {
        // Small MSM: the bucket method has a floor of ~1.2 ms of serial work that does not depend on n (running sums, the
        // 240-doubling combine chain).  Below ~2^17 terms one variable-base multiplication per term (all lanes in
        // parallel, ~0.5 ms of latency) and a tree sum of the products are faster.
        const size_t tstride = var_base_slots<C>(n);
        DevCall call(ctx, 0, {{ctx->proj, n * 3 * NS * 4}, {ctx->vtab, tstride * var_base_tab_words<C>() * 4},
                              {ctx->prefix, ((n + BLOCK - 1) / BLOCK + 1) * 3 * NS * 4}});
        if (call.rc != ECGPU_OK) return call.rc;
        call.mark(0);
        launch_var_base<C>(ctx->stream, (const uint8_t*)d_scalars, (const uint8_t*)d_xy, (const uint8_t*)d_inf, n,
                           (uint32_t*)ctx->vtab.p, tstride, (uint32_t*)ctx->proj.p, ctx->d_status);
        call.mark(3);
        launch_proj_sum<C>(ctx->stream, (uint32_t*)ctx->proj.p, n, (uint32_t*)ctx->prefix.p);
        call.mark(4);
        return call.normalized<C>(1, d_out_xy, d_out_inf, SPANS_MSM);
    }
    MsmPlan plan = msm_plan<C>(n, ctx->msm_c, msm_use_glv<C>(n));
    if (lanes)         // its output is ordered by ecgpu_synchronize only; it is no local half: the lane forgets its parts record
        return on_lane<C>(ctx, plan.workspace_bytes, xyz, d_xy, d_inf, n, [&](ecgpu_ctx::MsmLane& l) {
            l.parts_out = nullptr;
            const int rc = ensure_on(ctx, l.s, l.proj, 3 * NS * 4);
            return rc != ECGPU_OK ? rc : ensure_on(ctx, l.s, l.prefix, NS * 4);
        }, [&](ecgpu_ctx::MsmLane& l, const void* xy, const void* inf) {
            launch_msm<C>(plan, l.s, (const uint8_t*)d_scalars, (const uint8_t*)xy, (const uint8_t*)inf, n, l.ws.p, (uint32_t*)l.proj.p,
                          ctx->d_status, l.ev_a, l.ev_b, (uint8_t*)d_out_xy, (uint8_t*)d_out_inf);   // (the last kernel writes the wire record)
        });
    DevCall call(ctx, 0, {{ctx->proj, 3 * NS * 4}, {ctx->msm_ws, plan.workspace_bytes}});
    if (call.rc != ECGPU_OK) return call.rc;
    const bool detail = ctx->timing_on && ctx->ev[6];
    if (detail)
        for (int i = 0; i < 3; i++) plan.detail[i] = ctx->ev[6 + i];
    call.mark(0);
    launch_msm<C>(plan, ctx->stream, (const uint8_t*)d_scalars, (const uint8_t*)d_xy, (const uint8_t*)d_inf, n,
                  ctx->msm_ws.p, (uint32_t*)ctx->proj.p, ctx->d_status, ctx->timing_on ? ctx->ev[3] : nullptr, ctx->timing_on ? ctx->ev[4] : nullptr, (uint8_t*)d_out_xy,
                  (uint8_t*)d_out_inf);
    call.mark(1);     // (the conversion to affine happens inside the last kernel of the chain: "normalize" is an empty span)
    call.mark(2);
    return call.done(detail ? SpanList(SPANS_MSM_DETAIL) : SpanList(SPANS_MSM));
}

// ---- `LinearCombination::lincomb` in its constant-time form (primeorder/src/projective.rs:484-496 -> :532-557; k256
// mul.rs:84-98 -> :112-163): one uniform-schedule multiplication per term (k_var_base_ct: the reference's table, digits and
// additions for that term) and a tree of complete additions over the products, 256 per workgroup and level.  The reference
// interleaves the terms on one accumulator (Straus); the group element is the same and the schedule here depends on n only.
// xyz: d_xy holds projective records X || Y || Z (k_xyz_mul_ct) and d_inf is unused
template <class C>
int lincomb_ct_dev(ecgpu_ctx* ctx, const void* d_scalars, const void* d_xy, const void* d_inf, size_t n, void* d_out_xy,
                   void* d_out_inf, bool xyz = false) {
    constexpr int NS = Field<C>::NS, WB = WireBytes<C>::value;
    if (n == 0) {                              // a reducing call: the empty sum is the identity (no secret, no scratch, no marks)
        DevCall call(ctx, 0, {});
        if (call.rc != ECGPU_OK) return call.rc;
        HIP_TRY(ctx, hipMemsetAsync(d_out_xy, 0, 2 * WB, ctx->stream));
        if (d_out_inf) HIP_TRY(ctx, hipMemsetAsync(d_out_inf, 1, 1, ctx->stream));
        return call.done_unmarked();
    }
    const size_t tstride = var_base_slots<C>(n);
    DevCall call(ctx, WIPE_SCRATCH,
                 {{ctx->proj, n * 3 * NS * 4}, {ctx->vtab, tstride * var_base_tab_words<C>() * 4}, {ctx->ct_flags, n + 16},
                  {ctx->prefix, ((n + BLOCK - 1) / BLOCK + 1) * 3 * NS * 4}});
    if (call.rc != ECGPU_OK) return call.rc;
    call.mark(0);
    if (xyz)
        launch_xyz_mul_ct<C>(ctx->stream, (const uint8_t*)d_scalars, (const uint8_t*)d_xy, n, (uint32_t*)ctx->vtab.p, tstride,
                             (uint32_t*)ctx->proj.p, (uint8_t*)ctx->ct_flags.p, ctx->d_status);
    else
        launch_var_base_ct<C>(ctx->stream, (const uint8_t*)d_scalars, (const uint8_t*)d_xy, (const uint8_t*)d_inf, n,
                              (uint32_t*)ctx->vtab.p, tstride, (uint32_t*)ctx->proj.p, (uint8_t*)ctx->ct_flags.p, ctx->d_status);
    call.mark(3);
    launch_proj_sum<C>(ctx->stream, (uint32_t*)ctx->proj.p, n, (uint32_t*)ctx->prefix.p);
    return call.normalized<C>(1, d_out_xy, d_out_inf, SPANS_LINCOMB_CT);
}

// (the forms over decoded points: an empty ecgpu_batch_mul_xyz_dev returns at once; the other three run their decoder and their
// pipeline for n == 0 too — the MSM writes the identity, ecgpu_batch_mul_base_and_mul_add_xyz_dev builds the table)
template <class C>
int msm_compressed_dev(ecgpu_ctx* ctx, const void* d_scalars, const void* d_x, const void* d_tag, size_t n, void* d_out_xy,
                       void* d_out_inf) {
    return decoded(ctx, decode_compressed<C>, d_x, d_tag, n, [&](const void* xy, const void* inf) {
        return msm_dev<C>(ctx, d_scalars, xy, inf, n, d_out_xy, d_out_inf);
    });
}
template <class C>
int mul_var_compressed_dev(ecgpu_ctx* ctx, const void* d_scalars, const void* d_x, const void* d_tag, size_t n, void* d_out_xy,
                           void* d_out_inf) {
    return decoded(ctx, decode_compressed<C>, d_x, d_tag, n, [&](const void* xy, const void* inf) {
        return mul_var_dev<C>(ctx, d_scalars, xy, inf, n, d_out_xy, d_out_inf);
    });
}
template <class C>
int mul_var_xyz_dev(ecgpu_ctx* ctx, const void* d_scalars, const void* d_xyz, size_t n, void* d_out_xy, void* d_out_inf) {
    if (n == 0) return ECGPU_OK;
    return decoded(ctx, decode_xyz<C>, d_xyz, nullptr, n, [&](const void* xy, const void* inf) {
        return mul_var_dev<C>(ctx, d_scalars, xy, inf, n, d_out_xy, d_out_inf);
    });
}

// aG + bP per element = two-term lincomb (mul_backend.rs:29-40).  Evaluated as a*G (table kernel) and b*P (variable-base
// kernel) into projective scratch halves, then one complete addition per element.
template <class C>
int mul_add_dev(ecgpu_ctx* ctx, const void* d_a, const void* d_b, const void* d_points_xy, const void* d_points_inf, size_t n,
                void* d_out_xy, void* d_out_inf) {
    constexpr int NS = Field<C>::NS;
    int rc;
    if ((rc = ensure_table<C>(ctx, n)) != ECGPU_OK) return rc;
    if (n == 0) return ECGPU_OK;
    const size_t tstride = var_base_slots<C>(n);
    DevCall call(ctx, 0, {{ctx->proj, n * 3 * NS * 4}, {ctx->vtab, tstride * var_base_tab_words<C>() * 4}});
    if (call.rc != ECGPU_OK) return call.rc;
    const Table& t = ctx->table[C::ID];
    uint32_t* pa = (uint32_t*)ctx->proj.p;
    call.mark(0);
    launch_fixed_base<C>(ctx->stream, (const uint8_t*)d_a, n, (const uint32_t*)t.d, t.w, t.nwin, pa, ctx->d_status);
    launch_var_base<C>(ctx->stream, (const uint8_t*)d_b, (const uint8_t*)d_points_xy, (const uint8_t*)d_points_inf, n,
                       (uint32_t*)ctx->vtab.p, tstride, nullptr, ctx->d_status, pa);                                   // pa[i] += b[i] P[i]
    return call.normalized<C>(n, d_out_xy, d_out_inf);
}
template <class C>
int mul_add_xyz_dev(ecgpu_ctx* ctx, const void* d_a, const void* d_b, const void* d_xyz, size_t n, void* d_out_xy, void* d_out_inf) {
    if (n == 0) return mul_add_dev<C>(ctx, d_a, d_b, nullptr, nullptr, 0, d_out_xy, d_out_inf);
    return decoded(ctx, decode_xyz<C>, d_xyz, nullptr, n, [&](const void* xy, const void* inf) {
        return mul_add_dev<C>(ctx, d_a, d_b, xy, inf, n, d_out_xy, d_out_inf);
    });
}

// ---- an MSM whose terms are spread over several GPUs: local half / combining half ------------------------
// xyz: d_xy holds projective records X || Y || Z and d_inf is unused (converted as in msm_dev)
template <class C>
int msm_parts_dev(ecgpu_ctx* ctx, const void* d_scalars, const void* d_xy, const void* d_inf, size_t n, size_t plan_terms,
                  void* d_parts, bool xyz = false) {
    if (n > msm_max_terms<C>() || plan_terms > msm_max_terms<C>()) {
        ctx->err = "MSM shard of 2^31 (k256: 2^30) or more terms";
        return ECGPU_ERR_ARG;
    }
    if (plan_terms < n) {
        ctx->err = "ecgpu_msm_parts_dev: plan_terms must be at least the shard's term count (and the same on every GPU)";
        return ECGPU_ERR_ARG;
    }
    const bool lanes = ctx->async && ctx->msm_lanes > 1;
    if (xyz && !lanes)
        return decoded(ctx, decode_xyz<C>, d_xy, nullptr, n, [&](const void* xy, const void* inf) {
            return msm_parts_dev<C>(ctx, d_scalars, xy, inf, n, plan_terms, d_parts);
        });
    const int c = ctx->msm_c ? ctx->msm_c : msm_choose_window<C>(plan_terms);
    MsmPlan plan = msm_plan<C>(n, c, msm_use_glv<C>(plan_terms));
    if (lanes)
        // Local halves of CONSECUTIVE sharded MSMs on rotating lanes (throughput form): this one runs on its lane
        // beside the exchange and the combining half of the previous one, which the caller keeps on the context's stream:
        //     parts(i) -> lane i % L      ecgpu_msm_parts_join_dev(d_parts(i - 1)); all-gather(i - 1); ecgpu_msm_finish_dev(i - 1)
        // d_parts belongs to the lane until ecgpu_msm_parts_join_dev(d_parts) or an ecgpu_msm_finish_dev that reads it (the
        // context's stream then waits for it), or ecgpu_synchronize.
        return on_lane<C>(ctx, plan.workspace_bytes, xyz, d_xy, d_inf, n, [&](ecgpu_ctx::MsmLane& l) -> int {
            // A lane remembers ONE record.  If the record of its previous local half was never joined (more local halves in flight
            // than lanes), that half is joined now — the context's stream waits for it before anything queued later —, so that
            // whatever the caller does with the old record afterwards is still ordered behind the kernels that wrote it.
            if (l.parts_out) HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, l.ev_done, 0));
            return ECGPU_OK;
        }, [&](ecgpu_ctx::MsmLane& l, const void* xy, const void* inf) {
            launch_msm_parts<C>(plan, l.s, (const uint8_t*)d_scalars, (const uint8_t*)xy, (const uint8_t*)inf, n, l.ws.p, (uint32_t*)d_parts,
                                ctx->d_status, l.ev_a, l.ev_b);
            l.parts_out = d_parts;
        });
    DevCall call(ctx, 0, {{ctx->msm_ws, plan.workspace_bytes}});
    if (call.rc != ECGPU_OK) return call.rc;
    call.mark(0);
    launch_msm_parts<C>(plan, ctx->stream, (const uint8_t*)d_scalars, (const uint8_t*)d_xy, (const uint8_t*)d_inf, n, ctx->msm_ws.p,
                        (uint32_t*)d_parts, ctx->d_status, ctx->timing_on ? ctx->ev[3] : nullptr, ctx->timing_on ? ctx->ev[4] : nullptr);
    call.mark(1);
    return call.done(SPANS_MSM_PARTS);
}

template <class C>
int msm_finish_dev(ecgpu_ctx* ctx, const void* d_parts_all, int nranks, size_t plan_terms, void* d_out_xy, void* d_out_inf) {
    constexpr int NS = Field<C>::NS;
    const int c = ctx->msm_c ? ctx->msm_c : msm_choose_window<C>(plan_terms);
    MsmPlan plan = msm_plan<C>(0, c, msm_use_glv<C>(plan_terms));   // only c, nwin and nparts matter here
    // With local halves in flight on lanes this call does not wait for all of them (that is the point of the lanes), only for those
    // whose record lies inside d_parts_all: the one-rank form passes its own record, and a caller may skip the join when no exchange
    // of its own reads the record.  Joined records (parts_out cleared) cost nothing here.  So this branch stays outside the call
    // frame, whose first act is to join every lane; nor does it touch the timing marks: ecgpu_last_timing keeps reading the last lane's.
    if (ctx->async && ctx->msm_lanes > 1) {
        int rc;
        if ((rc = ensure(ctx, ctx->proj, 3 * NS * 4)) != ECGPU_OK) return rc;
        if ((rc = ensure(ctx, ctx->bases, (size_t)plan.nwin * 3 * NS * 4)) != ECGPU_OK) return rc;
        const uintptr_t lo = reinterpret_cast<uintptr_t>(d_parts_all), hi = lo + (size_t)nranks * plan.parts_bytes;
        for (auto& l : ctx->lane) {
            const uintptr_t p = reinterpret_cast<uintptr_t>(l.parts_out);
            if (l.s && l.ev_done && l.parts_out && p >= lo && p < hi) {
                HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, l.ev_done, 0));
                l.parts_out = nullptr;
            }
        }
        launch_msm_finish<C>(plan, ctx->stream, (const uint32_t*)d_parts_all, nranks, (uint32_t*)ctx->bases.p, (uint32_t*)ctx->proj.p,
                             (uint8_t*)d_out_xy, (uint8_t*)d_out_inf);
        return finish(ctx);
    }
    DevCall call(ctx, 0, {{ctx->proj, 3 * NS * 4}, {ctx->bases, (size_t)plan.nwin * 3 * NS * 4}});
    if (call.rc != ECGPU_OK) return call.rc;
    call.mark(0);
    launch_msm_finish<C>(plan, ctx->stream, (const uint32_t*)d_parts_all, nranks, (uint32_t*)ctx->bases.p, (uint32_t*)ctx->proj.p,
                         (uint8_t*)d_out_xy, (uint8_t*)d_out_inf);
    call.mark(1);
    call.mark(2);
    return call.done();
}

template <class C>
size_t msm_parts_bytes(const ecgpu_ctx* ctx, size_t plan_terms) {
    return msm_plan<C>(0, ctx->msm_c ? ctx->msm_c : msm_choose_window<C>(plan_terms), msm_use_glv<C>(plan_terms)).parts_bytes;
}

// ---- host-pointer plumbing ---------------------------------------------------------------------------------

int upload(ecgpu_ctx* ctx, DevBuf& b, const void* host, size_t bytes) {
    int rc = ensure(ctx, b, bytes ? bytes : 16);
    if (rc != ECGPU_OK) return rc;
    if (bytes) HIP_TRY(ctx, hipMemcpyAsync(b.p, host, bytes, hipMemcpyHostToDevice, ctx->stream));
    return ECGPU_OK;
}
int download(ecgpu_ctx* ctx, void* host, const DevBuf& b, size_t bytes) {
    if (bytes && host) {
        HIP_TRY(ctx, hipMemcpyAsync(host, b.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    return ECGPU_OK;
}

// ---- pipelined host-pointer calls --------------------------------------------------------------------------------------
// A batch of independent units handed over in host memory is cut into chunks of PIPE_CHUNK units: an upload thread and a
// download thread move chunk i + 1 in and chunk i - 1 out (each on its own stream, PCIe is full duplex) while the calling
// thread runs the ordinary device-pointer entry point on chunk i.  Serially the transfers of a 2^20-scalar fixed-base
// batch take five times its compute time.
constexpr size_t PIPE_CHUNK = (size_t)1 << 18;
constexpr size_t PIPE_MIN = (size_t)1 << 19;
constexpr size_t MSM_PIPE_CHUNK = (size_t)1 << 22;   // terms per partial MSM of the host-pointer ecgpu_msm
// ECGPU_MSM_PIPE_LOG2 moves that (tuning knob; the tests use it to drive the chunked path with small inputs); the
// chunked path needs chunk starts that keep p224's 28-byte records 4-byte aligned, which every power of two does
inline size_t msm_pipe_chunk() {
    if (const char* e = knob("ECGPU_MSM_PIPE_LOG2")) {
        int v = atoi(e);
        if (v >= 8 && v <= 26) return (size_t)1 << v;
    }
    return MSM_PIPE_CHUNK;
}

// One array of a host-pointer call: the caller's memory, the context buffer it is staged in, bytes per element.  `secret`: it
// holds a secret of a uniform-schedule call or a value derived from one, and `staged` zeroes the buffer behind the call.
struct PipeIn { const uint8_t* host; DevBuf* dev; size_t unit; bool secret = false; };
struct PipeOut { uint8_t* host; DevBuf* dev; size_t unit; bool secret = false; };
constexpr bool SECRET = true;

template <class F>
int pipelined(ecgpu_ctx* ctx, size_t n, const std::vector<PipeIn>& ins, const std::vector<PipeOut>& outs, F&& compute,
              const size_t chunk = PIPE_CHUNK) {
    HIP_TRY(ctx, ctx->up_stream ? hipSuccess : hipStreamCreateWithFlags(&ctx->up_stream, hipStreamNonBlocking));
    HIP_TRY(ctx, ctx->down_stream ? hipSuccess : hipStreamCreateWithFlags(&ctx->down_stream, hipStreamNonBlocking));
    int rc;
    for (auto& a : ins) if (a.host && (rc = ensure(ctx, *a.dev, n * a.unit + 16)) != ECGPU_OK) return rc;
    for (auto& o : outs) if ((rc = ensure(ctx, *o.dev, n * o.unit + 16)) != ECGPU_OK) return rc;
    const size_t nchunks = (n + chunk - 1) / chunk;
    std::mutex mu;
    std::condition_variable cv;
    size_t uploaded = 0, computed = 0;
    bool failed = false;
    const int device = ctx->device;
    auto span = [&](size_t i, size_t* off, size_t* m) { *off = i * chunk; *m = n - *off < chunk ? n - *off : chunk; };
    auto up_body = [&] {
        bool ok = hipSetDevice(device) == hipSuccess;
        for (size_t i = 0; i < nchunks; i++) {
            size_t off, m;
            span(i, &off, &m);
            for (auto& a : ins)
                if (ok && a.host)
                    ok = hipMemcpyAsync((uint8_t*)a.dev->p + off * a.unit, a.host + off * a.unit, m * a.unit, hipMemcpyHostToDevice,
                                        ctx->up_stream) == hipSuccess;
            ok = ok && hipStreamSynchronize(ctx->up_stream) == hipSuccess;
            std::lock_guard<std::mutex> g(mu);
            if (!ok) failed = true;
            uploaded = i + 1;
            cv.notify_all();
            if (failed) return;
        }
    };
    auto down_body = [&] {
        bool ok = hipSetDevice(device) == hipSuccess;
        for (size_t i = 0; i < nchunks; i++) {
            {
                std::unique_lock<std::mutex> g(mu);
                cv.wait(g, [&] { return computed > i || failed; });
                if (failed) return;
            }
            size_t off, m;
            span(i, &off, &m);
            for (auto& o : outs)
                if (ok && o.host)
                    ok = hipMemcpyAsync(o.host + off * o.unit, (const uint8_t*)o.dev->p + off * o.unit, m * o.unit, hipMemcpyDeviceToHost,
                                        ctx->down_stream) == hipSuccess;
            ok = ok && hipStreamSynchronize(ctx->down_stream) == hipSuccess;
            if (!ok) {
                std::lock_guard<std::mutex> g(mu);
                failed = true;
                cv.notify_all();
                return;
            }
        }
    };
    std::thread up, down;
    try {                                                   // no C++ exception may cross the C ABI
        up = std::thread(up_body);
        down = std::thread(down_body);
    } catch (...) {
        {
            std::lock_guard<std::mutex> g(mu);
            failed = true;
            cv.notify_all();
        }
        if (up.joinable()) up.join();
        ctx->err = "could not start the transfer threads";
        return ECGPU_ERR_HIP;
    }
    rc = ECGPU_OK;
    for (size_t i = 0; i < nchunks; i++) {
        {
            std::unique_lock<std::mutex> g(mu);
            cv.wait(g, [&] { return uploaded > i || failed; });
            if (failed) break;
        }
        size_t off, m;
        span(i, &off, &m);
        int r = compute(off, m);
        std::lock_guard<std::mutex> g(mu);
        if (r != ECGPU_OK) {
            rc = r;
            failed = true;
        }
        computed = i + 1;
        cv.notify_all();
        if (failed) break;
    }
    up.join();
    down.join();
    if (rc == ECGPU_OK && failed) {
        ctx->err = "host <-> device transfer failed";
        rc = ECGPU_ERR_HIP;
    }
    return rc;
}

bool check_ctx(ecgpu_ctx* ctx) {
    if (!ctx) return false;
    if (hipSetDevice(ctx->device) == hipSuccess) return true;
    ctx->err = "hipSetDevice failed";
    return false;
}

// every error return leaves a message for ecgpu_last_error (never a stale one)
int arg_error(ecgpu_ctx* ctx, const char* fn) {
    if (ctx) ctx->err = std::string(fn) + ": NULL, misaligned or inconsistent argument";
    return ECGPU_ERR_ARG;
}
int curve_error(ecgpu_ctx* ctx, const char* fn) {
    if (ctx) ctx->err = std::string(fn) + ": unknown curve id, or the operation does not exist for this curve";
    return ECGPU_ERR_CURVE;
}

// ---- the one argument check of the device-pointer entry points ------------------------------------------------------------
// An entry point lists its pointers once, each with what is asked of it: NEED = not NULL when n > 0, ALWAYS = not NULL whatever n is
// (the output of a reducing call, a parts record), OPT = may be NULL; A16 = 16-byte aligned where it is looked at at all (a NEED or
// OPT pointer when n > 0 and it is there, an ALWAYS pointer always).  In the order of the early returns: no (usable) context ->
// ECGPU_ERR_ARG without a message; a pointer that fails, or the entry point's own condition on its sizes (`also_bad`) -> arg_error;
// an operation that does not exist for the curve (`no_such_op`) -> curve_error.  Nothing is queued before this returns ECGPU_OK.
enum : int { OPT = 0, NEED = 1, ALWAYS = 2, A16 = 4 };
struct DevArg { const void* p; int how; };
int dev_args(ecgpu_ctx* ctx, const char* fn, size_t n, std::initializer_list<DevArg> ptrs, bool also_bad = false, bool no_such_op = false) {
    if (!check_ctx(ctx)) return ECGPU_ERR_ARG;
    bool bad = also_bad;
    for (const DevArg& a : ptrs) {
        const bool looked_at = (a.how & ALWAYS) || n;
        if (!a.p) bad = bad || ((a.how & (NEED | ALWAYS)) && looked_at);
        else bad = bad || ((a.how & A16) && looked_at && !aligned16(a.p));
    }
    if (bad) return arg_error(ctx, fn);
    return no_such_op ? curve_error(ctx, fn) : (int)ECGPU_OK;
}

// ---- the one staging path of the host-pointer entry points -------------------------------------------------------------
// What every such entry point begins with, in the order of its early returns: no (usable) context -> ECGPU_ERR_ARG without a
// message; the queued work of an asynchronous context drained (SyncScope, which restores the mode when the call ends) -> a
// failed drain's code; the curve's field bytes L -> curve_error; the entry point's own condition (`bad`) -> arg_error.  The
// messages name `fn`, the public function.
struct HostCall {
    ecgpu_ctx* ctx;
    const char* fn;
    int rc;
    SyncScope sync;
    size_t L;
    HostCall(ecgpu_ctx* c, const char* fn_, int curve)
        : ctx(c), fn(fn_), rc(check_ctx(c) ? ECGPU_OK : ECGPU_ERR_ARG), sync(rc == ECGPU_OK ? c : nullptr), L(ecgpu_field_bytes(curve)) {
        if (rc == ECGPU_OK) rc = sync.rc != ECGPU_OK ? sync.rc : L ? (int)ECGPU_OK : curve_error(ctx, fn);
    }
    // a call that takes no curve (X448): the same early returns without the curve's
    HostCall(ecgpu_ctx* c, const char* fn_)
        : ctx(c), fn(fn_), rc(check_ctx(c) ? ECGPU_OK : ECGPU_ERR_ARG), sync(rc == ECGPU_OK ? c : nullptr), L(0) {
        if (rc == ECGPU_OK) rc = sync.rc;
    }
    bool bad(bool args_bad) {
        if (rc == ECGPU_OK && args_bad) rc = arg_error(ctx, fn);
        return rc != ECGPU_OK;
    }
};

inline const void* piece_of(const PipeIn& a, size_t off) { return a.host ? (const uint8_t*)a.dev->p + off * a.unit : nullptr; }

// the uniform-schedule forms keep their scalars and results in the staging set of wipe_scratch; a list that marks a buffer
// outside that set gets it zeroed all the same
struct StagedWipe {
    ecgpu_ctx* ctx;
    const std::vector<PipeIn>& ins;
    const std::vector<PipeOut>& outs;
    ~StagedWipe() {
        std::vector<DevBuf*> marked;
        for (auto& a : ins) if (a.secret) marked.push_back(a.dev);
        for (auto& o : outs) if (o.secret) marked.push_back(o.dev);
        for (DevBuf* b : marked) wipe_bufs(ctx, {b});
        if (!marked.empty()) wipe_scratch(ctx, WIPE_STAGING);
    }
};

// Stage in, run the `_dev` entry, stage out.  An entry point states its arrays once (`ins`, `outs`) and its device call once:
// call(in, out, m) receives the device address of each array's first element of the piece it is given (in list order;
// nullptr for an input the caller left out: host == nullptr, which is not staged) and the piece's element count m.  From
// PIPE_MIN elements on a STAGE_BATCH call is `pipelined` piece by piece; otherwise everything goes up on the context's stream,
// the call runs once (for n == 0 too: it may build a table, and a reducing call writes the identity) and the results come
// down.  Whatever way the call leaves, the buffers marked `secret` are zeroed behind its last kernel.
enum StageMode {
    STAGE_BATCH,     // n independent elements in, n records out
    STAGE_WHOLE,     // the same, never cut (ecgpu_batch_normalize, the GLV and self-test entry points)
    STAGE_REDUCE     // n elements in, one record out
};
template <class F>
int staged(ecgpu_ctx* ctx, size_t n, const std::vector<PipeIn>& ins, const std::vector<PipeOut>& outs, F&& call,
           StageMode mode = STAGE_BATCH) {
    StagedWipe wipe{ctx, ins, outs};
    std::vector<const void*> in(ins.size());
    std::vector<void*> out(outs.size());
    auto piece = [&](size_t off, size_t m) {
        for (size_t i = 0; i < ins.size(); i++) in[i] = piece_of(ins[i], off);
        for (size_t i = 0; i < outs.size(); i++) out[i] = (uint8_t*)outs[i].dev->p + off * outs[i].unit;
        return call(in.data(), out.data(), m);
    };
    if (mode == STAGE_BATCH && n >= PIPE_MIN) return pipelined(ctx, n, ins, outs, piece);
    const size_t nout = mode == STAGE_REDUCE ? 1 : n;
    int rc;
    for (auto& a : ins) if (a.host && (rc = upload(ctx, *a.dev, a.host, n * a.unit)) != ECGPU_OK) return rc;
    for (auto& o : outs) if ((rc = ensure(ctx, *o.dev, nout * o.unit + 16)) != ECGPU_OK) return rc;
    if ((rc = piece(0, n)) != ECGPU_OK) return rc;
    for (auto& o : outs) if ((rc = download(ctx, o.host, *o.dev, nout * o.unit)) != ECGPU_OK) return rc;
    return ECGPU_OK;
}

// The host-pointer MSMs (result staged in out0 / out1).  partial(c, in, m, d_out_xy, d_out_inf) runs the internal MSM
// template of curve `c` on the m terms at in[] (the arrays of `ins`, as for `staged`).
template <class F>
int msm_staged(ecgpu_ctx* ctx, int curve, size_t n, const std::vector<PipeIn>& ins, uint8_t* out_xy, uint8_t* out_inf, F&& partial) {
    const size_t L = ecgpu_field_bytes(curve), pipe_chunk = msm_pipe_chunk();
    if (n < 2 * pipe_chunk)
        return staged(ctx, n, ins, {{out_xy, &ctx->out0, 2 * L}, {out_inf, &ctx->out1, 1}}, [&](auto in, auto out, size_t m) {
            return dispatch(curve, [&](auto c) { return partial(c, in, m, out[0], out[1]); });
        }, STAGE_REDUCE);
    // An MSM needs all of its terms before its sort can start, and 96 (144) bytes per term take longer to upload than
    // the MSM takes to compute: sum_i k_i P_i is computed as one MSM per chunk of 2^22 terms, each under the upload of
    // the next chunk, and the partial sums are added at the end.  The partial records sit at a pitch of 2L bytes
    // (56 for p224, 132 for p521: not 16-byte multiples), so the internal implementations are called directly — the
    // kernels of those curves use 4-byte / byte accesses; only the public *_dev entry points insist on 16-byte bases.
    const size_t nparts = (n + pipe_chunk - 1) / pipe_chunk;
    int rc;
    if ((rc = ensure(ctx, ctx->out0, (nparts + 1) * 2 * L + 64)) != ECGPU_OK) return rc;
    if ((rc = ensure(ctx, ctx->out1, nparts + 32)) != ECGPU_OK) return rc;
    uint8_t* part_xy = (uint8_t*)ctx->out0.p + (2 * L + 15) / 16 * 16;          // [0] is the final result
    uint8_t* part_inf = (uint8_t*)ctx->out1.p + 16;
    return dispatch(curve, [&](auto c) -> int {
        std::vector<const void*> in(ins.size());
        int r = pipelined(ctx, n, ins, {}, [&](size_t off, size_t m) {
            for (size_t i = 0; i < ins.size(); i++) in[i] = piece_of(ins[i], off);
            return partial(c, in.data(), m, part_xy + off / pipe_chunk * 2 * L, part_inf + off / pipe_chunk);
        }, pipe_chunk);
        if (r != ECGPU_OK) return r;
        if ((r = point_sum_dev<decltype(c)>(ctx, part_xy, part_inf, nparts, ctx->out0.p, ctx->out1.p)) != ECGPU_OK) return r;
        if ((r = download(ctx, out_xy, ctx->out0, 2 * L)) != ECGPU_OK) return r;
        return download(ctx, out_inf, ctx->out1, 1);
    });
}

// ---- hash-to-curve (ecgpu_h2c.h): expand -> u in scratch -> map to projective scratch -> the normalisation of the `_ct` forms ----
// RO: two field elements per message and Q0 + Q1; NU: one and Q0; SCALAR: one draw reduced mod n, written straight to the caller's
// array; MAP: the caller's u records (per_point of them per output) instead of hashed ones.  The u records live in sg_k, the verdict
// bytes in ct_flags, the points in proj: all wiped behind the call (hashed inputs may be secret).
enum : int { H2C_RO = 0, H2C_NU = 1, H2C_SCALAR = 2, H2C_MAP = 3 };

template <class C>
int h2c_dev(ecgpu_ctx* ctx, int mode, const void* d_in, size_t msg_len, int per_point, const void* d_dstp, size_t dstp_len, size_t n,
            void* d_out, void* d_out_inf) {
    constexpr int NS = Field<C>::NS;
    constexpr size_t WB = WireBytes<C>::value;
    if (n == 0) return ECGPU_OK;
    if (mode == H2C_SCALAR) {
        DevCall call(ctx, 0, {});
        if (call.rc != ECGPU_OK) return call.rc;
        call.mark(0);
        launch_h2c_expand<C>(ctx->stream, (const uint8_t*)d_in, msg_len, n, (const uint8_t*)d_dstp, dstp_len, 1, true, (uint8_t*)d_out);
        call.mark(1);
        return call.done(SPANS_NO_NORMALIZE);
    }
    const int count = mode == H2C_MAP ? per_point : mode == H2C_RO ? 2 : 1;
    DevCall call(ctx, WIPE_SCRATCH | WIPE_SIGN,
                 {{ctx->proj, n * 3 * NS * 4}, {ctx->ct_flags, n + 16}, {ctx->sg_k, n * count * WB + 16, mode != H2C_MAP}});
    if (call.rc != ECGPU_OK) return call.rc;
    call.mark(0);
    const uint8_t* d_u = (const uint8_t*)d_in;
    if (mode != H2C_MAP) {
        launch_h2c_expand<C>(ctx->stream, (const uint8_t*)d_in, msg_len, n, (const uint8_t*)d_dstp, dstp_len, count, false,
                             (uint8_t*)ctx->sg_k.p);
        d_u = (const uint8_t*)ctx->sg_k.p;
    }
    call.mark(3);
    launch_h2c_map<C>(ctx->stream, d_u, count, n, (uint32_t*)ctx->proj.p, (uint8_t*)ctx->ct_flags.p, ctx->d_status);
    return call.normalized<C>(n, d_out, d_out_inf, SPANS_H2C);
}

// whether the parameter set has a suite, and its hash: H2cSuite (ecgpu_h2c.h) is the one place that knows, asked through the
// translation unit of the curve.  Every id without a suite, p521 included, and every unknown id: false.
inline bool h2c_has_suite(int curve) {
    return dispatch(curve, [](auto c) { return h2c_supported<decltype(c)>() ? 1 : 0; }) == 1;
}
inline int h2c_suite_digest(int curve) {
    return dispatch(curve, [](auto c) { return h2c_digest<decltype(c)>(); });
}

// `Domain::xmd` on the host, once per call: DST' = DST || I2OSP(len(DST), 1), a DST above 255 bytes replaced by
// H("H2C-OVERSIZE-DST-" || DST) with the suite's hash first; uploaded to ec_id.  (The curve is known to have a suite.)  DST' is built
// in this frame's memory, so the upload has arrived before the function returns.
int h2c_stage_dst(ecgpu_ctx* ctx, int curve, const uint8_t* dst, size_t dst_len, size_t* dstp_len) {
    uint8_t dp[256];
    size_t len = dst_len;
    if (dst_len > 255) {
        static const uint8_t salt[] = "H2C-OVERSIZE-DST-";
        const HashPiece pc[2] = {{salt, sizeof(salt) - 1}, {dst, dst_len}};
        if (h2c_suite_digest(curve) == HASH_SHA384) {
            sha2_pieces<HASH_SHA384, 2>(dp, pc);
            len = HASH_SHA384;
        } else {
            sha2_pieces<HASH_SHA256, 2>(dp, pc);
            len = HASH_SHA256;
        }
    } else {
        memcpy(dp, dst, dst_len);
    }
    dp[len] = (uint8_t)len;
    *dstp_len = len + 1;
    if (int rc = upload(ctx, ctx->ec_id, dp, len + 1)) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return ECGPU_OK;
}

// the device-pointer call on a DST' that is already in ec_id: every chunk of a host-pointer call goes through it.  (There is no
// public `_dev` form of these calls yet: see include/ecgpu.h.)
int h2c_run(ecgpu_ctx* ctx, const char* fn, int curve, int mode, const void* d_in, size_t msg_len, int per_point, size_t dstp_len,
            size_t n, void* d_out, void* d_out_inf) {
    const bool bad_shape = mode == H2C_MAP && per_point != 1 && per_point != 2;
    if (int rc = dev_args(ctx, fn, n, {{d_in, mode == H2C_MAP ? NEED | A16 : (msg_len ? NEED : OPT)}, {d_out, NEED | A16}, {d_out_inf, OPT}},
                          bad_shape, !h2c_has_suite(curve))) return rc;
    const int rc = dispatch(curve, [&](auto c) {
        return h2c_dev<decltype(c)>(ctx, mode, d_in, msg_len, per_point, ctx->ec_id.p, dstp_len, n, d_out, d_out_inf);
    });
    return rc == ECGPU_ERR_CURVE ? curve_error(ctx, fn) : rc;
}

}  // namespace

// ================================================================================================================
// C ABI
// ================================================================================================================

namespace {
// ---- signature verification and public-key recovery ------------------------------------------------------------------------
// The one pipeline of the six schemes: prepare -> u1 G + u2 Q -> normalise -> finish.  A scheme (below) states its own scratch beside
// the common one, where the normalisation writes (d_xy: read after the reservations, ctx->ec_xy may have grown), and its two stages;
// both are handed the shared scratch by name.
struct VerifyScratch {
    uint8_t *u1, *u2, *q, *valid;      // prepare writes: the scalars of G and of Q, Q as x || y, the verdict so far
    uint8_t* xy;                       // finish reads: u1 G + u2 Q as x || y records (*d_xy) ...
    const uint8_t* inf;                // ... and their identity flags
};
template <class C, class Prepare, class Finish>
int verify_pipeline(ecgpu_ctx* ctx, size_t n, std::initializer_list<Reserve> extra, void* const* d_xy, Prepare&& prepare,
                    Finish&& finish) {
    constexpr int NS = Field<C>::NS;
    const size_t L = 4 * C::N;
    int rc;
    if ((rc = ensure_table<C>(ctx, n)) != ECGPU_OK) return rc;
    if (n == 0) return ECGPU_OK;
    const size_t tstride = var_base_slots<C>(n);
    DevCall call(ctx, 0,
                 {{ctx->proj, n * 3 * NS * 4}, {ctx->vtab, tstride * var_base_tab_words<C>() * 4}, {ctx->ec_u1, n * L}, {ctx->ec_u2, n * L},
                  {ctx->ec_q, n * 2 * L}, {ctx->ec_valid, n + 16}, {ctx->ec_inf, n + 16}}, extra);
    if (call.rc != ECGPU_OK) return call.rc;
    const Table& t = ctx->table[C::ID];
    uint32_t* pa = (uint32_t*)ctx->proj.p;
    const VerifyScratch v{(uint8_t*)ctx->ec_u1.p, (uint8_t*)ctx->ec_u2.p, (uint8_t*)ctx->ec_q.p, (uint8_t*)ctx->ec_valid.p,
                          (uint8_t*)*d_xy, (const uint8_t*)ctx->ec_inf.p};
    call.mark(0);
    prepare(v);
    call.mark(3);
    launch_fixed_base<C>(ctx->stream, v.u1, n, (const uint32_t*)t.d, t.w, t.nwin, pa, ctx->d_status);
    launch_var_base<C>(ctx->stream, v.u2, v.q, nullptr, n, (uint32_t*)ctx->vtab.p, tstride, nullptr, ctx->d_status, pa);   // pa[i] += u2[i] Q[i]
    call.mark(1);
    if ((rc = normalize_out<C>(ctx, n, v.xy, ctx->ec_inf.p)) != ECGPU_OK) return rc;
    finish(v);
    call.mark(2);
    return call.done(SPANS_VERIFY);
}

// ECDSA verification and recovery invert one scalar per signature: done for the whole batch by Montgomery's trick, the inverses in
// ec_winv, their prefix products in ctx->prefix (the size normalize_out asks for later)
template <class C>
int ecdsa_verify_dev(ecgpu_ctx* ctx, const void* d_z, const void* d_r, const void* d_s, const void* d_q_xy, size_t n, int reject_high_s,
                     void* d_ok) {
    static_assert(Field<C>::NS >= C::N, "the normalisation's prefix array holds the inverses' prefix products too");
    const size_t L = 4 * C::N;
    return verify_pipeline<C>(
        ctx, n, {{ctx->ec_xy, n * 2 * L}, {ctx->ec_winv, n * L + 16}, {ctx->prefix, n * Field<C>::NS * 4}}, &ctx->ec_xy.p,
        [&](const VerifyScratch& v) {
            launch_ecdsa_prepare<C>(ctx->stream, (const uint8_t*)d_z, (const uint8_t*)d_r, (const uint8_t*)d_s, (const uint8_t*)d_q_xy, n,
                                    reject_high_s, v.u1, v.u2, v.q, v.valid, (uint32_t*)ctx->prefix.p, (uint8_t*)ctx->ec_winv.p);
        },
        [&](const VerifyScratch& v) { launch_ecdsa_finish<C>(ctx->stream, v.xy, v.inf, (const uint8_t*)d_r, v.valid, n, (uint8_t*)d_ok); });
}

// (the keys are normalised straight into the caller's d_out_xy, which the finish kernel then fixes up in place: no ec_xy)
template <class C>
int ecdsa_recover_dev(ecgpu_ctx* ctx, const void* d_z, const void* d_r, const void* d_s, const void* d_recid, size_t n, int reject_high_s,
                      void* d_out_xy, void* d_ok) {
    static_assert(Field<C>::NS >= C::N, "the normalisation's prefix array holds the inverses' prefix products too");
    const size_t L = 4 * C::N;
    return verify_pipeline<C>(
        ctx, n, {{ctx->ec_winv, n * L + 16}, {ctx->prefix, n * Field<C>::NS * 4}}, &d_out_xy,
        [&](const VerifyScratch& v) {
            launch_ecdsa_recover_prepare<C>(ctx->stream, (const uint8_t*)d_z, (const uint8_t*)d_r, (const uint8_t*)d_s,
                                            (const uint8_t*)d_recid, n, reject_high_s, v.u1, v.u2, v.q, v.valid, (uint32_t*)ctx->prefix.p,
                                            (uint8_t*)ctx->ec_winv.p);
        },
        [&](const VerifyScratch& v) { launch_ecdsa_recover_finish<C>(ctx->stream, v.xy, v.inf, v.valid, n, (uint8_t*)d_ok); });
}

int schnorr_verify_dev(ecgpu_ctx* ctx, const void* d_e, const void* d_r, const void* d_s, const void* d_p_xy, size_t n, void* d_ok) {
    return verify_pipeline<K256Params>(
        ctx, n, {{ctx->ec_xy, n * 64}}, &ctx->ec_xy.p,
        [&](const VerifyScratch& v) {
            launch_schnorr_prepare(ctx->stream, (const uint8_t*)d_e, (const uint8_t*)d_r, (const uint8_t*)d_s, (const uint8_t*)d_p_xy, n,
                                   v.u1, v.u2, v.q, v.valid);
        },
        [&](const VerifyScratch& v) { launch_schnorr_finish(ctx->stream, v.xy, v.inf, (const uint8_t*)d_r, v.valid, n, (uint8_t*)d_ok); });
}

// (from wire bytes: the prepare kernel splits the signatures and leaves r in ec_r for the finish kernel)
int schnorr_verify_raw_dev(ecgpu_ctx* ctx, const void* d_pk_x, const void* d_msgs, size_t msg_len, const void* d_sigs, size_t n,
                           void* d_ok) {
    return verify_pipeline<K256Params>(
        ctx, n, {{ctx->ec_xy, n * 64}, {ctx->ec_r, n * 32}}, &ctx->ec_xy.p,
        [&](const VerifyScratch& v) {
            launch_schnorr_prepare_raw(ctx->stream, (const uint8_t*)d_pk_x, (const uint8_t*)d_msgs, msg_len, (const uint8_t*)d_sigs, n, v.u1,
                                       v.u2, v.q, (uint8_t*)ctx->ec_r.p, v.valid);
        },
        [&](const VerifyScratch& v) {
            launch_schnorr_finish(ctx->stream, v.xy, v.inf, (const uint8_t*)ctx->ec_r.p, v.valid, n, (uint8_t*)d_ok);
        });
}

int sm2dsa_verify_dev(ecgpu_ctx* ctx, const void* d_e, const void* d_r, const void* d_s, const void* d_q_xy, size_t n, void* d_ok) {
    return verify_pipeline<Sm2Params>(
        ctx, n, {{ctx->ec_xy, n * 64}}, &ctx->ec_xy.p,
        [&](const VerifyScratch& v) {
            launch_sm2dsa_prepare(ctx->stream, (const uint8_t*)d_r, (const uint8_t*)d_s, (const uint8_t*)d_q_xy, n, v.u1, v.u2, v.q, v.valid);
        },
        [&](const VerifyScratch& v) {
            launch_sm2dsa_finish(ctx->stream, (const uint8_t*)d_e, v.xy, v.inf, (const uint8_t*)d_r, v.valid, n, (uint8_t*)d_ok);
        });
}

// d_h: 32-byte hashes; d_sigs: 48-byte signatures S0 || S1
int bign_verify_dev(ecgpu_ctx* ctx, const void* d_h, const void* d_sigs, const void* d_q_xy, size_t n, void* d_ok) {
    return verify_pipeline<Bign256Params>(
        ctx, n, {{ctx->ec_xy, n * 64}}, &ctx->ec_xy.p,
        [&](const VerifyScratch& v) {
            launch_bign_prepare(ctx->stream, (const uint8_t*)d_h, (const uint8_t*)d_sigs, (const uint8_t*)d_q_xy, n, v.u1, v.u2, v.q, v.valid);
        },
        [&](const VerifyScratch& v) {
            launch_bign_finish(ctx->stream, (const uint8_t*)d_h, v.xy, v.inf, (const uint8_t*)d_sigs, v.valid, n, (uint8_t*)d_ok);
        });
}

// The one front stage of the message-level verifiers (the counterpart of `decoded`): the hash kernel `hash()` writes the prehash
// form into the scratch reserved here; the frame is opened before it, so the MSM lanes are joined before it reads the caller's
// messages; the scheme's pipeline `then()` runs as the second stage, under KeepStatus.
template <class Hash, class Then>
int hashed(ecgpu_ctx* ctx, std::initializer_list<Reserve> bufs, Hash&& hash, Then&& then) {
    DevCall front(ctx, 0, bufs);
    if (front.rc != ECGPU_OK) return front.rc;
    hash();
    KeepStatus keep(ctx);
    return then();
}
}  // namespace

extern "C" {

const char* ecgpu_version(void) { return "ecgpu 0.1 (gfx950)"; }

size_t ecgpu_field_bytes(int curve) {
    switch (curve) {
    case ECGPU_K256: case ECGPU_P256: return 32;
    case ECGPU_P384: case ECGPU_BP384: case ECGPU_BP384T1: return 48;
    case ECGPU_SM2: case ECGPU_BP256: case ECGPU_BP256T1: case ECGPU_BIGN256: return 32;
    case ECGPU_P224: return 28;
    case ECGPU_P192: return 24;
    case ECGPU_P521: return 66;
    default: return 0;
    }
}

int ecgpu_device_count(void) {
    int count = 0, usable = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
        (void)hipGetLastError();
        return 0;
    }
    for (int d = 0; d < count; d++) {          // the leading run of gfx950 devices: a group lists devices 0 .. count - 1
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, d) != hipSuccess || std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) break;
        usable++;
    }
    return usable;
}

int ecgpu_init(ecgpu_ctx** out, int device) {
    if (!out) return ECGPU_ERR_ARG;
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0 || device < 0 || device >= count) return ECGPU_ERR_NO_DEVICE;
    if (hipSetDevice(device) != hipSuccess) return ECGPU_ERR_NO_DEVICE;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return ECGPU_ERR_NO_DEVICE;
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        std::fprintf(stderr, "ecgpu: device %d is %s; this library is built for gfx950 only\n", device, prop.gcnArchName);
        return ECGPU_ERR_NO_DEVICE;
    }
    ecgpu_ctx* ctx = new (std::nothrow) ecgpu_ctx();
    if (!ctx) return ECGPU_ERR_OOM;
    ctx->device = device;
    bool ok = hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking) == hipSuccess;
    ctx->stream = ctx->own_stream;
    ok = ok && hipMalloc(reinterpret_cast<void**>(&ctx->d_status), sizeof(int)) == hipSuccess;
    ok = ok && hipHostMalloc(reinterpret_cast<void**>(&ctx->h_status), sizeof(int)) == hipSuccess;
    for (auto& e : ctx->ev) ok = ok && hipEventCreate(&e) == hipSuccess;
    if (!ok) {
        ecgpu_destroy(ctx);
        return ECGPU_ERR_HIP;
    }
    *out = ctx;
    return ECGPU_OK;
}

void ecgpu_destroy(ecgpu_ctx* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    for (DevBuf* b : {&ctx->proj, &ctx->prefix, &ctx->vtab, &ctx->bases, &ctx->in0, &ctx->in1, &ctx->in2, &ctx->in3,
                      &ctx->out0, &ctx->out1, &ctx->msm_ws, &ctx->ec_u1, &ctx->ec_u2, &ctx->ec_winv, &ctx->ec_q, &ctx->ec_valid, &ctx->ec_xy,
                      &ctx->ec_inf, &ctx->ec_r, &ctx->ec_e, &ctx->ec_s, &ctx->ec_id})
        if (b->p) (void)hipFree(b->p);
    for (DevBuf* b : {&ctx->ct_flags, &ctx->cx_xy, &ctx->cx_inf, &ctx->sg_k, &ctx->sg_flag, &ctx->sg_state, &ctx->sg_dp, &ctx->out2,
                      &ctx->out3})
        if (b->p) (void)hipFree(b->p);
    for (auto& l : ctx->lane) {
        if (l.s) (void)hipStreamSynchronize(l.s);
        for (DevBuf* b : {&l.ws, &l.proj, &l.prefix, &l.cx_xy, &l.cx_inf})
            if (b->p) (void)hipFree(b->p);
        for (hipEvent_t e : {l.ev_in, l.ev_a, l.ev_b, l.ev_done})
            if (e) (void)hipEventDestroy(e);
        if (l.s) (void)hipStreamDestroy(l.s);
    }
    for (int id = 0; id < 12; id++) {                            // the last context of the device frees the shared tables
        release_table(ctx, id);
        release_ct_lut(ctx, id);
    }
    if (ctx->d_status) (void)hipFree(ctx->d_status);
    if (ctx->h_status) (void)hipHostFree(ctx->h_status);
    for (auto& e : ctx->ev)
        if (e) (void)hipEventDestroy(e);
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
    if (ctx->up_stream) (void)hipStreamDestroy(ctx->up_stream);
    if (ctx->down_stream) (void)hipStreamDestroy(ctx->down_stream);
    delete ctx;
}

const char* ecgpu_last_error(const ecgpu_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

void* ecgpu_host_alloc(ecgpu_ctx* ctx, size_t bytes) {
    if (!check_ctx(ctx) || bytes == 0) return nullptr;
    void* p = nullptr;
    if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) {
        ctx->err = "hipHostMalloc failed";
        return nullptr;
    }
    return p;
}

void ecgpu_host_free(ecgpu_ctx* ctx, void* p) {
    if (p && check_ctx(ctx)) (void)hipHostFree(p);
}

void* ecgpu_dev_alloc(ecgpu_ctx* ctx, size_t bytes) {
    if (!check_ctx(ctx) || bytes == 0) return nullptr;
    void* p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess) {
        ctx->err = "hipMalloc failed";
        return nullptr;
    }
    return p;
}

void ecgpu_dev_free(ecgpu_ctx* ctx, void* d_ptr) {
    if (!d_ptr || !check_ctx(ctx)) return;
    (void)hipStreamSynchronize(ctx->stream);
    (void)hipFree(d_ptr);
}

int ecgpu_copy_to_device(ecgpu_ctx* ctx, void* d_dst, const void* h_src, size_t bytes) {
    if (!check_ctx(ctx)) return ECGPU_ERR_ARG;
    if (bytes == 0) return ECGPU_OK;
    if (!d_dst || !h_src) {
        ctx->err = "ecgpu_copy_to_device: null pointer";
        return arg_error(ctx, __func__);
    }
    if (int rc = join_lanes(ctx)) return rc;             // (an MSM on a lane may be writing / reading the buffer)
    HIP_TRY(ctx, hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return ECGPU_OK;
}

int ecgpu_copy_to_host(ecgpu_ctx* ctx, void* h_dst, const void* d_src, size_t bytes) {
    if (!check_ctx(ctx)) return ECGPU_ERR_ARG;
    if (bytes == 0) return ECGPU_OK;
    if (!h_dst || !d_src) {
        ctx->err = "ecgpu_copy_to_host: null pointer";
        return arg_error(ctx, __func__);
    }
    if (int rc = join_lanes(ctx)) return rc;             // (an MSM on a lane may be writing / reading the buffer)
    HIP_TRY(ctx, hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return ECGPU_OK;
}

int ecgpu_set_stream(ecgpu_ctx* ctx, void* stream) {
    if (!ctx) return arg_error(ctx, __func__);
    if (ctx->async && ctx->pending && check_ctx(ctx)) (void)drain(ctx);     // the status word follows the old stream
    ctx->stream = stream ? reinterpret_cast<hipStream_t>(stream) : ctx->own_stream;
    return ECGPU_OK;
}

int ecgpu_set_base_window(ecgpu_ctx* ctx, int curve, int window_bits) {
    if (!ctx || curve < 0 || curve > 11) return ECGPU_ERR_CURVE;
    if (window_bits == 0) {                                   // back to the automatic choice below the curve's default maximum
        ctx->want_w[curve] = ecgpu_ctx().want_w[curve];
        ctx->w_pinned[curve] = false;
        return ECGPU_OK;
    }
    if (window_bits < 4 || window_bits > 26) return arg_error(ctx, __func__);
    ctx->want_w[curve] = window_bits;
    ctx->w_pinned[curve] = true;
    return ECGPU_OK;
}

int ecgpu_set_table_policy(ecgpu_ctx* ctx, int policy) {
    if (!ctx || (policy != ECGPU_TABLE_ADAPTIVE && policy != ECGPU_TABLE_EAGER)) return arg_error(ctx, __func__);
    ctx->table_policy = policy;
    return ECGPU_OK;
}

int ecgpu_set_table_budget(ecgpu_ctx* ctx, size_t max_table_bytes) {
    if (!ctx) return arg_error(ctx, __func__);
    ctx->table_budget = max_table_bytes;
    return ECGPU_OK;
}

int ecgpu_base_table_info(ecgpu_ctx* ctx, int curve, int* window_bits, size_t* table_bytes, double* build_ms) {
    if (!ctx || curve < 0 || curve > 11) return ECGPU_ERR_CURVE;
    const Table& t = ctx->table[curve];
    int w = 0;
    size_t bytes = 0;
    double ms = 0;
    if (t.d) {
        TableRegistry& reg = table_registry(ctx->device);
        std::lock_guard<std::mutex> lock(reg.mu);
        auto it = reg.tabs.find(std::make_tuple(ctx->device, curve, t.w));
        if (it != reg.tabs.end()) {
            w = t.w;
            bytes = it->second.bytes;
            ms = it->second.build_ms;
        }
    }
    if (window_bits) *window_bits = w;
    if (table_bytes) *table_bytes = bytes;
    if (build_ms) *build_ms = ms;
    return ECGPU_OK;
}

int ecgpu_set_msm_window(ecgpu_ctx* ctx, int window_bits) {
    if (!ctx) return arg_error(ctx, __func__);
    if (window_bits != 0 && (window_bits < 4 || window_bits > 16)) return arg_error(ctx, __func__);
    ctx->msm_c = window_bits;
    return ECGPU_OK;
}

int ecgpu_set_msm_lanes(ecgpu_ctx* ctx, int lanes) {
    if (!check_ctx(ctx)) return ECGPU_ERR_ARG;
    if (lanes < 1 || lanes > 4) return arg_error(ctx, __func__);
    int rc = ctx->async ? drain(ctx) : ECGPU_OK;       // nothing in flight on a lane while the mode changes
    ctx->msm_lanes = lanes;
    return rc;
}

int ecgpu_set_timing(ecgpu_ctx* ctx, int on) {
    if (!check_ctx(ctx)) return ECGPU_ERR_ARG;
    ctx->timing_on = on != 0;
    if (!ctx->timing_on) {
        ctx->spans.clear();
        ctx->timing.clear();
    }
    return ECGPU_OK;
}

int ecgpu_set_async(ecgpu_ctx* ctx, int on) {
    if (!check_ctx(ctx)) return ECGPU_ERR_ARG;
    int rc = ecgpu_synchronize(ctx);          // what was queued so far is reported here
    if (on && !ctx->async) {
        HIP_TRY(ctx, hipMemsetAsync(ctx->d_status, 0, sizeof(int), ctx->stream));
        ctx->deferred = 0;
    }
    ctx->async = on != 0;
    return rc;
}

int ecgpu_synchronize(ecgpu_ctx* ctx) {
    if (!check_ctx(ctx)) return ECGPU_ERR_ARG;
    if (!ctx->async) {
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        return ECGPU_OK;
    }
    // (nothing queued since the last drain: the status word on the device is clear and there is nothing to wait for — a caller that
    // switches the mode around every call, like ecgpu_group_msm_dev, pays for one round trip per call, not two)
    if (ctx->pending || ctx->lanes_pending) {
        int rc = drain(ctx);
        if (rc != ECGPU_OK) return rc;
    } else {
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    const int st = ctx->deferred;
    ctx->deferred = 0;
    return status_error(ctx, st);
}

int ecgpu_wipe(ecgpu_ctx* ctx) {
    if (!check_ctx(ctx)) return ECGPU_ERR_ARG;
    for (auto& l : ctx->lane)
        if (l.s) HIP_TRY(ctx, hipStreamSynchronize(l.s));
    for (DevBuf* b : {&ctx->proj, &ctx->prefix, &ctx->vtab, &ctx->bases, &ctx->in0, &ctx->in1, &ctx->in2, &ctx->in3, &ctx->out0, &ctx->out1,
                      &ctx->msm_ws, &ctx->ec_u1, &ctx->ec_u2, &ctx->ec_winv, &ctx->ec_q, &ctx->ec_valid, &ctx->ec_xy, &ctx->ec_inf, &ctx->ec_r, &ctx->ec_e,
                      &ctx->ec_s, &ctx->ec_id, &ctx->ct_flags, &ctx->cx_xy, &ctx->cx_inf, &ctx->sg_k, &ctx->sg_flag, &ctx->sg_state, &ctx->sg_dp,
                      &ctx->out2, &ctx->out3})
        if (b->p) HIP_TRY(ctx, hipMemsetAsync(b->p, 0, b->cap, ctx->stream));
    for (auto& l : ctx->lane)
        for (DevBuf* b : {&l.ws, &l.proj, &l.prefix, &l.cx_xy, &l.cx_inf})
            if (b->p) HIP_TRY(ctx, hipMemsetAsync(b->p, 0, b->cap, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return ECGPU_OK;
}

// test-only (not in include/ecgpu.h): the candidate cap of the RFC 6979 generator of THIS context; anything outside [1, 128]
// restores 128
void ecgpu_testhook_rfc6979_max_candidates(ecgpu_ctx* ctx, int cap) {
    if (ctx) ctx->rfc6979_cap = cap >= 1 && cap <= 128 ? cap : 128;
}

// test-only (not in include/ecgpu.h): the bytes that are not zero in the buffers the secret-scalar calls wipe behind themselves
// (wipe_scratch's sets and the staging buffers a host-pointer call marks SECRET), over everything a call ever asked of them (the
// headroom of an allocation beyond that was never written by this context and is not its to vouch for); -1 on a failed copy.
// tests/test_gpu_pke.py reads it after an encryption and after a decryption.
long long ecgpu_testhook_wiped_scratch_nonzero(ecgpu_ctx* ctx) {
    if (!check_ctx(ctx) || hipStreamSynchronize(ctx->stream) != hipSuccess) return -1;
    long long count = 0;
    std::vector<uint8_t> host;
    for (DevBuf* b : {&ctx->proj, &ctx->prefix, &ctx->ec_xy, &ctx->ec_inf, &ctx->sg_k, &ctx->sg_flag, &ctx->sg_state, &ctx->sg_dp,
                      &ctx->ct_flags, &ctx->in0, &ctx->in3, &ctx->out0, &ctx->out1}) {
        const size_t len = b->used < b->cap ? b->used : b->cap;
        if (!b->p || !len) continue;
        host.resize(len);
        if (hipMemcpy(host.data(), b->p, len, hipMemcpyDeviceToHost) != hipSuccess) return -1;
        for (uint8_t v : host) count += v != 0;
    }
    return count;
}

// test-only (not in include/ecgpu.h): comb tables above `mb` MiB are refused as if the allocation had failed; 0 switches it off
void ecgpu_testhook_table_max_mb(size_t mb) {
    g_test_table_max_mb.store(mb);
    for (int dev = 0; dev < 64; dev++) {                          // what the hook made the registry remember goes with it
        TableRegistry& reg = table_registry(dev);
        std::lock_guard<std::mutex> lock(reg.mu);
        reg.nofit.clear();
    }
}

int ecgpu_last_timing(const ecgpu_ctx* ctx_in, const char* name, double* ms) {
    if (!ctx_in || !name || !ms) return ECGPU_ERR_ARG;
    ecgpu_ctx* ctx = const_cast<ecgpu_ctx*>(ctx_in);
    if (ctx->lane_last >= 0 && ctx->timing.empty() && ctx->spans.empty() && std::string(name) == "accumulate") {
        // the last MSM went to a lane: the duration of its accumulation kernel with whatever ran beside it
        ecgpu_ctx::MsmLane& l = ctx->lane[ctx->lane_last];
        float t = 0;
        if (!check_ctx(ctx) || !l.s || hipStreamSynchronize(l.s) != hipSuccess || hipEventElapsedTime(&t, l.ev_a, l.ev_b) != hipSuccess)
            return ECGPU_ERR_HIP;
        *ms = t;
        return ECGPU_OK;
    }
    if (!ctx->spans.empty()) {                 // asynchronous call: its events are complete once the stream has drained
        if (!check_ctx(ctx) || hipStreamSynchronize(ctx->stream) != hipSuccess) return ECGPU_ERR_HIP;
        resolve_timing(ctx);
    }
    auto it = ctx->timing.find(name);
    if (it == ctx->timing.end()) return ECGPU_ERR_ARG;
    *ms = it->second;
    return ECGPU_OK;
}

// ---- device-pointer entry points ----
// Each one is: its pointers, once, with what dev_args checks of them; its `_dev` implementation.

int ecgpu_batch_mul_base_dev(ecgpu_ctx* ctx, int curve, const void* d_scalars, size_t n, void* d_out_xy,
                             void* d_out_inf) {
    if (int rc = dev_args(ctx, __func__, n, {{d_scalars, NEED | A16}, {d_out_xy, NEED | A16}, {d_out_inf, OPT}})) return rc;
    return dispatch(curve, [&](auto c) { return mul_base_dev<decltype(c)>(ctx, d_scalars, n, d_out_xy, d_out_inf); });
}

int ecgpu_batch_mul_base_compressed_dev(ecgpu_ctx* ctx, int curve, const void* d_scalars, size_t n, void* d_out_x,
                                        void* d_out_tag) {
    if (int rc = dev_args(ctx, __func__, n, {{d_scalars, NEED | A16}, {d_out_x, NEED | A16}, {d_out_tag, NEED}})) return rc;
    return dispatch(curve, [&](auto c) { return mul_base_dev<decltype(c)>(ctx, d_scalars, n, d_out_x, d_out_tag, true); });
}

int ecgpu_batch_mul_dev(ecgpu_ctx* ctx, int curve, const void* d_scalars, const void* d_points_xy,
                        const void* d_points_inf, size_t n, void* d_out_xy, void* d_out_inf) {
    if (int rc = dev_args(ctx, __func__, n, {{d_scalars, NEED | A16}, {d_points_xy, NEED | A16}, {d_points_inf, OPT},
                                             {d_out_xy, NEED | A16}, {d_out_inf, OPT}})) return rc;
    return dispatch(curve, [&](auto c) {
        return mul_var_dev<decltype(c)>(ctx, d_scalars, d_points_xy, d_points_inf, n, d_out_xy, d_out_inf);
    });
}

int ecgpu_batch_mul_base_ct_dev(ecgpu_ctx* ctx, int curve, const void* d_scalars, size_t n, void* d_out_xy, void* d_out_inf) {
    if (int rc = dev_args(ctx, __func__, n, {{d_scalars, NEED | A16}, {d_out_xy, NEED | A16}, {d_out_inf, OPT}})) return rc;
    return dispatch(curve, [&](auto c) { return mul_base_ct_dev<decltype(c)>(ctx, d_scalars, n, d_out_xy, d_out_inf); });
}

int ecgpu_batch_mul_ct_dev(ecgpu_ctx* ctx, int curve, const void* d_scalars, const void* d_points_xy, const void* d_points_inf,
                           size_t n, void* d_out_xy, void* d_out_inf) {
    if (int rc = dev_args(ctx, __func__, n, {{d_scalars, NEED | A16}, {d_points_xy, NEED | A16}, {d_points_inf, OPT},
                                             {d_out_xy, NEED | A16}, {d_out_inf, OPT}})) return rc;
    return dispatch(curve, [&](auto c) {
        return mul_var_ct_dev<decltype(c)>(ctx, d_scalars, d_points_xy, d_points_inf, n, d_out_xy, d_out_inf);
    });
}

int ecgpu_batch_mul_ct_xyz_dev(ecgpu_ctx* ctx, int curve, const void* d_scalars, const void* d_points_xyz, size_t n, void* d_out_xy,
                               void* d_out_inf) {
    if (int rc = dev_args(ctx, __func__, n, {{d_scalars, NEED | A16}, {d_points_xyz, NEED | A16}, {d_out_xy, NEED | A16}, {d_out_inf, OPT}}))
        return rc;
    return dispatch(curve, [&](auto c) {
        return mul_var_ct_dev<decltype(c)>(ctx, d_scalars, d_points_xyz, nullptr, n, d_out_xy, d_out_inf, true);
    });
}

int ecgpu_msm_dev(ecgpu_ctx* ctx, int curve, const void* d_scalars, const void* d_points_xy, const void* d_points_inf,
                  size_t n, void* d_out_xy, void* d_out_inf) {
    if (int rc = dev_args(ctx, __func__, n, {{d_scalars, NEED | A16}, {d_points_xy, NEED | A16}, {d_points_inf, OPT},
                                             {d_out_xy, ALWAYS | A16}, {d_out_inf, OPT}})) return rc;
    return dispatch(curve, [&](auto c) {
        return msm_dev<decltype(c)>(ctx, d_scalars, d_points_xy, d_points_inf, n, d_out_xy, d_out_inf);
    });
}

int ecgpu_lincomb_ct_dev(ecgpu_ctx* ctx, int curve, const void* d_scalars, const void* d_points_xy, const void* d_points_inf,
                         size_t n, void* d_out_xy, void* d_out_inf) {
    if (int rc = dev_args(ctx, __func__, n, {{d_scalars, NEED | A16}, {d_points_xy, NEED | A16}, {d_points_inf, OPT},
                                             {d_out_xy, ALWAYS | A16}, {d_out_inf, OPT}})) return rc;
    return dispatch(curve, [&](auto c) {
        return lincomb_ct_dev<decltype(c)>(ctx, d_scalars, d_points_xy, d_points_inf, n, d_out_xy, d_out_inf);
    });
}

int ecgpu_lincomb_ct_xyz_dev(ecgpu_ctx* ctx, int curve, const void* d_scalars, const void* d_points_xyz, size_t n, void* d_out_xy,
                             void* d_out_inf) {
    if (int rc = dev_args(ctx, __func__, n, {{d_scalars, NEED | A16}, {d_points_xyz, NEED | A16}, {d_out_xy, ALWAYS | A16}, {d_out_inf, OPT}}))
        return rc;
    return dispatch(curve, [&](auto c) {
        return lincomb_ct_dev<decltype(c)>(ctx, d_scalars, d_points_xyz, nullptr, n, d_out_xy, d_out_inf, true);
    });
}

int ecgpu_batch_mul_xyz_dev(ecgpu_ctx* ctx, int curve, const void* d_scalars, const void* d_points_xyz, size_t n, void* d_out_xy,
                            void* d_out_inf) {
    if (int rc = dev_args(ctx, __func__, n, {{d_scalars, NEED | A16}, {d_points_xyz, NEED | A16}, {d_out_xy, NEED | A16}, {d_out_inf, OPT}}))
        return rc;
    return dispatch(curve, [&](auto c) { return mul_var_xyz_dev<decltype(c)>(ctx, d_scalars, d_points_xyz, n, d_out_xy, d_out_inf); });
}

int ecgpu_msm_xyz_dev(ecgpu_ctx* ctx, int curve, const void* d_scalars, const void* d_points_xyz, size_t n, void* d_out_xy,
                      void* d_out_inf) {
    if (int rc = dev_args(ctx, __func__, n, {{d_scalars, NEED | A16}, {d_points_xyz, NEED | A16}, {d_out_xy, ALWAYS | A16}, {d_out_inf, OPT}}))
        return rc;
    return dispatch(curve, [&](auto c) {
        return msm_dev<decltype(c)>(ctx, d_scalars, d_points_xyz, nullptr, n, d_out_xy, d_out_inf, true);
    });
}

int ecgpu_msm_compressed_dev(ecgpu_ctx* ctx, int curve, const void* d_scalars, const void* d_points_x, const void* d_points_tag,
                             size_t n, void* d_out_xy, void* d_out_inf) {
    if (int rc = dev_args(ctx, __func__, n, {{d_scalars, NEED | A16}, {d_points_x, NEED | A16}, {d_points_tag, NEED},
                                             {d_out_xy, ALWAYS | A16}, {d_out_inf, OPT}})) return rc;
    return dispatch(curve, [&](auto c) {
        return msm_compressed_dev<decltype(c)>(ctx, d_scalars, d_points_x, d_points_tag, n, d_out_xy, d_out_inf);
    });
}

int ecgpu_batch_mul_compressed_dev(ecgpu_ctx* ctx, int curve, const void* d_scalars, const void* d_points_x,
                                   const void* d_points_tag, size_t n, void* d_out_xy, void* d_out_inf) {
    if (int rc = dev_args(ctx, __func__, n, {{d_scalars, NEED | A16}, {d_points_x, NEED | A16}, {d_points_tag, NEED},
                                             {d_out_xy, NEED | A16}, {d_out_inf, OPT}})) return rc;
    return dispatch(curve, [&](auto c) {
        return mul_var_compressed_dev<decltype(c)>(ctx, d_scalars, d_points_x, d_points_tag, n, d_out_xy, d_out_inf);
    });
}

size_t ecgpu_msm_parts_bytes(ecgpu_ctx* ctx, int curve, size_t plan_terms) {
    if (!check_ctx(ctx)) return 0;
    size_t bytes = 0;
    (void)dispatch(curve, [&](auto c) {
        bytes = msm_parts_bytes<decltype(c)>(ctx, plan_terms);
        return (int)ECGPU_OK;
    });
    return bytes;
}

int ecgpu_msm_plan_window(ecgpu_ctx* ctx, int curve, size_t plan_terms) {
    if (!check_ctx(ctx)) return 0;
    int c = 0;
    (void)dispatch(curve, [&](auto cv) {
        c = ctx->msm_c ? ctx->msm_c : msm_choose_window<decltype(cv)>(plan_terms);
        return (int)ECGPU_OK;
    });
    return c;
}

int ecgpu_msm_parts_dev(ecgpu_ctx* ctx, int curve, const void* d_scalars, const void* d_points_xy, const void* d_points_inf,
                        size_t n, size_t plan_terms, void* d_parts) {
    if (int rc = dev_args(ctx, __func__, n, {{d_scalars, NEED | A16}, {d_points_xy, NEED | A16}, {d_points_inf, OPT}, {d_parts, ALWAYS | A16}}))
        return rc;
    return dispatch(curve, [&](auto c) {
        return msm_parts_dev<decltype(c)>(ctx, d_scalars, d_points_xy, d_points_inf, n, plan_terms, d_parts);
    });
}

int ecgpu_msm_parts_xyz_dev(ecgpu_ctx* ctx, int curve, const void* d_scalars, const void* d_points_xyz, size_t n, size_t plan_terms,
                            void* d_parts) {
    if (int rc = dev_args(ctx, __func__, n, {{d_scalars, NEED | A16}, {d_points_xyz, NEED | A16}, {d_parts, ALWAYS | A16}})) return rc;
    return dispatch(curve, [&](auto c) {
        return msm_parts_dev<decltype(c)>(ctx, d_scalars, d_points_xyz, nullptr, n, plan_terms, d_parts, true);
    });
}

int ecgpu_msm_parts_join_dev(ecgpu_ctx* ctx, const void* d_parts) {
    if (int rc = dev_args(ctx, __func__, 0, {{d_parts, ALWAYS}})) return rc;
    for (auto& l : ctx->lane)
        if (l.s && l.ev_done && l.parts_out == d_parts) {
            HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, l.ev_done, 0));
            l.parts_out = nullptr;
        }
    return ECGPU_OK;          // (written on the context's own stream, or already joined: nothing to wait for)
}

int ecgpu_msm_finish_dev(ecgpu_ctx* ctx, int curve, const void* d_parts_all, int nranks, size_t plan_terms, void* d_out_xy,
                         void* d_out_inf) {
    if (int rc = dev_args(ctx, __func__, 0, {{d_parts_all, ALWAYS | A16}, {d_out_xy, ALWAYS | A16}, {d_out_inf, OPT}},
                          nranks < 1 || nranks > 4096)) return rc;
    return dispatch(curve, [&](auto c) {
        return msm_finish_dev<decltype(c)>(ctx, d_parts_all, nranks, plan_terms, d_out_xy, d_out_inf);
    });
}

int ecgpu_batch_normalize_dev(ecgpu_ctx* ctx, int curve, const void* d_points_xyz, size_t n, void* d_out_xy,
                              void* d_out_inf) {
    if (int rc = dev_args(ctx, __func__, n, {{d_points_xyz, NEED | A16}, {d_out_xy, NEED | A16}, {d_out_inf, OPT}})) return rc;
    return dispatch(curve, [&](auto c) { return normalize_dev<decltype(c)>(ctx, d_points_xyz, n, d_out_xy, d_out_inf); });
}

int ecgpu_point_sum_dev(ecgpu_ctx* ctx, int curve, const void* d_points_xy, const void* d_points_inf, size_t n,
                        void* d_out_xy, void* d_out_inf) {
    if (int rc = dev_args(ctx, __func__, n, {{d_points_xy, NEED | A16}, {d_points_inf, OPT}, {d_out_xy, ALWAYS | A16}, {d_out_inf, OPT}}))
        return rc;
    return dispatch(curve, [&](auto c) {
        return point_sum_dev<decltype(c)>(ctx, d_points_xy, d_points_inf, n, d_out_xy, d_out_inf);
    });
}

int ecgpu_batch_mul_base_and_mul_add_dev(ecgpu_ctx* ctx, int curve, const void* d_a, const void* d_b,
                                         const void* d_points_xy, const void* d_points_inf, size_t n, void* d_out_xy,
                                         void* d_out_inf) {
    if (int rc = dev_args(ctx, __func__, n, {{d_a, NEED | A16}, {d_b, NEED | A16}, {d_points_xy, NEED | A16}, {d_points_inf, OPT},
                                             {d_out_xy, NEED | A16}, {d_out_inf, OPT}})) return rc;
    return dispatch(curve, [&](auto c) {
        return mul_add_dev<decltype(c)>(ctx, d_a, d_b, d_points_xy, d_points_inf, n, d_out_xy, d_out_inf);
    });
}

int ecgpu_batch_mul_base_and_mul_add_xyz_dev(ecgpu_ctx* ctx, int curve, const void* d_a, const void* d_b, const void* d_points_xyz,
                                             size_t n, void* d_out_xy, void* d_out_inf) {
    if (int rc = dev_args(ctx, __func__, n, {{d_a, NEED | A16}, {d_b, NEED | A16}, {d_points_xyz, NEED | A16}, {d_out_xy, NEED | A16},
                                             {d_out_inf, OPT}})) return rc;
    return dispatch(curve, [&](auto c) {
        return mul_add_xyz_dev<decltype(c)>(ctx, d_a, d_b, d_points_xyz, n, d_out_xy, d_out_inf);
    });
}

// sm2 signatures are SM2DSA (sm2/src/dsa.rs), bign's its own scheme (bignp256/src/ecdsa.rs) — not ECDSA; p192 has no
// `DigestAlgorithm` (p192/src/ecdsa.rs), so the forms that hash a message do not exist for it
inline bool not_ecdsa(int curve, bool hashes = false) {
    return curve == ECGPU_SM2 || curve == ECGPU_BIGN256 || (hashes && curve == ECGPU_P192);
}

int ecgpu_ecdsa_verify_batch_dev(ecgpu_ctx* ctx, int curve, const void* d_z, const void* d_r, const void* d_s,
                                 const void* d_q_xy, size_t n, int reject_high_s, void* d_ok) {
    // per element: u1 = z/s, u2 = r/s (mod n), R = u1 G + u2 Q (the kernels of ecgpu_batch_mul_base_and_mul_add),
    // ok = x(R) mod n == r.  See ecgpu_ecdsa.h.
    if (int rc = dev_args(ctx, __func__, n, {{d_z, NEED | A16}, {d_r, NEED | A16}, {d_s, NEED | A16}, {d_q_xy, NEED | A16}, {d_ok, NEED}},
                          false, not_ecdsa(curve))) return rc;
    return dispatch(curve, [&](auto c) {
        return ecdsa_verify_dev<decltype(c)>(ctx, d_z, d_r, d_s, d_q_xy, n, reject_high_s, d_ok);
    });
}

int ecgpu_ecdsa_verify_msg_batch_dev(ecgpu_ctx* ctx, int curve, const void* d_q_xy, const void* d_msgs, size_t msg_len,
                                     const void* d_sigs, size_t n, int reject_high_s, void* d_ok) {
    // Verifier::verify(msg, sig): the curve's digest on the device, z = bits2field(digest), then the prehash path.  See ecgpu_ecdsa.h.
    if (int rc = dev_args(ctx, __func__, n, {{d_q_xy, NEED | A16}, {d_msgs, msg_len ? NEED : OPT}, {d_sigs, NEED | A16}, {d_ok, NEED}},
                          false, not_ecdsa(curve, true))) return rc;
    return dispatch(curve, [&](auto c) {
        using C = decltype(c);
        if (n == 0) return (int)ECGPU_OK;
        const size_t L = WireBytes<C>::value;
        return hashed(ctx, {{ctx->ec_e, n * L + 16}, {ctx->ec_r, n * L + 16}, {ctx->ec_s, n * L + 16}},
                      [&] {
                          launch_ecdsa_hash_msg<C>(ctx->stream, (const uint8_t*)d_msgs, msg_len, (const uint8_t*)d_sigs, n,
                                                   (uint8_t*)ctx->ec_e.p, (uint8_t*)ctx->ec_r.p, (uint8_t*)ctx->ec_s.p);
                      },
                      [&] { return ecdsa_verify_dev<C>(ctx, ctx->ec_e.p, ctx->ec_r.p, ctx->ec_s.p, d_q_xy, n, reject_high_s, d_ok); });
    });
}

int ecgpu_ecdsa_recover_batch_dev(ecgpu_ctx* ctx, int curve, const void* d_z, const void* d_r, const void* d_s,
                                  const void* d_recid, size_t n, int reject_high_s, void* d_out_xy, void* d_ok) {
    // per element: R = decompress(r or r + n, parity), key = -(z/r) G + (s/r) R.  See ecgpu_ecdsa.h / ecgpu_verify.h.
    if (int rc = dev_args(ctx, __func__, n, {{d_z, NEED | A16}, {d_r, NEED | A16}, {d_s, NEED | A16}, {d_recid, NEED},
                                             {d_out_xy, NEED | A16}, {d_ok, NEED}}, false, not_ecdsa(curve))) return rc;
    return dispatch(curve, [&](auto c) {
        return ecdsa_recover_dev<decltype(c)>(ctx, d_z, d_r, d_s, d_recid, n, reject_high_s, d_out_xy, d_ok);
    });
}

int ecgpu_sm2dsa_verify_batch_dev(ecgpu_ctx* ctx, const void* d_e, const void* d_r, const void* d_s, const void* d_q_xy, size_t n,
                                  void* d_ok) {
    // SM2DSA on the prehash: t = r + s, (x1, y1) = s G + t Q, ok = (e + x1 mod n == r).  See ecgpu_ecdsa.h.
    if (int rc = dev_args(ctx, __func__, n, {{d_e, NEED | A16}, {d_r, NEED | A16}, {d_s, NEED | A16}, {d_q_xy, NEED | A16}, {d_ok, NEED}}))
        return rc;
    return sm2dsa_verify_dev(ctx, d_e, d_r, d_s, d_q_xy, n, d_ok);
}

int ecgpu_sm2dsa_verify_msg_batch_dev(ecgpu_ctx* ctx, const void* d_distid, size_t distid_len, const void* d_q_xy, const void* d_msgs,
                                      size_t msg_len, const void* d_sigs, size_t n, void* d_ok) {
    // VerifyingKey::new(distid, Q)?.verify(msg, sig): Z and e = SM3(Z || M) on the device, then the prehash path.  See ecgpu_ecdsa.h.
    if (int rc = dev_args(ctx, __func__, n, {{d_distid, distid_len ? NEED : OPT}, {d_q_xy, NEED | A16}, {d_msgs, msg_len ? NEED : OPT},
                                             {d_sigs, NEED | A16}, {d_ok, NEED}}, distid_len > 8191)) return rc;
    if (n == 0) return ECGPU_OK;
    return hashed(ctx, {{ctx->ec_e, n * 32}, {ctx->ec_r, n * 32}, {ctx->ec_s, n * 32}},
                  [&] {
                      launch_sm2dsa_hash_msg(ctx->stream, (const uint8_t*)d_distid, distid_len, (const uint8_t*)d_q_xy,
                                             (const uint8_t*)d_msgs, msg_len, (const uint8_t*)d_sigs, n, (uint8_t*)ctx->ec_e.p,
                                             (uint8_t*)ctx->ec_r.p, (uint8_t*)ctx->ec_s.p);
                  },
                  [&] { return sm2dsa_verify_dev(ctx, ctx->ec_e.p, ctx->ec_r.p, ctx->ec_s.p, d_q_xy, n, d_ok); });
}

int ecgpu_bign_verify_batch_dev(ecgpu_ctx* ctx, const void* d_h, const void* d_sigs, const void* d_q_xy, size_t n, void* d_ok) {
    // bign on the prehash: R = ((S1 + H) mod q) G + (S0 + 2^128) Q, ok = (S0 == belt-hash(OID || x(R) || H)[..16]).  See ecgpu_ecdsa.h.
    if (int rc = dev_args(ctx, __func__, n, {{d_h, NEED | A16}, {d_sigs, NEED | A16}, {d_q_xy, NEED | A16}, {d_ok, NEED}})) return rc;
    return bign_verify_dev(ctx, d_h, d_sigs, d_q_xy, n, d_ok);
}

int ecgpu_bign_verify_msg_batch_dev(ecgpu_ctx* ctx, const void* d_q_xy, const void* d_msgs, size_t msg_len, const void* d_sigs, size_t n,
                                    void* d_ok) {
    // VerifyingKey::verify(msg, sig): H = belt-hash(msg) on the device, then the prehash path.  See ecgpu_ecdsa.h.
    if (int rc = dev_args(ctx, __func__, n, {{d_q_xy, NEED | A16}, {d_msgs, msg_len ? NEED : OPT}, {d_sigs, NEED | A16}, {d_ok, NEED}}))
        return rc;
    if (n == 0) return ECGPU_OK;
    return hashed(ctx, {{ctx->ec_e, n * 32}},
                  [&] { launch_bign_hash_msg(ctx->stream, (const uint8_t*)d_msgs, msg_len, n, (uint8_t*)ctx->ec_e.p); },
                  [&] { return bign_verify_dev(ctx, ctx->ec_e.p, d_sigs, d_q_xy, n, d_ok); });
}

int ecgpu_schnorr_verify_batch_dev(ecgpu_ctx* ctx, const void* d_e, const void* d_r, const void* d_s, const void* d_p_xy,
                                   size_t n, void* d_ok) {
    // BIP340 over secp256k1: R = s G - e P, ok = R finite, y(R) even, x(R) == r.  See ecgpu_ecdsa.h.
    if (int rc = dev_args(ctx, __func__, n, {{d_e, NEED | A16}, {d_r, NEED | A16}, {d_s, NEED | A16}, {d_p_xy, NEED | A16}, {d_ok, NEED}}))
        return rc;
    return schnorr_verify_dev(ctx, d_e, d_r, d_s, d_p_xy, n, d_ok);
}

int ecgpu_schnorr_verify_raw_batch_dev(ecgpu_ctx* ctx, const void* d_pk_x, const void* d_msgs, size_t msg_len, const void* d_sigs,
                                       size_t n, void* d_ok) {
    // VerifyingKey::from_bytes(pk)?.verify_raw(msg, sig) from wire bytes: lift_x, challenge hash, s G - e P.  See ecgpu_ecdsa.h.
    if (int rc = dev_args(ctx, __func__, n, {{d_pk_x, NEED | A16}, {d_msgs, msg_len ? NEED : OPT}, {d_sigs, NEED | A16}, {d_ok, NEED}}))
        return rc;
    return schnorr_verify_raw_dev(ctx, d_pk_x, d_msgs, msg_len, d_sigs, n, d_ok);
}

// ---- signing (ecgpu_sign.h): the entry points around ecdsa_sign_dev and schnorr_sign_dev ----
// every argument is checked before anything is queued.  from_msg: d_z is the message array (NULL allowed when msg_len == 0); a
// nonce array is alignment-checked whenever there is one
static int ecdsa_sign_entry(ecgpu_ctx* ctx, const char* fn, int curve, bool rfc6979, const void* d_d, const void* d_k, const void* d_z,
                            size_t n, int normalize_s, void* d_sig, void* d_recid, void* d_ok, bool from_msg = false, size_t msg_len = 0) {
    if (int rc = dev_args(ctx, fn, n, {{d_d, NEED | A16}, {d_k, (rfc6979 ? OPT : NEED) | A16}, {d_z, from_msg ? (msg_len ? NEED : OPT) : NEED | A16},
                                       {d_sig, NEED | A16}, {d_recid, NEED}, {d_ok, NEED}}, false, not_ecdsa(curve, rfc6979))) return rc;
    const int rc = dispatch(curve, [&](auto c) {
        return ecdsa_sign_dev<decltype(c)>(ctx, d_d, rfc6979 ? nullptr : d_k, d_z, n, normalize_s, d_sig, d_recid, d_ok, from_msg, msg_len);
    });
    return rc == ECGPU_ERR_CURVE ? curve_error(ctx, fn) : rc;
}

int ecgpu_ecdsa_sign_batch_dev(ecgpu_ctx* ctx, int curve, const void* d_d, const void* d_k, const void* d_z, size_t n, int normalize_s,
                               void* d_out_sig, void* d_out_recid, void* d_ok) {
    // `hazmat::sign_prehashed` with the caller's nonce: R = k G, r = x(R) mod n, s = (z + r d) / k.  See ecgpu_sign.h.
    return ecdsa_sign_entry(ctx, __func__, curve, false, d_d, d_k, d_z, n, normalize_s, d_out_sig, d_out_recid, d_ok);
}

int ecgpu_ecdsa_sign_rfc6979_batch_dev(ecgpu_ctx* ctx, int curve, const void* d_d, const void* d_z, size_t n, int normalize_s,
                                       void* d_out_sig, void* d_out_recid, void* d_ok) {
    // `PrehashSigner::sign_prehash`: the nonce of RFC 6979 section 3.2 from the device's HMAC-DRBG.  See ecgpu_sign.h.
    return ecdsa_sign_entry(ctx, __func__, curve, true, d_d, nullptr, d_z, n, normalize_s, d_out_sig, d_out_recid, d_ok);
}

int ecgpu_ecdsa_sign_msg_batch_dev(ecgpu_ctx* ctx, int curve, const void* d_d, const void* d_msgs, size_t msg_len, size_t n,
                                   int normalize_s, void* d_out_sig, void* d_out_recid, void* d_ok) {
    // `Signer::sign(msg)`: the curve's digest on the device, z = bits2field(digest), then the RFC 6979 form.  See ecgpu_sign.h.
    return ecdsa_sign_entry(ctx, __func__, curve, true, d_d, nullptr, d_msgs, n, normalize_s, d_out_sig, d_out_recid, d_ok, true, msg_len);
}

int ecgpu_schnorr_sign_raw_batch_dev(ecgpu_ctx* ctx, const void* d_sk, const void* d_msgs, size_t msg_len, const void* d_aux_rand,
                                     size_t n, void* d_out_sig, void* d_ok) {
    // `SigningKey::sign_raw(msg, aux_rand)` with the key fix-up: P = d G, the nonce hashes, R = k G, s = k + e d.  See ecgpu_sign.h.
    if (int rc = dev_args(ctx, __func__, n, {{d_sk, NEED | A16}, {d_msgs, msg_len ? NEED : OPT}, {d_aux_rand, NEED | A16}, {d_out_sig, NEED | A16},
                                             {d_ok, NEED}})) return rc;
    return schnorr_sign_dev(ctx, d_sk, d_msgs, msg_len, d_aux_rand, n, d_out_sig, d_ok);
}

static int ecdh_dev(ecgpu_ctx* ctx, int curve, const void* d_scalars, const void* d_points_xy, size_t n, void* d_out_x, void* d_ok,
                    bool ct) {
    // SharedSecret_i = x(k_i * P_i): the variable-base kernel (ct: its uniform-schedule form), normalisation into scratch,
    // x extraction.  (The inputs are checked by the batch multiplication's own entry point below.)
    int rc;
    if ((rc = dev_args(ctx, __func__, n, {{d_out_x, NEED | A16}, {d_ok, NEED}}, false, !ecgpu_field_bytes(curve))) != ECGPU_OK) return rc;
    const size_t L = ecgpu_field_bytes(curve);
    CtWipe wipe(ctx, ct ? WIPE_EC : 0);             // (declared first: runs after the x extraction below has been queued)
    if ((rc = ensure(ctx, ctx->ec_xy, n * 2 * L + 16)) != ECGPU_OK) return rc;
    if ((rc = ensure(ctx, ctx->ec_inf, n + 16)) != ECGPU_OK) return rc;
    rc = ct ? ecgpu_batch_mul_ct_dev(ctx, curve, d_scalars, d_points_xy, nullptr, n, ctx->ec_xy.p, ctx->ec_inf.p)
            : ecgpu_batch_mul_dev(ctx, curve, d_scalars, d_points_xy, nullptr, n, ctx->ec_xy.p, ctx->ec_inf.p);
    if (rc != ECGPU_OK) return rc;
    if (n == 0) return ECGPU_OK;
    return dispatch(curve, [&](auto c) -> int {
        using C = decltype(c);
        launch_extract_x<C>(ctx->stream, (const uint8_t*)ctx->ec_xy.p, (const uint8_t*)ctx->ec_inf.p, n, (uint8_t*)d_out_x,
                            (uint8_t*)d_ok);
        HIP_TRY(ctx, hipGetLastError());
        if (!ctx->async) HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        return (int)ECGPU_OK;
    });
}
int ecgpu_batch_ecdh_dev(ecgpu_ctx* ctx, int curve, const void* d_scalars, const void* d_points_xy, size_t n, void* d_out_x,
                         void* d_ok) {
    return ecdh_dev(ctx, curve, d_scalars, d_points_xy, n, d_out_x, d_ok, false);
}
int ecgpu_batch_ecdh_ct_dev(ecgpu_ctx* ctx, int curve, const void* d_scalars, const void* d_points_xy, size_t n, void* d_out_x,
                            void* d_ok) {
    return ecdh_dev(ctx, curve, d_scalars, d_points_xy, n, d_out_x, d_ok, true);
}

int ecgpu_batch_decompress_dev(ecgpu_ctx* ctx, int curve, const void* d_xs, const void* d_y_is_odd, size_t n, void* d_out_xy,
                               void* d_ok) {
    if (int rc = dev_args(ctx, __func__, n, {{d_xs, NEED | A16}, {d_y_is_odd, NEED}, {d_out_xy, NEED | A16}, {d_ok, NEED}})) return rc;
    return dispatch(curve, [&](auto c) {
        using C = decltype(c);
        if (n == 0) return (int)ECGPU_OK;
        DevCall call(ctx, 0, {});
        if (call.rc != ECGPU_OK) return call.rc;
        call.mark(0);
        launch_decompress<C>(ctx->stream, (const uint8_t*)d_xs, (const uint8_t*)d_y_is_odd, n, (uint8_t*)d_out_xy, (uint8_t*)d_ok);
        call.mark(1);
        return call.done(SPANS_NO_NORMALIZE);
    });
}

// ---- host-pointer entry points ----
// Each one is: the preamble with its own NULL-argument condition (HostCall), the list of its arrays, its `_dev` call (staged).

// (ct: the uniform-schedule form; the host-side plumbing is the same, its scalars and results are marked for the wipe)
static int batch_mul_base_host(ecgpu_ctx* ctx, int curve, const uint8_t* scalars, size_t n, uint8_t* out_xy, uint8_t* out_inf,
                               bool ct, const char* fn) {
    HostCall h(ctx, fn, curve);
    if (h.bad(n && (!scalars || !out_xy))) return h.rc;
    const auto dev = ct ? ecgpu_batch_mul_base_ct_dev : ecgpu_batch_mul_base_dev;
    return staged(ctx, n, {{scalars, &ctx->in0, h.L, ct}}, {{out_xy, &ctx->out0, 2 * h.L, ct}, {out_inf, &ctx->out1, 1, ct}},
                  [&](auto in, auto out, size_t m) { return dev(ctx, curve, in[0], m, out[0], out[1]); });
}

int ecgpu_batch_mul_base(ecgpu_ctx* ctx, int curve, const uint8_t* scalars, size_t n, uint8_t* out_xy, uint8_t* out_inf) {
    return batch_mul_base_host(ctx, curve, scalars, n, out_xy, out_inf, false, __func__);
}
int ecgpu_batch_mul_base_ct(ecgpu_ctx* ctx, int curve, const uint8_t* scalars, size_t n, uint8_t* out_xy, uint8_t* out_inf) {
    return batch_mul_base_host(ctx, curve, scalars, n, out_xy, out_inf, true, __func__);
}

int ecgpu_batch_mul_base_compressed(ecgpu_ctx* ctx, int curve, const uint8_t* scalars, size_t n, uint8_t* out_x,
                                    uint8_t* out_tag) {
    HostCall h(ctx, __func__, curve);
    if (h.bad(n && (!scalars || !out_x || !out_tag))) return h.rc;
    return staged(ctx, n, {{scalars, &ctx->in0, h.L}}, {{out_x, &ctx->out0, h.L}, {out_tag, &ctx->out1, 1}},
                  [&](auto in, auto out, size_t m) { return ecgpu_batch_mul_base_compressed_dev(ctx, curve, in[0], m, out[0], out[1]); });
}

// the host-pointer batch multiplication over either point record: affine x || y (+ optional identity flags) for
// ecgpu_batch_mul[_ct], projective X || Y || Z (3L bytes, no flags) for ecgpu_batch_mul[_ct]_xyz
static int batch_mul_host(ecgpu_ctx* ctx, int curve, const uint8_t* scalars, const uint8_t* points, const uint8_t* points_inf,
                          size_t n, uint8_t* out_xy, uint8_t* out_inf, bool ct, bool xyz, const char* fn) {
    HostCall h(ctx, fn, curve);
    if (h.bad(n && (!scalars || !points || !out_xy))) return h.rc;
    const size_t PB = (xyz ? 3 : 2) * h.L;           // bytes per point record
    return staged(ctx, n, {{scalars, &ctx->in0, h.L, ct}, {points, &ctx->in1, PB}, {points_inf, &ctx->in2, 1}},
                  {{out_xy, &ctx->out0, 2 * h.L, ct}, {out_inf, &ctx->out1, 1, ct}}, [&](auto in, auto out, size_t m) {
                      if (xyz) return (ct ? ecgpu_batch_mul_ct_xyz_dev : ecgpu_batch_mul_xyz_dev)(ctx, curve, in[0], in[1], m, out[0], out[1]);
                      return (ct ? ecgpu_batch_mul_ct_dev : ecgpu_batch_mul_dev)(ctx, curve, in[0], in[1], in[2], m, out[0], out[1]);
                  });
}

int ecgpu_batch_mul(ecgpu_ctx* ctx, int curve, const uint8_t* scalars, const uint8_t* points_xy, const uint8_t* points_inf, size_t n,
                    uint8_t* out_xy, uint8_t* out_inf) {
    return batch_mul_host(ctx, curve, scalars, points_xy, points_inf, n, out_xy, out_inf, false, false, __func__);
}
int ecgpu_batch_mul_ct(ecgpu_ctx* ctx, int curve, const uint8_t* scalars, const uint8_t* points_xy, const uint8_t* points_inf, size_t n,
                       uint8_t* out_xy, uint8_t* out_inf) {
    return batch_mul_host(ctx, curve, scalars, points_xy, points_inf, n, out_xy, out_inf, true, false, __func__);
}

int ecgpu_batch_mul_ct_xyz(ecgpu_ctx* ctx, int curve, const uint8_t* scalars, const uint8_t* points_xyz, size_t n, uint8_t* out_xy,
                           uint8_t* out_inf) {
    return batch_mul_host(ctx, curve, scalars, points_xyz, nullptr, n, out_xy, out_inf, true, true, __func__);
}
int ecgpu_batch_mul_xyz(ecgpu_ctx* ctx, int curve, const uint8_t* scalars, const uint8_t* points_xyz, size_t n, uint8_t* out_xy,
                        uint8_t* out_inf) {
    return batch_mul_host(ctx, curve, scalars, points_xyz, nullptr, n, out_xy, out_inf, false, true, __func__);
}

// the host-pointer MSM over either point record: affine x || y (+ optional identity flags) for ecgpu_msm, projective
// X || Y || Z (3L bytes, no flags) for ecgpu_msm_xyz
static int msm_host(ecgpu_ctx* ctx, int curve, const uint8_t* scalars, const uint8_t* points_xy, const uint8_t* points_inf,
                    size_t n, uint8_t* out_xy, uint8_t* out_inf, bool xyz, const char* fn) {
    HostCall h(ctx, fn, curve);
    if (h.bad(!out_xy || (n && (!scalars || !points_xy)))) return h.rc;
    const size_t PB = (xyz ? 3 : 2) * h.L;           // bytes per point record
    return msm_staged(ctx, curve, n, {{scalars, &ctx->in0, h.L}, {points_xy, &ctx->in1, PB}, {points_inf, &ctx->in2, 1}}, out_xy, out_inf,
                      [&](auto c, auto in, size_t m, void* d_out_xy, void* d_out_inf) {
                          return msm_dev<decltype(c)>(ctx, in[0], in[1], in[2], m, d_out_xy, d_out_inf, xyz);
                      });
}

int ecgpu_msm(ecgpu_ctx* ctx, int curve, const uint8_t* scalars, const uint8_t* points_xy, const uint8_t* points_inf,
              size_t n, uint8_t* out_xy, uint8_t* out_inf) {
    return msm_host(ctx, curve, scalars, points_xy, points_inf, n, out_xy, out_inf, false, __func__);
}
int ecgpu_msm_xyz(ecgpu_ctx* ctx, int curve, const uint8_t* scalars, const uint8_t* points_xyz, size_t n, uint8_t* out_xy,
                  uint8_t* out_inf) {
    return msm_host(ctx, curve, scalars, points_xyz, nullptr, n, out_xy, out_inf, true, __func__);
}

int ecgpu_lincomb_ct(ecgpu_ctx* ctx, int curve, const uint8_t* scalars, const uint8_t* points_xy, const uint8_t* points_inf, size_t n,
                     uint8_t* out_xy, uint8_t* out_inf) {
    HostCall h(ctx, __func__, curve);
    if (h.bad(!out_xy || (n && (!scalars || !points_xy)))) return h.rc;
    return staged(ctx, n, {{scalars, &ctx->in0, h.L, SECRET}, {points_xy, &ctx->in1, 2 * h.L}, {points_inf, &ctx->in2, 1}},
                  {{out_xy, &ctx->out0, 2 * h.L, SECRET}, {out_inf, &ctx->out1, 1, SECRET}}, [&](auto in, auto out, size_t m) {
                      return ecgpu_lincomb_ct_dev(ctx, curve, in[0], in[1], in[2], m, out[0], out[1]);
                  }, STAGE_REDUCE);
}

int ecgpu_lincomb_ct_xyz(ecgpu_ctx* ctx, int curve, const uint8_t* scalars, const uint8_t* points_xyz, size_t n, uint8_t* out_xy,
                         uint8_t* out_inf) {
    HostCall h(ctx, __func__, curve);
    if (h.bad(!out_xy || (n && (!scalars || !points_xyz)))) return h.rc;
    return staged(ctx, n, {{scalars, &ctx->in0, h.L, SECRET}, {points_xyz, &ctx->in1, 3 * h.L}},
                  {{out_xy, &ctx->out0, 2 * h.L, SECRET}, {out_inf, &ctx->out1, 1, SECRET}}, [&](auto in, auto out, size_t m) {
                      return ecgpu_lincomb_ct_xyz_dev(ctx, curve, in[0], in[1], m, out[0], out[1]);
                  }, STAGE_REDUCE);
}

int ecgpu_msm_compressed(ecgpu_ctx* ctx, int curve, const uint8_t* scalars, const uint8_t* points_x, const uint8_t* points_tag,
                         size_t n, uint8_t* out_xy, uint8_t* out_inf) {
    HostCall h(ctx, __func__, curve);
    if (h.bad(!out_xy || (n && (!scalars || !points_x || !points_tag)))) return h.rc;
    return msm_staged(ctx, curve, n, {{scalars, &ctx->in0, h.L}, {points_x, &ctx->in1, h.L}, {points_tag, &ctx->in2, 1}}, out_xy, out_inf,
                      [&](auto c, auto in, size_t m, void* d_out_xy, void* d_out_inf) {
                          return msm_compressed_dev<decltype(c)>(ctx, in[0], in[1], in[2], m, d_out_xy, d_out_inf);
                      });
}

int ecgpu_batch_mul_compressed(ecgpu_ctx* ctx, int curve, const uint8_t* scalars, const uint8_t* points_x, const uint8_t* points_tag,
                               size_t n, uint8_t* out_xy, uint8_t* out_inf) {
    HostCall h(ctx, __func__, curve);
    if (h.bad(n && (!scalars || !points_x || !points_tag || !out_xy))) return h.rc;
    return staged(ctx, n, {{scalars, &ctx->in0, h.L}, {points_x, &ctx->in1, h.L}, {points_tag, &ctx->in2, 1}},
                  {{out_xy, &ctx->out0, 2 * h.L}, {out_inf, &ctx->out1, 1}}, [&](auto in, auto out, size_t m) {
                      return ecgpu_batch_mul_compressed_dev(ctx, curve, in[0], in[1], in[2], m, out[0], out[1]);
                  });
}

// the host-pointer aG + bP batch over either point record: affine x || y (+ optional identity flags) for
// ecgpu_batch_mul_base_and_mul_add, projective X || Y || Z (3L bytes, no flags) for its _xyz form
static int mul_add_host(ecgpu_ctx* ctx, int curve, const uint8_t* a_scalars, const uint8_t* b_scalars, const uint8_t* points_xy,
                        const uint8_t* points_inf, size_t n, uint8_t* out_xy, uint8_t* out_inf, bool xyz, const char* fn) {
    HostCall h(ctx, fn, curve);
    if (h.bad(n && (!a_scalars || !b_scalars || !points_xy || !out_xy))) return h.rc;
    const size_t PB = (xyz ? 3 : 2) * h.L;           // bytes per point record
    return staged(ctx, n, {{a_scalars, &ctx->in0, h.L}, {b_scalars, &ctx->in3, h.L}, {points_xy, &ctx->in1, PB}, {points_inf, &ctx->in2, 1}},
                  {{out_xy, &ctx->out0, 2 * h.L}, {out_inf, &ctx->out1, 1}}, [&](auto in, auto out, size_t m) {
                      if (xyz) return ecgpu_batch_mul_base_and_mul_add_xyz_dev(ctx, curve, in[0], in[1], in[2], m, out[0], out[1]);
                      return ecgpu_batch_mul_base_and_mul_add_dev(ctx, curve, in[0], in[1], in[2], in[3], m, out[0], out[1]);
                  });
}

int ecgpu_batch_mul_base_and_mul_add(ecgpu_ctx* ctx, int curve, const uint8_t* a_scalars, const uint8_t* b_scalars,
                                     const uint8_t* points_xy, const uint8_t* points_inf, size_t n, uint8_t* out_xy,
                                     uint8_t* out_inf) {
    return mul_add_host(ctx, curve, a_scalars, b_scalars, points_xy, points_inf, n, out_xy, out_inf, false, __func__);
}
int ecgpu_batch_mul_base_and_mul_add_xyz(ecgpu_ctx* ctx, int curve, const uint8_t* a_scalars, const uint8_t* b_scalars,
                                         const uint8_t* points_xyz, size_t n, uint8_t* out_xy, uint8_t* out_inf) {
    return mul_add_host(ctx, curve, a_scalars, b_scalars, points_xyz, nullptr, n, out_xy, out_inf, true, __func__);
}

int ecgpu_ecdsa_verify_batch(ecgpu_ctx* ctx, int curve, const uint8_t* z, const uint8_t* r, const uint8_t* s,
                             const uint8_t* q_xy, size_t n, int reject_high_s, uint8_t* ok) {
    HostCall h(ctx, __func__, curve);
    if (h.bad(n && (!z || !r || !s || !q_xy || !ok))) return h.rc;
    return staged(ctx, n, {{z, &ctx->in0, h.L}, {r, &ctx->in3, h.L}, {s, &ctx->in2, h.L}, {q_xy, &ctx->in1, 2 * h.L}}, {{ok, &ctx->out1, 1}},
                  [&](auto in, auto out, size_t m) {
                      return ecgpu_ecdsa_verify_batch_dev(ctx, curve, in[0], in[1], in[2], in[3], m, reject_high_s, out[0]);
                  });
}

// (the message-level verifiers: with msg_len == 0 there is no message array, and the device entry receives nullptr for it)
int ecgpu_ecdsa_verify_msg_batch(ecgpu_ctx* ctx, int curve, const uint8_t* q_xy, const uint8_t* msgs, size_t msg_len, const uint8_t* sigs,
                                 size_t n, int reject_high_s, uint8_t* ok) {
    HostCall h(ctx, __func__, curve);
    if (h.bad(n && (!q_xy || !sigs || !ok || (msg_len && !msgs)))) return h.rc;
    return staged(ctx, n, {{q_xy, &ctx->in1, 2 * h.L}, {msg_len ? msgs : nullptr, &ctx->in0, msg_len}, {sigs, &ctx->in3, 2 * h.L}},
                  {{ok, &ctx->out1, 1}}, [&](auto in, auto out, size_t m) {
                      return ecgpu_ecdsa_verify_msg_batch_dev(ctx, curve, in[0], in[1], msg_len, in[2], m, reject_high_s, out[0]);
                  });
}

int ecgpu_ecdsa_recover_batch(ecgpu_ctx* ctx, int curve, const uint8_t* z, const uint8_t* r, const uint8_t* s,
                              const uint8_t* recid, size_t n, int reject_high_s, uint8_t* out_xy, uint8_t* ok) {
    HostCall h(ctx, __func__, curve);
    if (h.bad(n && (!z || !r || !s || !recid || !out_xy || !ok))) return h.rc;
    return staged(ctx, n, {{z, &ctx->in0, h.L}, {r, &ctx->in3, h.L}, {s, &ctx->in1, h.L}, {recid, &ctx->in2, 1}},
                  {{out_xy, &ctx->out0, 2 * h.L}, {ok, &ctx->out1, 1}}, [&](auto in, auto out, size_t m) {
                      return ecgpu_ecdsa_recover_batch_dev(ctx, curve, in[0], in[1], in[2], in[3], m, reject_high_s, out[0], out[1]);
                  });
}

int ecgpu_sm2dsa_verify_batch(ecgpu_ctx* ctx, const uint8_t* e, const uint8_t* r, const uint8_t* s, const uint8_t* q_xy, size_t n,
                              uint8_t* ok) {
    HostCall h(ctx, __func__, ECGPU_SM2);
    if (h.bad(n && (!e || !r || !s || !q_xy || !ok))) return h.rc;
    return staged(ctx, n, {{e, &ctx->in0, h.L}, {r, &ctx->in3, h.L}, {s, &ctx->in2, h.L}, {q_xy, &ctx->in1, 2 * h.L}}, {{ok, &ctx->out1, 1}},
                  [&](auto in, auto out, size_t m) { return ecgpu_sm2dsa_verify_batch_dev(ctx, in[0], in[1], in[2], in[3], m, out[0]); });
}

int ecgpu_sm2dsa_verify_msg_batch(ecgpu_ctx* ctx, const uint8_t* distid, size_t distid_len, const uint8_t* q_xy, const uint8_t* msgs,
                                  size_t msg_len, const uint8_t* sigs, size_t n, uint8_t* ok) {
    HostCall h(ctx, __func__, ECGPU_SM2);
    if (h.bad(distid_len > 8191 || (distid_len && !distid) || (n && (!q_xy || !sigs || !ok || (msg_len && !msgs))))) return h.rc;
    int rc = upload(ctx, ctx->ec_id, distid, distid_len);          // one identifier for the whole batch: not an array of the list
    if (rc != ECGPU_OK) return rc;
    return staged(ctx, n, {{q_xy, &ctx->in1, 64}, {msg_len ? msgs : nullptr, &ctx->in0, msg_len}, {sigs, &ctx->in3, 64}},
                  {{ok, &ctx->out1, 1}}, [&](auto in, auto out, size_t m) {
                      return ecgpu_sm2dsa_verify_msg_batch_dev(ctx, ctx->ec_id.p, distid_len, in[0], in[1], msg_len, in[2], m, out[0]);
                  });
}

int ecgpu_bign_verify_batch(ecgpu_ctx* ctx, const uint8_t* h, const uint8_t* sigs, const uint8_t* q_xy, size_t n, uint8_t* ok) {
    HostCall call(ctx, __func__, ECGPU_BIGN256);
    if (call.bad(n && (!h || !sigs || !q_xy || !ok))) return call.rc;
    return staged(ctx, n, {{h, &ctx->in0, 32}, {sigs, &ctx->in3, 48}, {q_xy, &ctx->in1, 64}}, {{ok, &ctx->out1, 1}},
                  [&](auto in, auto out, size_t m) { return ecgpu_bign_verify_batch_dev(ctx, in[0], in[1], in[2], m, out[0]); });
}

int ecgpu_bign_verify_msg_batch(ecgpu_ctx* ctx, const uint8_t* q_xy, const uint8_t* msgs, size_t msg_len, const uint8_t* sigs, size_t n,
                                uint8_t* ok) {
    HostCall h(ctx, __func__, ECGPU_BIGN256);
    if (h.bad(n && (!q_xy || !sigs || !ok || (msg_len && !msgs)))) return h.rc;
    return staged(ctx, n, {{q_xy, &ctx->in1, 64}, {msg_len ? msgs : nullptr, &ctx->in0, msg_len}, {sigs, &ctx->in3, 48}},
                  {{ok, &ctx->out1, 1}}, [&](auto in, auto out, size_t m) {
                      return ecgpu_bign_verify_msg_batch_dev(ctx, in[0], in[1], msg_len, in[2], m, out[0]);
                  });
}

int ecgpu_schnorr_verify_batch(ecgpu_ctx* ctx, const uint8_t* e, const uint8_t* r, const uint8_t* s, const uint8_t* p_xy,
                               size_t n, uint8_t* ok) {
    HostCall h(ctx, __func__, ECGPU_K256);
    if (h.bad(n && (!e || !r || !s || !p_xy || !ok))) return h.rc;
    return staged(ctx, n, {{e, &ctx->in0, h.L}, {r, &ctx->in3, h.L}, {s, &ctx->in2, h.L}, {p_xy, &ctx->in1, 2 * h.L}}, {{ok, &ctx->out1, 1}},
                  [&](auto in, auto out, size_t m) { return ecgpu_schnorr_verify_batch_dev(ctx, in[0], in[1], in[2], in[3], m, out[0]); });
}

int ecgpu_schnorr_verify_raw_batch(ecgpu_ctx* ctx, const uint8_t* pk_x, const uint8_t* msgs, size_t msg_len, const uint8_t* sigs,
                                   size_t n, uint8_t* ok) {
    HostCall h(ctx, __func__, ECGPU_K256);
    if (h.bad(n && (!pk_x || !sigs || !ok || (msg_len && !msgs)))) return h.rc;
    return staged(ctx, n, {{pk_x, &ctx->in0, 32}, {msg_len ? msgs : nullptr, &ctx->in1, msg_len}, {sigs, &ctx->in3, 64}},
                  {{ok, &ctx->out1, 1}}, [&](auto in, auto out, size_t m) {
                      return ecgpu_schnorr_verify_raw_batch_dev(ctx, in[0], in[1], msg_len, in[2], m, out[0]);
                  });
}

// ---- signing: keys, nonces and aux_rand are staged as secrets (zeroed behind the call); signatures are public ----
int ecgpu_ecdsa_sign_batch(ecgpu_ctx* ctx, int curve, const uint8_t* d, const uint8_t* k, const uint8_t* z, size_t n, int normalize_s,
                           uint8_t* out_sig, uint8_t* out_recid, uint8_t* ok) {
    HostCall h(ctx, __func__, curve);
    if (h.bad(n && (!d || !k || !z || !out_sig || !out_recid || !ok))) return h.rc;
    return staged(ctx, n, {{d, &ctx->in0, h.L, SECRET}, {k, &ctx->in3, h.L, SECRET}, {z, &ctx->in2, h.L}},
                  {{out_sig, &ctx->out0, 2 * h.L}, {out_recid, &ctx->out2, 1}, {ok, &ctx->out1, 1}}, [&](auto in, auto out, size_t m) {
                      return ecgpu_ecdsa_sign_batch_dev(ctx, curve, in[0], in[1], in[2], m, normalize_s, out[0], out[1], out[2]);
                  });
}

int ecgpu_ecdsa_sign_rfc6979_batch(ecgpu_ctx* ctx, int curve, const uint8_t* d, const uint8_t* z, size_t n, int normalize_s,
                                   uint8_t* out_sig, uint8_t* out_recid, uint8_t* ok) {
    HostCall h(ctx, __func__, curve);
    if (h.bad(n && (!d || !z || !out_sig || !out_recid || !ok))) return h.rc;
    return staged(ctx, n, {{d, &ctx->in0, h.L, SECRET}, {z, &ctx->in2, h.L}},
                  {{out_sig, &ctx->out0, 2 * h.L}, {out_recid, &ctx->out2, 1}, {ok, &ctx->out1, 1}}, [&](auto in, auto out, size_t m) {
                      return ecgpu_ecdsa_sign_rfc6979_batch_dev(ctx, curve, in[0], in[1], m, normalize_s, out[0], out[1], out[2]);
                  });
}

int ecgpu_ecdsa_sign_msg_batch(ecgpu_ctx* ctx, int curve, const uint8_t* d, const uint8_t* msgs, size_t msg_len, size_t n, int normalize_s,
                               uint8_t* out_sig, uint8_t* out_recid, uint8_t* ok) {
    HostCall h(ctx, __func__, curve);
    if (h.bad(n && (!d || !out_sig || !out_recid || !ok || (msg_len && !msgs)))) return h.rc;
    return staged(ctx, n, {{d, &ctx->in0, h.L, SECRET}, {msg_len ? msgs : nullptr, &ctx->in1, msg_len}},
                  {{out_sig, &ctx->out0, 2 * h.L}, {out_recid, &ctx->out2, 1}, {ok, &ctx->out1, 1}}, [&](auto in, auto out, size_t m) {
                      return ecgpu_ecdsa_sign_msg_batch_dev(ctx, curve, in[0], in[1], msg_len, m, normalize_s, out[0], out[1], out[2]);
                  });
}

int ecgpu_schnorr_sign_raw_batch(ecgpu_ctx* ctx, const uint8_t* sk, const uint8_t* msgs, size_t msg_len, const uint8_t* aux_rand, size_t n,
                                 uint8_t* out_sig, uint8_t* ok) {
    HostCall h(ctx, __func__, ECGPU_K256);
    if (h.bad(n && (!sk || !aux_rand || !out_sig || !ok || (msg_len && !msgs)))) return h.rc;
    return staged(ctx, n, {{sk, &ctx->in0, 32, SECRET}, {msg_len ? msgs : nullptr, &ctx->in1, msg_len}, {aux_rand, &ctx->in3, 32, SECRET}},
                  {{out_sig, &ctx->out0, 64}, {ok, &ctx->out1, 1}}, [&](auto in, auto out, size_t m) {
                      return ecgpu_schnorr_sign_raw_batch_dev(ctx, in[0], in[1], msg_len, in[2], m, out[0], out[1]);
                  });
}

// ---- SM2DSA signing: keys and nonces are staged as secrets; prehashes, messages and signatures are public ----
// (host-pointer forms only, like the SM2 encryption calls: sm2dsa_sign_dev is internal, every chunk reaches it through `staged`)
int ecgpu_sm2dsa_sign_batch(ecgpu_ctx* ctx, const uint8_t* d, const uint8_t* k, const uint8_t* e, size_t n, uint8_t* out_sig, uint8_t* ok) {
    HostCall h(ctx, __func__, ECGPU_SM2);
    if (h.bad(n && (!d || !k || !e || !out_sig || !ok))) return h.rc;
    return staged(ctx, n, {{d, &ctx->in0, 32, SECRET}, {k, &ctx->in3, 32, SECRET}, {e, &ctx->in2, 32}},
                  {{out_sig, &ctx->out0, 64}, {ok, &ctx->out1, 1}}, [&](auto in, auto out, size_t m) {
                      return sm2dsa_sign_dev(ctx, in[0], in[1], in[2], m, out[0], out[1]);
                  });
}

int ecgpu_sm2dsa_sign_rfc6979_batch(ecgpu_ctx* ctx, const uint8_t* d, const uint8_t* e, size_t n, uint8_t* out_sig, uint8_t* ok) {
    HostCall h(ctx, __func__, ECGPU_SM2);
    if (h.bad(n && (!d || !e || !out_sig || !ok))) return h.rc;
    return staged(ctx, n, {{d, &ctx->in0, 32, SECRET}, {e, &ctx->in2, 32}}, {{out_sig, &ctx->out0, 64}, {ok, &ctx->out1, 1}},
                  [&](auto in, auto out, size_t m) { return sm2dsa_sign_dev(ctx, in[0], nullptr, in[1], m, out[0], out[1]); });
}

int ecgpu_sm2dsa_sign_msg_batch(ecgpu_ctx* ctx, const uint8_t* distid, size_t distid_len, const uint8_t* d, const uint8_t* msgs,
                                size_t msg_len, size_t n, uint8_t* out_sig, uint8_t* ok) {
    HostCall h(ctx, __func__, ECGPU_SM2);
    if (h.bad(distid_len > 8191 || (distid_len && !distid) || (n && (!d || !out_sig || !ok || (msg_len && !msgs))))) return h.rc;
    int rc = upload(ctx, ctx->ec_id, distid, distid_len);          // one identifier for the whole batch: not an array of the list
    if (rc != ECGPU_OK) return rc;
    return staged(ctx, n, {{d, &ctx->in0, 32, SECRET}, {msg_len ? msgs : nullptr, &ctx->in1, msg_len}},
                  {{out_sig, &ctx->out0, 64}, {ok, &ctx->out1, 1}}, [&](auto in, auto out, size_t m) {
                      return sm2dsa_sign_dev(ctx, in[0], nullptr, in[1], m, out[0], out[1], true, ctx->ec_id.p, distid_len, msg_len);
                  });
}

// ---- bign signing: keys and nonces are staged as secrets; prehashes, messages and signatures are public ----
// (host-pointer forms only, like the SM2DSA calls: bign_sign_dev is internal, every chunk reaches it through `staged`)
int ecgpu_bign_sign_batch(ecgpu_ctx* ctx, const uint8_t* d, const uint8_t* k, const uint8_t* h, size_t n, uint8_t* out_sig, uint8_t* ok) {
    HostCall c(ctx, __func__, ECGPU_BIGN256);
    if (c.bad(n && (!d || !k || !h || !out_sig || !ok))) return c.rc;
    return staged(ctx, n, {{d, &ctx->in0, 32, SECRET}, {k, &ctx->in3, 32, SECRET}, {h, &ctx->in2, 32}},
                  {{out_sig, &ctx->out0, 48}, {ok, &ctx->out1, 1}}, [&](auto in, auto out, size_t m) {
                      return bign_sign_dev(ctx, in[0], in[1], in[2], m, out[0], out[1]);
                  });
}

int ecgpu_bign_sign_prehash_batch(ecgpu_ctx* ctx, const uint8_t* d, const uint8_t* h, size_t n, uint8_t* out_sig, uint8_t* ok) {
    HostCall c(ctx, __func__, ECGPU_BIGN256);
    if (c.bad(n && (!d || !h || !out_sig || !ok))) return c.rc;
    return staged(ctx, n, {{d, &ctx->in0, 32, SECRET}, {h, &ctx->in2, 32}}, {{out_sig, &ctx->out0, 48}, {ok, &ctx->out1, 1}},
                  [&](auto in, auto out, size_t m) { return bign_sign_dev(ctx, in[0], nullptr, in[1], m, out[0], out[1]); });
}

int ecgpu_bign_sign_msg_batch(ecgpu_ctx* ctx, const uint8_t* d, const uint8_t* msgs, size_t msg_len, size_t n, uint8_t* out_sig,
                              uint8_t* ok) {
    HostCall c(ctx, __func__, ECGPU_BIGN256);
    if (c.bad(n && (!d || !out_sig || !ok || (msg_len && !msgs)))) return c.rc;
    return staged(ctx, n, {{d, &ctx->in0, 32, SECRET}, {msg_len ? msgs : nullptr, &ctx->in1, msg_len}},
                  {{out_sig, &ctx->out0, 48}, {ok, &ctx->out1, 1}}, [&](auto in, auto out, size_t m) {
                      return bign_sign_dev(ctx, in[0], nullptr, in[1], m, out[0], out[1], true, msg_len);
                  });
}

// ---- X448: scalars and results (shared secrets, and public keys all the same) are staged as secrets; points and verdicts are public ----
// (host-pointer forms only: x448_dev is internal, every chunk reaches it through `staged`; no curve argument)
int ecgpu_x448_batch(ecgpu_ctx* ctx, const uint8_t* scalars, const uint8_t* points_u, size_t n, uint8_t* out_u, uint8_t* ok) {
    HostCall c(ctx, __func__);
    if (c.bad(n && (!scalars || !points_u || !out_u || !ok))) return c.rc;
    if (n == 0) return ECGPU_OK;
    return staged(ctx, n, {{scalars, &ctx->in0, 56, SECRET}, {points_u, &ctx->in1, 56}}, {{out_u, &ctx->out0, 56, SECRET}, {ok, &ctx->out1, 1}},
                  [&](auto in, auto out, size_t m) { return x448_dev(ctx, X448_CHECKED, in[0], in[1], m, out[0], out[1]); });
}

int ecgpu_x448_unchecked_batch(ecgpu_ctx* ctx, const uint8_t* scalars, const uint8_t* points_u, size_t n, uint8_t* out_u) {
    HostCall c(ctx, __func__);
    if (c.bad(n && (!scalars || !points_u || !out_u))) return c.rc;
    if (n == 0) return ECGPU_OK;
    return staged(ctx, n, {{scalars, &ctx->in0, 56, SECRET}, {points_u, &ctx->in1, 56}}, {{out_u, &ctx->out0, 56, SECRET}},
                  [&](auto in, auto out, size_t m) { return x448_dev(ctx, X448_UNCHECKED, in[0], in[1], m, out[0], nullptr); });
}

int ecgpu_x448_base_batch(ecgpu_ctx* ctx, const uint8_t* scalars, size_t n, uint8_t* out_u) {
    HostCall c(ctx, __func__);
    if (c.bad(n && (!scalars || !out_u))) return c.rc;
    if (n == 0) return ECGPU_OK;
    return staged(ctx, n, {{scalars, &ctx->in0, 56, SECRET}}, {{out_u, &ctx->out0, 56, SECRET}},
                  [&](auto in, auto out, size_t m) { return x448_dev(ctx, X448_BASE, in[0], nullptr, m, out[0], nullptr); });
}

// ---- SM2 public-key encryption: k, d and the messages are staged as secrets; C1, C2 and C3 are public ----
// (host-pointer forms only: sm2_pke_dev is internal, every chunk reaches it through `staged`)
int ecgpu_sm2_pke_encrypt_batch(ecgpu_ctx* ctx, const uint8_t* pk_xy, const uint8_t* k, const uint8_t* msgs, size_t msg_len, size_t n,
                                uint8_t* out_c1_xy, uint8_t* out_c2, uint8_t* out_c3, uint8_t* ok) {
    HostCall h(ctx, __func__, ECGPU_SM2);
    if (h.bad(msg_len == 0 || msg_len > 0xFFFFFFFFull || (n && (!pk_xy || !k || !msgs || !out_c1_xy || !out_c2 || !out_c3 || !ok)))) return h.rc;
    return staged(ctx, n, {{pk_xy, &ctx->in1, 64}, {k, &ctx->in0, 32, SECRET}, {msgs, &ctx->in3, msg_len, SECRET}},
                  {{out_c1_xy, &ctx->out0, 64}, {out_c2, &ctx->out1, msg_len}, {out_c3, &ctx->out2, 32}, {ok, &ctx->out3, 1}},
                  [&](auto in, auto out, size_t m) {
                      return sm2_pke_dev(ctx, false, in[1], in[0], in[2], msg_len, m, out[0], out[1], out[2], out[3]);
                  });
}

int ecgpu_sm2_pke_decrypt_batch(ecgpu_ctx* ctx, const uint8_t* d, const uint8_t* c1_xy, const uint8_t* c2, size_t msg_len, const uint8_t* c3,
                                size_t n, uint8_t* out_msgs, uint8_t* ok) {
    HostCall h(ctx, __func__, ECGPU_SM2);
    if (h.bad(msg_len > 0xFFFFFFFFull || (n && (!d || !c1_xy || !c3 || !ok || (msg_len && (!c2 || !out_msgs)))))) return h.rc;
    // (msg_len == 0: nothing to stage for C2 and M'; the kernel touches neither and the verdict is SM3(x2 || y2) == C3)
    return staged(ctx, n, {{d, &ctx->in0, 32, SECRET}, {c1_xy, &ctx->in1, 64}, {msg_len ? c2 : nullptr, &ctx->in2, msg_len}, {c3, &ctx->in3, 32}},
                  {{msg_len ? out_msgs : nullptr, &ctx->out0, msg_len, SECRET}, {ok, &ctx->out1, 1}}, [&](auto in, auto out, size_t m) {
                      return sm2_pke_dev(ctx, true, in[0], in[1], in[2], msg_len, m, nullptr, out[0], const_cast<void*>(in[3]), out[1]);
                  });
}

static int batch_ecdh_host(ecgpu_ctx* ctx, int curve, const uint8_t* scalars, const uint8_t* points_xy, size_t n, uint8_t* out_x,
                           uint8_t* ok, bool ct, const char* fn) {
    HostCall h(ctx, fn, curve);
    if (h.bad(n && (!scalars || !points_xy || !out_x || !ok))) return h.rc;
    const auto dev = ct ? ecgpu_batch_ecdh_ct_dev : ecgpu_batch_ecdh_dev;
    return staged(ctx, n, {{scalars, &ctx->in0, h.L, ct}, {points_xy, &ctx->in1, 2 * h.L}}, {{out_x, &ctx->out0, h.L, ct}, {ok, &ctx->out1, 1, ct}},
                  [&](auto in, auto out, size_t m) { return dev(ctx, curve, in[0], in[1], m, out[0], out[1]); });
}

int ecgpu_batch_ecdh(ecgpu_ctx* ctx, int curve, const uint8_t* scalars, const uint8_t* points_xy, size_t n, uint8_t* out_x, uint8_t* ok) {
    return batch_ecdh_host(ctx, curve, scalars, points_xy, n, out_x, ok, false, __func__);
}
int ecgpu_batch_ecdh_ct(ecgpu_ctx* ctx, int curve, const uint8_t* scalars, const uint8_t* points_xy, size_t n, uint8_t* out_x,
                        uint8_t* ok) {
    return batch_ecdh_host(ctx, curve, scalars, points_xy, n, out_x, ok, true, __func__);
}

int ecgpu_batch_decompress(ecgpu_ctx* ctx, int curve, const uint8_t* xs, const uint8_t* y_is_odd, size_t n, uint8_t* out_xy,
                           uint8_t* ok) {
    HostCall h(ctx, __func__, curve);
    if (h.bad(n && (!xs || !y_is_odd || !out_xy || !ok))) return h.rc;
    return staged(ctx, n, {{xs, &ctx->in0, h.L}, {y_is_odd, &ctx->in2, 1}}, {{out_xy, &ctx->out0, 2 * h.L}, {ok, &ctx->out1, 1}},
                  [&](auto in, auto out, size_t m) { return ecgpu_batch_decompress_dev(ctx, curve, in[0], in[1], m, out[0], out[1]); });
}

// ---- hash-to-curve: messages and u are staged as secrets (an OPRF input is a password), the DST goes up once per call ----
// (for n == 0 too: the checks of `Domain::xmd` belong to the call)
static int h2c_hash_host(ecgpu_ctx* ctx, const char* fn, int curve, int mode, const uint8_t* msgs, size_t msg_len, size_t n,
                         const uint8_t* dst, size_t dst_len, uint8_t* out, uint8_t* out_inf) {
    HostCall h(ctx, fn, curve);
    if (h.bad(!dst || dst_len == 0 || (n && (!out || (msg_len && !msgs))))) return h.rc;
    if (!h2c_has_suite(curve)) return curve_error(ctx, fn);
    size_t dstp_len = 0;
    if (int rc = h2c_stage_dst(ctx, curve, dst, dst_len, &dstp_len)) return rc;
    std::vector<PipeOut> outs = {{out, &ctx->out0, (mode == H2C_SCALAR ? 1 : 2) * h.L, SECRET}};
    if (mode != H2C_SCALAR) outs.push_back({out_inf, &ctx->out1, 1, SECRET});
    return staged(ctx, n, {{msg_len ? msgs : nullptr, &ctx->in0, msg_len, SECRET}}, outs, [&](auto in, auto out_d, size_t m) {
        return h2c_run(ctx, fn, curve, mode, in[0], msg_len, 0, dstp_len, m, out_d[0], mode == H2C_SCALAR ? nullptr : out_d[1]);
    });
}
int ecgpu_hash_to_curve_batch(ecgpu_ctx* ctx, int curve, const uint8_t* msgs, size_t msg_len, size_t n, const uint8_t* dst,
                              size_t dst_len, uint8_t* out_xy, uint8_t* out_inf) {
    return h2c_hash_host(ctx, __func__, curve, H2C_RO, msgs, msg_len, n, dst, dst_len, out_xy, out_inf);
}
int ecgpu_encode_to_curve_batch(ecgpu_ctx* ctx, int curve, const uint8_t* msgs, size_t msg_len, size_t n, const uint8_t* dst,
                                size_t dst_len, uint8_t* out_xy, uint8_t* out_inf) {
    return h2c_hash_host(ctx, __func__, curve, H2C_NU, msgs, msg_len, n, dst, dst_len, out_xy, out_inf);
}
int ecgpu_hash_to_scalar_batch(ecgpu_ctx* ctx, int curve, const uint8_t* msgs, size_t msg_len, size_t n, const uint8_t* dst,
                               size_t dst_len, uint8_t* out_scalars) {
    return h2c_hash_host(ctx, __func__, curve, H2C_SCALAR, msgs, msg_len, n, dst, dst_len, out_scalars, nullptr);
}
int ecgpu_map_to_curve_batch(ecgpu_ctx* ctx, int curve, const uint8_t* u, int per_point, size_t n, uint8_t* out_xy, uint8_t* out_inf) {
    HostCall h(ctx, __func__, curve);
    if (h.bad((per_point != 1 && per_point != 2) || (n && (!u || !out_xy)))) return h.rc;
    if (!h2c_has_suite(curve)) return curve_error(ctx, __func__);
    return staged(ctx, n, {{u, &ctx->in0, (size_t)per_point * h.L, SECRET}}, {{out_xy, &ctx->out0, 2 * h.L, SECRET}, {out_inf, &ctx->out1, 1, SECRET}},
                  [&](auto in, auto out, size_t m) { return h2c_run(ctx, __func__, curve, H2C_MAP, in[0], 0, per_point, 0, m, out[0], out[1]); });
}

int ecgpu_batch_normalize(ecgpu_ctx* ctx, int curve, const uint8_t* points_xyz, size_t n, uint8_t* out_xy,
                          uint8_t* out_inf) {
    HostCall h(ctx, __func__, curve);
    if (h.bad(n && (!points_xyz || !out_xy))) return h.rc;
    return staged(ctx, n, {{points_xyz, &ctx->in0, 3 * h.L}}, {{out_xy, &ctx->out0, 2 * h.L}, {out_inf, &ctx->out1, 1}},
                  [&](auto in, auto out, size_t m) { return ecgpu_batch_normalize_dev(ctx, curve, in[0], m, out[0], out[1]); }, STAGE_WHOLE);
}

int ecgpu_point_sum(ecgpu_ctx* ctx, int curve, const uint8_t* points_xy, const uint8_t* points_inf, size_t n,
                    uint8_t* out_xy, uint8_t* out_inf) {
    HostCall h(ctx, __func__, curve);
    if (h.bad(!out_xy || (n && !points_xy))) return h.rc;
    return staged(ctx, n, {{points_xy, &ctx->in1, 2 * h.L}, {points_inf, &ctx->in2, 1}}, {{out_xy, &ctx->out0, 2 * h.L}, {out_inf, &ctx->out1, 1}},
                  [&](auto in, auto out, size_t m) { return ecgpu_point_sum_dev(ctx, curve, in[0], in[1], m, out[0], out[1]); }, STAGE_REDUCE);
}

// (the three below launch their kernel themselves, as the device call of `staged`)
int ecgpu_k256_glv_decompose(ecgpu_ctx* ctx, const uint8_t* scalars, size_t n, uint8_t* r1, uint8_t* r2) {
    HostCall h(ctx, __func__, ECGPU_K256);
    if (h.bad(n && (!scalars || !r1 || !r2))) return h.rc;
    if (n == 0) return ECGPU_OK;
    return staged(ctx, n, {{scalars, &ctx->in0, 32}}, {{r1, &ctx->out0, 32}, {r2, &ctx->in1, 32}}, [&](auto in, auto out, size_t m) {
        int rc = reset_status(ctx);
        if (rc != ECGPU_OK) return rc;
        launch_k256_glv(ctx->stream, (const uint8_t*)in[0], m, (uint8_t*)out[0], (uint8_t*)out[1], ctx->d_status);
        return finish(ctx);
    }, STAGE_WHOLE);
}

int ecgpu_selftest_field(ecgpu_ctx* ctx, int curve, int op, const uint8_t* a, const uint8_t* b, size_t n, uint8_t* out) {
    HostCall h(ctx, __func__, curve);
    if (h.bad(n && (!a || !out))) return h.rc;
    if (n == 0) return ECGPU_OK;
    return staged(ctx, n, {{a, &ctx->in0, h.L}, {b, &ctx->in1, h.L}}, {{out, &ctx->out0, h.L}}, [&](auto in, auto o, size_t m) {
        int rc = reset_status(ctx);
        if (rc != ECGPU_OK) return rc;
        rc = dispatch(curve, [&](auto c) {
            launch_selftest_field<decltype(c)>(ctx->stream, op, (const uint8_t*)in[0], (const uint8_t*)in[1], m, (uint8_t*)o[0], ctx->d_status);
            return (int)ECGPU_OK;
        });
        return rc != ECGPU_OK ? rc : finish(ctx);
    }, STAGE_WHOLE);
}

int ecgpu_selftest_point(ecgpu_ctx* ctx, int curve, int op, const uint8_t* p_xy, const uint8_t* p_inf, const uint8_t* q_xy,
                         const uint8_t* q_inf, size_t n, uint8_t* out_xy, uint8_t* out_inf) {
    HostCall h(ctx, __func__, curve);
    if (h.bad(n && (!p_xy || !out_xy || !out_inf))) return h.rc;
    // ops 20 - 26 (the cross-lane code of the MSM's tail; bits 8.. of op carry a count of doublings): whole waves, whole workgroups
    // for the tree, and a second operand for all but the lane-shared doubling of a single point
    const int code = op & 0xFF;
    const bool tail = code >= 20;
    if (h.bad(tail && (n % (code == 25 ? 256 : 64) != 0 || (op >> 8) > 64 || (code != 26 && !q_xy)))) return h.rc;
    if (n == 0) return ECGPU_OK;
    return staged(ctx, n, {{p_xy, &ctx->in0, 2 * h.L}, {p_inf, &ctx->in2, 1}, {q_xy, &ctx->in1, 2 * h.L}, {q_inf, &ctx->in3, 1}},
                  {{out_xy, &ctx->out0, 2 * h.L}, {out_inf, &ctx->out1, 1}}, [&](auto in, auto o, size_t m) {
                      int rc = reset_status(ctx);
                      if (rc != ECGPU_OK) return rc;
                      rc = dispatch(curve, [&](auto c) {
                          if (tail)
                              launch_selftest_msm<decltype(c)>(ctx->stream, op, (const uint8_t*)in[0], (const uint8_t*)in[1], (const uint8_t*)in[2],
                                                               (const uint8_t*)in[3], m, (uint8_t*)o[0], (uint8_t*)o[1], ctx->d_status);
                          else
                              launch_selftest_point<decltype(c)>(ctx->stream, op, (const uint8_t*)in[0], (const uint8_t*)in[1], (const uint8_t*)in[2],
                                                                 (const uint8_t*)in[3], m, (uint8_t*)o[0], (uint8_t*)o[1], ctx->d_status);
                          return (int)ECGPU_OK;
                      });
                      return rc != ECGPU_OK ? rc : finish(ctx);
                  }, STAGE_WHOLE);
}

int ecgpu_selftest_point_raw(ecgpu_ctx* ctx, int curve, int op, const uint8_t* p, const uint8_t* q, size_t n, uint8_t* out) {
    HostCall h(ctx, __func__, curve);
    if (h.bad(n && (!p || !out))) return h.rc;
    if (n == 0) return ECGPU_OK;
    size_t rec = 0;                                           // four slots of NL 32-bit limbs
    dispatch(curve, [&](auto c) { rec = 16 * (size_t) decltype(c)::NL; return (int)ECGPU_OK; });
    return staged(ctx, n, {{p, &ctx->in0, rec}, {q, &ctx->in1, rec}}, {{out, &ctx->out0, rec}}, [&](auto in, auto o, size_t m) {
        int rc = reset_status(ctx);
        if (rc != ECGPU_OK) return rc;
        rc = dispatch(curve, [&](auto c) {
            launch_selftest_point_raw<decltype(c)>(ctx->stream, op, (const uint32_t*)in[0], (const uint32_t*)in[1], m, (uint32_t*)o[0], ctx->d_status);
            return (int)ECGPU_OK;
        });
        return rc != ECGPU_OK ? rc : finish(ctx);
    }, STAGE_WHOLE);
}

// One op of csrc/ecgpu_fe448.h on raw limbs (test infrastructure: tests/fe448_vectors.py).  a, b, out: 16 little-endian 32-bit
// words per element, so that lazy representatives can be handed in; b may be NULL for the ops of one operand (it reads as zero).
// Ops: 0 mul, 1 sqr, 2 add, 3 sub, 4 mul_small(39082), 5 carry, 6 canon, 7 invert, 8 from_bytes -> to_bytes (ecgpu_x448.h).
int ecgpu_selftest_fe448(ecgpu_ctx* ctx, int op, const uint8_t* a, const uint8_t* b, size_t n, uint8_t* out) {
    HostCall c(ctx, __func__);
    if (c.bad(op < 0 || op >= FE448_OPS || (n && (!a || !out)))) return c.rc;
    if (n == 0) return ECGPU_OK;
    return staged(ctx, n, {{a, &ctx->in0, 64}, {b, &ctx->in1, 64}}, {{out, &ctx->out0, 64}}, [&](auto in, auto o, size_t m) -> int {
        int rc = reset_status(ctx);
        if (rc != ECGPU_OK) return rc;
        launch_selftest_fe448(ctx->stream, op, (const uint32_t*)in[0], (const uint32_t*)in[1], m, (uint32_t*)o[0]);
        return finish(ctx);
    }, STAGE_WHOLE);
}

// One lane body of csrc/ecgpu_h2c.h on the caller's records (test infrastructure: tests/h2c_vectors.py).  Ops: 0 reduce mod p,
// 1 reduce mod n (records of L = 48 / 72 bytes in, one wire record out), 2 sswu (u in, xn || xd || y out), 3 the secp256k1 isogeny
// (xn || xd || y in, X || Y || Z out).  The early returns are those of ecgpu_map_to_curve_batch, the op where it has per_point.
int ecgpu_selftest_h2c(ecgpu_ctx* ctx, int curve, int op, const uint8_t* in, size_t n, uint8_t* out) {
    HostCall h(ctx, __func__, curve);
    if (h.bad(op < 0 || op >= H2C_ST_OPS || (n && (!in || !out)))) return h.rc;
    if (!h2c_has_suite(curve) || (op == H2C_ST_ISO && curve != ECGPU_K256)) return curve_error(ctx, __func__);
    if (n == 0) return ECGPU_OK;
    const size_t draw = (size_t)dispatch(curve, [](auto c) { return h2c_draw_bytes<decltype(c)>(); });
    const bool reduce = op == H2C_ST_REDUCE_P || op == H2C_ST_REDUCE_N;
    const size_t in_unit = reduce ? draw : op == H2C_ST_SSWU ? h.L : 3 * h.L, out_unit = reduce ? h.L : 3 * h.L;
    return staged(ctx, n, {{in, &ctx->in0, in_unit}}, {{out, &ctx->out0, out_unit}}, [&](auto i, auto o, size_t m) -> int {
        int rc = reset_status(ctx);
        if (rc != ECGPU_OK) return rc;
        rc = dispatch(curve, [&](auto c) {
            launch_selftest_h2c<decltype(c)>(ctx->stream, op, (const uint8_t*)i[0], m, (uint8_t*)o[0]);
            return (int)ECGPU_OK;
        });
        return rc != ECGPU_OK ? rc : finish(ctx);
    }, STAGE_WHOLE);
}

// The signing pipelines' finish kernels on stages the caller supplies (test infrastructure: tests/sign_vectors.py).  Nothing is
// computed before the kernel: flag, affine R and r_inf are what the nonce, fixed-base and normalisation kernels would have left.
int ecgpu_selftest_sign_finish(ecgpu_ctx* ctx, int curve, int scheme, const uint8_t* d, const uint8_t* k, const uint8_t* flag,
                               const uint8_t* z, const uint8_t* r_xy, const uint8_t* r_inf, const uint8_t* msgs, size_t msg_len, size_t n,
                               int normalize_s, uint8_t* out_sig, uint8_t* out_recid, uint8_t* ok) {
    HostCall h(ctx, __func__, curve);
    if (h.rc != ECGPU_OK) return h.rc;
    const bool ecdsa = scheme == 0, sm2 = scheme == 1, schnorr = scheme == 2, bign = scheme == ECGPU_SIGN_SCHEME_BIGN;
    if (!(ecdsa || sm2 || schnorr || bign)) return arg_error(ctx, __func__);
    if ((ecdsa && not_ecdsa(curve)) || (sm2 && curve != ECGPU_SM2) || (schnorr && curve != ECGPU_K256) || (bign && curve != ECGPU_BIGN256))
        return curve_error(ctx, __func__);
    if (h.bad(n && (!d || !k || !flag || !r_xy || !r_inf || !out_sig || !ok || (!schnorr && !z) || (ecdsa && !out_recid) ||
                    (schnorr && msg_len && !msgs))))
        return h.rc;
    if (n == 0) return ECGPU_OK;
    const size_t L = h.L;
    return staged(ctx, n, {{d, &ctx->in0, schnorr ? 2 * L : L, SECRET}, {k, &ctx->in3, L, SECRET}, {flag, &ctx->sg_flag, 1},
                           {schnorr ? nullptr : z, &ctx->in2, L}, {r_xy, &ctx->ec_xy, 2 * L}, {r_inf, &ctx->ec_inf, 1},
                           {schnorr && msg_len ? msgs : nullptr, &ctx->in1, msg_len}},
                  {{out_sig, &ctx->out0, bign ? 48 : 2 * L}, {ecdsa ? out_recid : nullptr, &ctx->out2, 1}, {ok, &ctx->out1, 1}},
                  [&](auto in, auto o, size_t m) -> int {
                      auto u8 = [&](int i) { return (const uint8_t*)in[i]; };
                      if (ecdsa) {
                          const int rc = dispatch(curve, [&](auto c) {
                              launch_ecdsa_sign_finish<decltype(c)>(ctx->stream, u8(0), u8(1), u8(2), u8(3), u8(4), u8(5), m, normalize_s,
                                                                    (uint8_t*)o[0], (uint8_t*)o[1], (uint8_t*)o[2]);
                              return (int)ECGPU_OK;
                          });
                          if (rc != ECGPU_OK) return rc;
                      } else if (sm2) {
                          launch_sm2dsa_sign_finish<Sm2Params>(ctx->stream, u8(0), u8(1), u8(2), u8(3), u8(4), u8(5), m, (uint8_t*)o[0],
                                                               (uint8_t*)o[2]);
                      } else if (bign) {                       // z = the raw prehash, S0 = the first 16 bytes of each r_xy record
                          launch_bign_sign_finish<Bign256Params>(ctx->stream, u8(0), u8(1), u8(2), u8(3), u8(4), 64, u8(5), m,
                                                                 (uint8_t*)o[0], (uint8_t*)o[2]);
                      } else {
                          launch_schnorr_sign_finish<K256Params>(ctx->stream, u8(0), u8(1), u8(2), u8(4), u8(5), u8(6), msg_len, m,
                                                                 (uint8_t*)o[0], (uint8_t*)o[2]);
                      }
                      HIP_TRY(ctx, hipGetLastError());
                      return (int)ECGPU_OK;
                  }, STAGE_WHOLE);
}

// The generator kernels of bign signing with the caller's bound in place of q (test infrastructure: tests/test_gpu_bignsign.py).
// The prehash is reduced mod q as in the signing calls; k_bign_genk and k_bign_genk_retry run as bign_sign_dev launches them.
// out_k: the accepted candidate (1 where the cap was reached), out_rounds: the generator's round counter afterwards (4 bytes per element).
int ecgpu_selftest_bign_genk(ecgpu_ctx* ctx, const uint8_t* d, const uint8_t* h, const uint8_t* bound, size_t n, uint8_t* out_k,
                             uint8_t* out_rounds) {
    using C = Bign256Params;
    HostCall c(ctx, __func__, ECGPU_BIGN256);
    if (c.bad(!bound || (n && (!d || !h || !out_k || !out_rounds)))) return c.rc;
    if (n == 0) return ECGPU_OK;
    uint32_t bw[8];
    for (int j = 0; j < 8; j++)
        bw[j] = (uint32_t)bound[4 * j] | (uint32_t)bound[4 * j + 1] << 8 | (uint32_t)bound[4 * j + 2] << 16 | (uint32_t)bound[4 * j + 3] << 24;
    return staged(ctx, n, {{d, &ctx->in0, 32, SECRET}, {h, &ctx->in2, 32}},
                  {{out_k, &ctx->out0, 32, SECRET}, {out_rounds, &ctx->out1, 4}}, [&](auto in, auto o, size_t m) -> int {
                      DevCall call(ctx, WIPE_SIGN, {{ctx->sg_flag, m + 16}, {ctx->sg_state, m * bign_genk_state_bytes<C>() + 16}});
                      if (call.rc != ECGPU_OK) return call.rc;
                      uint32_t* state = (uint32_t*)ctx->sg_state.p;
                      launch_bign_genk<C>(ctx->stream, (const uint8_t*)in[0], (const uint8_t*)in[1], bw, m, ctx->rfc6979_cap, (uint8_t*)o[0],
                                          (uint8_t*)ctx->sg_flag.p, state);
                      HIP_TRY(ctx, hipMemcpyAsync(o[1], state + 16 * m, m * 4, hipMemcpyDeviceToDevice, ctx->stream));
                      return call.done_unmarked();
                  }, STAGE_WHOLE);
}

int ecgpu_valu_probe(ecgpu_ctx* ctx, int which, double* ops_per_sec) {
    if (!check_ctx(ctx) || !ops_per_sec) return ECGPU_ERR_ARG;
    int rc;
    if (which == 200) {
        // random 64-byte gathers over the k256 comb table (2^20 lanes x 16 entries): returns bytes per second
        if ((rc = ensure_table<K256Params>(ctx)) != ECGPU_OK) return rc;
        const Table& t = ctx->table[ECGPU_K256];
        const int gblocks = 4096, per_lane = 16;
        const size_t entries = ((size_t)1 << (t.w - 1)) * t.nwin;
        if ((rc = ensure(ctx, ctx->out0, (size_t)gblocks * BLOCK * 4)) != ECGPU_OK) return rc;
        launch_gather_probe(ctx->stream, (const uint32_t*)t.d, entries, 2, (uint32_t*)ctx->out0.p, gblocks);
        record(ctx, 0);
        launch_gather_probe(ctx->stream, (const uint32_t*)t.d, entries, per_lane, (uint32_t*)ctx->out0.p, gblocks);
        record(ctx, 1);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        float gms = 0;
        HIP_TRY(ctx, hipEventElapsedTime(&gms, ctx->ev[0], ctx->ev[1]));
        *ops_per_sec = (double)gblocks * BLOCK * per_lane * 64.0 / (gms * 1e-3);
        return ECGPU_OK;
    }
    if (which == 201 || which == 202) {
        // the per-lane table pattern of the variable-base kernels with known useful bytes (ecgpu_misc.hip k_tabrow_probe):
        // 201 = every lane of a wave reads the same entry (contiguous 256-byte rows), 202 = a per-lane entry.  2048 workgroups
        // like a 2^20-element variable-base call, 64 entry reads of 20 rows per lane: returns useful bytes read per second.
        const int tblocks = 2048, reps = 64;
        const size_t lanes = (size_t)tblocks * BLOCK;
        if ((rc = ensure(ctx, ctx->vtab, lanes * 8 * 30 * 4)) != ECGPU_OK) return rc;
        if ((rc = ensure(ctx, ctx->out0, lanes * 4)) != ECGPU_OK) return rc;
        record(ctx, 0);
        launch_tabrow_probe(ctx->stream, (uint32_t*)ctx->vtab.p, which == 202, reps, (uint32_t*)ctx->out0.p, tblocks);
        record(ctx, 1);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        float tms = 0;
        HIP_TRY(ctx, hipEventElapsedTime(&tms, ctx->ev[0], ctx->ev[1]));
        *ops_per_sec = (double)lanes * reps * 20 * 4.0 / (tms * 1e-3);
        return ECGPU_OK;
    }
    const int blocks = 256 * 8, iters = 2048;
    if ((rc = ensure(ctx, ctx->out0, (size_t)blocks * BLOCK * 4)) != ECGPU_OK) return rc;
    // which >= 100: exact inline-asm instruction probes (which - 100 selects the instruction, see ecgpu_misc.hip);
    // the result is then wave64-instructions per second x 64 (i.e. lane-operations per second).
    auto launch = [&](int it) {
        if (which >= 100) launch_isa_probe(ctx->stream, which - 100, (uint32_t*)ctx->out0.p, blocks, it);
        else launch_valu_probe(ctx->stream, which, (uint32_t*)ctx->out0.p, blocks, it);
    };
    launch(16);  // warm-up
    record(ctx, 0);
    launch(iters);
    record(ctx, 1);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    float ms = 0;
    HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]));
    double ops = (double)blocks * BLOCK * (double)iters * 64.0;
    *ops_per_sec = ops / (ms * 1e-3);
    return ECGPU_OK;
}

}  // extern "C"
