/*
 * ecgpu.h — C ABI of libecgpu.so, the MI355X (gfx950) batch scalar-multiplication / MSM engine
 * that drops in behind RustCrypto/elliptic-curves' scalar-mul surface for k256, p256 and p384.
 *
 * Every entry point names the reference interface it replaces (paths relative to the reference
 * root).  The reference's own API works on one element at a time; the GPU entry points are the
 * batch forms of the same operations, plus `lincomb`, which is already a batch.  INTEGRATION.md
 * shows the Rust `extern "C"` block and the `MulBackend` / `LinearCombination` adapter a
 * maintainer would add on the reference side.
 *
 * Wire format (identical for host- and device-pointer entry points)
 *   scalars   n * L bytes, big-endian, canonical (< group order n) — `Scalar::to_repr`
 *             (k256/src/arithmetic/scalar.rs:310-316, primefield/src/monty.rs:498-500);
 *             L = 32 (k256, p256, sm2, bp256 = brainpoolP256r1, bp256t1, bign256), 48 (p384, bp384 = brainpoolP384r1, bp384t1), 28 (p224), 24 (p192) or 66 (p521) = `FieldBytesSize`.  Records are packed without
 *             padding (p224: 28-byte scalars, 56-byte points); only the base pointers of device buffers must be 16-byte aligned
 *             (which also gives every record the alignment its codec reads with: 4 bytes for p224 / p192, 2 bytes for p521's
 *             66-byte records — a *_dev pointer into the middle of an array must keep to a whole number of records).
 *   points    n * 2L bytes, big-endian affine x || y — `AffinePoint::{x,y}`
 *             (primeorder/src/affine.rs:106-112) + optional n-byte identity flags
 *             (`AffinePoint::infinity`, k256/src/arithmetic/affine.rs:45-49); NULL flags = none.
 *             The identity is encoded as x = y = 0 with flag 1 on output.
 *   projective inputs (ecgpu_batch_normalize, the *_xyz entry points: ecgpu_batch_mul[_ct]_xyz, ecgpu_msm_xyz,
 *             ecgpu_lincomb_ct_xyz, ecgpu_batch_mul_base_and_mul_add_xyz, ecgpu_msm_parts_xyz_dev, ecgpu_group_msm_xyz): n * 3L bytes X || Y || Z,
 *             canonical big-endian, homogeneous (x = X/Z, y = Y/Z: `ProjectivePoint`, k256/src/arithmetic/projective.rs:40-45,
 *             primeorder/src/projective.rs:49-53); Z = 0 is the identity whatever X and Y are (`to_affine`); no flag array.
 *   ECGPU_BIGN256 (bign-curve256v1, `bignp256`) is the exception to "big-endian": its field elements and scalars travel
 *             LITTLE-endian, as in the reference (`FIELD_ENDIANNESS = LittleEndian`, bignp256/src/lib.rs:102); everything
 *             else about the records is the same.
 *
 * Ownership: the caller owns every buffer passed in; the library keeps no pointer after return.
 * Device memory, streams and the precomputed basepoint tables belong to the context
 * (the analogue of the reference's `static BASEPOINT_TABLE: LazyLock<..>`,
 * k256/src/arithmetic/tables.rs:18, primeorder/src/tables/basepoint.rs:29-31).
 *
 * Errors: every function returns ECGPU_OK (0) or a negative code; nothing aborts or throws across
 * the ABI.  Decoding failures mirror the reference's `CtOption`/`Error` results; the arithmetic
 * itself is total (complete formulas).  There is NO CPU fallback: without a usable gfx950 device
 * ecgpu_init fails with ECGPU_ERR_NO_DEVICE.
 *
 * Secret scalars: every entry point whose name does not end in `_ct` / `_ct_dev` is VARIABLE-TIME in its scalars (zero
 * digits are skipped; comb-table entries, per-point table entries and Pippenger buckets are addressed by scalar bits; the
 * kernels' duration and memory access pattern depend on the scalar).  Those stand behind the reference's `*_vartime` names —
 * `MulVartime::mul_vartime` (primeorder/src/projective.rs:888-921), `LinearCombination::lincomb_vartime` (:498-510,
 * k256/src/arithmetic/mul.rs:100-108), `MulByGeneratorVartime::{mul_by_generator_vartime,
 * mul_by_generator_and_mul_add_vartime}` (:923-940, k256 mul.rs:205-232,296-310) — with affine points, or with the reference's
 * `ProjectivePoint` itself through the *_xyz forms (below; primeorder/src/projective.rs:480-511,888-940, k256 mul.rs:84-109,296-310:
 * `lincomb_vartime`, `mul_vartime`, `mul_by_generator_and_mul_add_vartime` take projective points) — and is meant for PUBLIC scalars:
 * signature verification, MSMs over public data, batch derivation of public values.  It is NOT a replacement for the
 * constant-time `Mul` / `mul_by_generator` / `lincomb` (primeorder/src/projective.rs:532-557, tables/lookup.rs:43-65)
 * when the scalar is a long-term secret and an attacker can observe the device (timing of a shared GPU, its memory
 * traffic).  ecgpu_batch_mul_base* and ecgpu_batch_ecdh accept whatever scalars they are given: a caller that passes
 * private keys there has decided that its threat model allows it; the results are the same group elements either way.
 * For secret scalars there are the uniform-schedule entry points ecgpu_batch_mul_base_ct, ecgpu_batch_mul_ct,
 * ecgpu_batch_ecdh_ct and ecgpu_lincomb_ct, and ecgpu_batch_mul_ct_xyz / ecgpu_lincomb_ct_xyz for projective points
 * (below): the reference's constant-time drivers — fixed digit count, every table entry read and one
 * kept under a mask, complete additions — at 1.2-7x the cost of the variable-time kernels.
 *
 * Hashing to the curve: ecgpu_hash_to_curve_batch, ecgpu_encode_to_curve_batch, ecgpu_hash_to_scalar_batch and
 * ecgpu_map_to_curve_batch (below) turn byte strings into group elements and scalars (RFC 9380) for ECGPU_K256, ECGPU_P256 and
 * ECGPU_P384 only; their inputs may be secret (an OPRF input is a password), so their kernels follow the rule of the `_ct` forms and
 * their scratch is zeroed behind the call, although their names carry no `_ct`.
 *
 * Threading: a context may be used from one thread at a time (calls serialise on its stream);
 * create one context per thread / per GPU for concurrency.  The host-pointer forms of the per-unit batch calls
 * (everything except ecgpu_point_sum and ecgpu_batch_normalize) run batches of 2^19 units and more as a
 * pipeline over chunks of 2^18 units (ecgpu_msm: from 2^23 terms, as partial MSMs over chunks of 2^22 terms): two helper threads, alive for the duration of the call, move the next chunk in and
 * the previous one out on their own streams.  A pipelined call is not all-or-nothing: when a chunk fails validation
 * (ECGPU_ERR_SCALAR_RANGE / ECGPU_ERR_POINT) the results of the chunks before it may already have been written to the
 * caller's output buffers; below 2^19 units nothing is written on error.
 */
#ifndef ECGPU_H
#define ECGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ecgpu_ctx ecgpu_ctx;

enum { ECGPU_K256 = 0, ECGPU_P256 = 1, ECGPU_P384 = 2, ECGPU_SM2 = 3, ECGPU_P224 = 4, ECGPU_P192 = 5, ECGPU_P521 = 6, ECGPU_BP256 = 7, ECGPU_BP384 = 8, ECGPU_BP256T1 = 9, ECGPU_BP384T1 = 10, ECGPU_BIGN256 = 11 };

enum {
    ECGPU_OK = 0,
    ECGPU_ERR_CURVE = -1,        /* unknown curve id */
    ECGPU_ERR_SCALAR_RANGE = -2, /* a scalar >= n          (Scalar::from_repr -> None) */
    ECGPU_ERR_POINT = -3,        /* coordinate >= p or not on curve (AffinePoint::from_coordinates
                                    -> None, primeorder/src/affine.rs:100-109) */
    ECGPU_ERR_NO_DEVICE = -4,    /* no gfx950 device / HIP runtime unusable */
    ECGPU_ERR_HIP = -5,          /* a HIP call failed; see ecgpu_last_error */
    ECGPU_ERR_OOM = -6,          /* device or host allocation failed */
    ECGPU_ERR_ARG = -7           /* NULL / inconsistent argument */
};

/* ---- context -------------------------------------------------------------------------------- */

/* Number of gfx950 devices the HIP runtime shows this process (0: none / runtime unusable) — what a single-process
 * caller sizes its ecgpu_group from (elliptic-curves_amd/rust/ecgpu_shim.rs `NODE`). */
int ecgpu_device_count(void);

/* Creates a context on HIP device `device` (as numbered by the HIP runtime in this process).
 * Basepoint tables are built lazily on first use per curve and kept on the device: ONE table per (device, curve, width)
 * for the whole process, shared by every context on that device and freed with the last of them — the analogue of the
 * reference's process-wide `LazyLock<BasepointTable>` (k256/src/arithmetic/tables.rs:18).  Which width a call gets is the table
 * policy's decision (below: "the generator (comb) tables and their footprint").  If a table does not fit (k256's widest
 * is 21.5 GB) its comb width is lowered two bits at a time (a quarter of the memory, one or two more additions per
 * scalar, identical results) down to 16 bits before ECGPU_ERR_OOM is returned. */
int ecgpu_init(ecgpu_ctx **ctx, int device);
void ecgpu_destroy(ecgpu_ctx *ctx);

/* Human-readable text of the last error on this context (valid until the next call). */
const char *ecgpu_last_error(const ecgpu_ctx *ctx);

/* Field-byte length L of a curve (32 / 48 / 28 / 24 / 66), 0 for a bad id. */
size_t ecgpu_field_bytes(int curve);

/* Use an externally owned HIP stream (e.g. torch's current stream) for all later work on this
 * context; NULL restores the context's own stream.  `stream` is a hipStream_t. */
int ecgpu_set_stream(ecgpu_ctx *ctx, void *stream);

/* Page-locked host memory for the buffers of the host-pointer entry points.  Any host pointer works there, but
 * transfers from ordinary (pageable) memory go through the driver's bounce buffers at ~8 GB/s, which is 20x the
 * compute time of a fixed-base batch; from memory allocated here they run at PCIe DMA speed (DESIGN.md section 7 has
 * both numbers).  Returns NULL on failure.  ecgpu_host_free(NULL) is a no-op. */
void *ecgpu_host_alloc(ecgpu_ctx *ctx, size_t bytes);
void ecgpu_host_free(ecgpu_ctx *ctx, void *p);

/* Device memory for the *_dev entry points, for callers that have no HIP binding of their own (a Rust or C host that
 * wants its inputs to stay resident between calls; torch callers pass tensor data_ptr()s instead).  Allocations are
 * 256-byte aligned and live on the context's device until ecgpu_dev_free (ecgpu_destroy does not release them: free
 * them first).  The two copies are synchronous (they return when the bytes have arrived) and ordered after earlier
 * work on the context stream. */
void *ecgpu_dev_alloc(ecgpu_ctx *ctx, size_t bytes);
void ecgpu_dev_free(ecgpu_ctx *ctx, void *d_ptr);
int ecgpu_copy_to_device(ecgpu_ctx *ctx, void *d_dst, const void *h_src, size_t bytes);
int ecgpu_copy_to_host(ecgpu_ctx *ctx, void *h_dst, const void *d_src, size_t bytes);

/* ---- the generator (comb) tables and their footprint ----------------------------------------------------------------------
 * `mul_by_generator` reads a precomputed table of multiples of G that lives in device memory, shared by all contexts of a device:
 * ceil((bits - 1) / w) windows of 2^(w-1) affine entries (2L bytes each), w = the window width.  Wider tables mean fewer additions
 * per scalar and more memory and build time — k256: 16 bits = 34 MB built in ~1 ms, 15 additions per scalar, 0.83 ms per 2^20
 * scalars; 22 bits = 1.6 GB in ~6 ms, 11 additions, 0.73 ms; 26 bits = 21.5 GB in ~55 ms, 9 additions, 0.61 ms (measured: profiles/r05/table_tiers.txt, crossover batch sizes in
 * INTEGRATION.md).  The reference makes the same trade with its WINDOW_SIZE constants and builds lazily
 * (k256/src/arithmetic/mul.rs:191-192 prices a table half the size at 3 %; primeorder/src/tables/basepoint.rs:29-76).
 *
 * Default (ECGPU_TABLE_ADAPTIVE): the width follows the number of generator multiplications the DEVICE has been asked for so far,
 * the call being served included: 16 bits below 2^26, 22 bits below 2^29, then the curve's widest (k256 26, p256 / sm2 / the
 * other 256- and 224- / 192-bit sets 24, p384 / p521 / bp384 20) — each step where the time lost to the narrower table so far equals
 * the build time of the next one, so a caller never pays more than twice the best fixed choice and a 1,024-scalar call never
 * allocates gigabytes.  A step up costs the calling thread the build once — the call that crosses a tier waits for its stream and
 * builds the next table before it returns (k256: 1 / 6 / 55 ms), on an asynchronous context too —; the narrower table is freed when
 * its last user lets go.  Until a tier is reached the rate is the narrower table's (k256, per 2^20 scalars: ~0.93 ms at 16 bits,
 * ~0.74 at 22, ~0.59 at 26; bench.py prints the three as `fixed_k256_tier_ms`, its headline uses ECGPU_TABLE_EAGER).
 * ECGPU_TABLE_EAGER: the widest table at the first call (a long-lived service: pay ~55 ms once at start-up).
 * A table that does not fit is replaced by one two bits narrower, down to 16 bits, before ECGPU_ERR_OOM is returned. */
enum { ECGPU_TABLE_ADAPTIVE = 0, ECGPU_TABLE_EAGER = 1 };
int ecgpu_set_table_policy(ecgpu_ctx *ctx, int policy);

/* No comb table built for this context from now on takes more than max_table_bytes of device memory (0 = no limit, the default): the
 * width is lowered until the table fits the budget.  Tables already in use are kept until the next call on their curve. */
int ecgpu_set_table_budget(ecgpu_ctx *ctx, size_t max_table_bytes);

/* The comb table `curve` uses on this context right now: its window width (0 = none built yet), its bytes of device memory and
 * the wall time its construction took (whichever context of the device paid it).  Any of the three pointers may be NULL. */
int ecgpu_base_table_info(ecgpu_ctx *ctx, int curve, int *window_bits, size_t *table_bytes, double *build_ms);

/* Pins the width for later generator multiplications on `curve` to exactly window_bits (4..26), whatever the policy and the
 * budget; 0 returns the curve to the policy.  The table is rebuilt on next use.  A tuning knob, like the reference's WINDOW_SIZE
 * constants (k256/src/arithmetic/tables.rs:12, p384/src/arithmetic/tables.rs:8). */
int ecgpu_set_base_window(ecgpu_ctx *ctx, int curve, int window_bits);

/* Pippenger window width c for later ecgpu_msm* calls (4..16), 0 = choose from n (default). */
int ecgpu_set_msm_window(ecgpu_ctx *ctx, int window_bits);

/* Asynchronous mode for the device-pointer (`_dev`) entry points.  on != 0: a `_dev` call returns ECGPU_OK as soon as its
 * kernels are queued on the context's stream — argument errors are still reported at once — and the input checks
 * (ECGPU_ERR_SCALAR_RANGE, ECGPU_ERR_POINT) of all calls since the last ecgpu_synchronize are reported by the next
 * ecgpu_synchronize (outputs of the offending call are then unspecified, as in the synchronous mode).  Back-to-back batches
 * keep the GPU busy instead of paying a host round trip per call (0.70 -> 0.67 ms per 2^20-scalar fixed-base batch).
 * Buffers handed to a queued call must stay valid until ecgpu_synchronize.  ecgpu_last_timing waits for the stream.
 * Host-pointer entry points stay synchronous: on an asynchronous context they first wait for the queued work, whose
 * errors stay deferred.  ecgpu_set_async itself synchronises and returns what ecgpu_synchronize would.
 * ecgpu_synchronize on a synchronous context just waits for the stream. */
int ecgpu_set_async(ecgpu_ctx *ctx, int on);
int ecgpu_synchronize(ecgpu_ctx *ctx);

/* MSM lanes: with lanes = 2 .. 4 on an asynchronous context, consecutive ecgpu_msm_dev calls rotate over that many internal
 * streams, each with a workspace of its own, so that several independent MSMs are in flight: the sort and the reduction tail of
 * one (bandwidth- and latency-bound) run beside the accumulation of the other (issue-bound) — 8-12 % more MSMs per second on
 * one GPU (profiles/r03/msm_lanes.txt); the time of a single MSM does not change.  A lane starts after the work queued on
 * the context's stream at the time of the call (its inputs).  Ordering rules while MSMs are in flight on the lanes:
 *   - every MSM in flight needs output buffers of its own, and its INPUT buffers must stay untouched until it has finished;
 *   - any other entry point called later on this context (a batch call, ecgpu_point_sum_dev, ecgpu_copy_to_host, ...) first
 *     waits for all lanes, so it may read an MSM's output or overwrite its inputs;
 *   - a further ecgpu_msm_dev does NOT wait (that is the point), and neither does work the caller enqueues itself on the
 *     context's stream (ecgpu_set_stream): for those, inputs and outputs belong to the lanes until ecgpu_synchronize.
 * lanes = 1 (the default) restores one stream.  Synchronous contexts are unaffected.  Returns ECGPU_ERR_ARG for other values. */
int ecgpu_set_msm_lanes(ecgpu_ctx *ctx, int lanes);

/* Zeroes every staging and scratch buffer the context owns on the device (inputs copied in by host-pointer calls, projective
 * results, batch-inversion products, signature scratch, MSM workspaces) and waits for it.  The uniform-schedule (`_ct`) entry
 * points do this by themselves for what they touch — the reference keeps secret scalars and shared secrets in
 * zeroize-on-drop types (`NonZeroScalar`, `SharedSecret`) —; a caller that has passed secrets through a variable-time name
 * (private keys to ecgpu_batch_mul_base) calls this before it lets go of the context.  Buffers the CALLER allocated
 * (ecgpu_dev_alloc, ecgpu_host_alloc, torch tensors) are the caller's to wipe.  Basepoint tables are public data and stay. */
int ecgpu_wipe(ecgpu_ctx *ctx);

/* ---- host-pointer entry points (copy in, compute on the GPU, copy out) ------------------------ */

/* out[i] = k[i] * G.
 * Batch form of `ProjectivePoint::mul_by_generator` (k256/src/arithmetic/mul.rs:180-203) and
 * `MulBackend::mul_by_generator` (primeorder/src/mul_backend.rs:15-17,
 * p256/src/arithmetic/tables.rs:33-43), followed by `to_affine`. */
int ecgpu_batch_mul_base(ecgpu_ctx *ctx, int curve, const uint8_t *scalars, size_t n,
                         uint8_t *out_xy, uint8_t *out_inf);

/* The same with SEC1-compressed output, split in two arrays: out_x[i] = x of k[i] * G (L bytes), out_tag[i] = 0x02 / 0x03
 * (y even / odd), 0x00 with x = 0 for the identity — tag || x is `to_sec1_point(true)` (primeorder/src/affine.rs:387-401,
 * k256/src/arithmetic/affine.rs:341), what `PublicKey::to_sec1_bytes` ships.  Half the bytes of the x || y form come
 * back over PCIe, which is what bounds the host-pointer rate. */
int ecgpu_batch_mul_base_compressed(ecgpu_ctx *ctx, int curve, const uint8_t *scalars, size_t n, uint8_t *out_x,
                                    uint8_t *out_tag);

/* out[i] = k[i] * P[i].
 * Batch form of `impl Mul<Scalar> for ProjectivePoint` (k256/src/arithmetic/mul.rs:249-274,
 * primeorder/src/projective.rs:847-886) / `MulVartime` (:888-921), followed by `to_affine`. */
int ecgpu_batch_mul(ecgpu_ctx *ctx, int curve, const uint8_t *scalars, const uint8_t *points_xy,
                    const uint8_t *points_inf, size_t n, uint8_t *out_xy, uint8_t *out_inf);

/* out = sum_i k[i] * P[i].
 * `LinearCombination<[(ProjectivePoint, Scalar)]>::{lincomb, lincomb_vartime}`
 * (k256/src/arithmetic/mul.rs:84-109, primeorder/src/projective.rs:480-511); n == 0 gives the
 * identity. out_xy holds 2L bytes, out_inf one byte. */
int ecgpu_msm(ecgpu_ctx *ctx, int curve, const uint8_t *scalars, const uint8_t *points_xy,
              const uint8_t *points_inf, size_t n, uint8_t *out_xy, uint8_t *out_inf);

/* out[i] = a[i] * G + b[i] * P[i].
 * Batch form of `MulByGeneratorVartime::mul_by_generator_and_mul_add_vartime`
 * (primeorder/src/mul_backend.rs:29-40, k256/src/arithmetic/mul.rs:303-310) — the ECDSA/Schnorr
 * verification shape. */
int ecgpu_batch_mul_base_and_mul_add(ecgpu_ctx *ctx, int curve, const uint8_t *a_scalars,
                                     const uint8_t *b_scalars, const uint8_t *points_xy,
                                     const uint8_t *points_inf, size_t n, uint8_t *out_xy,
                                     uint8_t *out_inf);

/* Projective -> affine for n points.
 * `BatchNormalize::batch_normalize` (k256/src/arithmetic/projective.rs:367-391,
 * primeorder/src/projective.rs:452-478). */
int ecgpu_batch_normalize(ecgpu_ctx *ctx, int curve, const uint8_t *points_xyz, size_t n,
                          uint8_t *out_xy, uint8_t *out_inf);

/* ---- device-pointer entry points ------------------------------------------------------------- *
 * Same semantics, all buffers already resident in this context's device memory (e.g. torch CUDA
 * tensors' data_ptr()).  Work is enqueued on the context stream; the call returns after the
 * status word has been read back (one small D2H copy + stream sync), so errors are reported
 * synchronously exactly like the host-pointer forms.  The context stream is a non-blocking stream of its own: inputs
 * written by work on another stream (torch's current stream, the legacy default stream) are NOT ordered before these
 * calls — either make that stream the context's with ecgpu_set_stream, or synchronise it first. */

int ecgpu_batch_mul_base_dev(ecgpu_ctx *ctx, int curve, const void *d_scalars, size_t n,
                             void *d_out_xy, void *d_out_inf);
int ecgpu_batch_mul_base_compressed_dev(ecgpu_ctx *ctx, int curve, const void *d_scalars, size_t n, void *d_out_x,
                                        void *d_out_tag);
int ecgpu_batch_mul_dev(ecgpu_ctx *ctx, int curve, const void *d_scalars, const void *d_points_xy,
                        const void *d_points_inf, size_t n, void *d_out_xy, void *d_out_inf);
int ecgpu_msm_dev(ecgpu_ctx *ctx, int curve, const void *d_scalars, const void *d_points_xy,
                  const void *d_points_inf, size_t n, void *d_out_xy, void *d_out_inf);
int ecgpu_batch_mul_base_and_mul_add_dev(ecgpu_ctx *ctx, int curve, const void *d_a_scalars,
                                         const void *d_b_scalars, const void *d_points_xy,
                                         const void *d_points_inf, size_t n, void *d_out_xy,
                                         void *d_out_inf);
int ecgpu_batch_normalize_dev(ecgpu_ctx *ctx, int curve, const void *d_points_xyz, size_t n,
                              void *d_out_xy, void *d_out_inf);

/* Sum of n affine points (out = P[0] + ... + P[n-1]) — the combine step of a sharded MSM:
 * each GPU's partial `lincomb` result is all-gathered and added here.
 * Uses the same `Add` as `impl Sum for ProjectivePoint` (k256 projective.rs, primeorder
 * projective.rs `Sum` impls). */
int ecgpu_point_sum(ecgpu_ctx *ctx, int curve, const uint8_t *points_xy, const uint8_t *points_inf,
                    size_t n, uint8_t *out_xy, uint8_t *out_inf);
int ecgpu_point_sum_dev(ecgpu_ctx *ctx, int curve, const void *d_points_xy,
                        const void *d_points_inf, size_t n, void *d_out_xy, void *d_out_inf);

/* ---- an MSM whose terms are spread over several GPUs ------------------------------------------------ *
 * sum_i k_i P_i = sum over GPUs of the sum over that GPU's terms, and the bucket method is linear up to its last step:
 * every GPU runs the pipeline on its own terms down to the per-window partial sums ("parts", ecgpu_msm_parts_bytes bytes of
 * opaque internal-form points — 41 KiB for k256 at c = 16), the parts are exchanged (one all-gather: RCCL over xGMI in a
 * torch.distributed job, peer copies inside ecgpu_group_msm), and ONE combining step — window sums over all GPUs, then the
 * chain of doublings over the windows — produces the result.  The serial tail of the method runs once, not once per GPU
 * plus a point sum.  `plan_terms` is the term count the window width is chosen from and must be the same on every GPU
 * (at least the largest shard); so must ecgpu_set_msm_window.  `lincomb` semantics as for ecgpu_msm_dev. */
size_t ecgpu_msm_parts_bytes(ecgpu_ctx *ctx, int curve, size_t plan_terms);
/* The Pippenger window width (bits) the two halves use for `plan_terms` on this context — ecgpu_set_msm_window's override
 * or the measured default; every GPU of a sharded MSM must report the same value (ecgpu_group_msm_dev checks it).
 * 0 for an unknown curve id. */
int ecgpu_msm_plan_window(ecgpu_ctx *ctx, int curve, size_t plan_terms);
int ecgpu_msm_parts_dev(ecgpu_ctx *ctx, int curve, const void *d_scalars, const void *d_points_xy, const void *d_points_inf,
                        size_t n, size_t plan_terms, void *d_parts);
/* Throughput form for back-to-back sharded MSMs: on an asynchronous context (ecgpu_set_async) with ecgpu_set_msm_lanes(L > 1),
 * ecgpu_msm_parts_dev runs on one of L rotating internal streams + workspaces, ordered after what the context's stream holds at
 * the call (the inputs) — so the exchange and the combining half of MSM i - 1, which the caller keeps on the context's stream,
 * run beside the accumulation of MSM i:
 *     ecgpu_msm_parts_dev(i, d_parts[i % L]);
 *     ecgpu_msm_parts_join_dev(d_parts[(i - 1) % L]);  all-gather(i - 1);  ecgpu_msm_finish_dev(i - 1);
 * ecgpu_msm_parts_join_dev makes the context's stream wait (on the device; the host does not) for the local half that wrote
 * `d_parts`; until then the record belongs to its lane.  A no-op for a record written on the context's own stream.  A lane keeps
 * track of ONE record: a local half that is still un-joined when its lane comes around again (more halves in flight than lanes) is
 * joined by that call — correct, but the context's stream then waits for it.
 * ecgpu_msm_finish_dev waits only for the local halves in flight whose records lie inside its nranks records at d_parts_all
 * (the one-rank form, parts -> finish on the same record, needs no join); ecgpu_msm_parts_join_dev is still required before the
 * caller's own exchange reads a record.  One MSM alone gains nothing from lanes. */
int ecgpu_msm_parts_join_dev(ecgpu_ctx *ctx, const void *d_parts);
/* d_parts_all: nranks consecutive parts records (the all-gather's output). */
int ecgpu_msm_finish_dev(ecgpu_ctx *ctx, int curve, const void *d_parts_all, int nranks, size_t plan_terms, void *d_out_xy,
                         void *d_out_inf);

/* ---- all GPUs of a node from ONE process (`ecgpu_init(ctx**, devices, ndev)`; 8e) --------------------- *
 * A group owns one context per listed device and runs one worker thread per device for the duration of a call: what a
 * single-process caller — the Rust `lincomb` of the reference, which knows nothing about ranks — uses to reach the 8 GPUs
 * of a node.  (A torch.distributed job with one process per GPU uses ecgpu_msm_parts_dev / ecgpu_msm_finish_dev and its own
 * collective instead: bench.py.)  A device may be listed more than once (independent contexts; how the exchange is tested
 * on a one-GPU box).  Batch calls cut the index range into one contiguous slice per GPU and need no exchange; the MSM
 * cuts the terms the same way, runs ecgpu_msm_parts_dev per GPU and has ONE exchange step: RCCL ncclAllGather of the
 * per-window partial sums over xGMI when librccl can be dlopen()ed and the devices are distinct, a peer copy into
 * GPU 0 otherwise or after ecgpu_group_set_exchange(ECGPU_EXCHANGE_PEER); then ecgpu_msm_finish_dev once.
 * Results are identical to the single-GPU calls.  Not thread-safe: one call at a time per group. */
typedef struct ecgpu_group ecgpu_group;
int ecgpu_group_init(ecgpu_group **group, const int *devices, int ndev);
void ecgpu_group_destroy(ecgpu_group *group);
int ecgpu_group_size(const ecgpu_group *group);
ecgpu_ctx *ecgpu_group_ctx(ecgpu_group *group, int i);              /* borrowed: member i's context */
const char *ecgpu_group_last_error(const ecgpu_group *group);
const char *ecgpu_group_exchange(const ecgpu_group *group);         /* "rccl" or "peer" */
/* why: "rccl: ncclCommInitAll over 8 devices", "peer: ecgpu_group_set_exchange(ECGPU_EXCHANGE_PEER)", "peer: duplicate devices in the group",
 * "peer: librccl could not be loaded (...)", "peer: ncclCommInitAll failed (...)", "peer: ncclAllGather failed (...)": a
 * group whose RCCL exchange fails at run time falls back to peer copies for that call and all later ones */
const char *ecgpu_group_exchange_reason(const ecgpu_group *group);
/* Choose the exchange of an initialised group.  ECGPU_EXCHANGE_PEER: peer copies from now on (the communicators are released);
 * ECGPU_EXCHANGE_RCCL: ECGPU_OK if the group exchanges over RCCL, ECGPU_ERR_HIP if it does not (a caller who wants "RCCL or
 * nothing" instead of the silent fallback; the reason is in ecgpu_group_last_error).  The library reads no environment variable. */
enum { ECGPU_EXCHANGE_PEER = 1, ECGPU_EXCHANGE_RCCL = 2 };
int ecgpu_group_set_exchange(ecgpu_group *group, int mode);
int ecgpu_group_set_msm_window(ecgpu_group *group, int window_bits);
/* The exchange step of ecgpu_group_msm* never waits longer than this (default 10 s; seconds > 0): every member polls its exchange
 * stream against the deadline instead of blocking on it.  A collective that fails on any member, or has not completed by then
 * (the way RCCL has failed on this hardware is a hang, not an error code), is given up — communicators aborted (ncclCommAbort),
 * fresh exchange streams — and the call completes over peer copies, as do all later calls; ecgpu_group_exchange_reason reports it.
 * ECGPU_ERR_HIP only if the peer copies miss the deadline too. */
int ecgpu_group_set_exchange_timeout(ecgpu_group *group, double seconds);
/* `lincomb` over all GPUs of the group, host buffers (every GPU uploads its own shard over its own PCIe link). */
int ecgpu_group_msm(ecgpu_group *group, int curve, const uint8_t *scalars, const uint8_t *points_xy,
                    const uint8_t *points_inf, size_t n, uint8_t *out_xy, uint8_t *out_inf);
/* The same with the shards already resident: d_scalars[i] / d_points_xy[i] / d_points_inf[i] (the array or any entry may be
 * NULL) live on member i's device and hold n_per_device[i] terms; out_xy / out_inf are host buffers. */
int ecgpu_group_msm_dev(ecgpu_group *group, int curve, const void *const *d_scalars, const void *const *d_points_xy,
                        const void *const *d_points_inf, const size_t *n_per_device, uint8_t *out_xy, uint8_t *out_inf);
/* ecgpu_batch_mul_base / ecgpu_batch_mul over all GPUs of the group (index-range slices, no exchange). */
int ecgpu_group_batch_mul_base(ecgpu_group *group, int curve, const uint8_t *scalars, size_t n, uint8_t *out_xy,
                               uint8_t *out_inf);
int ecgpu_group_batch_mul(ecgpu_group *group, int curve, const uint8_t *scalars, const uint8_t *points_xy,
                          const uint8_t *points_inf, size_t n, uint8_t *out_xy, uint8_t *out_inf);

/* ecgpu_ecdsa_verify_batch / ecgpu_ecdsa_verify_msg_batch / ecgpu_ecdsa_recover_batch over all GPUs of the group (index-range
 * slices, no exchange; host buffers). */
int ecgpu_group_ecdsa_verify_batch(ecgpu_group *group, int curve, const uint8_t *z, const uint8_t *r, const uint8_t *s,
                                   const uint8_t *q_xy, size_t n, int reject_high_s, uint8_t *ok);
int ecgpu_group_ecdsa_verify_msg_batch(ecgpu_group *group, int curve, const uint8_t *q_xy, const uint8_t *msgs, size_t msg_len,
                                       const uint8_t *sigs, size_t n, int reject_high_s, uint8_t *ok);
int ecgpu_group_ecdsa_recover_batch(ecgpu_group *group, int curve, const uint8_t *z, const uint8_t *r, const uint8_t *s,
                                    const uint8_t *recid, size_t n, int reject_high_s, uint8_t *out_xy, uint8_t *ok);

/* ---- introspection / measurement ---------------------------------------------------------------- */

/* k256 GLV split on the device: k -> (r1, r2) with r1 + r2*lambda = k (mod n), canonical scalars
 * before sign folding — `glv::decompose_scalar` (k256/src/arithmetic/mul/glv.rs:149-156).
 * Host buffers of n*32 bytes each. */
int ecgpu_k256_glv_decompose(ecgpu_ctx *ctx, const uint8_t *scalars, size_t n, uint8_t *r1,
                             uint8_t *r2);

/* Batch ECDSA verification — SURVEY.md §8(f) rank 1, the dominant caller of
 * `mul_by_generator_and_mul_add_vartime` (primeorder/src/mul_backend.rs:29-40, k256/src/arithmetic/mul.rs:303-310).
 * The equation is `ecdsa::hazmat::verify_prehashed` (ecdsa 0.17.0, un-vendored, Cargo.lock:428-429; instantiated
 * at p256/src/ecdsa.rs:69, p384/src/ecdsa.rs, k256/src/ecdsa.rs:104-106), i.e. SEC1 v2 §4.1.4.  Per element i:
 *   z  L bytes big-endian: the leftmost L bytes of the message digest as an integer (`bits2field`); it is
 *      reduced mod n on the device like `Scalar::reduce`
 *   r, s  L bytes big-endian each; q_xy  the public key, affine x||y
 *   ok[i] = 1 iff 1 <= r, s < n, (reject_high_s == 0 or s <= (n-1)/2 — pass the curve's `NORMALIZE_S`,
 *      true for k256), Q is a valid non-identity curve point, R = (z/s) G + (r/s) Q is not the identity and
 *      x(R) mod n == r;  otherwise 0.  A bad element never fails the batch: the return value reports only
 *      argument / device errors. */
int ecgpu_ecdsa_verify_batch(ecgpu_ctx *ctx, int curve, const uint8_t *z, const uint8_t *r,
                             const uint8_t *s, const uint8_t *q_xy, size_t n, int reject_high_s,
                             uint8_t *ok);
int ecgpu_ecdsa_verify_batch_dev(ecgpu_ctx *ctx, int curve, const void *d_z, const void *d_r,
                                 const void *d_s, const void *d_q_xy, size_t n, int reject_high_s,
                                 void *d_ok);

/* Batch ECDSA verification of messages — `signature::Verifier::verify(msg, &signature)` of `ecdsa::VerifyingKey<C>`: the
 * curve's digest (the reference's `DigestAlgorithm`: SHA-256 for k256 / p256 / brainpoolP256 — k256/src/ecdsa.rs:117-119,
 * p256/src/ecdsa.rs:72-74 —, SHA-384 for p384 / brainpoolP384, SHA-224 for p224, SHA-512 for p521) is computed on the device,
 * z = bits2field(digest) (the leftmost L bytes, left-padded when the digest is shorter), then ecgpu_ecdsa_verify_batch.
 * The reference's message-level vectors: its Wycheproof blobs (k256/src/ecdsa.rs:263-384 and the new_wycheproof_test! calls).
 *   q_xy n*2L bytes, msgs n*msg_len bytes (one uniform length per call, 0 allowed), sigs n*2L bytes (r || s, the fixed-size
 *   `Signature::from_slice` form; DER is parsed by the caller).  ECGPU_ERR_CURVE for p192 (no DigestAlgorithm), sm2, bign256. */
int ecgpu_ecdsa_verify_msg_batch(ecgpu_ctx *ctx, int curve, const uint8_t *q_xy, const uint8_t *msgs, size_t msg_len,
                                 const uint8_t *sigs, size_t n, int reject_high_s, uint8_t *ok);
int ecgpu_ecdsa_verify_msg_batch_dev(ecgpu_ctx *ctx, int curve, const void *d_q_xy, const void *d_msgs, size_t msg_len,
                                     const void *d_sigs, size_t n, int reject_high_s, void *d_ok);

/* Batch ECDSA public-key recovery — `VerifyingKey::recover_from_prehash(prehash, &signature, recovery_id)` of the `ecdsa`
 * crate (0.17.0, un-vendored, Cargo.lock:428-429), which k256 / p256 re-export and the reference tests with its own vectors
 * (k256/src/ecdsa.rs:170-262: RECOVERY_TEST_VECTORS and the Ethereum example; p256/tests/ecdsa.rs:20-25).  It is a caller
 * of `ProjectivePoint::lincomb(&[(G, u1), (R, u2)])`.  Per element i (SEC1 v2 4.1.6 for ONE candidate):
 *   z, r, s  as for ecgpu_ecdsa_verify_batch
 *   recid    one byte, `RecoveryId::to_byte`: bit 0 = y(R) is odd, bit 1 = x(R) = r + n ("x reduced"); > 3 does not parse
 *   R = decompress(r or r + n, bit 0);  key = -(z/r) G + (s/r) R
 *   ok[i] = 1 and out_xy[i] = the key (affine x||y) iff 1 <= r, s < n, (reject_high_s == 0 or s <= (n-1)/2: the
 *      `verify_prehash` the crate runs on the recovered key applies the curve's NORMALIZE_S — pass 1 for k256), recid <= 3,
 *      the candidate x is below p and on the curve, and the key is not the identity;  otherwise ok[i] = 0 and a zero record.
 * ECGPU_ERR_CURVE for sm2 / bign256 (not ECDSA). */
int ecgpu_ecdsa_recover_batch(ecgpu_ctx *ctx, int curve, const uint8_t *z, const uint8_t *r,
                              const uint8_t *s, const uint8_t *recid, size_t n, int reject_high_s,
                              uint8_t *out_xy, uint8_t *ok);
int ecgpu_ecdsa_recover_batch_dev(ecgpu_ctx *ctx, int curve, const void *d_z, const void *d_r,
                                  const void *d_s, const void *d_recid, size_t n, int reject_high_s,
                                  void *d_out_xy, void *d_ok);

/* Batch BIP340 Schnorr verification over secp256k1 — `VerifyingKey::verify_raw`
 * (k256/src/schnorr/verifying.rs:76-99) without the hash: per element
 *   e  32 bytes big-endian = tagged_hash("BIP0340/challenge", r || pk || m), computed by the caller; reduced
 *      mod n on the device like `<Scalar as Reduce<FieldBytes>>::reduce`
 *   r, s  the two halves of the signature (k256/src/schnorr.rs:132-150: r < p, 0 < s < n)
 *   p_xy  the verifying key's affine point, i.e. the even-y lift of the 32-byte public key
 *      (`VerifyingKey::from_bytes`; use ecgpu_batch_decompress with y_is_odd = 0)
 *   ok[i] = 1 iff the fields are in range, P is on the curve, R = s G - e P is not the identity, y(R) is even
 *      and x(R) == r. */
int ecgpu_schnorr_verify_batch(ecgpu_ctx *ctx, const uint8_t *e, const uint8_t *r, const uint8_t *s,
                               const uint8_t *p_xy, size_t n, uint8_t *ok);
int ecgpu_schnorr_verify_batch_dev(ecgpu_ctx *ctx, const void *d_e, const void *d_r, const void *d_s,
                                   const void *d_p_xy, size_t n, void *d_ok);

/* Batch SM2DSA verification on the prehash — `PrehashVerifier::verify_prehash` of sm2::dsa::VerifyingKey
 * (sm2/src/dsa/verifying.rs:138-171; GB/T 32918.2, draft-shen-sm2-ecdsa 5.3), curve sm2 only.  Per element
 *   e     32 bytes big-endian = SM3(ZA || M), computed by the caller (ZA hashes the signer's identity and key,
 *         sm2/src/dsa.rs); reduced mod n on the device like `Scalar::reduce`
 *   r, s  the signature halves, q_xy the public key's affine point
 *   ok[i] = 1 iff 1 <= r, s < n, t = r + s mod n != 0, Q is a valid non-identity curve point and
 *         r == e + x(s G + t Q) mod n   (the `lincomb` at verifying.rs:161). */
int ecgpu_sm2dsa_verify_batch(ecgpu_ctx *ctx, const uint8_t *e, const uint8_t *r, const uint8_t *s, const uint8_t *q_xy,
                              size_t n, uint8_t *ok);
int ecgpu_sm2dsa_verify_batch_dev(ecgpu_ctx *ctx, const void *d_e, const void *d_r, const void *d_s, const void *d_q_xy,
                                  size_t n, void *d_ok);

/* SM2DSA verification of messages — `sm2::dsa::VerifyingKey::new(distid, public_key)?.verify(msg, &signature)`: the identity
 * hash Z = SM3(ENTL || ID || a || b || xG || yG || xA || yA) (`hash_z`, sm2/src/distid.rs:21-44) and e = SM3(Z || M)
 * (`hash_msg`, sm2/src/dsa/verifying.rs:126-130) are computed on the device, then the verification above.  The reference's
 * message-level vector: sm2/tests/sm2dsa.rs:16-35.
 *   distid  the signers' distinguishing identifier, distid_len <= 8191 bytes (ENTL is a 16-bit bit count), one per call
 *   q_xy    n*64 bytes, msgs n*msg_len bytes (one uniform length per call, 0 allowed), sigs n*64 bytes (r || s)
 *   ok[i] as for ecgpu_sm2dsa_verify_batch. */
int ecgpu_sm2dsa_verify_msg_batch(ecgpu_ctx *ctx, const uint8_t *distid, size_t distid_len, const uint8_t *q_xy,
                                  const uint8_t *msgs, size_t msg_len, const uint8_t *sigs, size_t n, uint8_t *ok);
int ecgpu_sm2dsa_verify_msg_batch_dev(ecgpu_ctx *ctx, const void *d_distid, size_t distid_len, const void *d_q_xy,
                                      const void *d_msgs, size_t msg_len, const void *d_sigs, size_t n, void *d_ok);

/* Batch bign verification on the prehash — `PrehashVerifier::verify_prehash` of bignp256::ecdsa::VerifyingKey
 * (bignp256/src/ecdsa/verifying.rs:100-155; STB 34.101.45-2013 §7.2), curve bign256 only.  Everything is little-endian, as
 * the crate's `FIELD_ENDIANNESS` (bignp256/src/lib.rs:90).  Per element
 *   h     32 bytes = belt-hash(message), as `verify_prehash` takes it (reduced mod q like `Scalar::reduce`)
 *   sigs  48 bytes S0 (16) || S1 (32) — `Signature::from_bytes`, bignp256/src/ecdsa.rs:72-88
 *   q_xy  the public key's affine point, 64 bytes
 *   ok[i] = 1 iff S0 != 0, 0 < S1 < q, Q is a valid non-identity curve point, R = ((S1 + H) mod q) G + (S0 + 2^128) Q is
 *         finite (the `lincomb` at verifying.rs:119-122) and S0 equals the first 16 bytes of
 *         belt-hash(OID(belt-hash) || x(R) as 32 bytes || h), hashed on the device (csrc/ecgpu_belt.h).
 * The reference's vector: bignp256/tests/ecdsa.rs:21-46. */
int ecgpu_bign_verify_batch(ecgpu_ctx *ctx, const uint8_t *h, const uint8_t *sigs, const uint8_t *q_xy, size_t n,
                            uint8_t *ok);
int ecgpu_bign_verify_batch_dev(ecgpu_ctx *ctx, const void *d_h, const void *d_sigs, const void *d_q_xy, size_t n,
                                void *d_ok);

/* bign verification of messages — `VerifyingKey::from_bytes(pk)?.verify(msg, &signature)` (bignp256/src/ecdsa/verifying.rs:
 * 157-169): h = belt-hash(msg) (`hash_msg`, :87-91) on the device, then the verification above.
 *   q_xy n*64 bytes, msgs n*msg_len bytes (one uniform length per call, 0 allowed), sigs n*48 bytes. */
int ecgpu_bign_verify_msg_batch(ecgpu_ctx *ctx, const uint8_t *q_xy, const uint8_t *msgs, size_t msg_len,
                                const uint8_t *sigs, size_t n, uint8_t *ok);
int ecgpu_bign_verify_msg_batch_dev(ecgpu_ctx *ctx, const void *d_q_xy, const void *d_msgs, size_t msg_len,
                                    const void *d_sigs, size_t n, void *d_ok);

/* The same verification from wire bytes — `VerifyingKey::from_bytes(pk)?.verify_raw(msg, sig)`
 * (k256/src/schnorr/verifying.rs:76-99,149-160): pk_x n*32 bytes (x-only keys, lifted on the device with even y),
 * msgs n*msg_len bytes (one uniform length per call, 0 allowed), sigs n*64 bytes (r || s).  The challenge
 * e = tagged_hash("BIP0340/challenge", r || pk || msg) is computed on the device (SHA-256).  ok[i] = 0 for keys that do
 * not lift, out-of-range signature halves, and signatures that do not verify. */
int ecgpu_schnorr_verify_raw_batch(ecgpu_ctx *ctx, const uint8_t *pk_x, const uint8_t *msgs, size_t msg_len,
                                   const uint8_t *sigs, size_t n, uint8_t *ok);
int ecgpu_schnorr_verify_raw_batch_dev(ecgpu_ctx *ctx, const void *d_pk_x, const void *d_msgs,
                                       size_t msg_len, const void *d_sigs, size_t n, void *d_ok);

/* Batch ECDH — `elliptic_curve::ecdh::diffie_hellman(secret, public)` (elliptic-curve 0.14.1, un-vendored; the
 * curves re-export it: k256/src/ecdh.rs, p256/src/ecdh.rs, p384/src/ecdh.rs): out_x[i] = the x-coordinate of
 * k_i * P_i as L big-endian bytes (`SharedSecret::raw_secret_bytes`), ok[i] = 1 unless the product is the identity
 * (k_i = 0).  Scalars >= n and points off the curve fail the call like ecgpu_batch_mul. */
int ecgpu_batch_ecdh(ecgpu_ctx *ctx, int curve, const uint8_t *scalars, const uint8_t *points_xy,
                     size_t n, uint8_t *out_x, uint8_t *ok);
int ecgpu_batch_ecdh_dev(ecgpu_ctx *ctx, int curve, const void *d_scalars, const void *d_points_xy,
                         size_t n, void *d_out_x, void *d_ok);

/* ---- uniform-schedule ("constant-time shaped") variants for SECRET scalars --------------------------------------------
 * Same arguments, results and error behaviour as ecgpu_batch_mul_base / ecgpu_batch_mul / ecgpu_batch_ecdh, computed by the
 * reference's constant-time algorithms (elliptic-curves_amd/csrc/ecgpu_ctmul.h):
 *   ecgpu_batch_mul_base_ct   `ProjectivePoint::mul_by_generator` (k256/src/arithmetic/mul.rs:180-197) /
 *                             `BasepointTable::mul` (primeorder/src/tables/basepoint.rs:82-99), with 6-bit windows where the
 *                             reference has nibbles: one LUT of the 32 multiples e 2^(6 i) G per window, one signed digit
 *                             and one complete mixed addition per window (43 for a 256-bit scalar), no doublings; every
 *                             LUT is scanned in full (`LookupTable::select`, primeorder/src/tables/lookup.rs:43-65)
 *   ecgpu_batch_mul_ct        `impl Mul<Scalar> for ProjectivePoint` (primeorder/src/projective.rs:847-886 -> `lincomb`
 *                             :532-557 with one term; k256/src/arithmetic/mul.rs:112-163,249-274 on the two GLV halves):
 *                             table [P..8P] by complete additions (lookup.rs:30-38), 65 / 97 (k256: 2 x 33) digits, four
 *                             doublings (complete ones on k256; Jacobian ones, which have no exceptional case on a
 *                             prime-order curve, with the identity patched under a mask elsewhere) and one complete
 *                             addition per digit, no digit skipped, the accumulator starts at the identity
 *   ecgpu_batch_ecdh_ct       `diffie_hellman(secret, public)` (k256/src/ecdh.rs:56-60 over the `Mul` above): x of
 *                             ecgpu_batch_mul_ct
 *   ecgpu_lincomb_ct          `LinearCombination::lincomb` (primeorder/src/projective.rs:484-496 -> :532-557;
 *                             k256/src/arithmetic/mul.rs:84-98 -> :112-163): out = sum_i k_i P_i with one ecgpu_batch_mul_ct
 *                             multiplication per term and a tree of complete additions over the n products (256 per workgroup
 *                             and level).  The reference interleaves the terms on one accumulator; the group element is the
 *                             same, and the instruction and memory schedule here is a function of n alone.  n == 0 gives the
 *                             identity.  Cost: n uniform-schedule multiplications — for PUBLIC scalars ecgpu_msm (the bucket
 *                             method) is 50-100x faster from a few thousand terms on
 * What is guaranteed, and checked on the gfx950 ISA of the two kernels by tools/ct_isa_check.py (a register-level taint
 * analysis from every loaded record to every branch condition and every memory address; tests/test_ct_isa.py): no
 * conditional branch and no load / store address depends on the contents of a scalar or point record; range and
 * on-curve verdicts are computed for every element and reported through the usual error codes after the kernel.
 * What is not: the conversion to affine output that follows branches on "the result is the identity" (k = 0 or
 * P = identity), as `to_affine` must distinguish that case for the wire format; power and clock side channels of the
 * device are outside what an ISA-level argument can cover.  Measured cost: DESIGN.md §7. */
int ecgpu_batch_mul_base_ct(ecgpu_ctx *ctx, int curve, const uint8_t *scalars, size_t n, uint8_t *out_xy, uint8_t *out_inf);
int ecgpu_batch_mul_base_ct_dev(ecgpu_ctx *ctx, int curve, const void *d_scalars, size_t n, void *d_out_xy, void *d_out_inf);
int ecgpu_batch_mul_ct(ecgpu_ctx *ctx, int curve, const uint8_t *scalars, const uint8_t *points_xy, const uint8_t *points_inf,
                       size_t n, uint8_t *out_xy, uint8_t *out_inf);
int ecgpu_batch_mul_ct_dev(ecgpu_ctx *ctx, int curve, const void *d_scalars, const void *d_points_xy, const void *d_points_inf,
                           size_t n, void *d_out_xy, void *d_out_inf);
int ecgpu_batch_ecdh_ct(ecgpu_ctx *ctx, int curve, const uint8_t *scalars, const uint8_t *points_xy, size_t n, uint8_t *out_x,
                        uint8_t *ok);
int ecgpu_batch_ecdh_ct_dev(ecgpu_ctx *ctx, int curve, const void *d_scalars, const void *d_points_xy, size_t n, void *d_out_x,
                            void *d_ok);
int ecgpu_lincomb_ct(ecgpu_ctx *ctx, int curve, const uint8_t *scalars, const uint8_t *points_xy, const uint8_t *points_inf,
                     size_t n, uint8_t *out_xy, uint8_t *out_inf);
int ecgpu_lincomb_ct_dev(ecgpu_ctx *ctx, int curve, const void *d_scalars, const void *d_points_xy, const void *d_points_inf,
                         size_t n, void *d_out_xy, void *d_out_inf);

/* ---- batch signing: ECDSA (the caller's nonce or RFC 6979) and BIP340 Schnorr ---------------------------------------------
 * The secret-scalar consumers of ecgpu_batch_mul_base_ct inside the library: every R = k G (and the Schnorr P = d G) is that
 * entry's kernel, and the kernels around it keep its rule — no branch and no address depends on a key, a nonce, a digest or
 * anything derived from them (tools/ct_isa_check.py --unit sign; tests/test_sign_isa.py).  k^-1 is one branch-free
 * division-step inversion per element.  Two pieces are variable-time, both on purpose: the RFC 6979 retry loop
 * (k_rfc6979_retry), whose trip count depends on the candidates it REJECTED — never used, and what the `loop` of the
 * reference's `generate_k` reveals — and, as for every entry point, `to_affine` of the public R.  Everything the call derives
 * from d, k or aux_rand on the device (the HMAC K / V state, nonces, projective and affine R, the staged copies of a
 * host-pointer call) is zeroed behind its last kernel, in stream order; ecgpu_wipe covers the same buffers.
 * An element that cannot be signed never fails the batch: it gets a zero record, recid 0 and ok[i] = 0, and its neighbours are
 * untouched.  Invalid keys and nonces are replaced under a mask, not branched on.
 *
 * ecgpu_ecdsa_sign_batch — the hazmat form with the caller's nonce: `ecdsa::hazmat::sign_prehashed` as `ecdsa_core::
 *   new_signing_test!` runs it (p256/src/ecdsa.rs:156-159).  d, k, z: n*L bytes each, big-endian; z = bits2field(prehash) is
 *   reduced mod n on the device as in ecgpu_ecdsa_verify_batch.  R = k G, r = x(R) mod n, s = k^-1 (z + r d) mod n.
 *   normalize_s != 0 is the curve's `NORMALIZE_S` (true for k256, k256/src/ecdsa.rs:104-106; false for p256): s > (n-1)/2
 *   becomes n - s and bit 0 of the recovery id flips.  out_sig: n*2L bytes r || s.  out_recid[i]: the byte
 *   ecgpu_ecdsa_recover_batch takes — bit 0 = y(R) odd, bit 1 = x(R) >= n.  ok[i] = 1 iff 1 <= d < n, 1 <= k < n, r != 0 and
 *   s != 0.  The ten ECDSA parameter sets; ECGPU_SM2 and ECGPU_BIGN256 return ECGPU_ERR_CURVE.
 * ecgpu_ecdsa_sign_rfc6979_batch — `PrehashSigner::sign_prehash` of `ecdsa::SigningKey<C>`: the nonce of RFC 6979 section 3.2
 *   generated on the device, HMAC over the curve's `DigestAlgorithm` (SHA-256: k256, p256, bp256; SHA-384: p384, bp384;
 *   SHA-224: p224; SHA-512: p521), x = d as L bytes, h1 = (z mod n) as L bytes, no additional data; a candidate is the first L
 *   bytes of T shifted right by 8L - bitlen(n) (7 bits for p521), accepted iff 1 <= k < n; after 128 rejected candidates
 *   ok[i] = 0.  ECGPU_ERR_CURVE also for ECGPU_P192 (no `DigestAlgorithm`, p192/src/ecdsa.rs).
 * ecgpu_ecdsa_sign_msg_batch — `Signer::sign(msg)`: the curve's digest of message i on the device (as in
 *   ecgpu_ecdsa_verify_msg_batch), z = bits2field(digest), then the RFC 6979 form.  msgs: n*msg_len bytes, one uniform length
 *   per call, 0 allowed.
 * ecgpu_schnorr_sign_raw_batch — `SigningKey::sign_raw(msg, aux_rand)` (k256/src/schnorr/signing.rs:97-137) with the key
 *   fix-up of `From<NonZeroScalar>` (:146-167); secp256k1 only.  sk n*32, msgs n*msg_len, aux_rand n*32 bytes, out_sig n*64
 *   bytes x(R) || s.  P = d G, d <- n - d if y(P) is odd, t = tagged_hash("BIP0340/aux", aux) ^ d, k = tagged_hash(
 *   "BIP0340/nonce", t || x(P) || msg) mod n, R = k G, k <- n - k if y(R) is odd, e = tagged_hash("BIP0340/challenge",
 *   x(R) || x(P) || msg) mod n, s = k + e d.  ok[i] = 0 for d = 0, d >= n, k = 0 or s = 0.
 * Device pointers: 16-byte aligned bases as everywhere.  Asynchronous contexts and deferred errors behave as for the other `_ct`
 * calls. */
int ecgpu_ecdsa_sign_batch(ecgpu_ctx *ctx, int curve, const uint8_t *d, const uint8_t *k, const uint8_t *z, size_t n,
                           int normalize_s, uint8_t *out_sig, uint8_t *out_recid, uint8_t *ok);
int ecgpu_ecdsa_sign_batch_dev(ecgpu_ctx *ctx, int curve, const void *d_d, const void *d_k, const void *d_z, size_t n,
                               int normalize_s, void *d_out_sig, void *d_out_recid, void *d_ok);
int ecgpu_ecdsa_sign_rfc6979_batch(ecgpu_ctx *ctx, int curve, const uint8_t *d, const uint8_t *z, size_t n, int normalize_s,
                                   uint8_t *out_sig, uint8_t *out_recid, uint8_t *ok);
int ecgpu_ecdsa_sign_rfc6979_batch_dev(ecgpu_ctx *ctx, int curve, const void *d_d, const void *d_z, size_t n, int normalize_s,
                                       void *d_out_sig, void *d_out_recid, void *d_ok);
int ecgpu_ecdsa_sign_msg_batch(ecgpu_ctx *ctx, int curve, const uint8_t *d, const uint8_t *msgs, size_t msg_len, size_t n,
                               int normalize_s, uint8_t *out_sig, uint8_t *out_recid, uint8_t *ok);
int ecgpu_ecdsa_sign_msg_batch_dev(ecgpu_ctx *ctx, int curve, const void *d_d, const void *d_msgs, size_t msg_len, size_t n,
                                   int normalize_s, void *d_out_sig, void *d_out_recid, void *d_ok);
int ecgpu_schnorr_sign_raw_batch(ecgpu_ctx *ctx, const uint8_t *sk, const uint8_t *msgs, size_t msg_len,
                                 const uint8_t *aux_rand, size_t n, uint8_t *out_sig, uint8_t *ok);
int ecgpu_schnorr_sign_raw_batch_dev(ecgpu_ctx *ctx, const void *d_sk, const void *d_msgs, size_t msg_len,
                                     const void *d_aux_rand, size_t n, void *d_out_sig, void *d_ok);

/* ---- batch SM2DSA signing (GB/T 32918.2 section 6.1): the signing half of `sm2::dsa` ---------------------------------------
 * The sm2 parameter set only, hence no `curve` argument (as for ecgpu_sm2dsa_verify_batch).  Everything the block above says
 * about the ECDSA calls holds here: R = k G (and PA = d G of the message form) is the kernel of ecgpu_batch_mul_base_ct; in the
 * kernels around it no branch and no address depends on d, k, e or anything derived from them
 * (tools/ct_isa_check.py --unit sm2sign; tests/test_sm2sign_isa.py); (1 + d)^-1 is one branch-free division-step inversion per
 * element; everything derived from d or k on the device (the nonces and their verdicts, e, projective and affine R, the staged
 * copies of d and k) is zeroed behind the last kernel in stream order, and ecgpu_wipe covers the same buffers.  An element that cannot be
 * signed never fails the batch: it gets a zero record and ok[i] = 0, and its neighbours are untouched.
 *     e = prehash mod n (`bytes2scalar`; exactly 32 bytes),  R = k G,  r = e + x(R) mod n,  s = (1 + d)^-1 (k - r d) mod n
 * out_sig: n*64 bytes r || s, big-endian.  There is no low-S rule and no recovery id.
 *
 * ecgpu_sm2dsa_sign_batch — the standard's steps A3-A7 with the caller's nonce.  THIS FORM IS OURS: the reference has no entry
 *   point that takes a nonce; it exists for callers with their own RNG and for the standard's known answer (GB/T 32918.5-2017
 *   Annex A).  d, k, e: n*32 bytes each.  ok[i] = 1 iff 1 <= d < n, d != n - 1 (1 + d has no inverse), 1 <= k < n, r != 0,
 *   r + k != 0 mod n and s != 0.
 * ecgpu_sm2dsa_sign_rfc6979_batch — `PrehashSigner::sign_prehash` (sm2/src/dsa/signing.rs:122-126, 213-258): the nonce of
 *   RFC 6979 section 3.2 over HMAC-SM3, x = d as 32 bytes, h1 = (e mod n) as 32 bytes, no additional data.  ONE candidate and no
 *   retry kernel: this follows the reference's single `fill_next_k` (its source carries a TODO for the loop) — a candidate
 *   outside [1, n) gives ok[i] = 0 and a zero record, where the ECDSA form above would try the next one.  One difference from
 *   the reference: k = 0 is refused here, the reference's `from_repr` would accept it (probability 2^-256).
 * ecgpu_sm2dsa_sign_msg_batch — `SigningKey::new(distid, sk)?.sign(msg)` (:81-88, 162-174): PA = d G, Z = SM3(ENTL || ID || a ||
 *   b || xG || yG || xA || yA) and e = SM3(Z || M) on the device, then the RFC 6979 form.  distid: distid_len <= 8191 bytes, one
 *   identifier per call (ECGPU_ERR_ARG above that); msgs: n*msg_len bytes, one uniform length per call, 0 allowed — the argument
 *   rules of ecgpu_sm2dsa_verify_msg_batch.
 * Out of scope: `RandomizedPrehashSigner` (32 bytes of additional data make the generator's HMAC message three blocks).
 * Host-pointer forms only, like the SM2 encryption calls below: there is no public `_dev` name yet (every chunk of a call reaches
 * the internal device-pointer pipeline through the staging path, from 2^19 elements on piece by piece under the transfers).  On
 * an asynchronous context a call first waits for the queued work and runs synchronously, as every host-pointer call does. */
int ecgpu_sm2dsa_sign_batch(ecgpu_ctx *ctx, const uint8_t *d, const uint8_t *k, const uint8_t *e, size_t n, uint8_t *out_sig,
                            uint8_t *ok);
int ecgpu_sm2dsa_sign_rfc6979_batch(ecgpu_ctx *ctx, const uint8_t *d, const uint8_t *e, size_t n, uint8_t *out_sig, uint8_t *ok);
int ecgpu_sm2dsa_sign_msg_batch(ecgpu_ctx *ctx, const uint8_t *distid, size_t distid_len, const uint8_t *d, const uint8_t *msgs,
                                size_t msg_len, size_t n, uint8_t *out_sig, uint8_t *ok);

/* ---- batch bign signing (STB 34.101.45-2013 section 7.1, l = 128): the signing half of `bignp256::ecdsa` ---------------------
 * bign-curve256v1 only, hence no `curve` argument (as for ecgpu_bign_verify_batch).  d, k, h: 32-byte LITTLE-endian records, as
 * every bign256 record; out_sig: n*48 bytes S0 (16) || S1 (32), the layout ecgpu_bign_verify_batch takes; ok: one byte per element.
 *     h = prehash mod q,  R = k G,  S0 = belt-hash(OID(h) || <x(R)>_256 || prehash)[..16],  S1 = k - h - (S0 + 2^128) d mod q
 * The prehash enters twice and NOT as the same value (bignp256/src/ecdsa/signing.rs:117-123, 141-144): the nonce generator and S1
 * use the prehash REDUCED mod q, the S0 hash absorbs the RAW 32 bytes.  The two differ exactly when the prehash is >= q as an
 * integer; both calls take any 32 bytes.
 * An element that cannot be signed never fails the batch: it gets a zero record and ok[i] = 0, and its neighbours are untouched.
 * Refused: d outside [1, q); a caller's k outside [1, q); S0 = 0 or S1 = 0 (`Signature::from_bytes`, bignp256/src/ecdsa.rs:85-87).
 * R = k G is the kernel of ecgpu_batch_mul_base_ct.  In the generator, load and finish kernels no branch and no address depends on
 * d, k, the prehash or anything derived from them (tools/ct_isa_check.py --unit bignsign; tests/test_bignsign_isa.py): belt's
 * S-box, which the generator looks up at secret indices, is computed there from byte permutes and bitwise selects over constants,
 * without a table in memory.  S0 hashes public values only (R can be recomputed from the signature and the public key) and uses
 * the table.  Everything derived from d or k on the device (the nonces and their verdicts, the generator's parked state, S0,
 * projective and affine R, the staged copies of d and k) is zeroed behind the last kernel in stream order, and ecgpu_wipe covers
 * the same buffers.
 *
 * ecgpu_bign_sign_batch - the standard's steps 3-7 with the caller's nonce.  THIS FORM IS OURS: the reference has no entry point
 *   that takes a nonce; it exists for known answers and for callers with their own RNG.  h: the prehash, any 32 bytes.
 * ecgpu_bign_sign_prehash_batch - `PrehashSigner::sign_prehash` (signing.rs:110-161): the nonce of STB 34.101.45 section 6.3.3
 *   (`bign_genk::KGenerator<BeltBlock>`), with additional data t empty, as the reference passes `&[]`:
 *       theta = belt-hash(OID(h) || <d>_256 || t),  r1 || r2 = <prehash mod q>_256,
 *       i = 1, 2, ...:  s = r1;  r1 = belt-block(s, theta) xor r2 xor <i>_128;  r2 = s;
 *       every fourth round r1 || r2 is a candidate, accepted if it is in (0, q).
 *   The retry rule: the first candidate (round 4) comes from a kernel of uniform schedule; an element whose candidate was rejected
 *   goes on in k_bign_genk_retry, which is launched once per call as k_rfc6979_retry is and is the one deliberately variable-time
 *   piece: its trip count follows the REJECTED candidates, never used.  With q > 2^256 - 2^129 that is one element in 2^130.  After 128
 *   rejected candidates the element gets ok = 0.
 * ecgpu_bign_sign_msg_batch - `Signer::try_sign` (signing.rs:164-176): H = belt-hash(message) on the device, then the prehash
 *   form.  msgs: n*msg_len bytes, one uniform length per call, 0 allowed.
 * Out of scope: additional data t (`bign_genk` with a non-empty t), public `_dev` names, ecgpu_group_* forms, the C++ mirror.
 * Host-pointer forms only, like the SM2DSA calls above: there is no public `_dev` name yet.  On an asynchronous context a call
 * first waits for the queued work and runs synchronously, as every host-pointer call does. */
int ecgpu_bign_sign_batch(ecgpu_ctx *ctx, const uint8_t *d, const uint8_t *k, const uint8_t *h, size_t n, uint8_t *out_sig,
                          uint8_t *ok);
int ecgpu_bign_sign_prehash_batch(ecgpu_ctx *ctx, const uint8_t *d, const uint8_t *h, size_t n, uint8_t *out_sig, uint8_t *ok);
int ecgpu_bign_sign_msg_batch(ecgpu_ctx *ctx, const uint8_t *d, const uint8_t *msgs, size_t msg_len, size_t n, uint8_t *out_sig,
                              uint8_t *ok);

/* ---- batch X448 (RFC 7748): Diffie-Hellman over Curve448, the `x448` crate --------------------------------------------------
 * Curve448 is not a short-Weierstrass curve: these calls take no `curve` argument, there is no id for it in the enum above, and no
 * generic entry point knows it.  Every record — scalar, u-coordinate, result — is 56 bytes, little-endian; ok: one byte per element.
 * The clamp: every scalar is clamped on the device, bytes[0] &= 252 and bytes[55] |= 128 (x448/src/lib.rs:122-126), and the clamped
 *   448-bit integer is used as it is, never reduced modulo the group order.  There is no unclamped form.
 * The point: any 56 bytes, taken modulo p = 2^448 - 2^224 - 1 (`FieldElement::from_bytes`, ed448-goldilocks/src/field/element.rs:370-372):
 *   u in [p, 2^448) is legal input.  Points on the twist go through like any other.
 * The result: U W^-1 of the Montgomery ladder (ed448-goldilocks/src/montgomery.rs:83-110,168-204) with 0^-1 = 0, canonical.  A
 *   result at infinity is the zero record: 56 zero bytes, and it is NOT an error of the multiplication.
 * The low-order rule is byte-wise: the checked form refuses an element exactly when the point's BYTES equal one of the three
 *   low-order records LOW_A (0), LOW_B (1), LOW_C (p - 1) (montgomery.rs:23-42,137-139); such an element gets ok[i] = 0 and the zero
 *   record, and its neighbours are untouched.  The two non-canonical aliases p (= 0) and p + 1 (= 1) are NOT refused: they give the
 *   zero record with ok[i] = 1, as the reference does.
 * Secrecy: scalars and results are secret (a shared secret is a key).  In k_x448_ladder no branch and no address depends on scalar
 *   bytes, ladder state or results (tools/ct_isa_check.py --unit x448; tests/test_x448_isa.py); the ladder state lives in registers
 *   only.  The staged copies of the scalars and of the results are zeroed behind the last kernel in stream order, and ecgpu_wipe
 *   covers the same buffers.  The caller's own arrays are the caller's to wipe.
 * n = 0 succeeds and touches nothing; a NULL array with n > 0 is ECGPU_ERR_ARG; without a context every call is ECGPU_ERR_ARG.
 *
 * ecgpu_x448_batch - `x448::x448(scalar, point)` (lib.rs:152-156), and equally `PublicKey::from_bytes` followed by
 *   `EphemeralSecret::diffie_hellman`: `None` there is ok[i] = 0 here.
 * ecgpu_x448_unchecked_batch - `x448::x448_unchecked` (lib.rs:159-163), and `diffie_hellman` on `from_bytes_unchecked`: the same
 *   without the low-order test; the three low-order records give the zero record.
 * ecgpu_x448_base_batch - `PublicKey::from(&EphemeralSecret)` (lib.rs:25-31): clamp, then the ladder on `GENERATOR` (u = 5), with
 *   the product by u as a product by a small constant.
 * Out of scope: a table-driven fixed base, Ed448 / Decaf448, ecgpu_group_* forms, the C++ mirror.
 * Host-pointer forms only, no `_dev` name yet.  From 2^19 elements a call is pipelined in pieces like every batch call; on an
 * asynchronous context a call first waits for the queued work and runs synchronously, as every host-pointer call does. */
int ecgpu_x448_batch(ecgpu_ctx *ctx, const uint8_t *scalars, const uint8_t *points_u, size_t n, uint8_t *out_u, uint8_t *ok);
int ecgpu_x448_unchecked_batch(ecgpu_ctx *ctx, const uint8_t *scalars, const uint8_t *points_u, size_t n, uint8_t *out_u);
int ecgpu_x448_base_batch(ecgpu_ctx *ctx, const uint8_t *scalars, size_t n, uint8_t *out_u);

/* The same two with projective points: point i is the record X || Y || Z of the wire format above (3L bytes, no flag array),
 * as the reference's `Mul<Scalar>` and `lincomb` take a `ProjectivePoint`.  For every input the results and the return code
 * are those of `to_affine` applied to each record followed by ecgpu_batch_mul_ct / ecgpu_lincomb_ct: X, Y or Z >= p, and a
 * record with Z != 0 and Y^2 Z != X^3 + a X Z^2 + b Z^3, fail the call with ECGPU_ERR_POINT; Z = 0 is the identity.  No
 * inversion: the per-term table starts from (X : Y : Z) by complete additions (k_xyz_mul_ct), and the verdicts are computed
 * for every record under the same rule as above — no branch and no address depends on X, Y or Z.  Host-pointer
 * ecgpu_batch_mul_ct_xyz runs the pipeline of ecgpu_batch_mul_ct from 2^19 points, with 3L-byte records. */
int ecgpu_batch_mul_ct_xyz(ecgpu_ctx *ctx, int curve, const uint8_t *scalars, const uint8_t *points_xyz, size_t n, uint8_t *out_xy,
                           uint8_t *out_inf);
int ecgpu_batch_mul_ct_xyz_dev(ecgpu_ctx *ctx, int curve, const void *d_scalars, const void *d_points_xyz, size_t n, void *d_out_xy,
                               void *d_out_inf);
int ecgpu_lincomb_ct_xyz(ecgpu_ctx *ctx, int curve, const uint8_t *scalars, const uint8_t *points_xyz, size_t n, uint8_t *out_xy,
                         uint8_t *out_inf);
int ecgpu_lincomb_ct_xyz_dev(ecgpu_ctx *ctx, int curve, const void *d_scalars, const void *d_points_xyz, size_t n, void *d_out_xy,
                             void *d_out_inf);

/* The variable-time forms with projective points: ecgpu_batch_mul, ecgpu_msm, ecgpu_batch_mul_base_and_mul_add,
 * ecgpu_msm_parts_dev and ecgpu_group_msm with point i given as the record X || Y || Z of the wire format above (3L bytes, no flag
 * array), as the reference's `mul_vartime`, `lincomb_vartime` and `mul_by_generator_and_mul_add_vartime` take a `ProjectivePoint`.
 * For every input the results and the return code are those of `to_affine` applied to each record (ecgpu_batch_normalize)
 * followed by the affine form, under the rule of the _ct_xyz forms above: X, Y or Z >= p (Z = 0 included), and a record with
 * Z != 0 and Y^2 Z != X^3 + a X Z^2 + b Z^3, fail the call with ECGPU_ERR_POINT; Z = 0 is the identity.  The records are
 * normalised on the device (k_xyz_affine: one field inversion per lane of up to 64 records, Montgomery's trick; Z = 0 and Z = 1
 * skip the product chain) into the context's scratch, and the affine pipeline runs unchanged behind that.  Host-pointer forms
 * pipeline at the sizes of their twins with 3L-byte records (ecgpu_msm_xyz from 2^23 terms in chunks of 2^22, the batch calls
 * from 2^19 units); `_dev` bases must be 16-byte aligned; errors are deferred on asynchronous contexts.  MSM lanes
 * (ecgpu_set_msm_lanes): an ecgpu_msm_xyz_dev / ecgpu_msm_parts_xyz_dev that goes to a lane converts its records on that lane,
 * into buffers of the lane, beside the MSM before it — the caller's X || Y || Z array belongs to the lane as an affine one would;
 * the small-MSM path (no lane) and the other calls convert on the context's stream, which first waits for the lanes. */
int ecgpu_batch_mul_xyz(ecgpu_ctx *ctx, int curve, const uint8_t *scalars, const uint8_t *points_xyz, size_t n, uint8_t *out_xy,
                        uint8_t *out_inf);
int ecgpu_batch_mul_xyz_dev(ecgpu_ctx *ctx, int curve, const void *d_scalars, const void *d_points_xyz, size_t n, void *d_out_xy,
                            void *d_out_inf);
int ecgpu_msm_xyz(ecgpu_ctx *ctx, int curve, const uint8_t *scalars, const uint8_t *points_xyz, size_t n, uint8_t *out_xy,
                  uint8_t *out_inf);
int ecgpu_msm_xyz_dev(ecgpu_ctx *ctx, int curve, const void *d_scalars, const void *d_points_xyz, size_t n, void *d_out_xy,
                      void *d_out_inf);
int ecgpu_batch_mul_base_and_mul_add_xyz(ecgpu_ctx *ctx, int curve, const uint8_t *a_scalars, const uint8_t *b_scalars,
                                         const uint8_t *points_xyz, size_t n, uint8_t *out_xy, uint8_t *out_inf);
int ecgpu_batch_mul_base_and_mul_add_xyz_dev(ecgpu_ctx *ctx, int curve, const void *d_a_scalars, const void *d_b_scalars,
                                             const void *d_points_xyz, size_t n, void *d_out_xy, void *d_out_inf);
int ecgpu_msm_parts_xyz_dev(ecgpu_ctx *ctx, int curve, const void *d_scalars, const void *d_points_xyz, size_t n, size_t plan_terms,
                            void *d_parts);
int ecgpu_group_msm_xyz(ecgpu_group *group, int curve, const uint8_t *scalars, const uint8_t *points_xyz, size_t n, uint8_t *out_xy,
                        uint8_t *out_inf);
int ecgpu_group_msm_xyz_dev(ecgpu_group *group, int curve, const void *const *d_scalars, const void *const *d_points_xyz,
                            const size_t *n_per_device, uint8_t *out_xy, uint8_t *out_inf);

/* Compressed points INTO the path (callers hold 33-byte SEC1 keys).  Like ecgpu_msm / ecgpu_batch_mul with
 * point i given as points_x[i] (L bytes, the curve's wire order) + points_tag[i]: 0x02 / 0x03 = the point with that x and even /
 * odd y (`FromSec1Point::from_sec1_point` of a compressed encoding -> `DecompressPoint::decompress`,
 * primeorder/src/affine.rs:183-200,352-366, k256/src/arithmetic/affine.rs:261-280), 0x00 (with x = 0) = the identity
 * (`Sec1Point::identity`).  The points are decoded on the device — one square root each, which costs about as much as 25 point
 * additions: at 2^24 k256 terms the decoding takes as long as the MSM itself — and the ordinary pipeline runs on the
 * result.  Any other tag, x >= p or an x that is on no point of the curve (the reference's `CtOption::None`) fails the call
 * with ECGPU_ERR_POINT.  Variable-time like the calls they feed; for secret scalars over compressed public keys decode with
 * ecgpu_batch_decompress_dev and pass the result to ecgpu_batch_mul_ct_dev. */
int ecgpu_msm_compressed(ecgpu_ctx *ctx, int curve, const uint8_t *scalars, const uint8_t *points_x, const uint8_t *points_tag,
                         size_t n, uint8_t *out_xy, uint8_t *out_inf);
int ecgpu_msm_compressed_dev(ecgpu_ctx *ctx, int curve, const void *d_scalars, const void *d_points_x, const void *d_points_tag,
                             size_t n, void *d_out_xy, void *d_out_inf);
int ecgpu_batch_mul_compressed(ecgpu_ctx *ctx, int curve, const uint8_t *scalars, const uint8_t *points_x,
                               const uint8_t *points_tag, size_t n, uint8_t *out_xy, uint8_t *out_inf);
int ecgpu_batch_mul_compressed_dev(ecgpu_ctx *ctx, int curve, const void *d_scalars, const void *d_points_x,
                                   const void *d_points_tag, size_t n, void *d_out_xy, void *d_out_inf);

/* Batch point decompression — `DecompressPoint::decompress(x_bytes, y_is_odd)`
 * (primeorder/src/affine.rs:183-200, k256/src/arithmetic/affine.rs:261-280; SEC1 tag 0x02 / 0x03 = y_is_odd 0 / 1;
 * BIP340 `decompact` = y_is_odd 0).  xs n*L bytes big-endian, y_is_odd n bytes.  out_xy[i] = (x, y) with
 * y^2 = x^3 + a x + b and the requested parity and ok[i] = 1, or a zero record and ok[i] = 0 when x >= p or
 * no such y exists (the reference's `CtOption::None`).  Every parameter set, p224 included (p = 1 mod 4: the square root
 * is a fixed-schedule Tonelli-Shanks over the 2^96-element subgroup, ~20 times the work of the other curves' single
 * exponentiation; primefield/src/monty.rs:467-469). */
int ecgpu_batch_decompress(ecgpu_ctx *ctx, int curve, const uint8_t *xs, const uint8_t *y_is_odd,
                           size_t n, uint8_t *out_xy, uint8_t *ok);
int ecgpu_batch_decompress_dev(ecgpu_ctx *ctx, int curve, const void *d_xs, const void *d_y_is_odd,
                               size_t n, void *d_out_xy, void *d_ok);

/* Batch hash-to-curve (RFC 9380) — the step in front of the multiplications: byte strings to group elements, as OPRF / VOPRF,
 * PAKE and BLS-style protocols need it per element.  Replaces, for a batch,
 *   ecgpu_hash_to_curve_batch     `hash2curve::GroupDigest::hash_from_bytes(&[msg], &[dst])` (hash2curve/src/group_digest.rs): the
 *                                 random-oracle suite — u0, u1 = hash_to_field(msg, 2), out = map_to_curve(u0) + map_to_curve(u1)
 *   ecgpu_encode_to_curve_batch   `GroupDigest::encode_from_bytes`: the non-uniform suite — u = hash_to_field(msg, 1), out = map_to_curve(u)
 *   ecgpu_hash_to_scalar_batch    `hash2curve::hash_to_scalar`: one draw of L bytes from the same expander, reduced mod n as
 *                                 `Reduce<Array<u8, L>> for Scalar` does; out_scalars n*FIELD bytes.  Zero is a legal output.
 *   ecgpu_map_to_curve_batch      `MapToCurve::map_to_curve(u)` on field elements the caller holds: u is n*per_point canonical
 *                                 elements of FIELD bytes; per_point = 1 gives map_to_curve(u), per_point = 2 gives
 *                                 map_to_curve(u[2i]) + map_to_curve(u[2i+1]).  A u >= p fails the call with ECGPU_ERR_POINT, as a
 *                                 coordinate >= p does; any other per_point is ECGPU_ERR_ARG.
 * SCOPE: the three tuned parameter sets, each with the suite the reference binds to it (all expand_message_xmd, all with the
 * simplified SWU map and sqrt_ratio for p = 3 mod 4; cofactor 1, so clear_cofactor does nothing):
 *   ECGPU_K256  secp256k1_XMD:SHA-256_SSWU_RO_ / _NU_  (RFC 9380 section 8.7)  SHA-256, L = 48, Z = -11, the map runs on the
 *               3-isogenous curve E' and the isogeny of Appendix E.1 follows (k256/src/arithmetic/hash2curve.rs)
 *   ECGPU_P256  P256_XMD:SHA-256_SSWU_RO_ / _NU_       (section 8.2)  SHA-256, L = 48, Z = -10 (p256/src/arithmetic/hash2curve.rs)
 *   ECGPU_P384  P384_XMD:SHA-384_SSWU_RO_ / _NU_       (section 8.3)  SHA-384, L = 72, Z = -12 (p384/src/arithmetic/hash2curve.rs)
 * Every other parameter set, ECGPU_P521 included, returns ECGPU_ERR_CURVE.
 * Arguments.  msgs: n*msg_len bytes, one uniform length per call, 0 allowed (the reference's `msg: &[&[u8]]` is a concatenation:
 * the caller concatenates).  dst: ONE domain separation tag per call, as distid is in ecgpu_sm2dsa_verify_msg_batch, with the rules
 * of `Domain::xmd` (hash2curve/src/hash2field/expand_msg.rs): dst_len == 0 (or dst == NULL) is ECGPU_ERR_ARG; a dst above 255 bytes
 * is replaced, on the host and once per call, by H("H2C-OVERSIZE-DST-" || dst) with the suite's hash.  out_xy: n*2*FIELD bytes; out_inf (may be NULL):
 * out_inf[i] = 1 with a zero record marks the identity, which only map_to_curve(u0) = -map_to_curve(u1) produces (for per_point
 * = 2: u1 = p - u0).
 * ONE DEPARTURE from the reference: the map is computed without a per-element inversion (x stays the fraction xn / xd, the isogeny
 * is evaluated on it, the batch shares one inversion), and where the reference inverts the isogeny's denominators with
 * `invert().unwrap()`, a zero denominator here yields the identity.  No u reaches that case — the double root of x_den is the x of no
 * point of E' — so the outputs are the reference's for every input; only code that calls the isogeny lane itself can see the difference.
 * SECRECY: hashed inputs may be secret (an OPRF input is a password).  The expand and map kernels take no branch and form no
 * address from message bytes, digests, u or points (tools/ct_isa_check.py --unit h2c); msg_len, dst, per_point and n are public.
 * The context's copies — u, the projective points, the staged messages and results of the host-pointer forms — are zeroed behind
 * the call like those of the `_ct` forms (and by ecgpu_wipe); the final `to_affine` is the batch normalisation every entry point uses.
 * These calls have host-pointer forms only so far; device-pointer twins are left for later.
 * From 2^19 elements on they run the chunked pipeline (see the preamble): after an error, chunks before the
 * offending one may already have been written to the outputs. */
int ecgpu_hash_to_curve_batch(ecgpu_ctx *ctx, int curve, const uint8_t *msgs, size_t msg_len, size_t n, const uint8_t *dst,
                              size_t dst_len, uint8_t *out_xy, uint8_t *out_inf);
int ecgpu_encode_to_curve_batch(ecgpu_ctx *ctx, int curve, const uint8_t *msgs, size_t msg_len, size_t n, const uint8_t *dst,
                                size_t dst_len, uint8_t *out_xy, uint8_t *out_inf);
int ecgpu_hash_to_scalar_batch(ecgpu_ctx *ctx, int curve, const uint8_t *msgs, size_t msg_len, size_t n, const uint8_t *dst,
                               size_t dst_len, uint8_t *out_scalars);
int ecgpu_map_to_curve_batch(ecgpu_ctx *ctx, int curve, const uint8_t *u, int per_point, size_t n, uint8_t *out_xy, uint8_t *out_inf);

/* Batch SM2 public-key encryption and decryption (GB/T 32918.4) — `sm2::pke`.  Replaces, for a batch,
 *   ecgpu_sm2_pke_encrypt_batch   `EncryptingKey::encrypt_cipher_with_buf` (sm2/src/pke/encrypting.rs:166-230) with the CALLER'S
 *                                 nonce, the hazmat shape ecgpu_ecdsa_sign_batch has: C1 = k G, (x2, y2) = k P_B,
 *                                 t = KDF(x2 || y2, msg_len), C2 = M ^ t, C3 = SM3(x2 || M || y2)
 *   ecgpu_sm2_pke_decrypt_batch   the point checks of `Cipher::from_slice` (sm2/src/pke.rs:131-143) and
 *                                 `DecryptingKey::decrypt_cipher_with_buf` (sm2/src/pke/decrypting.rs:174-222): (x2, y2) = d C1,
 *                                 M' = C2 ^ KDF(x2 || y2, msg_len), ok = (SM3(x2 || M' || y2) == C3)
 * with KDF block j (32 bytes) = SM3(x2 || y2 || I2OSP(j + 1, 4)) (sm2/src/pke.rs:349-381).  The reference's functions are generic
 * but instantiated for Sm2 with Sm3 only: the calls take no curve argument.
 * Wire format.  pk_xy, c1_xy: n*64 bytes, big-endian x || y; k, d: n*32 bytes, big-endian; msgs, c2, out_c2, out_msgs: n*msg_len
 * bytes, ONE uniform msg_len per call (as ecgpu_ecdsa_sign_msg_batch); c3, out_c3: n*32 bytes.  The `Mode` byte order (C1C3C2 /
 * C1C2C3), the SEC1 tag and the ASN.1 form stay with the caller, as DER stays outside the signing calls.
 * encrypt: ok[i] = 1 iff 1 <= k < n, P_B has both coordinates below p and lies on the curve, and t is not all zero (where the
 * reference's `loop` redraws k, the element gets ok = 0 here and the caller redraws).  An element with ok = 0 gets all-zero C1, C2
 * and C3 records and its neighbours are untouched; no element fails the batch.  Step A3 of the reference (S = [h] P_B, reject the
 * identity) multiplies by `Scalar::S`, the 2-adicity of n - 1, which is 1 for SM2's order, and the cofactor is 1 too: the step
 * reduces to "P_B is not the identity", which the x || y wire format cannot express anyway.
 * decrypt: ok[i] = 1 iff 1 <= d < n, C1 is on the curve with coordinates below p, and u == C3.  C1 and C3 come from an untrusted
 * ciphertext: a bad one is a per-element verdict, never ECGPU_ERR_POINT for the call.  With ok = 0 the output record is zero:
 * unauthenticated plaintext is not released.  One d per element (a server decrypting for many keys is one call; a caller with one
 * key repeats it).  msg_len == 0 is legal: ok = (SM3(x2 || y2) == C3), and c2 / out_msgs may be NULL.
 * ONE DEPARTURE from the reference: ecgpu_sm2_pke_encrypt_batch with msg_len == 0 returns ECGPU_ERR_ARG.  With an empty message the
 * reference's loop never terminates (`any` over an empty range is false on every draw).
 * Both: msg_len > 0xFFFFFFFF is ECGPU_ERR_ARG (the reference's i32 block counter cannot overflow below that); a NULL array with
 * n > 0 or a NULL ctx is ECGPU_ERR_ARG; n == 0 succeeds.
 * SECRECY: k, d, (x2, y2), t and the messages are secret.  Both multiplications are the uniform-schedule kernels of the `_ct`
 * forms; in the kernels around them (k_pke_load, k_pke_seal, k_pke_open) no branch and no address depends on k, d, x2, y2, t, a
 * message byte or the outcome of the C3 comparison (tools/ct_isa_check.py --unit pke); msg_len and n are public.  The public point
 * (P_B, C1) is checked by a kernel of its own that may branch on it.  (x2, y2) never leaves the device.  The context's copies —
 * the sanitised scalars, x2 || y2, the projective points, the staged k, d and messages — are zeroed behind the call like those of
 * the `_ct` forms (and by ecgpu_wipe).
 * These calls have host-pointer forms only; from 2^19 elements on they run the chunked pipeline (see the preamble). */
int ecgpu_sm2_pke_encrypt_batch(ecgpu_ctx *ctx, const uint8_t *pk_xy, const uint8_t *k, const uint8_t *msgs, size_t msg_len,
                                size_t n, uint8_t *out_c1_xy, uint8_t *out_c2, uint8_t *out_c3, uint8_t *ok);
int ecgpu_sm2_pke_decrypt_batch(ecgpu_ctx *ctx, const uint8_t *d, const uint8_t *c1_xy, const uint8_t *c2, size_t msg_len,
                                const uint8_t *c3, size_t n, uint8_t *out_msgs, uint8_t *ok);

/* Device-side known-answer tests of the arithmetic the kernels are built from — the same field / group code the CPU
 * host checks run (tests/hostcheck), here as gfx950 code, one lane per element; host buffers.
 * ecgpu_selftest_field: out[i] = op(a[i], b[i]) on canonical field elements (L bytes each; b may be NULL for unary ops).
 *   op 0 a + b, 1 a - b, 2 a * b, 3 a^2, 4 1/a by division steps (0 for 0), 5 -a, 7 2a, 8 pack / unpack round trip of the
 *   lazily reduced 2a + b, 9 the fused a*b - (a + b)*b, 10 1/a by Fermat, 11 sqrt(a) or 0, 12 a 25-step chain at the
 *   magnitudes the point formulas use, 13 / 14 the fused a*b - c and a^2 - c, 15 (k256) the reduction in assembly against the
 *   compiler's from the same columns (14 a b, or all ones on a mismatch), 16 (k256; n a multiple of 64) the row-parallel
 *   multiplication of the MSM's Horner chain: 13 a b of lane (i mod 4) of the wave in every lane i, 17 1/a by the variable-time
 *   division steps.  The reference's counterparts: `FieldElement::{add, sub, mul, square, invert,
 *   negate, double, sqrt}` (k256/src/arithmetic/field.rs, p256/src/arithmetic/field.rs, primefield/src/monty.rs).
 *   Ops 30 - 44 take operands as they are, NOT only canonical ones (a kernel of their own; csrc/ecgpu_selftest_raw.h).  30 - 39, the
 *   raw domain: a, b enter the internal domain as written (Field::unpack: limbs of all ones, values in [p, 2p) below 2^(8 L)) and
 *   are scaled by repeated addition to the magnitude limits of the parameter set; the result is the internal-domain value in
 *   [0, p).  With MP = MAXPROD, A1 = min(MP, MAXMAG), B1 = MP / A1, A2 = 5 / 4 / 3 / 2 for MP >= 25 / 16 / 9 / else, B2 = MP / A2,
 *   SQ = SQLIM: 30 mul(A1 a, B1 b), 31 mul(A2 a, B2 b), 32 sqr(SQ a), 33 mul(a, b), 34 the fused mul_sub(A2 a, B2 b, 6 b) and
 *   35 sqr_sub(SQ a, 6 b) of every parameter set, 36 mul2(A2 a, floor(B2 / 2) b, A2 b, ceil(B2 / 2) a), 37 3 a - 3 b (k256) or
 *   6 a - 6 b, 38 to_canonical(a), 39 is_zero(a) as 0 / 1.  40 - 44, scalars modulo the group order (a, b < n): 40 a * b,
 *   41 1 / a (0 for 0), 42 reduce_wire(a) for any a < 2^(8 L), 43 is_high(a) as 0 / 1, 44 a through to_mont and from_mont.
 *   46, 47, the raw domain again (45 is unknown): 1 / a by the branch-free and by the variable-time division steps on a as
 *   written, so that a < p is the very integer the division steps receive and a in [p, 2p) is reduced in front of them; the result is the
 *   internal-domain value a^-1 mod p (k256) or a^-1 R^2 mod p (the Montgomery sets), 0 for a = 0 mod p.
 * ecgpu_selftest_point: out[i] = op(P[i], Q[i]); op 0 P + Q (complete), 1 the same mixed, 2 2P, 3 -P, 4 P - Q, 5 the same
 *   mixed, and the incomplete formulas inside their domain (P, Q finite, P != +-Q): 6 2P (Jacobian), 7 2P + Q (Jacobian
 *   doubling + mixed addition), 8 P + Q (XYZZ mixed), 9 P + Q (XYZZ affine + affine), 10 (k256; n a multiple of 64) 32 P of
 *   the wave's FIRST point in every lane, by five row-parallel complete doublings.
 *   Ops 20 - 26, op = code | steps << 8 (steps <= 64): the cross-lane code behind the MSM's buckets, a kernel of its own
 *   (csrc/ecgpu_selftest_msm.h); q_xy is required except for 26, n is a multiple of 64 (of 256 for 25), else ECGPU_ERR_ARG.
 *   k256 on RAW records (a 64-byte record is sixteen little-endian 32-bit words, words 0 - 8 the nine 29-bit-radix limbs as they
 *   are, nothing checked; the nine result limbs come back the same way, out_inf = 0): 20 the row-parallel multiplication, row r of a
 *   wave on the p / q records of the wave's lane r, the product of row (i mod 4) in lane i; 21 its norm64 on the per-position
 *   64-bit values p word | q word << 32, laid out the same way; 22 the row doubling chain: X, Y, Z = the p records of the wave's
 *   lanes 0, 1, 2, `steps` doublings, coordinate (i mod 3) in lane i.  k256 on points: 23 the complete addition on the lanes of a
 *   quad, P + Q of each quad's first lane in all four lanes; 24 the same on Group::add(P, Q) and Group::dbl(Q): P + 3 Q; 25 the
 *   workgroup-wide tree sum of P over 256 lanes in the workgroup's first record (the identity in the others).  The a = -3 sets:
 *   26 2^steps (P + Q) (P alone without q_xy) of the wave's first lane in every lane, by the Jacobian doubling shared by three lanes.
 * ecgpu_selftest_point_raw: the point formulas on coordinates taken limb by limb (a kernel of its own; csrc/ecgpu_selftest_point_raw.h).
 *   A record is four coordinate slots of NL little-endian 32-bit words each (NL limbs of B bits: 9 x 29 k256; 10 x 28 p256, sm2,
 *   bp256, bp256t1, bign256; 15 x 27 p384, bp384, bp384t1; 9 x 27 p224; 8 x 26 p192; 20 x 27 p521), the words are the limbs of
 *   the internal form as they are (the Montgomery form where the set has one): nothing is converted, range-checked or checked
 *   against the curve, and out[i] comes back in the same layout with no inversion.  Slots: homogeneous X Y Z -, Jacobian X Y Z -,
 *   XYZZ X Y ZZ ZZZ, affine x y - -.  q may be NULL (zeros).  Any n.
 *     op  result        operation                           op  result        operation
 *      0  homogeneous   add(P, Q)                            8  Jacobian      jac_madd(J, q)
 *      1  homogeneous   add(P, -Q)                           9  Jacobian      jac_madd(J, -q)
 *      2  homogeneous   add_mixed(P, q)                     10  homogeneous   jac_to_proj(J)
 *      3  homogeneous   add_mixed(P, -q)                    11  XYZZ          xyzz_madd(S, q)
 *      4  homogeneous   dbl(P)                              12  XYZZ          xyzz_madd(S, -q)
 *      5  homogeneous   neg(P)                              13  XYZZ          xyzz_mmadd(p, q)
 *      6  homogeneous   ct_dbl4(P) = 16 P                   14  homogeneous   xyzz_to_proj(S)
 *      7  Jacobian      jac_dbl(J)                          17  first word    is_identity(P) as 0 / 1
 *     15 | steps << 8   homogeneous   acc = dbl(add(acc, Q)), steps times from acc = P        (steps <= 64)
 *     16 | steps << 8   Jacobian      acc = jac_madd(jac_dbl^4(acc), q), steps times from acc = J: the ladder step
 *   The Jacobian and XYZZ formulas are the incomplete ones: outside their domain (a finite P != +-Q) the result means nothing.
 * ECGPU_ERR_POINT: an input >= p (field ops 0 - 21) / off the curve; ECGPU_ERR_SCALAR_RANGE: unknown op. */
int ecgpu_selftest_field(ecgpu_ctx *ctx, int curve, int op, const uint8_t *a, const uint8_t *b, size_t n, uint8_t *out);
int ecgpu_selftest_point(ecgpu_ctx *ctx, int curve, int op, const uint8_t *p_xy, const uint8_t *p_inf, const uint8_t *q_xy,
                         const uint8_t *q_inf, size_t n, uint8_t *out_xy, uint8_t *out_inf);
int ecgpu_selftest_point_raw(ecgpu_ctx *ctx, int curve, int op, const uint8_t *p, const uint8_t *q, size_t n, uint8_t *out);

/* Test infrastructure: one op of the Goldilocks field (csrc/ecgpu_fe448.h, p = 2^448 - 2^224 - 1) on RAW limbs, modelled on
 * ecgpu_selftest_point_raw: a, b and out are records of 16 little-endian 32-bit words, the 28-bit limbs as they are, so that lazy
 * representatives can be handed in; nothing is converted or range-checked.  b may be NULL (zeros).  Any n; no curve argument.
 *     op  operation                    limbs accepted                 op  operation                    limbs accepted
 *      0  mul(a, b)                    <= 2 T each                     5  carry(a)                     any 32-bit words
 *      1  sqr(a)                       <= 2 T                          6  canon(a): [0, p)             <= 15 T
 *      2  add(a, b), lazy sum          <= T each                       7  invert(a) = a^(p-2), 0 -> 0  <= T
 *      3  sub(a, b)                    <= 2 T each                     8  from_bytes -> to_bytes: words 0..13 of a are the
 *      4  mul_small(a, 39082)          <= 2 T                             56-byte record; out words 14, 15 are zero
 *   T = 2^28 + 2^8, the limb bound of a tight element.  Beyond what an op accepts the result means nothing (the device does not
 *   check; the bounds-checking host build of tests/hostcheck_x448 traps).  ECGPU_ERR_ARG: unknown op or a missing array. */
int ecgpu_selftest_fe448(ecgpu_ctx *ctx, int op, const uint8_t *a, const uint8_t *b, size_t n, uint8_t *out);

/* Test infrastructure: one lane body of hash-to-curve (csrc/ecgpu_h2c.h) on records the CALLER supplies, so that a test can hand
 * the reductions and the map what no digest produces (pieces of all ones, OKM = k m, a final addition that lands on m, a u with
 * structured limbs, a forged isogeny denominator).  A kernel of its own that calls the functions k_h2c_expand and k_h2c_map call;
 * the device-side twin of tests/hostcheck_h2c.  Records are big-endian; L = 48 bytes (ECGPU_K256, ECGPU_P256) or 72 (ECGPU_P384)
 * is the suite's draw length, F = ecgpu_field_bytes(curve).
 *     op  function             in[i]                                   out[i]
 *      0  h2c_reduce_field     L bytes, any value                      F bytes: OS2IP(in) mod p
 *      1  h2c_reduce_scalar    L bytes, any value                      F bytes: OS2IP(in) mod n
 *      2  H2cMap::sswu         u, F bytes, below p (not checked)       xn || xd || y, 3 F bytes, canonical: the point (xn / xd, y)
 *                                                                      of the curve the map runs on (E' for secp256k1)
 *      3  H2cMap::iso_k256     xn || xd || y, 3 F bytes, each below p  X || Y || Z, 3 F bytes, canonical: the image of (xn / xd, y)
 *                              (need not be on E'; xd = 0 means nothing) under the 3-isogeny; a zero denominator gives (0 : 1 : 0)
 *   Op 3 exists for ECGPU_K256 only.  ECGPU_ERR_ARG: unknown op, or a NULL array with n > 0; ECGPU_ERR_CURVE: a curve without a
 *   suite (ECGPU_P521 included), or op 3 on another curve than ECGPU_K256.  n = 0 succeeds and touches nothing. */
int ecgpu_selftest_h2c(ecgpu_ctx *ctx, int curve, int op, const uint8_t *in, size_t n, uint8_t *out);

/* Test infrastructure: the finish kernels of the signing entry points on stages the CALLER supplies, so that a test can hand them
 * what no input of the pipelines produces (x(R) in [n, p), R at infinity, a cleared nonce flag beside a valid k, a Schnorr nonce that
 * cancels e d').  Nothing runs before the kernel: `flag` is the nonce's verdict byte, r_xy the affine R (x || y) and r_inf its
 * identity byte, as the nonce, fixed-base and normalisation kernels would have left them; k is the nonce AFTER the nonce kernel.
 *   scheme 0  k_ecdsa_sign_finish (any ECDSA set): d, k, z of L bytes; out_sig = r || s, out_recid, ok.
 *   scheme 1  k_sm2dsa_sign_finish (curve = ECGPU_SM2): z = the prehash e; out_recid unused (may be NULL).
 *   scheme 2  k_schnorr_sign_finish (curve = ECGPU_K256): d = d' || x(P), 64 bytes per element; z unused (may be NULL); msgs = n
 *             messages of msg_len bytes; out_recid unused.
 *   scheme 4  k_bign_sign_finish (ECGPU_SIGN_SCHEME_BIGN; curve = ECGPU_BIGN256): z = the RAW prehash; the first 16 bytes of each
 *             64-byte r_xy record are S0, handed to the kernel directly (0, 1, 2^128 - 1: the stages no input produces); out_sig =
 *             S0 || S1, 48 bytes per element; out_recid unused.  (3 is not a scheme.)
 * normalize_s applies to scheme 0 only.  ECGPU_ERR_ARG: unknown scheme or a missing array; ECGPU_ERR_CURVE: a curve the scheme
 * does not exist over.  Not a signing interface: it checks nothing that ties R to k. */
enum { ECGPU_SIGN_SCHEME_BIGN = 4 };
int ecgpu_selftest_sign_finish(ecgpu_ctx *ctx, int curve, int scheme, const uint8_t *d, const uint8_t *k, const uint8_t *flag,
                               const uint8_t *z, const uint8_t *r_xy, const uint8_t *r_inf, const uint8_t *msgs, size_t msg_len, size_t n,
                               int normalize_s, uint8_t *out_sig, uint8_t *out_recid, uint8_t *ok);

/* Test infrastructure: the nonce generator kernels of bign signing (k_bign_genk, k_bign_genk_retry) with the caller's 32-byte
 * little-endian `bound` in place of q.  No input makes a candidate >= q with the real q; with bound = 2^254 three candidates in four
 * are rejected, which runs the retry path on hardware.  d: the keys, h: the prehashes (reduced mod q first, as in the signing
 * calls); out_k: n*32 bytes, the accepted candidate; out_rounds: n*4 bytes, the round count as a little-endian 32-bit integer (a
 * multiple of 4).  An element that reached the cap of 128 candidates gets k = 1 and 512 rounds. */
int ecgpu_selftest_bign_genk(ecgpu_ctx *ctx, const uint8_t *d, const uint8_t *h, const uint8_t *bound, size_t n, uint8_t *out_k,
                             uint8_t *out_rounds);

/* Integer-VALU roof probe: runs a dependency-free v_mad_u64_u32 stream on every CU and returns
 * the measured 32x32->64 multiply-add rate in operations per second (SURVEY.md §8d "peak to
 * divide by").  `which` selects the instruction: 0 v_mad_u64_u32, 1 v_mul_lo_u32, 2 v_mul_hi_u32,
 * 3 v_add_u32, 4 v_lshl_add_u64, 5 v_mad_u32_u24, 6 v_fma_f64, 7 v_addc_co_u32 chain; 100 + i: exact
 * inline-asm instruction streams; 200: HBM gather probe — 2^20 lanes x 16 random 64-byte reads of the k256
 * comb table, returns BYTES per second (a known byte count in the fixed-base kernel's access pattern, used
 * to calibrate rocprofv3's FETCH_SIZE). */
int ecgpu_valu_probe(ecgpu_ctx *ctx, int which, double *ops_per_sec);

/* Milliseconds the device spent in the kernels of the last *_dev / host call on this context,
 * measured with HIP events on the context stream; `name` selects a stage:
 *   "total", "main" (the scalar-mul / bucket kernels), "normalize", "recode", "sort", "reduce". */
int ecgpu_last_timing(const ecgpu_ctx *ctx, const char *name, double *ms);

/* Per-call timing events on / off (default: on).  Every call brackets its kernels with HIP events so that ecgpu_last_timing
 * can report them; an event is a packet of its own on the stream, and on a queue of short batches they add up (measured: 8 us
 * of a 0.63 ms fixed-base batch).  on == 0: the calls record nothing and ecgpu_last_timing returns ECGPU_ERR_ARG for them. */
int ecgpu_set_timing(ecgpu_ctx *ctx, int on);

/* Library version string. */
const char *ecgpu_version(void);

#ifdef __cplusplus
}
#endif
#endif /* ECGPU_H */
