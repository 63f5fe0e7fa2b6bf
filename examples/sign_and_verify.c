/* examples/sign_and_verify.c — the signing entry points of the C ABI from plain C, on the reference's own vectors:
 *   - `Signer::sign(b"sample")` on p256 with the key of RFC 6979 appendix A.2.5 (p256/src/ecdsa.rs:92-102): the digest, the
 *     RFC 6979 nonce and the signature are computed on the device; the signature is compared with the reference's and verified
 *     with ecgpu_ecdsa_verify_msg_batch against d G;
 *   - BIP340 `sign_raw` on vector 1 of k256/src/schnorr.rs:271-281, verified with ecgpu_schnorr_verify_raw_batch.
 *
 *     make -C examples && ./examples/sign_and_verify      # needs an MI355X
 */
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../include/ecgpu.h"

#define CHECK(call)                                                                              \
    do {                                                                                         \
        int rc_ = (call);                                                                        \
        if (rc_ != ECGPU_OK) {                                                                   \
            fprintf(stderr, "%s failed: %d (%s)\n", #call, rc_, ctx ? ecgpu_last_error(ctx) : ""); \
            return 1;                                                                            \
        }                                                                                        \
    } while (0)

static void unhex(uint8_t *out, const char *hex) {
    for (size_t i = 0; hex[2 * i]; i++) {
        unsigned v;
        sscanf(hex + 2 * i, "%2x", &v);
        out[i] = (uint8_t)v;
    }
}

int main(void) {
    ecgpu_ctx *ctx = NULL;
    CHECK(ecgpu_init(&ctx, 0));
    enum { L = 32 };
    int good = 1;

    /* ---- ECDSA: sign a message, compare, verify ---- */
    static const char *MSG = "sample";
    uint8_t d[L], want[2 * L], sig[2 * L], recid[1], ok[1], q[2 * L], inf[1], vok[1];
    unhex(d, "c9afa9d845ba75166b5c215767b1d6934e50c3db36e89b127b8a622b120f6721");
    unhex(want, "efd48b2aacb6a8fd1140dd9cd45e81d69d2c877b56aaf991c34d0ea84eaf3716"
                "f7cb1c942d657c41d436c7a1b6e29f65f3e900dbb9aff4064dc4ab2f843acda8");
    CHECK(ecgpu_ecdsa_sign_msg_batch(ctx, ECGPU_P256, d, (const uint8_t *)MSG, strlen(MSG), 1, /* NORMALIZE_S */ 0, sig, recid, ok));
    const int same = ok[0] && memcmp(sig, want, 2 * L) == 0;
    printf("p256 signature of \"%s\" == the reference's: %s (recovery id %d)\n", MSG, same ? "yes" : "NO", recid[0]);
    good &= same;
    CHECK(ecgpu_batch_mul_base_ct(ctx, ECGPU_P256, d, 1, q, inf));                 /* the verifying key, on the constant-time path */
    CHECK(ecgpu_ecdsa_verify_msg_batch(ctx, ECGPU_P256, q, (const uint8_t *)MSG, strlen(MSG), sig, 1, 0, vok));
    printf("verified by ecgpu_ecdsa_verify_msg_batch: %s\n", vok[0] ? "yes" : "NO");
    good &= vok[0];

    /* ---- BIP340 ---- */
    uint8_t sk[32], aux[32], msg[32], swant[64], ssig[64], pkx[32], sok[1];
    unhex(sk, "b7e151628aed2a6abf7158809cf4f3c762e7160f38b4da56a784d9045190cfef");
    unhex(aux, "0000000000000000000000000000000000000000000000000000000000000001");
    unhex(msg, "243f6a8885a308d313198a2e03707344a4093822299f31d0082efa98ec4e6c89");
    unhex(pkx, "dff1d77f2a671c5f36183726db2341be58feae1da2deced843240f7b502ba659");
    unhex(swant, "6896bd60eeae296db48a229ff71dfe071bde413e6d43f917dc8dcf8c78de3341"
                 "8906d11ac976abccb20b091292bff4ea897efcb639ea871cfa95f6de339e4b0a");
    CHECK(ecgpu_schnorr_sign_raw_batch(ctx, sk, msg, 32, aux, 1, ssig, sok));
    const int ssame = sok[0] && memcmp(ssig, swant, 64) == 0;
    printf("BIP340 signature (vector 1) == the reference's: %s\n", ssame ? "yes" : "NO");
    good &= ssame;
    CHECK(ecgpu_schnorr_verify_raw_batch(ctx, pkx, msg, 32, ssig, 1, sok));
    printf("verified by ecgpu_schnorr_verify_raw_batch: %s\n", sok[0] ? "yes" : "NO");
    good &= sok[0];

    CHECK(ecgpu_wipe(ctx));       /* the key passed through staging buffers; the signing calls have wiped theirs already */
    memset(d, 0, sizeof d);
    memset(sk, 0, sizeof sk);
    ecgpu_destroy(ctx);
    puts(good ? "ok" : "MISMATCH");
    return good ? 0 : 1;
}
