/* examples/bign_sign.c — batch bign signing (STB 34.101.45) from plain C: the reference's own vector (bignp256/tests/ecdsa.rs:20-33;
 * with the standard's belt-based nonce generator it is the deterministic signature of its key and message) through the message
 * form — H = belt-hash(message), the nonce, R = k G, S0 and S1 all computed on the device —, then ecgpu_bign_verify_msg_batch
 * accepts the result, and an unusable key is refused per element.  Every record is little-endian.
 *
 *     make -C examples && ./examples/bign_sign      # needs an MI355X
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

static size_t unhex(uint8_t *out, const char *hex) {
    size_t i = 0;
    for (; hex[2 * i]; i++) {
        unsigned v;
        sscanf(hex + 2 * i, "%2x", &v);
        out[i] = (uint8_t)v;
    }
    return i;
}

static const char PRIVATE_KEY[] = "1F66B5B84B7339674533F0329C74F21834281FED0732429E0C79235FC273E269";
static const char MSG[] = "B194BAC80A08F53B366D008E58";
static const char SIG[] = "19D32B7E01E25BAE4A70EB6BCA42602C"
                          "CA6A13944451BCC5D4C54CFD8737619C328B8A58FB9C68FD17D569F7D06495FB";

int main(void) {
    ecgpu_ctx *ctx = NULL;
    CHECK(ecgpu_init(&ctx, 0));
    uint8_t d[32], msg[13], want[48], sig[48], ok[1];
    unhex(d, PRIVATE_KEY);
    const size_t msg_len = unhex(msg, MSG);
    unhex(want, SIG);
    /* `Signer::try_sign`: nothing but the key and the message goes in */
    CHECK(ecgpu_bign_sign_msg_batch(ctx, d, msg, msg_len, 1, sig, ok));
    printf("S0 || S1 = ");
    for (int i = 0; i < 48; i++) printf("%02X", sig[i]);
    printf("\n");
    const int vector_ok = ok[0] == 1 && memcmp(sig, want, 48) == 0;
    printf("the reference's vector: %s\n", vector_ok ? "yes" : "NO");
    /* the verifier's side: Q = d G, then the message form of the verification */
    uint8_t q[64], inf[1];
    CHECK(ecgpu_batch_mul_base_ct(ctx, ECGPU_BIGN256, d, 1, q, inf));
    CHECK(ecgpu_bign_verify_msg_batch(ctx, q, msg, msg_len, sig, 1, ok));
    const int verified = vector_ok && ok[0] == 1;
    printf("verified on the device: %s\n", verified ? "yes" : "NO");
    /* a key that cannot sign (d = 0): ok = 0 and a zero record, the call itself succeeds */
    uint8_t sig2[48];
    memset(d, 0, 32);
    CHECK(ecgpu_bign_sign_msg_batch(ctx, d, msg, msg_len, 1, sig2, ok));
    const int refused = ok[0] == 0 && sig2[0] == 0 && sig2[47] == 0;
    printf("an unusable key is refused per element: %s\n", refused ? "yes" : "NO");
    ecgpu_destroy(ctx);
    return vector_ok && verified && refused ? 0 : 2;
}
