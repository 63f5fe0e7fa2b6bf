/* examples/sm2dsa_sign.c — batch SM2DSA signing from plain C: the known answer of GB/T 32918.5-2017 Annex A (ID "1234567812345678",
 * M "message digest") through the form with the caller's nonce, then the same key signs a message with the nonce of RFC 6979 over
 * HMAC-SM3 — PA = d G, Z and e = SM3(Z || M) computed on the device — and ecgpu_sm2dsa_verify_msg_batch accepts the result.
 *
 *     make -C examples && ./examples/sm2dsa_sign      # needs an MI355X
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

static const char D[] = "3945208F7B2144B13F36E38AC6D39F95889393692860B51A42FB81EF4DF7C5B8";
static const char K[] = "59276E27D506861A16680F3AD9C02DCCEF3CC1FA3CDBE4CE6D54B80DEAC1BC21";
static const char E[] = "F0B43E94BA45ACCAACE692ED534382EB17E6AB5A19CE7B31F4486FDFC0D28640";
static const char SIG[] = "F5A03B0648D2C4630EEAC513E1BB81A15944DA3827D5B74143AC7EACEEE720B3"
                          "B1B6AA29DF212FD8763182BC0D421CA1BB9038FD1F7F42D4840B69C485BBC1AA";

int main(void) {
    ecgpu_ctx *ctx = NULL;
    CHECK(ecgpu_init(&ctx, 0));
    uint8_t d[32], k[32], e[32], want[64], sig[64], ok[1];
    unhex(d, D);
    unhex(k, K);
    unhex(e, E);
    unhex(want, SIG);
    /* the standard's steps A3-A7 with its own nonce (a real caller draws k from a CSPRNG, or uses the two forms below) */
    CHECK(ecgpu_sm2dsa_sign_batch(ctx, d, k, e, 1, sig, ok));
    const int vector_ok = ok[0] == 1 && memcmp(sig, want, 64) == 0;
    printf("the standard's known answer: %s\n", vector_ok ? "yes" : "NO");

    /* `SigningKey::new(distid, sk)?.sign(msg)`: nothing but the key, the identifier and the message goes in */
    const char *distid = "1234567812345678", *msg = "message digest";
    uint8_t pa[64], inf[1];
    CHECK(ecgpu_sm2dsa_sign_msg_batch(ctx, (const uint8_t *)distid, strlen(distid), d, (const uint8_t *)msg, strlen(msg), 1, sig, ok));
    const int signed_ok = ok[0] == 1;
    printf("r || s = ");
    for (int i = 0; i < 64; i++) printf("%02x", sig[i]);
    printf("\n");
    CHECK(ecgpu_batch_mul_base_ct(ctx, ECGPU_SM2, d, 1, pa, inf));              /* the verifier's side: PA = d G */
    CHECK(ecgpu_sm2dsa_verify_msg_batch(ctx, (const uint8_t *)distid, strlen(distid), pa, (const uint8_t *)msg, strlen(msg), sig, 1, ok));
    const int verified = signed_ok && ok[0] == 1;
    printf("signed and verified on the device: %s\n", verified ? "yes" : "NO");
    /* the same e through the prehash form gives the same signature: the nonce is a function of d and e alone */
    uint8_t sig2[64];
    CHECK(ecgpu_sm2dsa_sign_rfc6979_batch(ctx, d, e, 1, sig2, ok));
    const int same = ok[0] == 1 && memcmp(sig, sig2, 64) == 0;
    printf("the prehash form agrees: %s\n", same ? "yes" : "NO");
    /* a key that cannot sign (d = 0): ok = 0 and a zero record, the call itself succeeds */
    memset(d, 0, 32);
    CHECK(ecgpu_sm2dsa_sign_rfc6979_batch(ctx, d, e, 1, sig2, ok));
    const int refused = ok[0] == 0 && sig2[0] == 0 && sig2[63] == 0;
    printf("an unusable key is refused per element: %s\n", refused ? "yes" : "NO");
    ecgpu_destroy(ctx);
    return vector_ok && verified && same && refused ? 0 : 2;
}
