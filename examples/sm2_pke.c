/* examples/sm2_pke.c — batch SM2 public-key encryption from plain C: the reference's ciphertext (sm2/tests/sm2pke.rs: CIPHER,
 * 04 || C1 || C3 || C2, decrypts to "plaintext" under PRIVATE_KEY) is decrypted on the device, and one message goes round: the
 * public key d G from ecgpu_batch_mul_base_ct, encryption with a nonce of the caller's, decryption of the result.  The SEC1 tag and
 * the C1C3C2 byte order are the caller's, as DER is outside the signing calls; (x2, y2) never leaves the device.
 *
 *     make -C examples && ./examples/sm2_pke      # needs an MI355X
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

static const char PRIVATE_KEY[] = "3ddd2a3679bf6f1dfc3b49d3e99114718e48ec170eb4e4d3a82052dab19e8b50";
static const char CIPHER[] =
    "041ed68db303f5bc6bce516d5a62e1cd16781d3007df6864d970a56d46a6cecca0e0d33bfc71e78c440ae6afeef1a18cce473b3e27002189a058ddadc9182c80"
    "a3f13be66476ba6ef66d95a7fb11f30de441b3b66d566e48348bd830e584e7ec37f9b704ef32eba9055c";

int main(void) {
    ecgpu_ctx *ctx = NULL;
    CHECK(ecgpu_init(&ctx, 0));
    uint8_t d[32], ct[256], msg[64], ok[1];
    unhex(d, PRIVATE_KEY);
    const size_t ct_len = unhex(ct, CIPHER), msg_len = ct_len - 1 - 64 - 32;
    /* Mode::C1C3C2: tag, C1 (64 bytes), C3 (32 bytes), C2 */
    CHECK(ecgpu_sm2_pke_decrypt_batch(ctx, d, ct + 1, ct + 97, msg_len, ct + 65, 1, msg, ok));
    const int vector_ok = ok[0] == 1 && msg_len == 9 && memcmp(msg, "plaintext", 9) == 0;
    printf("the reference's ciphertext decrypts to \"%.*s\": %s\n", (int)msg_len, (const char *)msg, vector_ok ? "yes" : "NO");

    /* the round trip: P_B = d G, a nonce of the caller's (any value in [1, n); a real caller draws it from a CSPRNG) */
    uint8_t pk[64], inf[1], k[32], c1[64], c2[64], c3[32], back[64];
    const char *text = "batch SM2 encryption on the device";
    const size_t len = strlen(text);
    CHECK(ecgpu_batch_mul_base_ct(ctx, ECGPU_SM2, d, 1, pk, inf));
    unhex(k, "59276e27d506861a16680f3ad9c02dccef3cc1fa3cdbe4ce6d54b80deac1bc21");
    CHECK(ecgpu_sm2_pke_encrypt_batch(ctx, pk, k, (const uint8_t *)text, len, 1, c1, c2, c3, ok));
    const int sealed = ok[0] == 1;
    CHECK(ecgpu_sm2_pke_decrypt_batch(ctx, d, c1, c2, len, c3, 1, back, ok));
    const int round_ok = sealed && ok[0] == 1 && memcmp(back, text, len) == 0;
    printf("C3 = ");
    for (int i = 0; i < 32; i++) printf("%02x", c3[i]);
    printf("\nround trip of %zu bytes: %s\n", len, round_ok ? "yes" : "NO");
    /* one flipped bit of C2: the element gets ok = 0 and a zero record, the call itself succeeds */
    c2[0] ^= 1;
    CHECK(ecgpu_sm2_pke_decrypt_batch(ctx, d, c1, c2, len, c3, 1, back, ok));
    const int refused = ok[0] == 0 && back[0] == 0 && back[len - 1] == 0;
    printf("a tampered ciphertext is refused per element: %s\n", refused ? "yes" : "NO");
    ecgpu_destroy(ctx);
    return vector_ok && round_ok && refused ? 0 : 2;
}
