/* examples/x448_dh.c — batch X448 from plain C: the Alice / Bob exchange of RFC 7748 section 6.2 (the reference's
 * test_rfc_test_vectors_alice_bob, x448/src/lib.rs:326-371).  Both public keys come from ecgpu_x448_base_batch
 * (`PublicKey::from(&EphemeralSecret)`), both shared secrets from ecgpu_x448_batch (`diffie_hellman`) in one call of two elements,
 * and a low-order point is refused per element.  Every record is 56 bytes, little-endian; the scalars are clamped on the device.
 *
 *     make -C examples && ./examples/x448_dh      # needs an MI355X
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

static const char ALICE_PRIVATE[] = "9a8f4925d1519f5775cf46b04b5800d4ee9ee8bae8bc5565d498c28d"
                                    "d9c9baf574a9419744897391006382a6f127ab1d9ac2d8c0a598726b";
static const char ALICE_PUBLIC[] = "9b08f7cc31b7e3e67d22d5aea121074a273bd2b83de09c63faa73d2c"
                                   "22c5d9bbc836647241d953d40c5b12da88120d53177f80e532c41fa0";
static const char BOB_PRIVATE[] = "1c306a7ac2a0e2e0990b294470cba339e6453772b075811d8fad0d1d"
                                  "6927c120bb5ee8972b0d3e21374c9c921b09d1b0366f10b65173992d";
static const char BOB_PUBLIC[] = "3eb7a829b0cd20f5bcfc0b599b6feccf6da4627107bdb0d4f345b430"
                                 "27d8b972fc3e34fb4232a13ca706dcb57aec3dae07bdc1c67bf33609";
static const char SHARED[] = "07fff4181ac6cc95ec1c16a94a0f74d12da232ce40a77552281d282b"
                             "b60c0b56fd2464c335543936521c24403085d59a449a5037514a879d";

int main(void) {
    ecgpu_ctx *ctx = NULL;
    CHECK(ecgpu_init(&ctx, 0));
    uint8_t priv[2 * 56], pub[2 * 56], want_pub[2 * 56], want_shared[56];
    unhex(priv, ALICE_PRIVATE);
    unhex(priv + 56, BOB_PRIVATE);
    unhex(want_pub, ALICE_PUBLIC);
    unhex(want_pub + 56, BOB_PUBLIC);
    unhex(want_shared, SHARED);
    /* `PublicKey::from(&secret)`: both public keys in one call */
    CHECK(ecgpu_x448_base_batch(ctx, priv, 2, pub));
    const int keys_ok = memcmp(pub, want_pub, sizeof pub) == 0;
    printf("public keys as in RFC 7748 section 6.2: %s\n", keys_ok ? "yes" : "NO");
    /* `diffie_hellman`: Alice multiplies Bob's key, Bob multiplies Alice's */
    uint8_t peer[2 * 56], shared[2 * 56], ok[2];
    memcpy(peer, pub + 56, 56);
    memcpy(peer + 56, pub, 56);
    CHECK(ecgpu_x448_batch(ctx, priv, peer, 2, shared, ok));
    printf("shared secret = ");
    for (int i = 0; i < 56; i++) printf("%02x", shared[i]);
    printf("\n");
    const int agree = ok[0] == 1 && ok[1] == 1 && memcmp(shared, shared + 56, 56) == 0;
    printf("both sides agree: %s\n", agree ? "yes" : "NO");
    const int expected = agree && memcmp(shared, want_shared, 56) == 0;
    printf("the expected shared secret: %s\n", expected ? "yes" : "NO");
    /* a low-order point (u = 1) beside a good one: ok = 0 and a zero record for it alone, the call itself succeeds */
    memset(peer, 0, 56);
    peer[0] = 1;
    CHECK(ecgpu_x448_batch(ctx, priv, peer, 2, shared, ok));
    uint8_t any = 0;
    for (int i = 0; i < 56; i++) any |= shared[i];
    const int refused = ok[0] == 0 && any == 0 && ok[1] == 1 && memcmp(shared + 56, want_shared, 56) == 0;
    printf("a low-order point is refused per element: %s\n", refused ? "yes" : "NO");
    memset(priv, 0, sizeof priv);
    memset(shared, 0, sizeof shared);
    CHECK(ecgpu_wipe(ctx));
    ecgpu_destroy(ctx);
    return keys_ok && expected && refused ? 0 : 2;
}
