"""tests/x448_model.py pinned to the reference's own vectors (x448/src/lib.rs:326-494, tests/golden/x448.json): the two fixed vectors
of RFC 7748 section 5.2, the Alice / Bob exchange of section 6.2 and the iterated vector after 1 and after 1,000 iterations; then
the behaviour no vector shows — the aliases p and p + 1, 2^448 - 1, points on the twist, the clamp.  CPU only."""
import json
import os
import random

import x448_model as m

VEC = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "x448.json")))
P = m.P


def h(s):
    return bytes.fromhex(s)


def test_the_golden_vectors_including_the_thousandth_iteration():
    for v in VEC["fixed"]:
        assert m.x448(h(v["scalar"]), h(v["point"])) == (h(v["expected"]), 1)
        assert m.x448_unchecked(h(v["scalar"]), h(v["point"])) == h(v["expected"])
    ab = {k: h(v) for k, v in VEC["alice_bob"].items()}
    assert m.public_key(ab["alice_private"]) == ab["alice_public"] and m.public_key(ab["bob_private"]) == ab["bob_public"]
    assert m.x448(ab["alice_private"], ab["bob_public"]) == (ab["shared"], 1) == m.x448(ab["bob_private"], ab["alice_public"])
    assert [h(r) for r in VEC["low_order"]] == list(m.LOW_ORDER)
    k = u = h(VEC["iterated"]["start"])
    assert u == m.le(m.BASE_U)
    for i in range(1, 1001):
        r, ok = m.x448(k, u)
        assert ok == 1
        k, u = r, k
        if i == 1:
            assert r == h(VEC["iterated"]["after_1"])
    assert r == h(VEC["iterated"]["after_1000"])


def test_low_order_rule_is_on_bytes_and_the_aliases_pass():
    rng = random.Random("x448-model-alias")
    k = bytes(rng.getrandbits(8) for _ in range(56))
    for name in ("0", "1", "p-1"):
        assert m.x448(k, m.SPECIAL_U[name]) == (m.ZERO, 0)
        assert m.x448_unchecked(k, m.SPECIAL_U[name]) == m.ZERO
    for name in ("p", "p+1"):                                                # accepted, and the product is the zero record
        assert m.x448(k, m.SPECIAL_U[name]) == (m.ZERO, 1)
    assert set(m.ZERO_PRODUCT) == {n for n, u in m.SPECIAL_U.items() if m.x448_unchecked(k, u) == m.ZERO}
    # 2^448 - 1 = p + 2^224: treated as 2^224
    assert m.x448(k, m.SPECIAL_U["2^448-1"]) == m.x448(k, m.SPECIAL_U["2^224"]) and m.x448(k, m.SPECIAL_U["2^224"])[0] != m.ZERO
    assert m.x448(k, m.le(P + 5)) == (m.public_key(k), 1)


def test_twist_points_go_through():
    rng = random.Random("x448-model-twist")
    for _ in range(4):
        u = m.twist_u(rng)
        ui = int.from_bytes(u, "little")
        assert not m.on_curve(ui) and pow((ui ** 3 + m.A * ui * ui + ui) % P, (P - 1) // 2, P) == P - 1
        a, b = (bytes(rng.getrandbits(8) for _ in range(56)) for _ in range(2))
        ra, oka = m.x448(a, u)
        assert oka == 1 and ra != m.ZERO and not m.on_curve(int.from_bytes(ra, "little"))     # the product stays on the twist
        assert m.x448(b, ra) == m.x448(a, m.x448(b, u)[0])                                    # and the ladder commutes there too
    assert m.on_curve(m.BASE_U)


def test_the_clamp():
    assert m.clamp(bytes(56)) == 1 << 447 and m.clamp(b"\xff" * 56) == 2 ** 448 - 4
    u = m.le(5)
    assert m.x448_unchecked(b"\x03" + bytes(55), u) == m.x448_unchecked(bytes(56), u)        # bits 0, 1 are cleared
    assert m.x448_unchecked(bytes(55) + b"\x80", u) == m.x448_unchecked(bytes(56), u)        # bit 447 is set
    assert m.x448_unchecked(b"\x04" + bytes(55), u) != m.x448_unchecked(bytes(56), u)
    # DH agreement
    rng = random.Random("x448-model-dh")
    a, b = (bytes(rng.getrandbits(8) for _ in range(56)) for _ in range(2))
    assert m.x448(a, m.public_key(b)) == m.x448(b, m.public_key(a))
