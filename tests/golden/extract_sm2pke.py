#!/usr/bin/env python3
"""Extract the reference's SM2 public-key encryption vectors into tests/golden/sm2pke.json (data only).

    python tests/golden/extract_sm2pke.py <checkout of the reference>

Source: sm2/tests/sm2pke.rs — PRIVATE_KEY, MSG, CIPHER (04 || C1 || C3 || C2, the C1C3C2 mode) and ASN1_CIPHER (the DER form
`openssl pkeyutl -encrypt` writes).  Only the constants are taken; no reference source code is copied.
"""
import ast
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def hex_const(text, name):
    m = re.search(r'const %s: \[u8; (\d+)\] =\s*hex!\(\s*"([0-9a-fA-F\s]+)"\s*\);' % name, text)
    value = re.sub(r"\s", "", m.group(2)).lower()
    assert len(value) == 2 * int(m.group(1)), name
    return value


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    text = open(os.path.join(sys.argv[1], "sm2", "tests", "sm2pke.rs")).read()
    msg = ast.literal_eval("b" + re.search(r'const MSG: &\[u8\] = b("(?:[^"\\]|\\.)*");', text).group(1))
    out = {"private_key": hex_const(text, "PRIVATE_KEY"), "msg": msg.hex(), "cipher": hex_const(text, "CIPHER"),
           "asn1_cipher": hex_const(text, "ASN1_CIPHER")}
    path = os.path.join(HERE, "sm2pke.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
