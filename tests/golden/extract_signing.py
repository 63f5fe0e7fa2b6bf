#!/usr/bin/env python3
"""Extract the reference's signing known-answer vectors into tests/golden/signing.json (data only: hex constants, message
literals and the name of the hash a test applies; no reference source code is copied).

    python tests/golden/extract_signing.py [path to the reference checkout]

Sources:
  k256/src/schnorr.rs                     BIP340_SIGN_VECTORS 0-3 with secret_key and aux_rand (the public bip-0340 vectors)
  {p224,p256,p384,p521}/src/ecdsa.rs      `rfc6979()`: RFC 6979 appendix A.2 key, messages ("sample" / "test"), signatures
  p256/src/ecdsa.rs, p384/src/ecdsa.rs    `prehash_signer_signing_with_sha384` / `..._with_sha256`: a digest longer / shorter than
                                          the field, which pins bits2field
"""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "..", "..", "..", "reference")      # a checkout beside this repository
HEXLIT = re.compile(r'hex!\(\s*((?:"[0-9A-Fa-f\s]*"\s*)+)\)')


def clean(lit):
    return re.sub(r'[\s"]+', "", lit).lower()


def fn_body(text, name):
    start = text.index("fn %s()" % name)
    end = text.index("\n    }\n", start)
    return text[start:end]


def schnorr_sign_vectors():
    text = open(os.path.join(REF, "k256/src/schnorr.rs")).read()
    start = text.index("const BIP340_SIGN_VECTORS")
    block = text[start:text.index("\n    ];", start)]
    out = []
    for body in re.findall(r"SignVector\s*\{(.*?)\n        \},", block, re.S):
        rec = {"index": int(re.search(r"index:\s*(\d+)", body).group(1))}
        for name in ("secret_key", "public_key", "aux_rand", "message", "signature"):
            rec[name] = clean(re.search(r"%s:\s*hex!\(\s*((?:\"[0-9A-Fa-f\s]*\"\s*)+)\)" % name, body).group(1))
        out.append(rec)
    return out


def rfc6979_vectors(curve):
    body = fn_body(open(os.path.join(REF, curve, "src/ecdsa.rs")).read(), "rfc6979")
    lits = [clean(h) for h in HEXLIT.findall(body)]
    msgs = re.findall(r'\.sign\(b"([^"]*)"\)', body)
    assert len(lits) == 1 + len(msgs), (curve, len(lits), msgs)
    return [{"d": lits[0], "msg": m, "sig": s} for m, s in zip(msgs, lits[1:])]


def prehash_vector(curve, fn):
    body = fn_body(open(os.path.join(REF, curve, "src/ecdsa.rs")).read(), fn)
    lits = [clean(h) for h in HEXLIT.findall(body)]
    m = re.search(r'sha2::(Sha\d+)::digest\(b"([^"]*)"\)', body)
    assert len(lits) == 2 and m, (curve, fn)
    return {"d": lits[0], "hash": m.group(1).lower(), "msg": m.group(2), "sig": lits[1]}


def main():
    out = {
        "source": "tests/golden/extract_signing.py",
        "bip340_sign": schnorr_sign_vectors(),
        "rfc6979": {c: rfc6979_vectors(c) for c in ("p224", "p256", "p384", "p521")},
        "prehash": {"p256": prehash_vector("p256", "prehash_signer_signing_with_sha384"),
                    "p384": prehash_vector("p384", "prehash_signer_signing_with_sha256")},
    }
    with open(os.path.join(HERE, "signing.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("bip340_sign %d, rfc6979 %s, prehash %s" % (len(out["bip340_sign"]), {c: len(v) for c, v in out["rfc6979"].items()},
                                                     sorted(out["prehash"])))


if __name__ == "__main__":
    main()
