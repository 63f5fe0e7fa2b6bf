#!/usr/bin/env python3
"""Run by tests/test_gpu_comb_table.py::test_adaptive_tiers_in_a_fresh_process, one scenario per fresh process:

    gpu_table_tiers_check.py <sync | async | second_context | verifier> [oracle result file]

The default policy moves a device from the 16-bit generator table to the 22-bit one once it has been asked for 2^26 generator
multiplications of a curve, and to the widest (26 bits for k256) at 2^29 (csrc/ecgpu_api.hip table_tier / ensure_table; the count
includes the call being served).  The count is per device and process, and this script makes no generator call beyond those it
lists, so the count is known exactly before every call: ecgpu_batch_mul_base[_dev] and the verifications add their n; the signing
calls run on the uniform-schedule LUTs (ensure_ct_lut) and add nothing.

  sync            walks call by call to the first call at or above 2^29: window_bits is 16 / 16 -> 22 / 22 -> 26 around the two
                  thresholds, the bytes of the calls around them equal the oracle's, bytes / build_ms of the tables are plausible
  async           the same walk queued on an asynchronous context without a synchronize in between: the crossing call builds its
                  table before it returns, and the buffers written by the last narrow-table call and the first wide-table call hold
                  the right bytes at the end (the crossing call waits for its stream before the narrow table goes)
  second_context  B has work queued on the 16-bit table while A crosses: B's results are right, the 16-bit table is still B's, and
                  B's next call takes the table A paid for without a second build
  verifier        the call that reaches 2^26 is an ecdsa_verify of 4,096 valid signatures

k256, default policy, no pin, no budget.  Results never depend on the width (oracle: the checker)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]
import comb_vectors as cv
import oracle_lib
import pyec
from gpu_common import comb_corner_scalars, ecgpu_module, rand_scalars

CURVE = pyec.CURVES["k256"]
N = (1 << 20) + 12345
NSIG = 4096


def head():
    return [k for w in cv.WIDTHS["k256"] for k in comb_corner_scalars(CURVE, w)]


def batch():
    scal = rand_scalars(CURVE.cid, N, 0xC03B71E5).copy()
    h = head()
    scal[: len(h) * CURVE.L] = np.frombuffer(cv.enc(CURVE, h), np.uint8)
    return scal


def crossing_calls():
    """(i1, i2): the 1-based indices of the first calls of N scalars each that find the count at or above the two thresholds"""
    t1, t2 = cv.tier_thresholds()
    i1, i2 = -(-t1 // N), -(-t2 // N)
    w = cv.widest(CURVE)
    assert cv.table_tier((i1 - 1) * N, w) == 16 and cv.table_tier(i1 * N, w) == 22
    assert cv.table_tier((i2 - 1) * N, w) == 22 and cv.table_tier(i2 * N, w) == w == 26
    return i1, i2


def table_bytes(w):
    return (1 << (w - 1)) * cv.window_count(CURVE, w) * 2 * cv.words(CURVE) * 4


def plausible(info, w):
    assert info["window_bits"] == w and info["bytes"] == table_bytes(w) and 0 < info["build_ms"] < 60000, (w, info)


class Walk:
    def __init__(self, want_file):
        self.ecgpu = ecgpu_module()
        self.c = CURVE
        self.scal = batch()
        if want_file:
            both = np.load(want_file)
            self.want, self.winf = both[: N * 64], both[N * 64:]
        else:
            self.want, self.winf = oracle_lib.batch_mul_base_mt(self.c.cid, self.scal)
        assert self.want.size == N * 64 and self.winf.size == N

    def buffers(self, eng, count):
        return [(eng.dev_alloc(N * 64), eng.dev_alloc(N)) for _ in range(count)]

    def right(self, eng, buf, what):
        xy, inf = eng.to_host(buf[0], N * 64), eng.to_host(buf[1], N)
        assert bytes(xy) == bytes(self.want) and bytes(inf) == bytes(self.winf), what

    def width(self, eng):
        return eng.base_table_info(self.c.cid)["window_bits"]


def walk(wk, asynchronous):
    i1, i2 = crossing_calls()
    named = {1: 16, i1 - 1: 16, i1: 22, i2 - 1: 22, i2: 26}
    a = wk.ecgpu.Engine(0)
    assert wk.width(a) == 0
    if asynchronous:
        a.set_async(True)
    d_s = a.to_device(wk.scal)
    ring = wk.buffers(a, 4)
    kept = {i: buf for i, buf in zip(sorted(named), wk.buffers(a, len(named)))}     # the named calls write buffers of their own
    infos = {}
    for i in range(1, i2 + 1):
        buf = kept.get(i) or ring[i % 4]
        a.mul_by_generator_dev(wk.c.cid, d_s, N, buf[0], buf[1])
        if i in named:
            # on an asynchronous context too the table is there when the crossing call returns
            infos[i] = a.base_table_info(wk.c.cid)
            plausible(infos[i], named[i])
            if not asynchronous:
                wk.right(a, buf, "call %d at %d bits" % (i, named[i]))
    if asynchronous:
        a.synchronize()
        for i in sorted(named):
            wk.right(a, kept[i], "call %d at %d bits (queued, read at the end)" % (i, named[i]))
    assert infos[i1]["build_ms"] != infos[i1 - 1]["build_ms"] and infos[i2]["bytes"] > infos[i1]["bytes"] > infos[1]["bytes"]
    a.close()
    print("tiers %s ok: 16 bits to call %d, 22 to call %d, 26 from call %d; builds %.1f / %.1f / %.1f ms" % (
        "async" if asynchronous else "sync", i1 - 1, i2 - 1, i2, infos[1]["build_ms"], infos[i1]["build_ms"], infos[i2]["build_ms"]))


def second_context(wk):
    i1, _ = crossing_calls()
    queued = 3
    assert i1 - 1 - queued >= 1
    a, b = wk.ecgpu.Engine(0), wk.ecgpu.Engine(0)
    d_sa, d_sb = a.to_device(wk.scal), b.to_device(wk.scal)
    ring = wk.buffers(a, 2)
    for i in range(1, i1 - queued):                               # calls 1 .. i1 - 1 - queued on A
        a.mul_by_generator_dev(wk.c.cid, d_sa, N, *ring[i % 2])
    assert wk.width(a) == 16
    b.set_async(True)
    bq = wk.buffers(b, queued + 1)
    for buf in bq[:queued]:                                       # calls i1 - queued .. i1 - 1, queued on B's stream
        b.mul_by_generator_dev(wk.c.cid, d_sb, N, *buf)
    assert wk.width(b) == 16
    a.mul_by_generator_dev(wk.c.cid, d_sa, N, *ring[0])           # call i1: A crosses while B's work is in flight
    info_a = a.base_table_info(wk.c.cid)
    plausible(info_a, 22)
    wk.right(a, ring[0], "A's crossing call")
    b.synchronize()
    for k, buf in enumerate(bq[:queued]):
        wk.right(b, buf, "B's queued call %d on the 16-bit table" % k)
    plausible(b.base_table_info(wk.c.cid), 16)                    # still B's: A's release did not free it
    b.mul_by_generator_dev(wk.c.cid, d_sb, N, *bq[queued])
    b.synchronize()
    info_b = b.base_table_info(wk.c.cid)
    assert info_b == info_a, (info_a, info_b)                     # the table A paid for: same bytes, same build time, no second build
    wk.right(b, bq[queued], "B's first call on A's table")
    b.close()
    a.mul_by_generator_dev(wk.c.cid, d_sa, N, *ring[1])
    assert wk.width(a) == 22
    wk.right(a, ring[1], "A after B has gone")
    a.close()
    print("tiers second_context ok: B moved to A's 22-bit table (built once, %.1f ms)" % info_a["build_ms"])


def verifier(wk):
    import random
    c = wk.c
    t1, _ = cv.tier_thresholds()
    rng = random.Random(0xC03B5167)
    a = wk.ecgpu.Engine(0)
    seen = 0
    keys = cv.enc(c, [rng.randrange(1, c.n) for _ in range(NSIG)])
    q, qinf = a.mul_by_generator(c.cid, keys)                     # counts NSIG
    seen += NSIG
    assert not qinf.any()
    z = bytes(rng.randrange(256) for _ in range(NSIG * c.L))
    sig, _, ok = a.ecdsa_sign_rfc6979(c.cid, keys, z, normalize_s=True)      # the uniform-schedule LUTs: counts nothing
    assert ok.all()
    S = np.asarray(sig).reshape(NSIG, 2 * c.L)
    r, s = np.ascontiguousarray(S[:, : c.L]).reshape(-1), np.ascontiguousarray(S[:, c.L:]).reshape(-1)
    d_s = a.to_device(wk.scal)
    out = wk.buffers(a, 1)[0]
    while seen + N < t1:
        a.mul_by_generator_dev(c.cid, d_s, N, *out)
        seen += N
    last = t1 - 1 - seen                                          # one short call: the count stands at 2^26 - 1
    assert 0 < last <= N
    a.mul_by_generator_dev(c.cid, d_s, last, *out)
    seen += last
    assert seen == t1 - 1 and wk.width(a) == 16
    got = a.ecdsa_verify(c.cid, z, r, s, q)                       # the call that reaches 2^26
    assert got.size == NSIG and got.all(), int(got.sum())
    plausible(a.base_table_info(c.cid), 22)
    a.mul_by_generator_dev(c.cid, d_s, N, *out)
    wk.right(a, out, "after the verifier's crossing")
    a.close()
    print("tiers verifier ok: %d valid signatures verified by the call that reached 2^26" % NSIG)


if __name__ == "__main__":
    mode = sys.argv[1]
    wk = Walk(sys.argv[2] if len(sys.argv) > 2 else None)
    {"sync": lambda: walk(wk, False), "async": lambda: walk(wk, True), "second_context": lambda: second_context(wk),
     "verifier": lambda: verifier(wk)}[mode]()
