#!/usr/bin/env python3
"""The X448 entry points on the GPU box: wall time per call at 2^20 elements in host memory, their kernel split, and the nearest
existing secret-scalar variable-base work of the same run beside them.

    python tools/gpu_x448_rates.py [LOG2N]        (default 20; writes to standard output: profiles/x448/rates.txt is a copy)

One process.  Host-pointer calls (there is no other form): PCIe staging included, the output arrays made once and reused.  One
warm-up round, then ROUNDS rounds with the calls alternating inside a round; median (min .. max).  The calls:
    ecgpu_x448_batch, ecgpu_x448_unchecked_batch, ecgpu_x448_base_batch
    ecgpu_batch_ecdh_ct on p384 and p521: a 384-bit and a 521-bit uniform-schedule variable-base multiplication per element
The kernel split comes from ecgpu_last_timing: from 2^19 elements a call is pipelined in pieces of 2^18, and the span reported is
the LAST piece's, so it is printed with the piece size beside it and scaled to the call.
"""
import ctypes
import importlib
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ROUNDS = 5
PIPE_MIN_LOG2, PIPE_CHUNK_LOG2 = 19, 18           # csrc/ecgpu_api.hip


def main():
    lg = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    n = 1 << lg
    ecgpu = importlib.import_module("elliptic-curves_amd")
    from gpu_common import rand_scalars
    eng = ecgpu.Engine(0)
    lib, ctx = eng._lib, eng._ctx
    u8p = ctypes.POINTER(ctypes.c_uint8)
    p = lambda a: a.ctypes.data_as(u8p)
    rng = np.random.default_rng(0x448)
    ks, us = rng.integers(0, 256, n * 56, dtype=np.uint8), rng.integers(0, 256, n * 56, dtype=np.uint8)
    out, ok = np.zeros(n * 56, np.uint8), np.zeros(n, np.uint8)
    calls = {
        "ecgpu_x448_batch": lambda: lib.ecgpu_x448_batch(ctx, p(ks), p(us), ctypes.c_size_t(n), p(out), p(ok)),
        "ecgpu_x448_unchecked_batch": lambda: lib.ecgpu_x448_unchecked_batch(ctx, p(ks), p(us), ctypes.c_size_t(n), p(out)),
        "ecgpu_x448_base_batch": lambda: lib.ecgpu_x448_base_batch(ctx, p(ks), ctypes.c_size_t(n), p(out)),
    }
    keep = []
    for name, cid in (("p384", ecgpu.P384), ("p521", ecgpu.P521)):
        L = ecgpu.FIELD_BYTES[cid]
        sc = np.ascontiguousarray(rand_scalars(cid, n, 0x5448 + cid)).reshape(-1)
        pts, _ = eng.mul_by_generator(cid, np.ascontiguousarray(rand_scalars(cid, n, 0x6448 + cid)).reshape(-1))
        x, okx = np.zeros(n * L, np.uint8), np.zeros(n, np.uint8)
        keep.append((sc, pts, x, okx))
        calls["ecgpu_batch_ecdh_ct (%s)" % name] = (lambda cid=cid, sc=sc, pts=pts, x=x, okx=okx:
                                                   lib.ecgpu_batch_ecdh_ct(ctx, cid, p(sc), p(pts), ctypes.c_size_t(n), p(x), p(okx)))
    pieces = (n >> PIPE_CHUNK_LOG2) if lg >= PIPE_MIN_LOG2 else 1
    print("2^%d elements in pageable host memory (host-pointer calls: PCIe staging included), one process, output arrays reused;" % lg)
    print("median of %d rounds after one warm-up round, the calls alternating inside a round; ms per call (min .. max);" % ROUNDS)
    print("kernels: ecgpu_last_timing \"total\" of the call's last piece (%d piece%s of 2^%d), times the pieces" % (
        pieces, "" if pieces == 1 else "s", lg if pieces == 1 else PIPE_CHUNK_LOG2))
    times, spans = {k: [] for k in calls}, {k: [] for k in calls}
    for rnd in range(ROUNDS + 1):
        for name, fn in calls.items():
            t0 = time.perf_counter()
            rc = fn()
            ms = (time.perf_counter() - t0) * 1e3
            if rc != 0:
                print("STOPPED: %s returned %d (%s)" % (name, rc, eng.last_error() if hasattr(eng, "last_error") else ""), flush=True)
                return 1
            if rnd:
                times[name].append(ms)
                spans[name].append((eng.last_timing("total") or 0.0) * pieces)
    for name, v in times.items():
        med, ker = statistics.median(v), statistics.median(spans[name])
        print("  %-30s %9.2f ms  (%8.2f .. %8.2f)   %6.2f M/s   kernels %8.2f ms = %5.1f ns per element" % (
            name, med, min(v), max(v), n / med / 1e3, ker, ker * 1e6 / n), flush=True)
    assert int(ok.sum()) == n
    eng.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
