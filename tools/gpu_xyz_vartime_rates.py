#!/usr/bin/env python3
"""The variable-time entry points on projective records (ecgpu_msm_xyz_dev, ecgpu_msm_parts_xyz_dev, ecgpu_batch_mul_xyz_dev,
ecgpu_batch_mul_base_and_mul_add_xyz_dev) on the GPU box, in the style of tools/gpu_ct_xyz_rates.py: each xyz call alternated
with its affine twin on the same device-resident points (a random z under every record), wall time of the whole call, median
of five, and whether the results are equal.  Then the conversion kernel alone (k_xyz_affine) at 2^24 k256 records under
`rocprofv3 --kernel-trace --stats` in a child process, with the bandwidth its byte formula gives.

    python tools/gpu_xyz_vartime_rates.py            rates, then the trace
    python tools/gpu_xyz_vartime_rates.py --rates    the rates only
    python tools/gpu_xyz_vartime_rates.py --trace    the trace only
    python tools/gpu_xyz_vartime_rates.py --child    (internal) the traced process

Bytes per record of k_xyz_affine: Z read in the product pass (L), the prefix entry written (4 NS) and read back (4 NS), X || Y || Z
read in the back pass (3 L), x || y + flag written (2 L + 1): 289 bytes for k256 (L = 32, NS = 12)."""
import csv
import ctypes
import glob
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import importlib  # noqa: E402

HBM_TBS = 6.3            # achievable HBM bandwidth of MI355X the guides quote (TB/s)


def setup():
    ecgpu = importlib.import_module("elliptic-curves_amd")
    import pyec
    from gpu_common import fast_scalars
    from test_xyz_vartime import build_helper
    return ecgpu, pyec, fast_scalars, build_helper()


def points(eng, hx, c, n, seed, fast_scalars):
    """device-resident affine points s_i G and their X || Y || Z records under random z (compiled generator)"""
    import ctypes
    u8p = ctypes.POINTER(ctypes.c_uint8)
    L = c.L
    s = fast_scalars(c, n, seed).reshape(-1)
    d_s = eng.to_device(s)
    d_a = eng.dev_alloc(n * 2 * L)
    eng.mul_by_generator_dev(c.cid, d_s, n, d_a, None)
    d_s.free()
    xy = eng.to_host(d_a)
    f = np.zeros(n, np.uint8)
    xyz = np.empty(n * 3 * L, np.uint8)
    assert hx.hx_rescale(c.cid, xy.ctypes.data_as(u8p), f.ctypes.data_as(u8p), ctypes.c_size_t(n), ctypes.c_uint64(seed), 0,
                         xyz.ctypes.data_as(u8p)) == 0
    del xy
    d_x = eng.to_device(xyz)
    return d_a, d_x


def wall(eng, fn):
    t0 = time.perf_counter()
    fn()
    eng.synchronize()
    return (time.perf_counter() - t0) * 1e3


def alternate(eng, fx, fa, same, reps=5):
    tx, ta = [], []
    fx(), fa()                                                   # warm: scratch allocations, tables
    for _ in range(reps):
        tx.append(wall(eng, fx))
        ta.append(wall(eng, fa))
    mx, ma = statistics.median(tx), statistics.median(ta)
    return "xyz %9.3f ms   affine twin %9.3f ms   xyz / twin %.4f  (%+.2f %%)   results equal: %s" % (
        mx, ma, mx / ma, (mx / ma - 1) * 100, same())


def rates():
    ecgpu, pyec, fast_scalars, hx = setup()
    eng = ecgpu.Engine(0)
    print("rates: device-resident inputs, wall time of the whole call (to its end on the device), median of 5, xyz and affine "
          "twin alternated")
    c = pyec.CURVES["k256"]
    L = c.L
    for lg in (24, 21):
        n = 1 << lg
        d_a, d_x = points(eng, hx, c, n, 0x5150 + lg, fast_scalars)
        d_k = eng.to_device(fast_scalars(c, n, 0x5160 + lg).reshape(-1))
        o1, f1, o2, f2 = eng.dev_alloc(64), eng.dev_alloc(16), eng.dev_alloc(64), eng.dev_alloc(16)
        same = lambda: bytes(eng.to_host(o1, 2 * L)) == bytes(eng.to_host(o2, 2 * L))
        print("  k256  msm 2^%d        %s" % (lg, alternate(eng, lambda: eng.lincomb_xyz_dev(c.cid, d_k, d_x, n, o1, f1),
                                                          lambda: eng.lincomb_dev(c.cid, d_k, d_a, None, n, o2, f2), same)), flush=True)
        if lg == 21:
            # four back-to-back local halves on two lanes (asynchronous context), each joined and finished behind the next
            pb = (eng.msm_parts_bytes(c.cid, n) + 15) // 16 * 16
            parts = [eng.dev_alloc(pb) for _ in range(2)]

            def run(xyz):
                for i in range(4):
                    if xyz:
                        eng.msm_parts_xyz_dev(c.cid, d_k, d_x, n, n, parts[i % 2])
                    else:
                        eng.msm_parts_dev(c.cid, d_k, d_a, None, n, n, parts[i % 2])
                    if i:
                        eng.msm_parts_join_dev(parts[(i - 1) % 2])
                        eng.msm_finish_dev(c.cid, parts[(i - 1) % 2], 1, n, o1 if xyz else o2, f1 if xyz else f2)
                eng.msm_parts_join_dev(parts[1])
                eng.msm_finish_dev(c.cid, parts[1], 1, n, o1 if xyz else o2, f1 if xyz else f2)
            eng.set_async(True)
            eng.set_msm_lanes(2)
            try:
                line = alternate(eng, lambda: run(True), lambda: run(False), lambda: True)
            finally:
                eng.set_msm_lanes(1)
                eng.set_async(False)
            print("  k256  4 x parts 2^21 on 2 lanes   %s (records: %s)" % (line.split("   results")[0], same()), flush=True)
            for b in parts:
                b.free()
        for b in (d_a, d_x, d_k, o1, f1, o2, f2):
            b.free()
    n = 1 << 20
    for name, what in (("p256", "mul"), ("p384", "mul"), ("k256", "mul_add"), ("p256", "mul_add")):
        c = pyec.CURVES[name]
        L = c.L
        d_a, d_x = points(eng, hx, c, n, 0x5170 + c.cid, fast_scalars)
        d_k = eng.to_device(fast_scalars(c, n, 0x5180 + c.cid).reshape(-1))
        d_b = eng.to_device(fast_scalars(c, n, 0x5190 + c.cid).reshape(-1))
        o1, f1, o2, f2 = eng.dev_alloc(n * 2 * L), eng.dev_alloc(n), eng.dev_alloc(n * 2 * L), eng.dev_alloc(n)
        same = lambda: bytes(eng.to_host(o1)) == bytes(eng.to_host(o2)) and bytes(eng.to_host(f1)) == bytes(eng.to_host(f2))
        if what == "mul":
            line = alternate(eng, lambda: eng.mul_vartime_xyz_dev(c.cid, d_k, d_x, n, o1, f1),
                             lambda: eng.mul_dev(c.cid, d_k, d_a, None, n, o2, f2), same)
        else:
            line = alternate(eng, lambda: eng.mul_by_generator_and_mul_add_xyz_dev(c.cid, d_b, d_k, d_x, n, o1, f1),
                             lambda: eng._chk(eng._lib.ecgpu_batch_mul_base_and_mul_add_dev(      # (no Engine method for the affine _dev form)
                                 eng._ctx, c.cid, ecgpu._dp(d_b), ecgpu._dp(d_k), ecgpu._dp(d_a), None, ctypes.c_size_t(n),
                                 ecgpu._dp(o2), ecgpu._dp(f2))), same)
        print("  %-5s %-7s 2^20    %s" % (name, what, line), flush=True)
        for b in (d_a, d_x, d_k, d_b, o1, f1, o2, f2):
            b.free()
    eng.close()


def child():
    ecgpu, pyec, fast_scalars, hx = setup()
    eng = ecgpu.Engine(0)
    c = pyec.CURVES["k256"]
    n = 1 << 24
    d_a, d_x = points(eng, hx, c, n, 0x5200, fast_scalars)
    d_k = eng.to_device(fast_scalars(c, n, 0x5201).reshape(-1))
    o, f = eng.dev_alloc(64), eng.dev_alloc(16)
    for _ in range(5):
        eng.lincomb_xyz_dev(c.cid, d_k, d_x, n, o, f)
    eng.close()


def trace():
    out = "/tmp/xyz_vartime_trace"
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "kt", "--", sys.executable,
           os.path.abspath(__file__), "--child"]
    r = subprocess.run(cmd, cwd="/tmp", env=dict(os.environ, TMPDIR="/tmp"), capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        print("rocprofv3 exited with %d\n%s" % (r.returncode, r.stderr[-2000:]))
        return 1
    durs = []
    for fn in glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True):
        for row in csv.DictReader(open(fn)):
            if "k_xyz_affine" in row["Kernel_Name"]:
                durs.append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e6)
    if not durs:
        print("k_xyz_affine not in the trace")
        return 1
    n, L, NS = 1 << 24, 32, 12
    per = L + 4 * NS + 4 * NS + 3 * L + 2 * L + 1
    ms = statistics.median(durs)
    gbs = n * per / (ms * 1e-3) / 1e9
    print("k_xyz_affine<K256Params>, 2^24 records, %d launches: median %.3f ms (min %.3f, max %.3f)" % (
        len(durs), ms, min(durs), max(durs)))
    print("  byte formula %d B per record = %.2f GB -> %.0f GB/s = %.1f %% of %.1f TB/s" % (
        per, n * per / 1e9, gbs, gbs / (HBM_TBS * 10), HBM_TBS))
    top = sorted(glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True))
    if top:
        rows = list(csv.DictReader(open(top[0])))
        rows.sort(key=lambda r: -float(r.get("TotalDurationNs", 0)))
        print("  kernel stats of the child (top 8 by total time):")
        for r in rows[:8]:
            print("    %-60s calls %5s  total %9.3f ms  avg %8.3f ms" % (r["Name"][:60], r["Calls"], float(r["TotalDurationNs"]) / 1e6,
                                                                      float(r["AverageNs"]) / 1e6))
    return 0


def main():
    if "--child" in sys.argv:
        return child()
    if "--trace" not in sys.argv:
        rates()
    if "--rates" in sys.argv:
        return 0
    return trace()


if __name__ == "__main__":
    sys.exit(main() or 0)
