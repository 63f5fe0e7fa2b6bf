#!/usr/bin/env python3
"""The uniform-schedule entry points on projective records (ecgpu_batch_mul_ct_xyz, ecgpu_lincomb_ct_xyz) on the GPU box:
rates beside their affine twins, and the dynamic twin of `tools/ct_isa_check.py --kernels k_xyz_mul_ct`, in the style of
tools/gpu_ct_rates.py.

    python tools/gpu_ct_xyz_rates.py               rates, then the counters
    python tools/gpu_ct_xyz_rates.py --rates       the rates only
    python tools/gpu_ct_xyz_rates.py --counters    the counters only
    python tools/gpu_ct_xyz_rates.py --child CLASS (internal) one launch set under rocprofv3 --pmc for input class CLASS

Rates: 2^20 device-resident elements, the xyz call and its affine twin on the same points, alternated (HIP-event times of
the whole call, median of five); and the single-thread CPU cost of what a caller without the xyz forms pays first, `to_affine`
per point (the oracle's batch_normalize of one point at a time, a sample timed and extrapolated).

Counter check: each input class {scalars: zero, n - 1, random} x {records: random points with Z = 1, random points under a
random z each, G under a random z each, Z = 0 with random X, Y < p} runs in a process of its own under
`rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_INSTS_LDS` (no tracing alongside);
k_xyz_mul_ct and the tree k_proj_sum_level of ecgpu_lincomb_ct_xyz must show IDENTICAL counts across the classes.  The
variable-time k_var_base of the same scalars over the same points (as affine records) runs in the same processes and must
DIFFER: the check can see a difference.  Sizes are fixed so that the launch geometry is the same."""
import csv
import glob
import os
import random
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import importlib  # noqa: E402

CURVES = {"k256": 0, "p256": 1, "p384": 2}
N_PMC = 1 << 14
CLASSES = ["zero_z1", "nm1_randz", "rand_randz", "rand_Gz", "rand_Z0", "zero_Z0"]


def engine():
    ecgpu = importlib.import_module("elliptic-curves_amd")
    return ecgpu, ecgpu.Engine(0)


def rand_scalars(cid, n, seed):
    from gpu_common import rand_scalars as rs
    return rs(cid, n, seed)


def to_xyz(c, pts, zs):
    """affine wire records (no identities) -> X || Y || Z with Z = zs[i]"""
    L = c.L
    P = np.asarray(pts).reshape(-1, 2, L)
    out = bytearray()
    for i in range(P.shape[0]):
        x, y, z = int.from_bytes(bytes(P[i, 0]), c.order), int.from_bytes(bytes(P[i, 1]), c.order), zs[i]
        out += (x * z % c.p).to_bytes(L, c.order) + (y * z % c.p).to_bytes(L, c.order) + z.to_bytes(L, c.order)
    return np.frombuffer(bytes(out), np.uint8).copy()


def make_inputs(eng, ecgpu, cid, n, cls):
    import pyec
    c = [v for v in pyec.CURVES.values() if v.cid == cid][0]
    L = c.L
    kind_k, kind_p = cls.split("_")
    if kind_k == "zero":
        ks = np.zeros(n * L, np.uint8)
    elif kind_k == "nm1":
        ks = np.frombuffer((c.n - 1).to_bytes(L, c.order) * n, np.uint8).copy()
    else:
        ks = rand_scalars(cid, n, 0xC7A0 + cid)
    rng = random.Random(0xC7A2 + cid)
    if kind_p == "Gz":
        one = np.frombuffer((1).to_bytes(L, c.order) * n, np.uint8)
        pts, _ = eng.mul_by_generator(cid, one)
    else:
        pts, _ = eng.mul_by_generator(cid, rand_scalars(cid, n, 0xC7A1 + cid))
    if kind_p == "z1":
        xyz = to_xyz(c, pts, [1] * n)
    elif kind_p == "Z0":
        xyz = np.frombuffer(b"".join(rng.randrange(c.p).to_bytes(L, c.order) + rng.randrange(c.p).to_bytes(L, c.order) + bytes(L)
                                     for _ in range(n)), np.uint8).copy()
    else:
        xyz = to_xyz(c, pts, [rng.randrange(1, c.p) for _ in range(n)])
    return ks, pts, xyz


def child(cls):
    ecgpu, eng = engine()
    for name, cid in CURVES.items():
        L = ecgpu.FIELD_BYTES[cid]
        ks, pts, xyz = make_inputs(eng, ecgpu, cid, N_PMC, cls)
        d_k, d_p, d_x = eng.to_device(ks), eng.to_device(pts), eng.to_device(xyz)
        d_o, d_f = eng.dev_alloc(N_PMC * 2 * L), eng.dev_alloc(N_PMC)
        eng.mul_dev(cid, d_k, d_p, None, N_PMC, d_o, d_f)                    # variable-time: must differ across classes
        eng.mul_xyz_dev(cid, d_k, d_x, N_PMC, d_o, d_f, constant_time=True)
        eng.lincomb_ct_xyz_dev(cid, d_k, d_x, N_PMC, d_o, d_f)              # k_xyz_mul_ct once more + the k_proj_sum_level tree
    eng.close()


def counters(cls):
    out = "/tmp/ct_xyz_pmc_%s" % cls
    cmd = ["rocprofv3", "--pmc", "SQ_INSTS_VALU", "SQ_INSTS_SALU", "SQ_INSTS_VMEM_RD", "SQ_INSTS_VMEM_WR", "SQ_INSTS_LDS",
           "--output-format", "csv", "-d", out, "-o", "pmc", "--", sys.executable, os.path.abspath(__file__), "--child", cls]
    r = subprocess.run(cmd, cwd="/tmp", env=dict(os.environ, TMPDIR="/tmp"), capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError("class %s: rocprofv3 exited with %d\n%s" % (cls, r.returncode, r.stderr[-2000:]))
    res = {}
    for f in glob.glob(os.path.join(out, "**", "*counter_collection.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            k = row["Kernel_Name"].split("(")[0].replace("void ", "").replace("ecgpu::", "")
            if not (k.startswith("k_xyz_mul_ct") or k.startswith("k_proj_sum_level") or k.startswith("k_var_base<")):
                continue
            if k.startswith("k_proj_sum_level"):      # the levels of the tree: all launches of the process, summed
                d = res.setdefault(k, {})
                d[row["Counter_Name"]] = d.get(row["Counter_Name"], 0.0) + float(row["Counter_Value"])
                continue
            res.setdefault(k, {})[row["Counter_Name"]] = float(row["Counter_Value"])     # the last launch of the kernel
    if not res:
        raise RuntimeError("no counters for %s:\n%s" % (cls, r.stderr[-1500:]))
    return res


def timed(eng, fn, reps=5):
    ts = []
    for _ in range(reps):
        fn()
        ts.append(eng.last_timing("total"))
    return statistics.median(ts)


def rates():
    import oracle_lib
    import pyec
    ecgpu, eng = engine()
    n = 1 << 20
    print("rates, 2^20 device-resident elements, whole-call HIP-event time, median of 5, xyz and affine twin alternated:")
    for name, cid in CURVES.items():
        c = pyec.CURVES[name]
        L = c.L
        ks = rand_scalars(cid, n, 0xC7B0 + cid)
        pts, _ = eng.mul_by_generator(cid, rand_scalars(cid, n, 0xC7B1 + cid))
        rng = random.Random(0xC7B2 + cid)
        xyz = to_xyz(c, pts, [rng.randrange(1, c.p) for _ in range(n)])
        d_k, d_p, d_x = eng.to_device(ks), eng.to_device(pts), eng.to_device(xyz)
        d_o, d_f = eng.dev_alloc(n * 2 * L), eng.dev_alloc(n)
        d_o2, d_f2 = eng.dev_alloc(n * 2 * L), eng.dev_alloc(n)
        for what in ("mul_ct", "lincomb_ct"):
            tx, ta = [], []
            for rnd in range(3):
                if what == "mul_ct":
                    tx.append(timed(eng, lambda: eng.mul_xyz_dev(cid, d_k, d_x, n, d_o, d_f, constant_time=True)))
                    ta.append(timed(eng, lambda: eng.mul_dev(cid, d_k, d_p, None, n, d_o2, d_f2, constant_time=True)))
                    same = bytes(eng.to_host(d_o, n * 2 * L)) == bytes(eng.to_host(d_o2, n * 2 * L))
                else:
                    tx.append(timed(eng, lambda: eng.lincomb_ct_xyz_dev(cid, d_k, d_x, n, d_o, d_f)))
                    ta.append(timed(eng, lambda: eng.lincomb_ct_dev(cid, d_k, d_p, None, n, d_o2, d_f2)))
                    same = bytes(eng.to_host(d_o, 2 * L)) == bytes(eng.to_host(d_o2, 2 * L))
            mx, ma = statistics.median(tx), statistics.median(ta)
            print("  %-5s %-10s xyz %8.3f ms   affine twin %8.3f ms   xyz / twin %.4f  (%+.2f %%)   results equal: %s" % (
                name, what, mx, ma, mx / ma, (mx / ma - 1) * 100, same), flush=True)
        for b in (d_k, d_p, d_x, d_o, d_f, d_o2, d_f2):
            b.free()
    # the path the xyz forms replace: to_affine on the CPU, one inversion per point, one thread
    print("single-thread CPU to_affine (oracle batch_normalize of one point per call), sampled and extrapolated:")
    for name in CURVES:
        c = pyec.CURVES[name]
        rng = random.Random(0xC7C0 + c.cid)
        P = pyec.mul(c, rng.randrange(1, c.n), pyec.G(c))
        recs = []
        for _ in range(2000):
            z = rng.randrange(1, c.p)
            recs.append(np.frombuffer((P[0] * z % c.p).to_bytes(c.L, c.order) + (P[1] * z % c.p).to_bytes(c.L, c.order)
                                      + z.to_bytes(c.L, c.order), np.uint8).copy())
        t0 = time.perf_counter()
        for r in recs:
            oracle_lib.batch_normalize(c.cid, r)
        per = (time.perf_counter() - t0) / len(recs)
        print("  %-5s %.2f us per point (incl. the ctypes call)  ->  2^20: %.0f ms   2^24: %.2f s" % (
            name, per * 1e6, per * (1 << 20) * 1e3, per * (1 << 24)), flush=True)
    eng.close()


def check_counters():
    print("executed-instruction counters per launch (%d elements), one process per input class:" % N_PMC)
    allc = {cls: counters(cls) for cls in CLASSES}
    kernels = sorted({k for c in allc.values() for k in c})
    bad = 0
    for k in kernels:
        rows = {cls: allc[cls].get(k, {}) for cls in CLASSES}
        names = sorted({c for r in rows.values() for c in r})
        uniform = all(len({rows[cls].get(c) for cls in CLASSES}) == 1 for c in names)
        is_ct = k.startswith("k_xyz_mul_ct") or k.startswith("k_proj_sum_level")
        ok = uniform == is_ct
        bad += 0 if ok else 1
        print("  %-40s %s across %s  [%s]" % (k, "IDENTICAL" if uniform else "DIFFER", "/".join(CLASSES),
                                             "as required" if ok else "UNEXPECTED"))
        for c in names:
            print("      %-18s %s" % (c, "  ".join("%.0f" % rows[cls].get(c, float("nan")) for cls in CLASSES)))
    if not any(k.startswith("k_xyz_mul_ct") for k in kernels):
        bad += 1
        print("  k_xyz_mul_ct not seen")
    print("counter check: %s" % ("PASS" if bad == 0 else "FAIL (%d kernels)" % bad))
    return bad


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        return child(sys.argv[2])
    if "--counters" not in sys.argv:
        rates()
    if "--rates" in sys.argv:
        return 0
    return check_counters()


if __name__ == "__main__":
    sys.exit(main() or 0)
