#!/usr/bin/env python3
"""The signing entry points on the GPU box: rates beside ecgpu_batch_mul_base_ct, the kernel split of each call, and the dynamic
twin of tools/ct_isa_check.py --unit sign — executed-instruction counters of the data-independent kernels for inputs that differ as
much as inputs can.

    python tools/gpu_sign_rates.py              the three parts below, one after the other
    python tools/gpu_sign_rates.py --rates      wall time per call at 2^20 device-resident elements, k256 and p256: the three ECDSA
                                                forms, BIP340 (k256), and ecgpu_batch_mul_base_ct at the same n in the same process
    python tools/gpu_sign_rates.py --trace      each form once per curve under `rocprofv3 --kernel-trace --stats`, a run of its own
                                                per form: the kernels of the call by share of its GPU time
    python tools/gpu_sign_rates.py --pmc        one process per curve and input class under `rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_SALU` (no
                                                tracing alongside): the counters of k_sign_nonce_load, k_rfc6979_first,
                                                k_ecdsa_sign_finish, k_schnorr_nonce, k_schnorr_sign_finish and k_fixed_base_ct must be
                                                IDENTICAL across the classes zeros / ones / random / n - 1 / invalid (0xff bytes)
    python tools/gpu_sign_rates.py --sm2        SM2DSA signing (ecgpu_sm2dsa_sign_batch / _sign_rfc6979_batch / _sign_msg_batch): the rates part and
                                                the trace part for the three forms on sm2, beside sm2's ecgpu_batch_mul_base_ct of the
                                                same run (profiles/sm2sign/rates.txt).  These calls have host-pointer forms only: their
                                                wall time includes the PCIe staging, and so does the yardstick's (its host-pointer
                                                form), which is timed again with reused and with page-locked arrays
    python tools/gpu_sign_rates.py --bign       bign signing (ecgpu_bign_sign_batch / _sign_prehash_batch / _sign_msg_batch): the rates part and the
                                                trace part for the three forms on bign256, beside bign256's ecgpu_batch_mul_base_ct of
                                                the same run (profiles/bignsign/rates.txt), host-pointer calls like --sm2.  The trace
                                                part ends with the share of each call spent in k_bign_genk beside its k_fixed_base_ct
    python tools/gpu_sign_rates.py --child FORM CURVE CLASS LOG2N     (internal) one call

Every part after the first starts GPU processes of its own.  The first child that does not exit with status 0 ends the whole
script there (ChildFailed): its exit status and the end of its output are printed, and nothing more is started on the GPU.
"""
import csv
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

CURVES = {"k256": 0, "p256": 1}
FORMS = ("sign", "rfc6979", "msg", "schnorr")
SM2_CURVES = {"sm2": 3}
SM2_FORMS = ("sm2_sign", "sm2_rfc6979", "sm2_msg")
SM2_DISTID = b"1234567812345678"
BIGN_CURVES = {"bign256": 11}
BIGN_FORMS = ("bign_sign", "bign_prehash", "bign_msg")
CLASSES = ("zeros", "ones", "random", "nm1", "invalid")
CT_KERNELS = ("k_sign_nonce_load", "k_rfc6979_first", "k_ecdsa_sign_finish", "k_schnorr_nonce", "k_schnorr_sign_finish",
              "k_fixed_base_ct")
MSG_LEN = 32
N_PMC_LOG2 = 14


def engine():
    ecgpu = importlib.import_module("elliptic-curves_amd")
    return ecgpu, ecgpu.Engine(0)


def class_bytes(ecgpu, cid, n, cls, seed, width=None):
    L = width or ecgpu.FIELD_BYTES[cid]
    if cls == "zeros":
        return np.zeros(n * L, np.uint8)
    if cls == "ones":
        return np.frombuffer((1).to_bytes(L, "big") * n, np.uint8).copy()
    if cls == "nm1":
        return np.frombuffer((ecgpu.GROUP_ORDERS[cid] - 1).to_bytes(L, "big") * n, np.uint8).copy()
    if cls == "invalid":
        return np.full(n * L, 0xFF, np.uint8)
    from gpu_common import rand_scalars
    if width:
        return np.random.default_rng(seed).integers(0, 256, n * L, dtype=np.uint8)
    return rand_scalars(cid, n, seed)


class Call:
    """one signing form on device-resident inputs of one class"""

    def __init__(self, ecgpu, eng, form, cid, n, cls):
        L = ecgpu.FIELD_BYTES[cid]
        self.eng, self.form, self.cid, self.n = eng, form, cid, n
        mk = lambda seed, width=None: eng.to_device(class_bytes(ecgpu, cid, n, cls, seed, width))
        self.d, self.k, self.z = mk(0x5161), mk(0x5162), mk(0x5163)
        self.msgs, self.aux = mk(0x5164, MSG_LEN), mk(0x5165, 32)
        self.sig, self.recid, self.ok = eng.dev_alloc(n * 2 * L + 16), eng.dev_alloc(n + 16), eng.dev_alloc(n + 16)
        self.normalize_s = cid == 0

    def run(self):
        e, c, n = self.eng, self.cid, self.n
        if self.form == "sign":
            e.ecdsa_sign_dev(c, self.d, self.k, self.z, n, self.normalize_s, self.sig, self.recid, self.ok)
        elif self.form == "rfc6979":
            e.ecdsa_sign_rfc6979_dev(c, self.d, self.z, n, self.normalize_s, self.sig, self.recid, self.ok)
        elif self.form == "msg":
            e.ecdsa_sign_msg_dev(c, self.d, self.msgs, MSG_LEN, n, self.normalize_s, self.sig, self.recid, self.ok)
        elif self.form == "schnorr":
            e.schnorr_sign_raw_dev(self.d, self.msgs, MSG_LEN, self.aux, n, self.sig, self.ok)
        else:                                     # the yardstick: the parent's kernel alone
            e.mul_by_generator_dev(c, self.d, n, self.sig, self.ok, constant_time=True)

    def signed(self):
        return int(self.eng.to_host(self.ok, self.n).sum())


def rates():
    ecgpu, eng = engine()
    n = 1 << 20
    print("wall time per call (synchronous device-pointer calls, best of 5 after 2 warm-up calls), 2^20 elements:")
    for name, cid in CURVES.items():
        base = None
        for form in ("mul_base_ct",) + FORMS:
            if form == "schnorr" and cid != 0:
                continue
            call = Call(ecgpu, eng, form, cid, n, "random")
            best = None
            for rep in range(7):
                t0 = time.perf_counter()
                call.run()
                dt = (time.perf_counter() - t0) * 1e3
                if rep >= 2:
                    best = dt if best is None else min(best, dt)
            if form == "mul_base_ct":
                base = best
            print("  %-5s %-12s %8.3f ms  %10.4g /s  x%.2f of ecgpu_batch_mul_base_ct  (kernel span %.3f ms%s)" % (
                name, form, best, n / best * 1e3, best / base, eng.last_timing("total"),
                "" if form == "mul_base_ct" else ", %d signed" % call.signed()), flush=True)
            del call
    eng.close()


class Sm2Host:
    """The SM2DSA signing forms and their yardstick on 2^lg elements in host memory: these calls have host-pointer forms only, so
    a call is its staging and its kernels together.  Nothing is built that the forms do not use."""

    def __init__(self, ecgpu, eng, n, cls="random"):
        self.eng, self.n = eng, n
        self.d, self.k, self.e = (class_bytes(ecgpu, SM2_CURVES["sm2"], n, cls, seed) for seed in (0x5161, 0x5162, 0x5163))
        self.msgs = class_bytes(ecgpu, SM2_CURVES["sm2"], n, cls, 0x5164, MSG_LEN)
        # the output arrays are made (and touched) once and reused: a fresh numpy array's pages are first touched by the copy that
        # fills it, which takes several times as long as the whole call (the probe at the end of sm2_rates measures it)
        self.xy, self.inf, self.sig, self.ok = (np.zeros(n * w, np.uint8) for w in (64, 1, 64, 1))
        self.calls = {
            "ecgpu_batch_mul_base_ct (sm2)": lambda: eng.mul_by_generator(SM2_CURVES["sm2"], self.d, out=self.xy, inf=self.inf, constant_time=True),
            "sm2_sign": lambda: eng.sm2dsa_sign(self.d, self.k, self.e, out=self.sig, ok=self.ok),
            "sm2_rfc6979": lambda: eng.sm2dsa_sign_rfc6979(self.d, self.e, out=self.sig, ok=self.ok),
            "sm2_msg": lambda: eng.sm2dsa_sign_msg(SM2_DISTID, self.d, self.msgs, MSG_LEN, out=self.sig, ok=self.ok),
        }


class BignHost:
    """The bign signing forms and their yardstick on n elements in host memory (host-pointer forms only, as for SM2DSA).  Records are
    little-endian; the top bit of every key, nonce and prehash is cleared, which keeps them below q."""

    def __init__(self, ecgpu, eng, n):
        self.eng, self.n = eng, n
        bign = BIGN_CURVES["bign256"]

        def rec(seed, width=32):
            a = np.random.default_rng(seed).integers(0, 256, n * width, dtype=np.uint8)
            if width == 32:
                a[31::32] &= 0x7F
                a[0::32] |= 1
            return a
        self.d, self.k, self.h, self.msgs = rec(0x5161), rec(0x5162), rec(0x5163), rec(0x5164, MSG_LEN + 1)[:n * MSG_LEN]
        self.xy, self.inf, self.sig, self.ok = (np.zeros(n * w, np.uint8) for w in (64, 1, 48, 1))
        self.calls = {
            "ecgpu_batch_mul_base_ct (bign256)": lambda: eng.mul_by_generator(bign, self.d, out=self.xy, inf=self.inf, constant_time=True),
            "bign_sign": lambda: eng.bign_sign(self.d, self.k, self.h, out=self.sig, ok=self.ok),
            "bign_prehash": lambda: eng.bign_sign_prehash(self.d, self.h, out=self.sig, ok=self.ok),
            "bign_msg": lambda: eng.bign_sign_msg(self.d, self.msgs, MSG_LEN, out=self.sig, ok=self.ok),
        }


def timed(fn):
    t0 = time.perf_counter()
    out = fn()                                             # (a host-pointer call returns after its last copy has arrived)
    return (time.perf_counter() - t0) * 1e3, out


def sm2_rates(rounds=5):
    """the four host-pointer calls alternating inside a round, median (min .. max) over the rounds after a warm-up round; then the
    yardstick again with its output arrays reused and with page-locked arrays: what of its wall time is the host side of the staging"""
    ecgpu, eng = engine()
    n, sm2 = 1 << 20, SM2_CURVES["sm2"]
    h = Sm2Host(ecgpu, eng, n)
    print("SM2DSA signing, 2^20 elements in pageable host memory (host-pointer calls: PCIe staging included, there is no other form),")
    print("one process, the output arrays reused from call to call;")
    print("median of %d rounds after one warm-up round, the calls alternating inside a round; ms per call (min .. max)" % rounds)
    times = {name: [] for name in h.calls}
    signed = {}
    for rnd in range(rounds + 1):
        for name, fn in h.calls.items():
            ms, out = timed(fn)
            if rnd:
                times[name].append(ms)
            if name.startswith("sm2_"):
                signed[name] = int(out[1].sum())
    for name, v in times.items():
        med = statistics.median(v)
        print("  %-32s %9.2f ms  (%8.2f .. %8.2f)   %6.2f M/s%s" % (name, med, min(v), max(v), n / med / 1e3,
                                                                   ", %d signed" % signed[name] if name in signed else ""), flush=True)
    # the staging of the yardstick three ways: fresh output arrays every call (what the Engine methods do when they are given
    # none), the same two arrays every call (as above), page-locked input and output arrays
    out, inf = h.xy, h.inf
    pin_d, pin_out, pin_inf = eng.host_alloc(n * 32), eng.host_alloc(n * 64), eng.host_alloc(n)
    pin_d[:] = h.d
    probes = {
        "fresh pageable outputs": lambda: eng.mul_by_generator(sm2, h.d, constant_time=True),
        "reused pageable outputs": lambda: eng.mul_by_generator(sm2, h.d, out=out, inf=inf, constant_time=True),
        "page-locked input and outputs": lambda: eng.mul_by_generator(sm2, pin_d, out=pin_out, inf=pin_inf, constant_time=True),
    }
    ptimes = {name: [] for name in probes}
    for rnd in range(rounds + 1):
        for name, fn in probes.items():
            ms, _ = timed(fn)
            if rnd:
                ptimes[name].append(ms)
    print("the yardstick's staging, same process (ecgpu_batch_mul_base_ct on sm2, host-pointer form; 32 MB up, 65 MB down):")
    for name, v in ptimes.items():
        print("  %-32s %9.2f ms  (%8.2f .. %8.2f)" % (name, statistics.median(v), min(v), max(v)), flush=True)
    for a in (pin_d, pin_out, pin_inf):
        eng.host_free(a)
    eng.close()


def bign_rates(rounds=5):
    """the four host-pointer calls alternating inside a round, median (min .. max) over the rounds after a warm-up round"""
    ecgpu, eng = engine()
    n = 1 << 20
    h = BignHost(ecgpu, eng, n)
    print("bign signing, 2^20 elements in pageable host memory (host-pointer calls: PCIe staging included, there is no other form),")
    print("one process, the output arrays reused from call to call;")
    print("median of %d rounds after one warm-up round, the calls alternating inside a round; ms per call (min .. max)" % rounds)
    times = {name: [] for name in h.calls}
    signed = {}
    for rnd in range(rounds + 1):
        for name, fn in h.calls.items():
            ms, out = timed(fn)
            if rnd:
                times[name].append(ms)
            if name.startswith("bign_"):
                signed[name] = int(out[1].sum())
    for name, v in times.items():
        med = statistics.median(v)
        print("  %-34s %9.2f ms  (%8.2f .. %8.2f)   %6.2f M/s%s" % (name, med, min(v), max(v), n / med / 1e3,
                                                                   ", %d signed" % signed[name] if name in signed else ""), flush=True)
    eng.close()


def child(form, curve, cls, lg):
    """form "all": every form of the curve once (the counter runs); otherwise the one form twice (the second call is the warm one)"""
    ecgpu, eng = engine()
    cid = dict(CURVES, **SM2_CURVES, **BIGN_CURVES)[curve]
    if form == "all":
        for f in FORMS:
            if f != "schnorr" or cid == 0:
                Call(ecgpu, eng, f, cid, 1 << lg, cls).run()
    elif form in SM2_FORMS:
        h = Sm2Host(ecgpu, eng, 1 << lg, cls)
        h.calls[form]()
        h.calls[form]()
    elif form in BIGN_FORMS:
        h = BignHost(ecgpu, eng, 1 << lg)
        h.calls[form]()
        h.calls[form]()
    else:
        call = Call(ecgpu, eng, form, cid, 1 << lg, cls)
        call.run()
        call.run()
    eng.close()


class ChildFailed(Exception):
    pass


def run_child(cmd, what):
    """one GPU child under rocprofv3; anything but exit status 0 (an abort, a fault, a time limit) ends the script"""
    try:
        r = subprocess.run(cmd, cwd="/tmp", env=dict(os.environ, TMPDIR="/tmp"), capture_output=True, text=True, timeout=600)
    except subprocess.TimeoutExpired as e:
        raise ChildFailed("%s: no exit within 600 s\n%s" % (what, (e.stderr or b"")[-800:]))
    if r.returncode != 0:
        raise ChildFailed("%s: exit status %d\n%s\n%s" % (what, r.returncode, r.stdout[-800:], r.stderr[-1500:]))
    return r


def short(kernel):
    return kernel.split("(")[0].replace("void ", "").replace("ecgpu::", "")


def trace(curves=CURVES, forms=FORMS):
    print("\nkernels of one call at 2^20 (second of two calls in a process of its own, rocprofv3 --kernel-trace --stats):")
    for curve in curves:
        for form in forms:
            if form == "schnorr" and curve != "k256":
                continue
            out = "/tmp/sign_trace_%s_%s" % (curve, form)
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "t", "--", sys.executable,
                   os.path.abspath(__file__), "--child", form, curve, "random", "20"]
            run_child(cmd, "trace %s %s" % (curve, form))
            rows = []
            for f in glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True):
                rows += [row for row in csv.DictReader(open(f)) if "ecgpu::" in row["Name"]]
            if not rows:
                raise ChildFailed("trace %s %s: the run left no kernel statistics under %s" % (curve, form, out))
            # the LUT build of the first call runs k_window_bases / k_table_entries / one more k_normalize: named as they are
            tot = sum(float(row["TotalDurationNs"]) for row in rows)
            rows.sort(key=lambda row: -float(row["TotalDurationNs"]))
            print("  %s %s (two calls): %.3f ms of kernels; dominant: %s" % (curve, form, tot / 1e6, short(rows[0]["Name"])))
            for row in rows[:8]:
                print("      %-44s calls %3s  %9.3f ms  %5.1f %%" % (short(row["Name"])[:44], row["Calls"], float(row["TotalDurationNs"]) / 1e6,
                                                                   100 * float(row["TotalDurationNs"]) / tot))
            if form in BIGN_FORMS:               # what the generator costs beside the multiplication of the same run
                ms = lambda kernel: sum(float(row["TotalDurationNs"]) for row in rows if short(row["Name"]).startswith(kernel + "<")) / 1e6
                print("      k_bign_genk %.3f ms = %.1f %% of the call's kernels, beside k_fixed_base_ct %.3f ms" % (
                    ms("k_bign_genk"), 100 * ms("k_bign_genk") * 1e6 / tot, ms("k_fixed_base_ct")))
            sys.stdout.flush()


def counters(curve, cls):
    res = {}
    out = "/tmp/sign_pmc_%s_%s" % (curve, cls)
    cmd = ["rocprofv3", "--pmc", "SQ_INSTS_VALU", "SQ_INSTS_SALU", "--output-format", "csv", "-d", out, "-o", "pmc", "--",
           sys.executable, os.path.abspath(__file__), "--child", "all", curve, cls, str(N_PMC_LOG2)]
    run_child(cmd, "counters %s %s" % (curve, cls))
    for f in glob.glob(os.path.join(out, "**", "*counter_collection.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            k = short(row["Kernel_Name"])
            if not k.startswith(("k_sign", "k_rfc6979", "k_ecdsa_sign", "k_schnorr_nonce", "k_schnorr_sign", "k_fixed_base_ct", "k_normalize")):
                continue
            d = res.setdefault(k, {})                     # all launches of the kernel in the process, summed
            d[row["Counter_Name"]] = d.get(row["Counter_Name"], 0.0) + float(row["Counter_Value"])
    if not res:
        raise ChildFailed("counters %s %s: the run left no counters under %s" % (curve, cls, out))
    return res


def pmc():
    print("\nexecuted-instruction counters (every form once, 2^%d elements, all launches of a kernel summed), one process per curve and input class:" % N_PMC_LOG2)
    bad = 0
    for curve in CURVES:
        allc = {cls: counters(curve, cls) for cls in CLASSES}
        for k in sorted({k for c in allc.values() for k in c}):
            rows = {cls: allc[cls].get(k, {}) for cls in CLASSES}
            names = sorted({c for r in rows.values() for c in r})
            uniform = all(len({rows[cls].get(c) for cls in CLASSES}) == 1 for c in names)
            required = any(w + "<" in k for w in CT_KERNELS)
            verdict = "IDENTICAL" if uniform else "DIFFER"
            note = "as required" if (uniform and required) else "REQUIRED IDENTICAL" if required else "variable time by design"
            bad += 1 if (required and not uniform) else 0
            print("  %-5s %-46s %s  [%s]" % (curve, k[:46], verdict, note))
            for c in names:
                print("        %-14s %s" % (c, "  ".join("%.0f" % rows[cls].get(c, float("nan")) for cls in CLASSES)))
            sys.stdout.flush()
    print("counter check (%s): %s" % (" / ".join(CLASSES), "PASS" if bad == 0 else "FAIL (%d kernels)" % bad))
    return bad


def main():
    if len(sys.argv) > 5 and sys.argv[1] == "--child":
        return child(sys.argv[2], sys.argv[3], sys.argv[4], int(sys.argv[5]))
    parts = [a for a in sys.argv[1:] if a in ("--rates", "--trace", "--pmc", "--sm2", "--bign")] or ["--rates", "--trace", "--pmc"]
    bad = 0
    try:
        if "--sm2" in parts:
            sm2_rates()
            trace(SM2_CURVES, SM2_FORMS)
        if "--bign" in parts:
            bign_rates()
            trace(BIGN_CURVES, BIGN_FORMS)
        if "--rates" in parts:
            rates()                      # (in this process: an exception or a fault here ends the script by itself)
        if "--trace" in parts:
            trace()
        if "--pmc" in parts:
            bad = pmc()
    except ChildFailed as e:
        print("STOPPED, nothing further was started on the GPU: %s" % e, flush=True)
        return 1
    return bad


if __name__ == "__main__":
    sys.exit(main() or 0)
