#!/usr/bin/env python3
"""The SM2 public-key encryption entry points on the GPU box: rates beside the two uniform-schedule multiplications they are built
from, and the kernel split of each call.

    python tools/gpu_pke_rates.py              both parts below, one after the other
    python tools/gpu_pke_rates.py --rates      in ONE process, 2^20 elements in host memory, msg_len 32 and 1024: wall time per call of
                                               ecgpu_sm2_pke_encrypt_batch and ecgpu_sm2_pke_decrypt_batch, and of
                                               ecgpu_batch_mul_base_ct and ecgpu_batch_mul_ct on ECGPU_SM2 with the same scalars and
                                               points.  One warm-up round, then REPEATS rounds in which the four calls alternate;
                                               the median of each.  The comparison base is the sum of the two multiplications of
                                               THIS run (encrypt: both; decrypt: the variable-base one), never another day's number.
    python tools/gpu_pke_rates.py --trace      each call once per msg_len under `rocprofv3 --kernel-trace --stats`, a run of its
                                               own per call: the kernels of the call by share of its GPU time
    python tools/gpu_pke_rates.py --child CALL MSG_LEN LOG2N     (internal) the call twice

All four calls are host-pointer forms (the encryption calls have no other): every figure includes staging over PCIe, for the
multiplications too.  The first child that does not exit with status 0 ends the whole script there (ChildFailed): nothing more is
started on the GPU.
"""
import csv
import glob
import importlib
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SM2 = 3
LOG2N = 20
MSG_LENS = (32, 1024)
REPEATS = 5


def inputs(eng, n, msg_len):
    rng = np.random.default_rng(0x5D2 + msg_len)

    def scalars():
        s = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        s[:, 0] &= 0x7F                                    # below the group order
        s[:, 31] |= 1                                      # not zero
        return s.reshape(-1)
    d, k = scalars(), scalars()
    pk, inf = eng.mul_by_generator(SM2, d)
    assert not inf.any()
    return d, k, pk, rng.integers(0, 256, n * msg_len, dtype=np.uint8)


def timed(fn):
    t = time.perf_counter()
    out = fn()                                             # (a host-pointer call returns after its last copy has arrived)
    return (time.perf_counter() - t) * 1e3, out


def rates():
    ecgpu = importlib.import_module("elliptic-curves_amd")
    eng = ecgpu.Engine(0)
    n = 1 << LOG2N
    print("SM2 public-key encryption, 2^%d elements in host memory, one process, one MI355X; median of %d rounds after one warm-up round,"
          % (LOG2N, REPEATS))
    print("the calls alternating inside a round; ms per call (min .. max), elements per second from the median")
    for msg_len in MSG_LENS:
        d, k, pk, msgs = inputs(eng, n, msg_len)
        c1, c2, c3, ok = eng.sm2_pke_encrypt(pk, k, msgs, msg_len)
        assert ok.all()
        calls = {
            "ecgpu_batch_mul_base_ct (sm2)": lambda: eng.mul_by_generator(SM2, k, constant_time=True),
            "ecgpu_batch_mul_ct (sm2)": lambda: eng.mul(SM2, k, pk, constant_time=True),
            "ecgpu_sm2_pke_encrypt_batch": lambda: eng.sm2_pke_encrypt(pk, k, msgs, msg_len),
            "ecgpu_sm2_pke_decrypt_batch": lambda: eng.sm2_pke_decrypt(d, c1, c2, msg_len, c3),
        }
        times = {name: [] for name in calls}
        for rnd in range(REPEATS + 1):
            for name, fn in calls.items():
                ms, out = timed(fn)
                if rnd:
                    times[name].append(ms)
                if name.endswith("decrypt_batch"):
                    assert out[1].all() and bytes(out[0][:4096]) == bytes(msgs[:4096])
        med = {name: statistics.median(v) for name, v in times.items()}
        print("\nmsg_len = %d" % msg_len)
        for name, v in times.items():
            print("  %-32s %9.2f ms  (%8.2f .. %8.2f)   %6.2f M/s" % (name, med[name], min(v), max(v), n / med[name] / 1e3))
        base_enc = med["ecgpu_batch_mul_base_ct (sm2)"] + med["ecgpu_batch_mul_ct (sm2)"]
        base_dec = med["ecgpu_batch_mul_ct (sm2)"]
        print("  encrypt / (mul_base_ct + mul_ct of this run) = %.3f     decrypt / mul_ct of this run = %.3f"
              % (med["ecgpu_sm2_pke_encrypt_batch"] / base_enc, med["ecgpu_sm2_pke_decrypt_batch"] / base_dec))
        sys.stdout.flush()
    eng.close()


def child(call, msg_len, lg):
    ecgpu = importlib.import_module("elliptic-curves_amd")
    eng = ecgpu.Engine(0)
    n = 1 << lg
    d, k, pk, msgs = inputs(eng, n, msg_len)
    c1, c2, c3, ok = eng.sm2_pke_encrypt(pk, k, msgs, msg_len)
    if call == "encrypt":
        eng.sm2_pke_encrypt(pk, k, msgs, msg_len)
    else:
        eng.sm2_pke_decrypt(d, c1, c2, msg_len, c3)
        eng.sm2_pke_decrypt(d, c1, c2, msg_len, c3)
    eng.close()


class ChildFailed(Exception):
    pass


def run_child(cmd, what):
    """one GPU child under rocprofv3; anything but exit status 0 (an abort, a fault, a time limit) ends the script"""
    try:
        r = subprocess.run(cmd, cwd="/tmp", env=dict(os.environ, TMPDIR="/tmp"), capture_output=True, text=True, timeout=400)
    except subprocess.TimeoutExpired as e:
        raise ChildFailed("%s: no exit within 400 s\n%s" % (what, (e.stderr or b"")[-800:]))
    if r.returncode != 0:
        raise ChildFailed("%s: exit status %d\n%s\n%s" % (what, r.returncode, r.stdout[-800:], r.stderr[-1500:]))
    return r


def short(kernel):
    return kernel.split("(")[0].replace("void ", "").replace("ecgpu::", "")


def trace():
    print("\nkernels of two calls at 2^%d in a process of its own (rocprofv3 --kernel-trace --stats; the key generation and, for the" % LOG2N)
    print("decryption rows, the one encryption that makes the ciphertexts are in the same process and are named as they are):")
    for msg_len in MSG_LENS:
        for call in ("encrypt", "decrypt"):
            out = "/tmp/pke_trace_%s_%d" % (call, msg_len)
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "t", "--", sys.executable,
                   os.path.abspath(__file__), "--child", call, str(msg_len), str(LOG2N)]
            run_child(cmd, "trace %s %d" % (call, msg_len))
            rows = []
            for f in glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True):
                rows += [row for row in csv.DictReader(open(f)) if "ecgpu::" in row["Name"]]
            if not rows:
                raise ChildFailed("trace %s %d: the run left no kernel statistics under %s" % (call, msg_len, out))
            tot = sum(float(row["TotalDurationNs"]) for row in rows)
            rows.sort(key=lambda row: -float(row["TotalDurationNs"]))
            print("  %s, msg_len = %d: %.3f ms of kernels" % (call, msg_len, tot / 1e6))
            for row in rows[:10]:
                print("      %-44s calls %3s  %9.3f ms  %5.1f %%" % (short(row["Name"])[:44], row["Calls"], float(row["TotalDurationNs"]) / 1e6,
                                                                   100 * float(row["TotalDurationNs"]) / tot))
            sys.stdout.flush()


def main():
    if len(sys.argv) > 4 and sys.argv[1] == "--child":
        return child(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]))
    parts = [a for a in sys.argv[1:] if a in ("--rates", "--trace")] or ["--rates", "--trace"]
    try:
        if "--rates" in parts:
            rates()                      # (in this process: an exception or a fault here ends the script by itself)
        if "--trace" in parts:
            trace()
    except ChildFailed as e:
        print("STOPPED, nothing further was started on the GPU: %s" % e, flush=True)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
