"""-m gpu: the argument checks of every device-pointer entry point of the C ABI (the ecgpu_group_* ones excepted), driven from
one table through the Python binding's raw ctypes handle.

Per entry point: valid arguments (n = 2) succeed; each pointer in turn NULL, then offset by 4 bytes, is rejected with
ECGPU_ERR_ARG and a message that names the function — or accepted, where the table says the pointer is optional resp. not
alignment-checked; n = 0 with every array NULL succeeds and leaves the context usable.  Rejected calls are made on an
asynchronous context: they return before anything is queued, so ecgpu_synchronize is clean after each of them.

The table is a transcript of the checks in csrc/ecgpu_api.hip (it pins them; include/ecgpu.h describes the same contract in prose).
Pointer flags: "n" required when n > 0, "a" required always (the output of a reducing call, a parts record), "o" optional,
"m" required when n > 0 and msg_len != 0, "d" required when n > 0 and distid_len != 0; "16" must be 16-byte aligned."""
import ctypes

import numpy as np
import pytest

import pyec
from gpu_common import ecgpu_module

pytestmark = pytest.mark.gpu
OK, ERR_ARG = 0, -7
N = 2
MSG_LEN = 16
SLACK = 32          # bytes behind every buffer: room for the 4-byte offset

K, SM2, BIGN = "k256", "sm2", "bign256"
C, CNT = "curve", "n"


def P(kind, flags):
    return ("ptr", kind, flags)


def I(v):
    return ("int", v)


def Z(v):
    return ("size", v)


OUT = "out"
# name, curve, arguments in the order of the C prototype (after ctx)
TABLE = [
    ("ecgpu_batch_mul_base_dev", K, [C, P("scalar", "n16"), CNT, P(OUT, "n16"), P(OUT, "o")]),
    ("ecgpu_batch_mul_base_compressed_dev", K, [C, P("scalar", "n16"), CNT, P(OUT, "n16"), P(OUT, "n")]),
    ("ecgpu_batch_mul_dev", K, [C, P("scalar", "n16"), P("xy", "n16"), P("inf", "o"), CNT, P(OUT, "n16"), P(OUT, "o")]),
    ("ecgpu_batch_mul_base_ct_dev", K, [C, P("scalar", "n16"), CNT, P(OUT, "n16"), P(OUT, "o")]),
    ("ecgpu_batch_mul_ct_dev", K, [C, P("scalar", "n16"), P("xy", "n16"), P("inf", "o"), CNT, P(OUT, "n16"), P(OUT, "o")]),
    ("ecgpu_batch_mul_ct_xyz_dev", K, [C, P("scalar", "n16"), P("xyz", "n16"), CNT, P(OUT, "n16"), P(OUT, "o")]),
    ("ecgpu_msm_dev", K, [C, P("scalar", "n16"), P("xy", "n16"), P("inf", "o"), CNT, P(OUT, "a16"), P(OUT, "o")]),
    ("ecgpu_lincomb_ct_dev", K, [C, P("scalar", "n16"), P("xy", "n16"), P("inf", "o"), CNT, P(OUT, "a16"), P(OUT, "o")]),
    ("ecgpu_lincomb_ct_xyz_dev", K, [C, P("scalar", "n16"), P("xyz", "n16"), CNT, P(OUT, "a16"), P(OUT, "o")]),
    ("ecgpu_batch_mul_xyz_dev", K, [C, P("scalar", "n16"), P("xyz", "n16"), CNT, P(OUT, "n16"), P(OUT, "o")]),
    ("ecgpu_msm_xyz_dev", K, [C, P("scalar", "n16"), P("xyz", "n16"), CNT, P(OUT, "a16"), P(OUT, "o")]),
    ("ecgpu_msm_compressed_dev", K, [C, P("scalar", "n16"), P("x", "n16"), P("tag", "n"), CNT, P(OUT, "a16"), P(OUT, "o")]),
    ("ecgpu_batch_mul_compressed_dev", K, [C, P("scalar", "n16"), P("x", "n16"), P("tag", "n"), CNT, P(OUT, "n16"), P(OUT, "o")]),
    ("ecgpu_msm_parts_dev", K, [C, P("scalar", "n16"), P("xy", "n16"), P("inf", "o"), CNT, Z(N), P("parts_out", "a16")]),
    ("ecgpu_msm_parts_xyz_dev", K, [C, P("scalar", "n16"), P("xyz", "n16"), CNT, Z(N), P("parts_out", "a16")]),
    ("ecgpu_msm_parts_join_dev", None, [P("parts", "a")]),
    ("ecgpu_msm_finish_dev", K, [C, P("parts", "a16"), I(1), Z(N), P(OUT, "a16"), P(OUT, "o")]),
    ("ecgpu_batch_normalize_dev", K, [C, P("xyz", "n16"), CNT, P(OUT, "n16"), P(OUT, "o")]),
    ("ecgpu_point_sum_dev", K, [C, P("xy", "n16"), P("inf", "o"), CNT, P(OUT, "a16"), P(OUT, "o")]),
    ("ecgpu_batch_mul_base_and_mul_add_dev", K,
     [C, P("scalar", "n16"), P("scalar", "n16"), P("xy", "n16"), P("inf", "o"), CNT, P(OUT, "n16"), P(OUT, "o")]),
    ("ecgpu_batch_mul_base_and_mul_add_xyz_dev", K,
     [C, P("scalar", "n16"), P("scalar", "n16"), P("xyz", "n16"), CNT, P(OUT, "n16"), P(OUT, "o")]),
    ("ecgpu_ecdsa_verify_batch_dev", K,
     [C, P("scalar", "n16"), P("scalar", "n16"), P("scalar", "n16"), P("xy", "n16"), CNT, I(0), P(OUT, "n")]),
    ("ecgpu_ecdsa_verify_msg_batch_dev", K, [C, P("xy", "n16"), P("msgs", "m"), Z(MSG_LEN), P("sig", "n16"), CNT, I(0), P(OUT, "n")]),
    ("ecgpu_ecdsa_recover_batch_dev", K,
     [C, P("scalar", "n16"), P("scalar", "n16"), P("scalar", "n16"), P("inf", "n"), CNT, I(0), P(OUT, "n16"), P(OUT, "n")]),
    ("ecgpu_sm2dsa_verify_batch_dev", SM2,
     [P("scalar", "n16"), P("scalar", "n16"), P("scalar", "n16"), P("xy", "n16"), CNT, P(OUT, "n")]),
    ("ecgpu_sm2dsa_verify_msg_batch_dev", SM2,
     [P("distid", "d"), Z(16), P("xy", "n16"), P("msgs", "m"), Z(MSG_LEN), P("sig", "n16"), CNT, P(OUT, "n")]),
    ("ecgpu_bign_verify_batch_dev", BIGN, [P("scalar", "n16"), P("sig", "n16"), P("xy", "n16"), CNT, P(OUT, "n")]),
    ("ecgpu_bign_verify_msg_batch_dev", BIGN, [P("xy", "n16"), P("msgs", "m"), Z(MSG_LEN), P("sig", "n16"), CNT, P(OUT, "n")]),
    ("ecgpu_schnorr_verify_batch_dev", K,
     [P("scalar", "n16"), P("scalar", "n16"), P("scalar", "n16"), P("xy", "n16"), CNT, P(OUT, "n")]),
    ("ecgpu_schnorr_verify_raw_batch_dev", K, [P("x", "n16"), P("msgs", "m"), Z(MSG_LEN), P("sig", "n16"), CNT, P(OUT, "n")]),
    ("ecgpu_ecdsa_sign_batch_dev", K,
     [C, P("scalar", "n16"), P("scalar", "n16"), P("scalar", "n16"), CNT, I(0), P(OUT, "n16"), P(OUT, "n"), P(OUT, "n")]),
    ("ecgpu_ecdsa_sign_rfc6979_batch_dev", K, [C, P("scalar", "n16"), P("scalar", "n16"), CNT, I(0), P(OUT, "n16"), P(OUT, "n"), P(OUT, "n")]),
    ("ecgpu_ecdsa_sign_msg_batch_dev", K,
     [C, P("scalar", "n16"), P("msgs", "m"), Z(MSG_LEN), CNT, I(0), P(OUT, "n16"), P(OUT, "n"), P(OUT, "n")]),
    ("ecgpu_schnorr_sign_raw_batch_dev", K, [P("scalar", "n16"), P("msgs", "m"), Z(MSG_LEN), P("scalar", "n16"), CNT, P(OUT, "n16"), P(OUT, "n")]),
    # the ECDH forms check their outputs themselves and leave the inputs to ecgpu_batch_mul[_ct]_dev: the message names whichever
    # function rejected the pointer (NAMED below)
    ("ecgpu_batch_ecdh_dev", K, [C, P("scalar", "n16"), P("xy", "n16"), CNT, P(OUT, "n16"), P(OUT, "n")]),
    ("ecgpu_batch_ecdh_ct_dev", K, [C, P("scalar", "n16"), P("xy", "n16"), CNT, P(OUT, "n16"), P(OUT, "n")]),
    ("ecgpu_batch_decompress_dev", K, [C, P("x", "n16"), P("odd", "n"), CNT, P(OUT, "n16"), P(OUT, "n")]),
]
# (entry point, argument position) -> the function its rejection names, where that is not the entry point
NAMED = {("ecgpu_batch_ecdh_dev", 1): "ecgpu_batch_mul_dev", ("ecgpu_batch_ecdh_dev", 2): "ecgpu_batch_mul_dev",
         ("ecgpu_batch_ecdh_dev", 4): "ecdh_dev", ("ecgpu_batch_ecdh_dev", 5): "ecdh_dev",
         ("ecgpu_batch_ecdh_ct_dev", 1): "ecgpu_batch_mul_ct_dev", ("ecgpu_batch_ecdh_ct_dev", 2): "ecgpu_batch_mul_ct_dev",
         ("ecgpu_batch_ecdh_ct_dev", 4): "ecdh_dev", ("ecgpu_batch_ecdh_ct_dev", 5): "ecdh_dev"}


def test_the_table_lists_every_device_pointer_entry_point():
    """against the prototypes of include/ecgpu.h: every name, and the kind of every argument"""
    import os
    import abi_parse
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ecgpu.h")
    protos = {name: args for name, _, args in abi_parse.parse_header(header) if name.endswith("_dev") and not name.startswith("ecgpu_group_")}
    assert set(protos) == {t[0] for t in TABLE}
    kinds = {"void *": "ptr", "const void *": "ptr", "int": "int", "size_t": "size"}
    for name, _, spec in TABLE:
        want = [kinds[t] for t, _ in protos[name][1:]]
        assert ["int" if a == C else "size" if a == CNT else a[0] for a in spec] == want, name


def host_data(c, kind):
    """valid inputs for N = 2 elements: scalars 1 and 2, the points G and 2 G, signatures with small non-zero halves"""
    le = c.name == "bign256"                                   # bign's wire order is little-endian
    num = lambda v: int(v).to_bytes(c.L, "little" if le else "big")
    pts = [pyec.G(c), pyec.mul(c, 2, pyec.G(c))]
    if kind == "scalar":
        return b"".join(num(i + 1) for i in range(N))
    if kind == "xy":
        return b"".join(num(x) + num(y) for x, y in pts)
    if kind == "xyz":
        return b"".join(num(x) + num(y) + num(1) for x, y in pts)
    if kind == "x":
        return b"".join(num(x) for x, _ in pts)
    if kind == "tag":
        return bytes(2 + (y & 1) for _, y in pts)
    if kind == "odd":
        return bytes(y & 1 for _, y in pts)
    if kind == "inf":                                          # identity flags, and the recovery ids of ecgpu_ecdsa_recover_batch_dev
        return bytes(N)
    if kind == "sig":
        return b"".join((1).to_bytes(16, "little") + (1).to_bytes(32, "little") if le else num(1) + num(1) for _ in range(N))
    if kind == "msgs":
        return bytes(range(N * MSG_LEN))
    if kind == "distid":
        return b"1234567812345678"
    raise KeyError(kind)


class Bench:
    """the two contexts (synchronous for the calls that must succeed, asynchronous for the rejected ones) and their buffers"""

    def __init__(self):
        mod = ecgpu_module()
        self.sync, self.asyn = mod.Engine(0), mod.Engine(0)
        self.asyn.set_async(True)
        self.lib = self.sync._lib
        self.bufs = {}
        self.parts = None

    def close(self):
        self.bufs.clear()
        self.parts = None
        self.asyn.close()
        self.sync.close()

    def data(self, c, kind, shift):
        """device address of the input `kind` (the same bytes at a 4-byte offset for shift = 4)"""
        key = (c.name, kind, shift)
        if key not in self.bufs:
            h = np.frombuffer(bytes(shift) + host_data(c, kind), np.uint8)
            buf = self.sync.dev_alloc(h.size + SLACK)
            self.sync.to_device(h, buf)
            self.bufs[key] = buf
        return self.bufs[key].at(shift)

    def out(self, i, nbytes=4096):
        key = ("out", i, nbytes)
        if key not in self.bufs:
            self.bufs[key] = self.sync.dev_alloc(nbytes + SLACK)
        return self.bufs[key]

    def parts_record(self, c):
        """a parts record the synchronous context wrote (ecgpu_msm_parts_dev, plan for N terms), behind 4 spare bytes of its own copy
        for the offset case"""
        if self.parts is None:
            nb = self.sync.msm_parts_bytes(c.cid, N)
            rec = self.out("parts", nb)
            self.sync.msm_parts_dev(c.cid, self.data(c, "scalar", 0), self.data(c, "xy", 0), None, N, N, rec)
            shifted = self.sync.dev_alloc(nb + SLACK)
            self.sync.to_device(np.concatenate([np.zeros(4, np.uint8), self.sync.to_host(rec, nb)]), shifted)
            self.parts = (rec, shifted)
        return self.parts

    def call(self, eng, name, c, spec, n=N, null=None, shift=None, sizes=None):
        """-> (return code, message).  null / shift: the argument position to pass as NULL / 4 bytes further; sizes: {position:
        value} in place of a size argument of the table"""
        args = [eng._ctx]
        for i, a in enumerate(spec):
            if a == C:
                args.append(ctypes.c_int(c.cid))
            elif a == CNT:
                args.append(ctypes.c_size_t(n))
            elif a[0] == "int":
                args.append(ctypes.c_int((sizes or {}).get(i, a[1])))
            elif a[0] == "size":
                args.append(ctypes.c_size_t((sizes or {}).get(i, a[1])))
            else:
                _, kind, flags = a
                off = 4 if shift == i else 0
                if null == i or (n == 0 and "a" not in flags):
                    p = None
                elif kind == OUT:
                    p = self.out(i).at(off)
                elif kind == "parts_out":
                    p = self.out("parts_out", self.sync.msm_parts_bytes(c.cid, N)).at(off)
                elif kind == "parts":
                    p = self.parts_record(c)[1].at(4) if off else self.parts_record(c)[0].at(0)
                else:
                    p = self.data(c, kind, off)
                args.append(ctypes.c_void_p(p))
        rc = getattr(self.lib, name)(*args)
        return rc, (self.lib.ecgpu_last_error(eng._ctx) or b"").decode()


@pytest.fixture(scope="module")
def bench():
    b = Bench()
    yield b
    b.close()


def required(flags, what):
    return any(f in flags for f in what)


@pytest.mark.parametrize("name,curve,spec", TABLE, ids=[t[0] for t in TABLE])
def test_argument_checks(bench, name, curve, spec):
    c = pyec.CURVES[curve or K]
    sync = lambda **kw: bench.call(bench.sync, name, c, spec, **kw)

    def rejected(pos, **kw):
        rc, msg = bench.call(bench.asyn, name, c, spec, **kw)
        assert rc == ERR_ARG, (name, pos, kw, rc, msg)
        assert NAMED.get((name, pos), name) in msg, (name, pos, kw, msg)
        assert bench.lib.ecgpu_synchronize(bench.asyn._ctx) == OK, (name, pos, kw)      # nothing was queued

    rc, msg = sync()
    assert rc == OK, (name, "valid arguments", rc, msg)
    ptrs = [(i, a[1], a[2]) for i, a in enumerate(spec) if a[0] == "ptr"]
    for i, kind, flags in ptrs:
        if required(flags, "namd"):                           # (msg_len and distid_len are non-zero in the table)
            rejected(i, null=i)
        else:
            assert sync(null=i)[0] == OK, (name, i, "NULL")
        if "16" in flags:
            rejected(i, shift=i)
        else:
            rc, msg = sync(shift=i)
            assert rc == OK, (name, i, "offset", rc, msg)
    for i, a in enumerate(spec):                              # the conditions on sizes
        if a[0] == "ptr" and "m" in a[2]:                     # no message bytes: no message array
            assert sync(null=i, sizes={i + 1: 0})[0] == OK, (name, "msg_len 0")
        if a[0] == "ptr" and "d" in a[2]:
            assert sync(null=i, sizes={i + 1: 0})[0] == OK, (name, "distid_len 0")
            rejected(i, sizes={i + 1: 8192})
            rejected(i, n=0, sizes={i + 1: 8192})             # (checked before n)
    if name == "ecgpu_msm_finish_dev":
        for nranks in (0, -1, 4097):
            rejected(2, sizes={2: nranks})
    # n = 0: every array may be NULL; the context goes on working
    if any(a == CNT for a in spec):
        rc, msg = sync(n=0)
        assert rc == OK, (name, "n = 0", rc, msg)
        rc, msg = bench.call(bench.asyn, name, c, spec, n=0)
        assert rc == OK and bench.lib.ecgpu_synchronize(bench.asyn._ctx) == OK, (name, "n = 0, asynchronous", rc, msg)
    rc, msg = sync()
    assert rc == OK, (name, "after n = 0", rc, msg)
