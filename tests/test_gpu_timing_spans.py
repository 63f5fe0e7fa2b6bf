"""-m gpu: which stage names ecgpu_last_timing resolves after one small call of each family of device-pointer entry points (and of
the signing and encryption families that have host-pointer forms only), through the Python binding's raw ctypes handle.  The table below was taken from a run and is written out literally: a name
outside a family's row returns ECGPU_ERR_ARG, and for a row that has them total >= main >= 0.

Before every call the spans of the call before are dropped (timing off and on again), so that a call that records none — the empty
ecgpu_lincomb_ct_dev, any call with timing off, an MSM that went to a lane — shows as a row of its own.  The detail marks of the
bucket-path MSM ("prepare", "finish", "tree", "combine") are recorded whenever timing is on — their events exist from ecgpu_init
on —, so the MSM "without the detail events" is the untimed one."""
import ctypes

import numpy as np
import pytest

import pyec
from gpu_common import ecgpu_module

pytestmark = pytest.mark.gpu
OK, ERR_ARG = 0, -7
NAMES = ("main", "normalize", "total", "sort", "accumulate", "reduce", "recode", "prepare", "finish", "tree", "combine")
S, I = ctypes.c_size_t, ctypes.c_int
CID = pyec.K256.cid
L = 32
NB, NM, NS_ = 257, 300, 4           # one workgroup plus one element; the bucket-path MSM; the signature families
MSM_WINDOW = 8                      # a forced window switches the small-MSM path off

THREE = ("main", "normalize", "total")
MSM6 = THREE + ("sort", "accumulate", "reduce")
MSM10 = MSM6 + ("prepare", "finish", "tree", "combine")
VERIFY = THREE + ("recode",)
EXPECTED = {
    "mul_base": THREE, "mul_base_compressed": THREE, "mul_base_ct": THREE,
    "mul": THREE, "mul_xyz": THREE, "mul_compressed": THREE, "mul_ct": THREE, "mul_ct_xyz": THREE,
    "mul_add": THREE, "mul_add_xyz": THREE,
    "normalize": THREE, "point_sum": THREE,
    "lincomb_ct_empty": (), "lincomb_ct": THREE + ("accumulate", "reduce"),
    "msm_small": MSM6, "msm_small_untimed": (),
    "msm_buckets": MSM10, "msm_buckets_untimed": (),
    "msm_parts": ("main", "total", "sort", "accumulate", "reduce"), "msm_finish": THREE,
    "msm_on_lanes": ("accumulate",),
    "ecdsa_verify": VERIFY, "ecdsa_recover": VERIFY, "schnorr_verify": VERIFY,
    "ecdsa_sign": THREE, "ecdsa_sign_rfc6979": THREE, "ecdsa_sign_msg": THREE, "schnorr_sign": THREE,
    "decompress": ("main", "total"),
    "sm2dsa_sign": THREE, "sm2dsa_sign_rfc6979": THREE, "sm2dsa_sign_msg": THREE,
    "bign_sign": THREE, "bign_sign_prehash": THREE, "bign_sign_msg": THREE,
    "sm2_pke_encrypt": THREE, "sm2_pke_decrypt": THREE,
}


class Rig:
    def __init__(self):
        mod = ecgpu_module()
        self.eng = mod.Engine(0)
        self.lib = self.eng._lib
        e = self.eng
        n = NM
        scalars = np.frombuffer(b"".join((3 * i + 1).to_bytes(L, "big") for i in range(n)), np.uint8)
        xy, inf = e.mul_by_generator(CID, scalars)
        xy = np.asarray(xy, np.uint8).reshape(n, 2 * L)
        assert not np.asarray(inf).any()
        one = np.zeros((n, L), np.uint8)
        one[:, -1] = 1
        self.k = e.to_device(scalars)
        self.xy = e.to_device(xy.reshape(-1))
        self.xyz = e.to_device(np.concatenate([xy, one], axis=1).reshape(-1))
        self.x = e.to_device(np.ascontiguousarray(xy[:, :L]).reshape(-1))
        self.odd = e.to_device(np.ascontiguousarray(xy[:, 2 * L - 1] & 1))
        self.tag = e.to_device(np.ascontiguousarray(2 + (xy[:, 2 * L - 1] & 1)).astype(np.uint8))
        self.zero = e.to_device(np.zeros(n * 64, np.uint8))          # identity flags, recovery ids, messages, aux_rand
        self.out, self.out2, self.out3 = e.dev_alloc(n * 64 + 64), e.dev_alloc(n + 64), e.dev_alloc(n + 64)
        # the host-pointer families (NS_ elements): scalars, points, messages, and four outputs
        self.h_k, self.h_xy, self.h_zero = scalars[:NS_ * L].copy(), xy[:NS_].reshape(-1).copy(), np.zeros(NS_ * 64, np.uint8)
        self.h_out = [np.zeros(NS_ * 64, np.uint8) for _ in range(4)]
        e.set_msm_window(MSM_WINDOW)
        assert e.msm_plan_window(CID, NM) == MSM_WINDOW
        self.parts = e.dev_alloc(e.msm_parts_bytes(CID, NM) + 64)
        e.set_msm_window(0)

    def close(self):
        for b in (self.k, self.xy, self.xyz, self.x, self.odd, self.tag, self.zero, self.out, self.out2, self.out3, self.parts):
            b.free()
        self.eng.close()

    def call(self, name, *args):
        conv = [a if isinstance(a, (ctypes.c_size_t, ctypes.c_int)) else a.ctypes.data_as(ctypes.c_void_p) if isinstance(a, np.ndarray)
                else ctypes.c_void_p(a.ptr if a is not None else None) for a in args]
        rc = getattr(self.lib, name)(self.eng._ctx, *conv)
        assert rc == OK, (name, rc, self.lib.ecgpu_last_error(self.eng._ctx))

    def resolved(self):
        got = {}
        for name in NAMES:
            ms = ctypes.c_double(-1)
            rc = self.lib.ecgpu_last_timing(self.eng._ctx, name.encode(), ctypes.byref(ms))
            assert rc in (OK, ERR_ARG), (name, rc)
            if rc == OK:
                got[name] = ms.value
        return got


@pytest.fixture(scope="module")
def rig():
    r = Rig()
    yield r
    r.close()


def run_family(r, family):
    c, e = r.call, r.eng
    k, xy, xyz, x, tag, odd, zero, out, o2, o3 = r.k, r.xy, r.xyz, r.x, r.tag, r.odd, r.zero, r.out, r.out2, r.out3
    nb, nm, ns, cid = S(NB), S(NM), S(NS_), I(CID)
    if family == "mul_base":
        c("ecgpu_batch_mul_base_dev", cid, k, nb, out, o2)
    elif family == "mul_base_compressed":
        c("ecgpu_batch_mul_base_compressed_dev", cid, k, nb, out, o2)
    elif family == "mul_base_ct":
        c("ecgpu_batch_mul_base_ct_dev", cid, k, nb, out, o2)
    elif family == "mul":
        c("ecgpu_batch_mul_dev", cid, k, xy, None, nb, out, o2)
    elif family == "mul_xyz":
        c("ecgpu_batch_mul_xyz_dev", cid, k, xyz, nb, out, o2)
    elif family == "mul_compressed":
        c("ecgpu_batch_mul_compressed_dev", cid, k, x, tag, nb, out, o2)
    elif family == "mul_ct":
        c("ecgpu_batch_mul_ct_dev", cid, k, xy, None, nb, out, o2)
    elif family == "mul_ct_xyz":
        c("ecgpu_batch_mul_ct_xyz_dev", cid, k, xyz, nb, out, o2)
    elif family == "mul_add":
        c("ecgpu_batch_mul_base_and_mul_add_dev", cid, k, k, xy, None, nb, out, o2)
    elif family == "mul_add_xyz":
        c("ecgpu_batch_mul_base_and_mul_add_xyz_dev", cid, k, k, xyz, nb, out, o2)
    elif family == "normalize":
        c("ecgpu_batch_normalize_dev", cid, xyz, nb, out, o2)
    elif family == "point_sum":
        c("ecgpu_point_sum_dev", cid, xy, None, nb, out, o2)
    elif family == "lincomb_ct_empty":
        c("ecgpu_lincomb_ct_dev", cid, None, None, None, S(0), out, o2)
    elif family == "lincomb_ct":
        c("ecgpu_lincomb_ct_dev", cid, k, xy, None, nb, out, o2)
    elif family in ("msm_small", "msm_small_untimed"):
        c("ecgpu_msm_dev", cid, k, xy, None, S(3), out, o2)
    elif family in ("msm_buckets", "msm_buckets_untimed", "msm_on_lanes"):
        c("ecgpu_msm_dev", cid, k, xy, None, nm, out, o2)
    elif family == "msm_parts":
        c("ecgpu_msm_parts_dev", cid, k, xy, None, nm, nm, r.parts)
    elif family == "msm_finish":
        c("ecgpu_msm_parts_dev", cid, k, xy, None, nm, nm, r.parts)
        c("ecgpu_msm_finish_dev", cid, r.parts, I(1), nm, out, o2)
    elif family == "ecdsa_verify":
        c("ecgpu_ecdsa_verify_batch_dev", cid, k, k, k, xy, ns, I(0), o2)
    elif family == "ecdsa_recover":
        c("ecgpu_ecdsa_recover_batch_dev", cid, k, k, k, zero, ns, I(0), out, o2)
    elif family == "schnorr_verify":
        c("ecgpu_schnorr_verify_batch_dev", k, k, k, xy, ns, o2)
    elif family == "ecdsa_sign":
        c("ecgpu_ecdsa_sign_batch_dev", cid, k, k, k, ns, I(0), out, o2, o3)
    elif family == "ecdsa_sign_rfc6979":
        c("ecgpu_ecdsa_sign_rfc6979_batch_dev", cid, k, k, ns, I(0), out, o2, o3)
    elif family == "ecdsa_sign_msg":
        c("ecgpu_ecdsa_sign_msg_batch_dev", cid, k, zero, S(16), ns, I(0), out, o2, o3)
    elif family == "schnorr_sign":
        c("ecgpu_schnorr_sign_raw_batch_dev", k, zero, S(16), zero, ns, out, o2)
    elif family == "decompress":
        c("ecgpu_batch_decompress_dev", cid, x, odd, ns, out, o2)
    elif family.startswith(("sm2dsa_", "bign_", "sm2_pke_")):
        hk, hxy, hz, (h0, h1, h2, h3) = r.h_k, r.h_xy, r.h_zero, r.h_out
        if family == "sm2dsa_sign":
            c("ecgpu_sm2dsa_sign_batch", hk, hk, hk, ns, h0, h1)
        elif family == "sm2dsa_sign_rfc6979":
            c("ecgpu_sm2dsa_sign_rfc6979_batch", hk, hk, ns, h0, h1)
        elif family == "sm2dsa_sign_msg":
            c("ecgpu_sm2dsa_sign_msg_batch", hz, S(16), hk, hz, S(16), ns, h0, h1)
        elif family == "bign_sign":
            c("ecgpu_bign_sign_batch", hk, hk, hk, ns, h0, h1)
        elif family == "bign_sign_prehash":
            c("ecgpu_bign_sign_prehash_batch", hk, hk, ns, h0, h1)
        elif family == "bign_sign_msg":
            c("ecgpu_bign_sign_msg_batch", hk, hz, S(16), ns, h0, h1)
        elif family == "sm2_pke_encrypt":
            c("ecgpu_sm2_pke_encrypt_batch", hxy, hk, hz, S(16), ns, h0, h1, h2, h3)
        elif family == "sm2_pke_decrypt":
            c("ecgpu_sm2_pke_decrypt_batch", hk, hxy, hz, S(16), hz, ns, h0, h1)
        else:
            raise KeyError(family)
    else:
        raise KeyError(family)


@pytest.mark.parametrize("family", list(EXPECTED))
def test_stage_names_of_the_family(rig, family):
    e = rig.eng
    forced = family.startswith("msm_buckets") or family in ("msm_parts", "msm_finish", "msm_on_lanes")
    untimed, lanes = family.endswith("_untimed"), family == "msm_on_lanes"
    try:
        e.set_msm_window(MSM_WINDOW if forced else 0)
        if lanes:
            e.set_async(True)
            e.set_msm_lanes(2)
        e.set_timing(False)                      # drops what the call before left
        e.set_timing(not untimed)
        run_family(rig, family)
        got = rig.resolved()
        if lanes:
            e.synchronize()
    finally:
        if lanes:
            e.set_msm_lanes(1)
            e.set_async(False)
        e.set_timing(True)
        e.set_msm_window(0)
    print(family, sorted(got))
    assert tuple(n for n in NAMES if n in got) == tuple(n for n in NAMES if n in EXPECTED[family]), (family, got)
    assert all(v >= 0 for v in got.values()), got
    if "total" in got:
        assert got["total"] >= got["main"] >= 0, got
