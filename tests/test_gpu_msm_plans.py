"""-m gpu: the MSM at every boundary of its planner, each case against the exact value.

The MSM (ecgpu_msm_dev) runs one of several plans, chosen by the term count n (csrc/ecgpu_msm.h msm_plan, csrc/ecgpu_api.hip
msm_dev).  The formulas, which `_plan` below restates:
  - small path (msm_small_max): 1 <= n <= 2^16 on the 8-word sets, n <= 2^10 on the wider ones -> one variable-base
    multiplication per term and a tree sum, no buckets;
  - GLV (msm_use_glv): k256 with n < MSM_GLV_MAX_TERMS = 13 * 2^17 -> two 128-bit halves per term;
  - window c (msm_window_bits), lg = floor(log2 n): GLV 13 for lg 16..18, 15 from 19; plain lg - 3 up to lg 16, 13 for lg 17..19,
    14 for lg 20 below 13 * 2^17, 16 from there on;
  - entries per window ne = (GLV ? 2 : 1) * npad, npad = n rounded up to 64.  Two-level sort when ne >= 2^17 and c - 1 > 8;
    its packed form keeps bb = min(c - 9, 31 - idx_bits, 8) low bucket bits, idx_bits = ceil(log2 ne), and holds when the
    c - 1 - bb level-A bits are at most 9 and k_msm_prepare's histogram nwin * (nb >> bb) * 4 bytes fits 64 KiB; otherwise
    the unpacked (round-3) sort kernels run.  At c = 16 that is 8 level-A bits up to 2^24 entries, 9 up to 2^25, unpacked
    above (and p521's 34 windows stay unpacked above 2^24: 34 * 512 * 4 > 64 KiB);
  - record of a local half (ecgpu_msm_parts_bytes): nwin * nparts * 3 * NS * 4 bytes, nwin = kbits / c + 1 (kbits 128 with
    GLV, else 32 N - 1), nparts = min(32, ceil(2^(c - 1) / 4 / 256)), NS the words of the raw field form.
Every case asserts the window and the record size the library reports (so that a retuned threshold fails here instead of
quietly moving the case to the other side) and compares the MSM with (sum k_i s_i mod n) G, where P_i = s_i G are made on the
device (and sampled against the oracle).  Identity terms sit at a fixed stride and at the first and last index of every size.
All sizes of a curve are prefixes of one set of terms."""
import numpy as np
import pytest

import oracle_lib
import pyec
from gpu_common import dot_mod, ecgpu_module, fast_scalars, rand_scalars, scalars_to_int_sum

pytestmark = pytest.mark.gpu

MSM_GLV_MAX_TERMS = 13 << 17
WORDS = {"k256": 8, "p256": 8, "p384": 12, "p521": 17}               # C::N
RAW_WORDS = {"k256": 12, "p256": 12, "p384": 16, "p521": 24}          # Field<C>::NS = (NL / 4 + 1) * 4, NL = 9 / 10 / 15 / 20
IDENTITY_STRIDE = 1021
ORACLE_MSM_MAX = 8192


def _plan(curve, n):
    """(window bits, parts bytes, form) the planner gives n terms; form: "small", "single" (one-level counting sort),
    "packed8" / "packed9" (two-level sort, packed, with that many level-A bits) or "unpacked"."""
    N, NS = WORDS[curve], RAW_WORDS[curve]
    glv = curve == "k256" and n < MSM_GLV_MAX_TERMS
    lg = n.bit_length() - 1
    if glv:
        c = lg - 2 if lg <= 15 else (13 if lg <= 18 else 15)
    elif lg <= 16:
        c = lg - 3
    elif lg <= 19:
        c = 13
    elif lg == 20:
        c = 14 if n < MSM_GLV_MAX_TERMS else 16
    else:
        c = 16
    c = min(max(c, 4), 16)
    nwin = (128 if glv else 32 * N - 1) // c + 1
    nb = 1 << (c - 1)
    nseg = nb // min(4, nb)
    parts_bytes = nwin * min(32, -(-nseg // 256)) * 3 * NS * 4
    ne = (2 if glv else 1) * (-(-n // 64) * 64)
    if n <= (1 << (16 if N <= 8 else 10)):
        form = "small"
    elif ne < (1 << 17) or c - 1 <= 8:
        form = "single"
    else:
        idx_bits = max(1, (ne - 1).bit_length())
        bb = min(c - 9, 31 - idx_bits, 8)
        packed = bb >= 1 and c - 1 - bb <= 9 and nwin * (nb >> bb) * 4 <= 64 * 1024
        form = "packed%d" % (c - 1 - bb) if packed else "unpacked"
    return c, parts_bytes, form


# (curve, n, the form n is on): each boundary with a size on either side
CASES = [
    ("k256", 1 << 16, "small"), ("k256", (1 << 16) + 1, "packed8"),                        # small path -> GLV buckets
    ("k256", (1 << 19) - 1, "packed8"), ("k256", 1 << 19, "packed8"),                      # GLV c 13 -> 15
    ("k256", MSM_GLV_MAX_TERMS - 1, "packed8"), ("k256", MSM_GLV_MAX_TERMS, "packed8"),    # GLV c 15 -> plain c 16
    ("k256", (1 << 24) + 1, "packed9"), ("k256", 1 << 25, "packed9"), ("k256", (1 << 25) + 1, "unpacked"),
    ("p256", 1 << 16, "small"), ("p256", (1 << 16) + 1, "single"),                         # small path -> buckets
    ("p256", (1 << 17) - 64, "single"), ("p256", 1 << 17, "packed8"),                      # one- -> two-level sort
    ("p256", 1 << 20, "packed8"), ("p256", MSM_GLV_MAX_TERMS - 1, "packed8"), ("p256", MSM_GLV_MAX_TERMS, "packed8"),   # c 14 -> 16
    ("p384", 1 << 10, "small"), ("p384", (1 << 10) + 1, "single"),
    ("p384", MSM_GLV_MAX_TERMS, "packed8"), ("p384", (1 << 24) + 1, "packed9"),            # 24 windows: 48 KiB of level-A counters
    ("p521", (1 << 10) + 1, "single"),
    ("p521", MSM_GLV_MAX_TERMS, "packed8"), ("p521", (1 << 24) + 1, "unpacked"),           # 34 windows: the LDS guard
]
SIZES = {}
for _cv, _n, _ in CASES:
    SIZES.setdefault(_cv, []).append(_n)
SKEW_SIZES = [1 << 25, (1 << 25) + 1]                    # k256


class Terms:
    """k_i and P_i = s_i G (with identity flags) for the largest size of a curve, on the device; every size is a prefix.
    Host arrays are made in chunks and dropped once the exact prefix sums are known."""

    CHUNK = 1 << 22

    def __init__(self, eng, curve, sizes):
        c = pyec.CURVES[curve]
        L, n = c.L, max(sizes)
        self.c, self.L, self.n = c, L, n
        if curve == "p521":                              # fast_scalars needs an order that starts with 32 one bits
            gen = lambda m, seed: rand_scalars(c.cid, m, seed).reshape(m, L)
        else:
            gen = lambda m, seed: fast_scalars(c, m, seed)
        k, s = np.empty((n, L), np.uint8), np.empty((n, L), np.uint8)
        for j, lo in enumerate(range(0, n, self.CHUNK)):
            hi = min(n, lo + self.CHUNK)
            k[lo:hi] = gen(hi - lo, 0xEC00A100 + 64 * c.cid + j)
            s[lo:hi] = gen(hi - lo, 0xEC00A200 + 64 * c.cid + j)
        for i, v in ((1, c.n - 1), (2, 0), (3, 1)):
            k[i] = np.frombuffer(v.to_bytes(L, "big"), np.uint8)
        self.identity = sorted(set(range(0, n, IDENTITY_STRIDE)) | {m - 1 for m in sizes})
        s[self.identity] = 0                             # P_i = 0 G: flagged identities, and out of the dot product
        self.dot, acc, lo = {}, 0, 0
        for m in sorted(sizes):
            acc = (acc + dot_mod(k[lo:m], s[lo:m], c.n)) % c.n
            self.dot[m], lo = acc, m
        # k256: sums of s_i over i = j mod 3 (the skewed scalar set)
        self.third_sums = {m: [scalars_to_int_sum(s[j:m:3], L, c.n) for j in range(3)] for m in SKEW_SIZES if m in sizes}
        self.sample = sorted(set(np.linspace(0, n - 1, 48).astype(int).tolist()) | {1, 2, 3, IDENTITY_STRIDE}
                             | {m - 1 for m in sizes})
        self.sample_s = s[self.sample].copy()
        self.head = min(n, ORACLE_MSM_MAX)
        self.k_head = k[:self.head].copy()
        self.d_k = self.d_p = self.d_inf = None
        d_s = eng.to_device(s.reshape(-1))
        try:
            self.d_k = eng.to_device(k.reshape(-1))
            del k, s
            self.d_p, self.d_inf = eng.dev_alloc(n * 2 * L), eng.dev_alloc(n + 16)
            eng.mul_by_generator_dev(c.cid, d_s, n, self.d_p, self.d_inf)
        finally:
            d_s.free()

    def free(self):
        for b in (self.d_k, self.d_p, self.d_inf):
            if b is not None:
                b.free()


@pytest.fixture(scope="module")
def eng():
    e = ecgpu_module().Engine(0)
    oracle_lib.build()
    yield e
    e.close()


@pytest.fixture(scope="module")
def terms(eng):
    made = {}

    def get(curve):                                      # (all four sets together: about 9 GB of device memory)
        if curve not in made:
            made[curve] = Terms(eng, curve, SIZES[curve])
        return made[curve]

    yield get
    for t in made.values():
        t.free()


def _msm(eng, t, n, d_k=None, off=0):
    """the one-call MSM of terms [off, off + n) -> (xy bytes, identity flag)"""
    L = t.L
    d_k = t.d_k if d_k is None else d_k
    d_o, d_f = eng.dev_alloc(256), eng.dev_alloc(16)
    try:
        eng.lincomb_dev(t.c.cid, d_k.at(off * L), t.d_p.at(off * 2 * L), t.d_inf.at(off), n, d_o, d_f)
        return bytes(eng.to_host(d_o, 2 * L)), int(eng.to_host(d_f, 1)[0])
    finally:
        d_o.free()
        d_f.free()


def _exact(c, v):
    """v G by the oracle -> (xy bytes, identity flag)"""
    w, wf = oracle_lib.batch_mul_base(c.cid, pyec.enc_scalar(c, v % c.n))
    return bytes(w), int(wf[0])


@pytest.mark.parametrize("curve", list(SIZES))
def test_msm_plan_terms_are_s_i_g(eng, terms, curve):
    """The points every case of the curve uses: a strided sample (the edges, the identities at the first index, at the stride
    and at each size's last index included) against the oracle's fixed-base multiplication, flags included."""
    t = terms(curve)
    L = t.L
    got = b"".join(bytes(eng.to_host(t.d_p, 2 * L, i * 2 * L)) for i in t.sample)
    ginf = b"".join(bytes(eng.to_host(t.d_inf, 1, i)) for i in t.sample)
    want, winf = oracle_lib.batch_mul_base(t.c.cid, t.sample_s.reshape(-1))
    assert got == bytes(want) and ginf == bytes(winf)
    assert int(winf.sum()) == len(set(t.sample) & set(t.identity)) > 0


@pytest.mark.parametrize("curve,n,form", CASES, ids=["%s-%d" % (cv, n) for cv, n, _ in CASES])
def test_msm_at_plan_boundary(eng, terms, curve, n, form):
    c_bits, parts_bytes, model_form = _plan(curve, n)
    assert model_form == form, "the planner's formulas no longer put %d terms on the %s side" % (n, form)
    t = terms(curve)
    cid = t.c.cid
    assert eng.msm_plan_window(cid, n) == c_bits
    assert eng.msm_parts_bytes(cid, n) == parts_bytes
    got = _msm(eng, t, n)
    assert got == _exact(t.c, t.dot[n]), (curve, n, form)
    if n <= ORACLE_MSM_MAX:
        pts, inf = eng.to_host(t.d_p, n * 2 * t.L), eng.to_host(t.d_inf, n)
        w, wf = oracle_lib.msm(cid, t.k_head[:n].reshape(-1), pts, inf, vartime=True)
        assert got == (bytes(w), wf)


@pytest.mark.parametrize("n", SKEW_SIZES)
def test_msm_skewed_scalars_past_2p24(eng, terms, n):
    """Three distinct scalars tiled over every term: each window has three buckets of ~n / 3 entries, far above the limit of
    k_msm_sort_b (the big-partition sort k_msm_sort_b_big of the packed form at 2^25, the unpacked sort at 2^25 + 1) and of
    one accumulation lane (k_msm_big_buckets).  Exact value: sum_j k_j (sum of s_i over i = j mod 3)."""
    t = terms("k256")
    c, L = t.c, t.L
    three = fast_scalars(c, 3, 0xEC00A300)
    want = sum(int.from_bytes(bytes(three[j]), "big") * t.third_sums[n][j] for j in range(3)) % c.n
    d_ks = eng.to_device(np.tile(three, (-(-n // 3), 1))[:n].reshape(-1))
    try:
        assert _msm(eng, t, n, d_k=d_ks) == _exact(c, want)
    finally:
        d_ks.free()


@pytest.mark.parametrize("n", SKEW_SIZES)
def test_msm_split_linearity_past_2p24(eng, terms, n):
    """MSM(all) == MSM(first 2^24) + MSM(rest): the new sort forms (9 level-A bits at 2^25, unpacked at 2^25 + 1) against the
    form test_gpu_fullsize covers (8 level-A bits at 2^24) and, at 2^25 + 1, the 9-bit form of the 2^24 + 1 rest."""
    t = terms("k256")
    h = 1 << 24
    full = _msm(eng, t, n)
    a, b = _msm(eng, t, h), _msm(eng, t, n - h, off=h)
    sm, sf = eng.point_sum(0, np.frombuffer(a[0] + b[0], np.uint8), np.array([a[1], b[1]], np.uint8))
    assert (bytes(sm), sf) == full == _exact(t.c, t.dot[n])


def test_msm_parts_one_shard_past_2p24(eng, terms):
    """ecgpu_msm_parts_dev on one shard of 2^24 + 1 terms (plan_terms the same: the 9-bit packed sort) and ecgpu_msm_finish_dev
    with one rank == the one-call MSM == the exact value."""
    t = terms("k256")
    n, L = (1 << 24) + 1, t.L
    d_parts, d_o, d_f = eng.dev_alloc(eng.msm_parts_bytes(0, n)), eng.dev_alloc(256), eng.dev_alloc(16)
    try:
        eng.msm_parts_dev(0, t.d_k, t.d_p, t.d_inf, n, n, d_parts)
        eng.msm_finish_dev(0, d_parts, 1, n, d_o, d_f)
        got = bytes(eng.to_host(d_o, 2 * L)), int(eng.to_host(d_f, 1)[0])
    finally:
        for b in (d_parts, d_o, d_f):
            b.free()
    assert got == _msm(eng, t, n) == _exact(t.c, t.dot[n])


def test_msm_finish_on_lanes_waits_for_unjoined_local_halves():
    """Asynchronous context, two MSM lanes, k256 at 2^21 terms (a local half of ~2 ms on its lane).  The record buffers first
    hold the parts of ANOTHER MSM.  Then, without ecgpu_msm_parts_join_dev: (a) one rank, the record itself passed to
    ecgpu_msm_finish_dev; (b) two shards written at offsets of one buffer, finished with nranks = 2; and (c) the joined order of
    test_sharded_msm_steps_on_rotating_lanes.  After ecgpu_synchronize all three must be the one-call MSM: the combining half
    waits for the local halves whose records lie inside what it reads."""
    ecgpu = ecgpu_module()
    e = ecgpu.Engine(0)
    bufs = []

    def alloc(nbytes):
        bufs.append(e.dev_alloc(nbytes))
        return bufs[-1]

    try:
        c, L, n = pyec.K256, 32, 1 << 21
        h = n // 2
        s = fast_scalars(c, n, 0xEC00A400)
        ka, kb = fast_scalars(c, n, 0xEC00A401), fast_scalars(c, n, 0xEC00A402)
        pts, _ = e.mul_by_generator(0, s.reshape(-1))
        want = e.lincomb(0, ka.reshape(-1), pts)
        assert (bytes(want[0]), want[1]) == _exact(c, dot_mod(ka, s, c.n))
        stale = e.lincomb(0, kb.reshape(-1), pts)
        assert bytes(stale[0]) != bytes(want[0])
        d_p, d_ka, d_kb = alloc(n * 2 * L), alloc(n * L), alloc(n * L)
        e.to_device(pts, d_p)
        e.to_device(ka.reshape(-1), d_ka)
        e.to_device(kb.reshape(-1), d_kb)
        nb1, nb2 = e.msm_parts_bytes(0, n), e.msm_parts_bytes(0, h)
        d_one, d_two, d_joined = alloc(nb1), alloc(2 * nb2), alloc(2 * nb2)
        outs = [(alloc(256), alloc(16)) for _ in range(3)]
        # the stale records: kb's local halves, written synchronously
        e.msm_parts_dev(0, d_kb, d_p, None, n, n, d_one)
        for buf in (d_two, d_joined):
            for r in range(2):
                e.msm_parts_dev(0, d_kb.at(r * h * L), d_p.at(r * h * 2 * L), None, h, h, buf.at(r * nb2))
        e.set_async(True)
        e.set_msm_lanes(2)
        e.msm_parts_dev(0, d_ka, d_p, None, n, n, d_one)                                     # (a)
        e.msm_finish_dev(0, d_one, 1, n, *outs[0])
        for r in range(2):                                                                    # (b)
            e.msm_parts_dev(0, d_ka.at(r * h * L), d_p.at(r * h * 2 * L), None, h, h, d_two.at(r * nb2))
        e.msm_finish_dev(0, d_two, 2, h, *outs[1])
        for r in range(2):                                                                    # (c)
            e.msm_parts_dev(0, d_ka.at(r * h * L), d_p.at(r * h * 2 * L), None, h, h, d_joined.at(r * nb2))
        for r in range(2):
            e.msm_parts_join_dev(d_joined.at(r * nb2))
        e.msm_finish_dev(0, d_joined, 2, h, *outs[2])
        e.synchronize()
        e.set_msm_lanes(1)
        e.set_async(False)
        for what, (d_o, d_f) in zip(("one rank, no join", "two shards, no join", "joined"), outs):
            got = bytes(e.to_host(d_o, 2 * L)), int(e.to_host(d_f, 1)[0])
            assert got[0] != bytes(stale[0]), "%s: the stale record was combined" % what
            assert got == (bytes(want[0]), want[1]), what
    finally:
        for b in bufs:
            b.free()
        e.close()
