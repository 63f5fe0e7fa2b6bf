"""Launch geometries in which ONE lane walks SEVERAL records and carries state from one to the next, restated in Python, and a
planting helper that puts degenerate records at every position of such a chain (shared by tests/test_lane_chains.py and
tests/test_gpu_lane_chains.py; numpy only).

A "chain" is the list of records one lane owns, in the order it walks them: lane t of T owns records t, t + T, t + 2T, ...

  * The Montgomery-trick kernels (k_normalize, k_xyz_affine, k_scalar_batch_inv) build a running product over the chain, invert
    once and peel the inverses off on the way back; a record that is the identity (Z = 0; a scalar outside [1, n - 1]) has to
    stay out of the product on both passes.
  * The variable-base kernels (k_var_base, k_var_base_ct, k_xyz_mul_ct) stride over the batch above 524,288 lanes; the second
    record of a lane reuses the lane's table slot.
"""
import numpy as np

NORM_RECORDS_PER_LANE_STEP = 65536      # K = ceil(n / 65536) ...
NORM_K_MAX = 64                         # ... at most 64
NORM_K_KNOB_MAX = 1024                  # ECGPU_NORM_K is honoured in [1, 1024]
BLOCK = 256
VAR_MAX_SLOTS = 256 * 8 * BLOCK         # 524,288 resident lanes

CLASSES = ("first", "middle", "last", "adjacent", "all", "all-but-one", "ragged-last", "record n-1", "record T-1", "record T")


def norm_geometry(n, K=None):
    """(K, T) of launch_normalize, launch_normalize_compressed, launch_xyz_affine (csrc/ecgpu_inst_base.hip:28-73) and
    launch_scalar_batch_inv (:93-99): K = min(64, ceil(n / 65536)) records per lane, T = ceil(n / K) lanes.  An explicit K is the
    ECGPU_NORM_K override of the tool build (:33-36), which only launch_normalize honours."""
    assert n >= 1
    if K is None:
        K = min(NORM_K_MAX, (n + NORM_RECORDS_PER_LANE_STEP - 1) // NORM_RECORDS_PER_LANE_STEP)
    assert 1 <= K <= NORM_K_KNOB_MAX
    return K, (n + K - 1) // K


def var_geometry(n):
    """T of var_base_slots (csrc/ecgpu_inst_var.hip:10-14): n rounded up to whole workgroups, at most 524,288; lane `slot` does
    records slot, slot + T, ... (csrc/ecgpu_var.h:47)."""
    return min((n + BLOCK - 1) // BLOCK * BLOCK, VAR_MAX_SLOTS)


def chain(t, n, T):
    """The records of lane t, in the order of the forward pass (csrc/ecgpu_kernels.h:420; k_xyz_affine and
    k_scalar_batch_inv: batch_inv_lane's walk, csrc/ecgpu_batchinv.h:24-35 and :54)."""
    return np.arange(t, n, T, dtype=np.int64)


def chain_lengths(n, T):
    """(length of a full chain, number of lanes that have it): lanes [0, full) own `length` records, lanes [full, T) — the
    ragged group, empty when T divides n — one fewer."""
    length = (n + T - 1) // T
    return length, n - (length - 1) * T


def plant(n, T, m, degenerate_ids, seed, avoid=()):
    """-> (idx_map int32[n], report).  idx_map[i] = i % m tiles a table of m cases over the batch (m prime and no divisor of T, so
    that the records of one lane are different cases); then one lane per position class is rewritten: its planted positions get
    indices from `degenerate_ids`, all its other records ordinary cases.  Lanes in `avoid` are left to the caller.

    report = {"length", "full_lanes", "T", "n", "classes": {name: {"lane", "positions", "records"}}, "absent": {name: why},
              "lane_class": {lane: [names]}}.  Every class has a lane of its own, so that the lane is degenerate at the class's
    positions and nowhere else; a class is absent when the geometry has no chain of the shape it needs, or no lane left for it
    (two classes share a lane only when they name the very same records)."""
    deg = [int(d) for d in degenerate_ids]
    assert deg and all(0 <= d < m for d in deg) and len(set(deg)) < m
    assert m >= 2 and (T == 1 or T % m), "m must not divide T"
    ordinary = np.array([j for j in range(m) if j not in set(deg)], np.int32)
    is_deg = np.zeros(m, bool)
    is_deg[deg] = True
    rng = np.random.default_rng(seed)
    idx_map = (np.arange(n, dtype=np.int64) % m).astype(np.int32)
    length, full = chain_lengths(n, T)
    avoid = set(int(a) for a in avoid)
    report = {"n": n, "T": T, "length": length, "full_lanes": full, "classes": {}, "absent": {}, "lane_class": {}}
    used = {}                                        # lane -> its planted positions

    def put(name, t, positions):
        recs = chain(t, n, T)
        if t not in used:
            cur = idx_map[recs]                      # every record of the lane ordinary first ...
            bad = is_deg[cur]
            cur[bad] = ordinary[(recs[bad] + 1) % len(ordinary)]
            idx_map[recs] = cur
            for p in positions:                      # ... then the planted positions
                idx_map[recs[p]] = deg[int(rng.integers(len(deg)))]
            used[t] = list(positions)
        report["classes"][name] = {"lane": t, "positions": list(positions), "records": [int(recs[p]) for p in positions]}
        report["lane_class"].setdefault(t, []).append(name)

    # the classes whose lane is given by a record number
    fixed = {"record n-1": ((n - 1) % T, [(n - 1) // T]), "record T-1": (T - 1, [0])}
    if n > T:
        fixed["record T"] = (0, [1])
    else:
        report["absent"]["record T"] = "one record per lane"
    reserved = {t for t, _ in fixed.values()}

    def free_lane(lo, hi, may_take_reserved):
        """a lane of [lo, hi) that no class uses yet: a random one (any wave, any workgroup), else the first; a lane that a record
        class names only when there is no other (that record class is then absent)"""
        ok = lambda t, res: t not in used and t not in avoid and (res or t not in reserved)
        for _ in range(64):
            t = int(rng.integers(lo, hi))
            if ok(t, False):
                return t
        for res in (False, True) if may_take_reserved else (False,):
            for t in range(lo, min(hi, lo + 4096)):
                if ok(t, res):
                    return t
        return None

    # (name, lane range — full-length lanes, or the ragged group —, positions as a function of the chain length, reason if absent)
    wanted = []
    wanted.append(("middle", (0, full), lambda k: [k // 2] if k >= 3 else None, "no chain of 3 or more"))
    wanted.append(("adjacent", (0, full), lambda k: [k // 2, k // 2 + 1] if k >= 3 else None, "no chain of 3 or more"))
    wanted.append(("last", (0, full), lambda k: [k - 1] if k >= 2 else None, "no chain of 2 or more"))
    wanted.append(("first", (0, full), lambda k: [0] if k >= 2 else None, "no chain of 2 or more"))
    wanted.append(("ragged-last", (full, T), lambda k: [k - 1] if k >= 1 else None, "no ragged lanes"))
    wanted.append(("all", (0, full), lambda k: list(range(k)), ""))
    wanted.append(("all-but-one", (0, full), lambda k: [p for p in range(k) if p != min(1, k - 1)] if k >= 2 else None, "no chain of 2 or more"))
    for name, (lo, hi), pos, why in wanted:
        if hi <= lo:
            report["absent"][name] = why or "no such lane"
            continue
        positions = pos(length if lo < full else length - 1)
        if positions is None:
            report["absent"][name] = why
            continue
        t = free_lane(lo, hi, name not in ("all", "all-but-one"))
        if t is None:
            report["absent"][name] = "no lane left"
            continue
        put(name, t, positions)
    for name, (t, positions) in fixed.items():
        if t in used and used[t] != positions:       # (the same records under two names are one planting)
            report["absent"][name] = "its lane holds %s" % "+".join(report["lane_class"][t])
            continue
        put(name, t, positions)
    return idx_map, report


def describe(i, report):
    """'record i = lane t, position p of k, class ...' for a failure message"""
    T, n = report["T"], report["n"]
    t, p = int(i) % T, int(i) // T
    k = len(range(t, n, T))
    cls = report["lane_class"].get(t)
    return "record %d = lane %d, chain position %d of %d, class %s" % (i, t, p, k, "+".join(cls) if cls else "tiled")


def first_mismatch(got, want, report, what=""):
    """None when the two (n, width) row arrays are equal, else a message: the first mismatching record with its lane, chain position
    and class, and the classes of every lane that holds a mismatch."""
    got = np.asarray(got).reshape(report["n"], -1)
    want = np.asarray(want).reshape(report["n"], -1)
    if np.array_equal(got, want):
        return None
    bad = np.nonzero((got != want).any(axis=1))[0]
    lanes = np.unique(bad % report["T"])
    classes = sorted({c for t in lanes.tolist() for c in report["lane_class"].get(t, ["tiled"])})
    return "%s: %d records differ; first: %s; classes hit: %s" % (what, bad.size, describe(int(bad[0]), report), ", ".join(classes))
