"""bench.py's plain run and --dump-outputs: the result line of a plain run, and the dumped outputs are the last timed step's."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bench_module():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def test_dump_outputs_writes_float32_and_one_seeded_sample(tmp_path):
    """Up to DUMP_ROWS rows are written whole; beyond, every array is cut to the same seeded sample of rows, the same in every run."""
    import torch
    bench = bench_module()
    n = bench.DUMP_ROWS + 1000
    pts = torch.arange(n * 4, dtype=torch.int64).remainder(256).to(torch.uint8).reshape(n, 4)
    flags = torch.arange(n, dtype=torch.int64).remainder(2).to(torch.uint8)
    for d in ("a", "b"):
        bench.dump_outputs(torch, str(tmp_path / d), n, {"points": pts, "infinity": flags})
    rows = np.load(tmp_path / "a" / "rows.npy")
    assert rows.dtype == np.float64 and rows.shape == (bench.DUMP_ROWS,) and np.all(np.diff(rows) > 0) and rows[-1] < n
    idx = rows.astype(np.int64)
    for name, t in (("points", pts), ("infinity", flags)):
        a, b = np.load(tmp_path / "a" / (name + ".npy")), np.load(tmp_path / "b" / (name + ".npy"))
        assert a.dtype == np.float32 and np.array_equal(a, b) and np.array_equal(a, t.numpy()[idx].astype(np.float32))
    assert np.array_equal(np.load(tmp_path / "b" / "rows.npy"), rows)
    bench.dump_outputs(torch, str(tmp_path / "c"), 16, {"points": pts})      # a small output: every row, no index file
    assert np.array_equal(np.load(tmp_path / "c" / "points.npy"), pts.numpy()[:16].astype(np.float32))
    assert not (tmp_path / "c" / "rows.npy").exists()


def test_steps_must_be_positive():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--steps" in r.stderr


@pytest.mark.gpu
def test_plain_run_line_and_dumped_outputs(tmp_path, oracle):
    """A plain run prints the headline fields and nothing of --full; what it dumps is the output of its last timed step (the
    input set of that step regenerated from its seed), point for point against the oracle on a sample of the dumped rows."""
    import torch
    bench = bench_module()
    n, steps, warmup = 1 << 17, 3, 2
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--n", str(n), "--steps", str(steps),
                        "--warmup", str(warmup), "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    rec = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert rec["metric"] == bench.WORKLOADS["fixed_k256"]["metric"] and rec["unit"] == "scalar-muls/s" and rec["higher_is_better"] is True
    assert rec["dtype"] == "u32 limbs (v_mad_u64_u32)" and rec["steps"] == steps and rec["warmup"] == warmup
    assert rec["ms_per_step"] > 0 and abs(rec["value"] - n / (rec["ms_per_step"] * 1e-3)) < 1e-6 * rec["value"]
    assert "roofline" not in rec and "check_vs_oracle" not in rec and "configs" not in rec and "cpu_baseline" not in rec

    pts, inf, rows = (np.load(out / (k + ".npy")) for k in ("points", "infinity", "rows"))
    assert pts.dtype == inf.dtype == np.float32 and pts.shape == (bench.DUMP_ROWS, 64) and inf.shape == (bench.DUMP_ROWS,)
    assert sum(os.path.getsize(out / f) for f in os.listdir(out)) <= 64 << 20
    j = (warmup + steps - 1) % 4                                    # the input set of the last timed step (four sets in turn)
    d_k = bench.device_random_scalars(torch, n, 32, 0xEC000000 + bench.SEEDS["fixed_k256"] + 7919 * j, "cuda:0")
    pick = np.arange(0, bench.DUMP_ROWS, bench.DUMP_ROWS // 512)
    k = d_k.cpu().numpy()[rows[pick].astype(np.int64)].reshape(-1)
    want, winf = oracle.batch_mul_base(0, k)
    assert pts[pick].astype(np.uint8).tobytes() == bytes(want) and not inf[pick].any() and not np.asarray(winf).any()
