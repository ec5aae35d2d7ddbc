"""bench.py prints exactly ONE JSON line on stdout with the fields the driver and the judge read: a plain run the headline
fields only (and, with --dump-outputs, the factor and statistics of its last timed step), a --full run the roofline object
beside them (quick settings: 3 steps, no CPU baseline, no full solve, no dense figures -- --full alone adds those objects)."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import bench
from conftest import golden_path

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_prints_one_json_line_with_the_contract_fields():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1",
                        "--full", "--no-cpu-baseline", "--no-kkt", "--no-dense"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline"):
        assert key in d, key
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1
    assert d["dtype"] == "f64" and d["vs_baseline"] is None and d["higher_is_better"] is True
    assert "workload" in d["config"] and "model" not in d["config"]
    assert d["value"] > 0 and d["ms_per_step"] > 0
    rf = d["roofline"]
    for key in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert key in rf, key
    assert rf["bound"] == "hbm" and rf["peak"] == 8000.0 and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-12
    # value = Hess-vecs of all steps / wall time
    assert abs(d["value"] - d["config"]["hessvecs_per_step"] / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]


def test_plain_run_is_the_headline_and_dumps_its_last_step(tmp_path):
    out = tmp_path / "outputs"
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "2",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600)
    wall = time.perf_counter() - t0
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 4 and d["warmup"] == 2 and d["n_gpus"] == 1
    assert d["metric"] == "tCG Hess-vec prods/sec (n,p), G81 MaxCut" and d["unit"] == "Hess-vec/s"
    assert d["dtype"] == "f64" and d["higher_is_better"] is True
    assert 0 < d["ms_per_step"] * 1e-3 * (4 + 2) < wall
    assert abs(d["value"] - d["config"]["hessvecs_per_step"] / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]
    for key in ("roofline", "cpu_baseline", "g81_kkt", "dense_mfma", "large_sparse_trip", "affine_hessvec", "cross_rank_trip",
                "hessvec_by_p"):
        assert key not in d, key
    Y = np.load(out / "Y.npy")
    assert Y.dtype == np.float64 and Y.shape == (d["config"]["n"], d["config"]["p"])
    assert np.abs(np.linalg.norm(Y, axis=1) - 1.0).max() < 1e-12
    st = {k: np.load(out / (k + ".npy")) for k in bench.DUMP_STATS}
    assert all(v.dtype == np.float64 and v.shape == (1,) for v in st.values())
    assert st["hessvecs"][0] == d["config"]["hessvecs_per_step"]
    assert sum(f.stat().st_size for f in out.iterdir()) <= 64 << 20
    # the dumped cost is that of the dumped factor (oracle: ManiSDP_onlyunitdiag.m's cost of the same point)
    from manisdp_matlab_amd import problems
    from oracle import manisdp_ref
    C = problems.maxcut_cost_matrix(golden_path("G81.txt.gz"))
    f = manisdp_ref._OnlyUnitDiagProblem(C, Y.shape[0], Y.shape[1]).cost(Y)
    assert abs(st["cost"][0] - f) <= 1e-10 * abs(f)
