"""GPU test of bench.py's plain run, the command every benchmark figure is quoted on: it times the headline workload and prints the contract's
line without any of the side measurements that only `--full` runs (roofline micro-benchmark, other configurations, end-to-end CLI processes,
ingest, CPU baseline)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FULL_ONLY = {"roofline", "roofline_hbm", "roofline_coverage", "configs", "e2e", "e2e_wall_s", "e2e_config2", "ingest", "cpu_baseline"}


def test_plain_bench_run_prints_the_headline_line_only(tmp_path):
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "1", "--warmup", "1", "--dump-outputs", str(out)], cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    line = json.loads(lines[0])
    assert line["metric"] == "precursor windows folded+filtered/sec (L=300)" and line["unit"] == "windows/s" and line["higher_is_better"] is True
    assert line["dtype"] == "int16/int32 (energies in 0.01 kcal/mol)" and line["steps"] == 1 and line["warmup"] == 1 and line["n_gpus"] == 1
    assert line["config"]["windows_total"] == 19686 and line["config"]["loci_found"] == 4002
    assert line["value"] > 0 and abs(line["ms_per_step"] * line["value"] / 1e3 - 19686) < 1e-6 * 19686
    assert set(line["stage_ms"]) >= {"coverage", "candidate_rest", "fold", "fold_fill_kernel", "fold_epilogue_kernel", "predict"}
    assert not FULL_ONLY & set(line), sorted(FULL_ONLY & set(line))
    assert len(np.load(out / "locus_fold_s.npy")) == 4002
