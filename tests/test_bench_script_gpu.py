"""bench.py end to end on a small grid: a plain run prints the headline line and dumps the iterate of its last timed
cycle, which is the oracle's cycle on the same hierarchy; --full adds the kernel, PCG and CPU-baseline figures and passes
its parity gate."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID = 32


def _bench(*args):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--grid", str(GRID), "--steps", "3",
           "--warmup", "2", *args]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-3000:]
    return json.loads(lines[0])


def test_plain_run_prints_the_headline_and_dumps_the_last_cycle(gpu_lib, oracle, tmp_path):
    from hypre_amd import binding as B, ij
    r = _bench("--dump-outputs", str(tmp_path))
    assert r["unit"] == "DOF/s" and r["higher_is_better"] is True and r["dtype"] == "f64" and r["steps"] == 3
    assert r["metric"].startswith("BoomerAMG V-cycle DOF/s (%d^3 7-pt Laplacian per GPU" % GRID)
    assert r["ms_per_step"] > 0
    assert abs(r["value"] - GRID ** 3 / (r["ms_per_step"] * 1e-3)) <= 1e-9 * r["value"]
    for key in ("roofline", "pcg", "cpu_baseline", "vcycle", "spmv_fine_as_launched"):
        assert key not in r
    u = np.load(tmp_path / "u.npy")
    assert u.dtype == np.float64 and u.shape == (GRID ** 3,)

    # the same hierarchy here, its cycle from zero on the oracle
    opt = ij.IJOptions(n=(GRID,) * 3, P=(1, 1, 1), coarsen_type=8, interp_type=6, P_max_elmts=4, relax_type=18, num_sweeps=1)
    A = ij.build_matrix(opt)
    s = ij.create_amg(opt, memory_location=B.HYPRE_MEMORY_DEVICE)
    gpu_lib.hypre_ParCSRMatrixMigrate(A, B.HYPRE_MEMORY_DEVICE)
    gpu_lib.HYPRE_BoomerAMGSetup(s, A, None, None)
    B.check()
    amg = oracle.amg_from_solvers([s])
    ur = np.zeros(GRID ** 3)
    amg.cycle(np.ones(GRID ** 3), ur, u_all_zeros=True)
    gpu_lib.HYPRE_BoomerAMGDestroy(s)
    gpu_lib.hypre_ParCSRMatrixDestroy(A)
    B.check()
    assert np.max(np.abs(u - ur)) <= 1e-11 * np.max(np.abs(ur))


def test_full_run_adds_the_figures_and_passes_the_parity_gate():
    r = _bench("--full", "--cpu-cycles", "1")
    for key in ("roofline", "pcg", "cpu_baseline", "vcycle", "spmv_fine_as_launched", "ms_per_step_codes_off"):
        assert key in r
    assert "exchanges_by_level" in r["config"] and "parity_failed" not in r
    assert r["cpu_baseline"]["gpu_vs_cpu_cycle_rel_max_diff"] <= 1e-11
    assert r["pcg"]["final_rel_resid"] <= 1e-8
