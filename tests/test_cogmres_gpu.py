"""COGMRES (`ij -solver 16 | 17`, HYPRE_ParCSRCOGMRES*) on the device: the reference's own job lines and the single-rank
lines recorded from its driver (tests/golden/ij_saved_cogmres.json) replayed through `python -m hypre_amd.ij`, and the
solver through the C ABI against a residual computed in numpy."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = json.load(open(os.path.join(HERE, "golden", "ij_saved_cogmres.json")))


def _replay(case, timeout=600):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    from conftest import free_port
    args = case["cmd"].split()
    if case["np"] == 1:
        cmd = [sys.executable, "-m", "hypre_amd.ij"] + args
    else:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(case["np"]),
               "--master-addr", "127.0.0.1", "--master-port", str(free_port()),
               "-m", "hypre_amd.ij"] + args
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stderr[-2000:]
    return p.stdout


@pytest.mark.parametrize("name", sorted(GOLD))
def test_replay_cogmres_job_on_the_device(name):
    """Iteration count exactly; final relative residual within 1.5e-6 relative, the bar the GMRES lines of the same
    `.saved` file are held to (the reference's own summation-order change between solvers.out.13 and .16 moves it by 1e-7)."""
    case = GOLD[name]
    out = _replay(case)
    exp = case["expect"]
    m = re.search(r"^Final COGMRES Relative Residual Norm = (\S+)$", out, re.M)
    print(name, re.findall(r"^COGMRES Iterations = \d+$", out, re.M), m and m.group(1), "expected", exp)
    assert re.search(r"^COGMRES Iterations = %d$" % exp["iterations"], out, re.M), out
    assert m and abs(float(m.group(1)) - exp["rel_resid"]) <= 1.5e-6 * exp["rel_resid"], out


def _laplacian_8(lib):
    from hypre_amd import binding as B
    A = B.laplacian(8, 8, 8)
    ii, jj, aa = B.csr_to_arrays(A.contents.diag)
    import scipy.sparse as sp
    M = sp.csr_matrix((aa, jj, ii), shape=(512, 512))
    lib.hypre_ParCSRMatrixMigrate(A, B.HYPRE_MEMORY_DEVICE)
    B.check()
    return A, M


def _create(lib, cgs, k_dim=5):
    g = C.c_void_p()
    lib.HYPRE_ParCSRCOGMRESCreate(0, C.byref(g))
    lib.HYPRE_COGMRESSetKDim(g, k_dim)
    lib.HYPRE_COGMRESSetCGS(g, cgs)
    lib.HYPRE_COGMRESSetTol(g, 1e-8)
    lib.HYPRE_COGMRESSetPrecond(g, C.cast(lib.HYPRE_ParCSRDiagScale, C.c_void_p), C.cast(lib.HYPRE_ParCSRDiagScaleSetup, C.c_void_p), None)
    return g


@pytest.mark.parametrize("cgs", [1, 2])
def test_reported_residual_is_the_true_one(gpu_lib, cgs):
    """8^3 7-point Laplacian, diagonal scaling, tol 1e-8: the norm COGMRES reports is the recomputed b - A x, so the
    same number formed in numpy from the returned x differs from it by the rounding of one 512-term dot only."""
    from hypre_amd import binding as B
    lib = gpu_lib
    A, M = _laplacian_8(lib)
    b = np.random.default_rng(7).standard_normal(512)
    db, dx = B.parvec_from_numpy(b), B.parvec_from_numpy(np.zeros(512))
    g = _create(lib, cgs)
    lib.HYPRE_ParCSRCOGMRESSetup(g, A, db, dx)
    lib.HYPRE_ParCSRCOGMRESSolve(g, A, db, dx)
    B.check()
    its, rel, conv = C.c_int(), C.c_double(), C.c_int()
    lib.HYPRE_COGMRESGetNumIterations(g, C.byref(its))
    lib.HYPRE_COGMRESGetFinalRelativeResidualNorm(g, C.byref(rel))
    lib.HYPRE_COGMRESGetConverged(g, C.byref(conv))
    x = B.parvec_to_numpy(dx)
    true = float(np.linalg.norm(b - M @ x) / np.linalg.norm(b))
    print("cgs", cgs, "iterations", its.value, "reported", rel.value, "numpy", true)
    assert abs(true - rel.value) <= 1e-9 * true
    assert true <= 1e-8
    assert conv.value == 1 and its.value > 5                  # more than one restart cycle of k_dim 5
    lib.HYPRE_ParCSRCOGMRESDestroy(g)
    lib.hypre_ParVectorDestroy(db); lib.hypre_ParVectorDestroy(dx); lib.hypre_ParCSRMatrixDestroy(A)


def test_solve_after_set_k_dim_needs_a_new_setup(gpu_lib):
    from hypre_amd import binding as B
    lib = gpu_lib
    A, _ = _laplacian_8(lib)
    db, dx = B.parvec_from_numpy(np.ones(512)), B.parvec_from_numpy(np.zeros(512))
    g = _create(lib, 1)
    lib.HYPRE_ParCSRCOGMRESSetup(g, A, db, dx)
    B.check()
    lib.HYPRE_COGMRESSetKDim(g, 7)
    assert lib.HYPRE_ParCSRCOGMRESSolve(g, A, db, dx) != 0
    assert b"HYPRE_ParCSRCOGMRESSetup" in lib.hypre_amd_LastErrorMessage()
    lib.HYPRE_ClearAllErrors()
    assert B.parvec_to_numpy(dx).tobytes() == np.zeros(512).tobytes()         # nothing was solved
    lib.HYPRE_ParCSRCOGMRESSetup(g, A, db, dx)
    assert lib.HYPRE_ParCSRCOGMRESSolve(g, A, db, dx) == 0
    B.check()
    lib.HYPRE_ParCSRCOGMRESDestroy(g)
    lib.hypre_ParVectorDestroy(db); lib.hypre_ParVectorDestroy(dx); lib.hypre_ParCSRMatrixDestroy(A)
