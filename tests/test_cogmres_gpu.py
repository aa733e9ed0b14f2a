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


_big = {}


def _past_one_grid_pass(lib, oracle):
    """104 x 101 x 101 7-point Laplacian: 1 060 904 rows, just above the 1 048 576 elements one pass of the BLAS-1 grids
    covers, so every vector kernel of a Krylov solve takes a partial second trip (a dot product a partial third).  The
    operator on the device, the oracle's copy of it and a right-hand side, made once for the two solvers below."""
    if not _big:
        from hypre_amd import binding as B, ij
        opt = ij.IJOptions(n=(104, 101, 101), solver=2, tol=0.0, k_dim=5)
        A = ij.build_matrix(opt)
        Ao = oracle.par_from_handles([A])
        lib.hypre_ParCSRMatrixMigrate(A, B.HYPRE_MEMORY_DEVICE)
        B.check()
        n = 104 * 101 * 101
        assert Ao.nrows == n > 1048576
        b = np.random.default_rng(17).uniform(-1.0, 1.0, n)
        b.setflags(write=False)
        _big.update(opt=opt, A=A, Ao=Ao, b=b, n=n)
    return _big


@pytest.mark.parametrize("solver", ["ds_pcg", "ds_cogmres"])
def test_krylov_iterations_past_one_pass_of_the_vector_grids(gpu_lib, oracle, solver):
    """Diagonally scaled PCG (pcg_update_kernel, pcg_direction_kernel, the dots) and diagonally scaled COGMRES (the batched
    dots and updates) at tol 0 for 1, 2 and 3 iterations from zero: after each count the relative residual is the
    oracle's after as many iterations of its PCG / GMRES (1e-6 relative, the bar of test_amg_gpu.py's Krylov tests; in exact
    arithmetic COGMRES is GMRES, and three steps without a restart lose no orthogonality to speak of), and the iterate after
    three is the oracle's to 1e-9 of its largest entry."""
    from hypre_amd import binding as B, ij
    lib = gpu_lib
    h = _past_one_grid_pass(lib, oracle)
    opt, A, n = h["opt"], h["A"], h["n"]
    for k in (1, 2, 3):
        opt.max_iter = k
        X = np.zeros((n, 1))
        if solver == "ds_pcg":
            oits, orel, _ = oracle.pcg_ds_multi(h["Ao"], h["b"][:, None], X, tol=0.0, max_iter=k, two_norm=opt.two_norm)
        else:
            oits, orel, _ = oracle.gmres_ds_multi(h["Ao"], h["b"][:, None], X, tol=0.0, max_iter=k, k_dim=opt.k_dim)
        db, dx = B.parvec_from_numpy(h["b"]), B.parvec_from_numpy(np.zeros(n))
        its, rel = (ij.solve_ds_pcg if solver == "ds_pcg" else ij.solve_cogmres)(opt, A, db, dx)
        lib.HYPRE_ClearError(256)                       # (tol 0: "not converged" is the expected end)
        B.check()
        x = B.parvec_to_numpy(dx)
        lib.hypre_ParVectorDestroy(db); lib.hypre_ParVectorDestroy(dx)
        xerr = float(np.max(np.abs(x - X[:, 0])) / np.max(np.abs(X[:, 0])))
        print(solver, "iterations", its, oits, "relative residual", rel, orel, "difference", abs(rel - orel) / orel, "iterate", xerr)
        assert its == oits == k
        assert 0.0 < orel < 1.0 and abs(rel - orel) <= 1e-6 * orel
    assert xerr <= 1e-9


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
