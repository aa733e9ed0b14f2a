"""BoomerAMG on several right-hand sides: hypre_BoomerAMGSolve with f and u of num_vectors = NV columns (stored one after
the other), cycled column by column.  Every column of an NV-column solve is, byte for byte, the single-vector solve of that column on the same
solver with the same switches; the convergence test takes its norms over all columns (par_amg_solve.c); smoothers without a
multicomponent path are refused before anything is written."""
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

PROBLEMS = {
    "7pt": dict(n=(10, 9, 8)),
    "27pt": dict(n=(8, 8, 7), problem="27pt"),
    "difconv": dict(n=(9, 9, 8), problem="difconv", c=(1.0, 1.0, 0.001), a=(0.0, 0.0, 0.0)),
}


def _setup(lib, **kw):
    from hypre_amd import binding as B, ij
    kw.setdefault("coarsen_type", 8)
    opt = ij.IJOptions(**kw)
    A = ij.build_matrix(opt)
    s = ij.create_amg(opt, memory_location=B.HYPRE_MEMORY_DEVICE)
    lib.HYPRE_BoomerAMGSetup(s, A, None, None)
    B.check()
    lib.hypre_ParCSRMatrixMigrate(A, B.HYPRE_MEMORY_DEVICE)
    return opt, A, s, A.contents.diag.contents.num_rows


def _columns(n, nv, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (n, nv))


def _solve_single(lib, s, A, f, u0, zero):
    from hypre_amd import binding as B
    df, du = B.parvec_from_numpy(f), B.parvec_from_numpy(u0)
    if zero:
        lib.hypre_ParVectorSetZeros(du)
    lib.HYPRE_BoomerAMGSolve(s, A, df, du)
    B.check()
    u = B.parvec_to_numpy(du)
    lib.hypre_ParVectorDestroy(df); lib.hypre_ParVectorDestroy(du)
    return u


def _solve_multi(lib, s, A, F, U0, zero):
    from hypre_amd import binding as B
    df, du = B.parmultivec_from_numpy(F), B.parmultivec_from_numpy(U0)
    if zero:
        lib.hypre_ParVectorSetZeros(du)
    lib.HYPRE_BoomerAMGSolve(s, A, df, du)
    B.check()
    U = B.parmultivec_to_numpy(du)
    lib.hypre_ParVectorDestroy(df); lib.hypre_ParVectorDestroy(du)
    return U


def _same_bits_per_column(lib, s, A, n, nv, k, seed):
    F, U0 = _columns(n, nv, seed), _columns(n, nv, seed + 1)
    lib.HYPRE_BoomerAMGSetTol(s, 0.0)
    lib.HYPRE_BoomerAMGSetMaxIter(s, k)
    for zero in (True, False):
        start = np.zeros_like(U0) if zero else U0
        U = _solve_multi(lib, s, A, F, start, zero)
        assert not np.array_equal(U, start)
        for v in range(nv):
            u = _solve_single(lib, s, A, F[:, v], start[:, v], zero)
            assert U[:, v].tobytes() == u.tobytes(), (v, zero, float(np.max(np.abs(U[:, v] - u))))


@pytest.mark.parametrize("problem,relax,nv", [
    ("7pt", 18, 2), ("7pt", 18, 5), ("7pt", 7, 4), ("7pt", 11, 3), ("7pt", 12, 8),
    ("27pt", 18, 4), ("27pt", 12, 5), ("difconv", 18, 3), ("difconv", 11, 8), ("difconv", 7, 2)])
def test_every_column_is_the_single_vector_solve(gpu_lib, problem, relax, nv):
    lib = gpu_lib
    opt, A, s, n = _setup(lib, relax_type=relax, **PROBLEMS[problem])
    _same_bits_per_column(lib, s, A, n, nv, 2, 11)
    lib.HYPRE_BoomerAMGDestroy(s)


@pytest.mark.parametrize("relax", [18, 12])
def test_every_column_is_the_single_vector_solve_with_every_switch(gpu_lib, relax):
    """Fused multivector passes, one-workgroup tail, cycle fusion and the coarse-tail graph each on and off."""
    lib = gpu_lib
    opt, A, s, n = _setup(lib, relax_type=relax, n=(12, 11, 10))
    try:
        for fused, tail, fusion in ((1, 1, 1), (0, 1, 1), (1, 0, 1), (1, 1, 0), (0, 0, 0)):
            lib.hypre_amd_SpmvSetFusedMultivectors(fused)
            lib.hypre_amd_SetSmallTail(tail)
            lib.hypre_amd_SetCycleFusion(fusion)
            _same_bits_per_column(lib, s, A, n, 4, 3, 21)
        lib.hypre_amd_BoomerAMGSetGraphThreshold(s, 0)       # HYPRE_AMD_CYCLE_GRAPH_ROWS=0: no recorded tail
        _same_bits_per_column(lib, s, A, n, 5, 3, 31)
        lev, nodes = C.c_int(), C.c_int()
        lib.hypre_amd_BoomerAMGGetGraphInfo(s, C.byref(lev), C.byref(nodes))
        assert lev.value == -1
    finally:
        lib.hypre_amd_SpmvSetFusedMultivectors(1)
        lib.hypre_amd_SetSmallTail(1)
        lib.hypre_amd_SetCycleFusion(1)
    lib.HYPRE_BoomerAMGDestroy(s)


@pytest.mark.parametrize("relax", [18, 7, 11, 12])
def test_one_cycle_per_column_matches_oracle(gpu_lib, oracle, relax):
    lib = gpu_lib
    opt, A, s, n = _setup(lib, relax_type=relax, n=(12, 11, 10))
    amg = oracle.amg_from_solvers([s], num_threads=opt.num_threads)
    nv = 3
    F, U0 = _columns(n, nv, 5), _columns(n, nv, 6)
    lib.HYPRE_BoomerAMGSetTol(s, 0.0)
    lib.HYPRE_BoomerAMGSetMaxIter(s, 1)
    U = _solve_multi(lib, s, A, F, U0, False)
    for v in range(nv):
        ur = U0[:, v].copy()
        amg.cycle(F[:, v].copy(), ur, u_all_zeros=False)
        assert np.max(np.abs(U[:, v] - ur)) <= 1e-11 * np.max(np.abs(ur)), v
    lib.HYPRE_BoomerAMGDestroy(s)


def test_multicolumn_residual_takes_the_fused_pass(gpu_lib):
    """The outer loop's residual of an NV = 4 solve with tol > 0 is one multivector product (the fused pass serves the
    finest operator at 64^3), not four single-column products."""
    lib = gpu_lib
    opt, A, s, n = _setup(lib, relax_type=18, n=(64, 64, 64))
    nv = 4
    F = _columns(n, nv, 3)
    lib.HYPRE_BoomerAMGSetTol(s, 1e-3)
    lib.HYPRE_BoomerAMGSetMaxIter(s, 2)
    before = lib.hypre_amd_SpmvFusedMultivectorLaunches()
    from hypre_amd import binding as B
    df, du = B.parmultivec_from_numpy(F), B.parmultivec_from_numpy(np.zeros((n, nv)))
    lib.HYPRE_BoomerAMGSolve(s, A, df, du)
    lib.HYPRE_ClearError(256)
    B.check()
    assert lib.hypre_amd_SpmvFusedMultivectorLaunches() - before >= 3      # initial residual and one per cycle
    lib.hypre_ParVectorDestroy(df); lib.hypre_ParVectorDestroy(du)
    lib.HYPRE_BoomerAMGDestroy(s)


def test_single_vector_solves_are_untouched_by_a_multicolumn_solve(gpu_lib):
    lib = gpu_lib
    opt, A, s, n = _setup(lib, relax_type=18, n=(12, 11, 10))
    f, u0 = _columns(n, 1, 7)[:, 0], _columns(n, 1, 8)[:, 0]
    lib.HYPRE_BoomerAMGSetTol(s, 0.0)
    lib.HYPRE_BoomerAMGSetMaxIter(s, 3)
    lev, nodes = C.c_int(), C.c_int()

    def state():
        lib.hypre_amd_BoomerAMGGetGraphInfo(s, C.byref(lev), C.byref(nodes))
        return lev.value, nodes.value, lib.hypre_amd_BoomerAMGGetSmallTailLevel(s)
    first = _solve_single(lib, s, A, f, u0, False)
    st = state()
    _solve_multi(lib, s, A, _columns(n, 4, 9), _columns(n, 4, 10), False)
    assert state() == st
    again = _solve_single(lib, s, A, f, u0, False)
    assert first.tobytes() == again.tobytes()
    assert state() == st
    lib.HYPRE_BoomerAMGDestroy(s)


@pytest.mark.parametrize("relax", [18, 11])
def test_one_iteration_count_and_residual_over_all_columns(gpu_lib, relax):
    lib = gpu_lib
    opt, A, s, n = _setup(lib, relax_type=relax, n=(14, 13, 12))
    f = _columns(n, 1, 12)[:, 0]
    lib.HYPRE_BoomerAMGSetTol(s, 1e-7)
    lib.HYPRE_BoomerAMGSetMaxIter(s, 100)
    its, rel = C.c_int(), C.c_double()
    out = {}
    for nv in (1, 3):
        if nv == 1:
            _solve_single(lib, s, A, f, np.zeros(n), True)
        else:
            _solve_multi(lib, s, A, np.repeat(f[:, None], nv, axis=1), np.zeros((n, nv)), True)
        lib.HYPRE_BoomerAMGGetNumIterations(s, C.byref(its))
        lib.HYPRE_BoomerAMGGetFinalRelativeResidualNorm(s, C.byref(rel))
        out[nv] = (its.value, rel.value)
    assert out[1][0] == out[3][0] and out[1][0] > 1
    assert abs(out[3][1] - out[1][1]) <= 1e-12 * out[1][1]
    lib.HYPRE_BoomerAMGDestroy(s)


REFUSED = [(dict(relax_type=t), "Hybrid GS relaxation doesn't support multicomponent vectors") for t in (3, 4, 6, 8, 13, 14, 88, 89)] + [
    (dict(relax_type=0), "Jacobi relaxation doesn't support multicomponent vectors"),
    (dict(relax_type=16), "doesn't support multicomponent vectors"),
    (dict(relax_type=15), "doesn't support multicomponent vectors"),
    (dict(relax_type=17), "doesn't support multicomponent vectors"),
    (dict(relax_type=18, relax_order=1), "C/F-ordered relaxation doesn't support multicomponent vectors"),
    (dict(relax_type=18, mixed=True), "mixed precision doesn't support multicomponent vectors"),
]


@pytest.mark.parametrize("kw,msg", REFUSED)
def test_unserved_options_are_refused_and_leave_u_alone(gpu_lib, kw, msg):
    from hypre_amd import binding as B
    lib = gpu_lib
    opt, A, s, n = _setup(lib, n=(8, 8, 8), **kw)
    if kw.get("mixed"):
        lib.hypre_amd_BoomerAMGSetMixedPrecision(s, 1)
    nv = 2
    F, U0 = _columns(n, nv, 1), _columns(n, nv, 2)
    df, du = B.parmultivec_from_numpy(F), B.parmultivec_from_numpy(U0)
    lib.HYPRE_BoomerAMGSetTol(s, 0.0)
    lib.HYPRE_BoomerAMGSetMaxIter(s, 1)
    assert lib.HYPRE_BoomerAMGSolve(s, A, df, du) != 0
    assert lib.HYPRE_GetError() != 0
    assert msg in lib.hypre_amd_LastErrorMessage().decode()
    lib.HYPRE_ClearAllErrors()
    assert B.parmultivec_to_numpy(du).tobytes() == U0.tobytes()
    lib.hypre_ParVectorDestroy(df); lib.hypre_ParVectorDestroy(du)
    lib.HYPRE_BoomerAMGDestroy(s)


def test_mismatched_column_counts_are_refused(gpu_lib):
    from hypre_amd import binding as B
    lib = gpu_lib
    opt, A, s, n = _setup(lib, relax_type=18, n=(8, 8, 8))
    U0 = _columns(n, 3, 2)
    df, du = B.parmultivec_from_numpy(_columns(n, 2, 1)), B.parmultivec_from_numpy(U0)
    assert lib.HYPRE_BoomerAMGSolve(s, A, df, du) != 0
    assert "Error: num_vectors for RHS and LHS do not match!" in lib.hypre_amd_LastErrorMessage().decode()
    lib.HYPRE_ClearAllErrors()
    assert B.parmultivec_to_numpy(du).tobytes() == U0.tobytes()
    # a single-column f against a multicolumn u as well
    d1 = B.parvec_from_numpy(_columns(n, 1, 3)[:, 0])
    assert lib.HYPRE_BoomerAMGSolve(s, A, d1, du) != 0
    lib.HYPRE_ClearAllErrors()
    assert B.parmultivec_to_numpy(du).tobytes() == U0.tobytes()
    for v in (df, du, d1):
        lib.hypre_ParVectorDestroy(v)
    lib.HYPRE_BoomerAMGDestroy(s)


def test_grid_relax_points_are_refused(gpu_lib, oracle):
    """The "old version" cycle (grid_relax_points set, par_cycle.c) has no multicomponent path."""
    from hypre_amd import binding as B
    lib = gpu_lib
    opt, A, s, n = _setup(lib, relax_type=18, n=(8, 8, 8))
    libc = C.CDLL(None)
    libc.malloc.restype = C.c_void_p
    libc.malloc.argtypes = [C.c_size_t]
    # four arrays of one sweep's points each, in malloc'd memory: the solver frees them when it is destroyed
    rows = C.cast(libc.malloc(4 * C.sizeof(C.c_void_p)), C.POINTER(C.c_void_p))
    for k in range(4):
        p = libc.malloc(4 * C.sizeof(C.c_int))
        C.cast(p, C.POINTER(C.c_int * 4)).contents[:] = [0, 0, 0, 0]
        rows[k] = p
    view = C.cast(s, C.POINTER(oracle.AmgDataView)).contents
    view.grid_relax_points = C.cast(rows, C.c_void_p).value
    U0 = _columns(n, 2, 2)
    df, du = B.parmultivec_from_numpy(_columns(n, 2, 1)), B.parmultivec_from_numpy(U0)
    assert lib.HYPRE_BoomerAMGSolve(s, A, df, du) != 0
    assert "grid_relax_points don't support multicomponent vectors" in lib.hypre_amd_LastErrorMessage().decode()
    lib.HYPRE_ClearAllErrors()
    assert B.parmultivec_to_numpy(du).tobytes() == U0.tobytes()
    lib.hypre_ParVectorDestroy(df); lib.hypre_ParVectorDestroy(du)
    lib.HYPRE_BoomerAMGDestroy(s)


def test_columns_not_stored_one_after_the_other_are_refused(gpu_lib):
    from hypre_amd import binding as B
    lib = gpu_lib
    opt, A, s, n = _setup(lib, relax_type=18, n=(8, 8, 8))
    nv = 2
    F = _columns(n, nv, 1)
    df = B.parmultivec_from_numpy(F)
    # u with its columns interleaved (multivec_storage_method 1: vecstride 1, idxstride NV)
    part = np.array([0, n], dtype=np.int64)
    du = lib.hypre_ParMultiVectorCreate(0, n, B._bp(part), nv)
    du.contents.local_vector.contents.multivec_storage_method = 1
    lib.hypre_ParVectorInitialize_v2(du, B.HYPRE_MEMORY_DEVICE)
    B.check()
    lv = du.contents.local_vector.contents
    assert lv.vecstride == 1 and lv.idxstride == nv
    U0 = np.random.default_rng(3).uniform(-1.0, 1.0, n * nv)
    lib.hypre_Memcpy(C.cast(lv.data, C.c_void_p), U0.ctypes.data_as(C.c_void_p), U0.nbytes, B.HYPRE_MEMORY_DEVICE, B.HYPRE_MEMORY_HOST)
    assert lib.HYPRE_BoomerAMGSolve(s, A, df, du) != 0
    assert "one after the other" in lib.hypre_amd_LastErrorMessage().decode()
    lib.HYPRE_ClearAllErrors()
    assert B.fetch(lv.data, n * nv, np.float64, lv.memory_location).tobytes() == U0.tobytes()
    lib.hypre_ParVectorDestroy(df); lib.hypre_ParVectorDestroy(du)
    lib.HYPRE_BoomerAMGDestroy(s)


def test_setup_refuses_mismatched_column_counts(gpu_lib):
    from hypre_amd import binding as B, ij
    lib = gpu_lib
    opt = ij.IJOptions(n=(8, 8, 8), relax_type=18, coarsen_type=8)
    A = ij.build_matrix(opt)
    n = A.contents.diag.contents.num_rows
    s = ij.create_amg(opt, memory_location=B.HYPRE_MEMORY_DEVICE)
    df, du = B.parmultivec_from_numpy(_columns(n, 2, 1)), B.parmultivec_from_numpy(_columns(n, 3, 2))
    assert lib.HYPRE_BoomerAMGSetup(s, A, df, du) != 0
    assert "Error: num_vectors for RHS and LHS do not match!" in lib.hypre_amd_LastErrorMessage().decode()
    lib.HYPRE_ClearAllErrors()
    # the same columns in both: accepted, and the solve then takes them
    du2 = B.parmultivec_from_numpy(np.zeros((n, 2)))
    lib.HYPRE_BoomerAMGSetup(s, A, df, du2)
    B.check()
    lib.hypre_ParCSRMatrixMigrate(A, B.HYPRE_MEMORY_DEVICE)
    lib.HYPRE_BoomerAMGSetTol(s, 0.0)
    lib.HYPRE_BoomerAMGSetMaxIter(s, 1)
    lib.HYPRE_BoomerAMGSolve(s, A, df, du2)
    B.check()
    assert np.all(np.abs(B.parmultivec_to_numpy(du2)) > 0)
    for v in (df, du, du2):
        lib.hypre_ParVectorDestroy(v)
    lib.HYPRE_BoomerAMGDestroy(s)


def _column_residuals(lib, A, db, dx, n, nv):
    from hypre_amd import binding as B
    dr = B.parmultivec_from_numpy(np.zeros((n, nv)))
    lib.hypre_ParCSRMatrixMatvecOutOfPlace(-1.0, A, dx, 1.0, db, dr)
    B.check()
    R, Bm = B.parmultivec_to_numpy(dr), B.parmultivec_to_numpy(db)
    lib.hypre_ParVectorDestroy(dr)
    return np.linalg.norm(R, axis=0) / np.linalg.norm(Bm, axis=0)


@pytest.mark.parametrize("krylov", ["pcg", "gmres"])
def test_amg_preconditioned_krylov_on_four_columns(gpu_lib, krylov):
    from hypre_amd import binding as B, ij
    lib = gpu_lib
    opt, A, s, n = _setup(lib, relax_type=18, n=(16, 15, 14))
    nv = 4
    F = _columns(n, nv, 41)
    db, dx = B.parmultivec_from_numpy(F), B.parmultivec_from_numpy(np.zeros((n, nv)))
    opt.tol, opt.max_iter = 1e-8, 200
    its = C.c_int()
    if krylov == "gmres":
        its.value, _ = ij.solve_gmres(opt, s, A, db, dx)
    else:
        lib.HYPRE_BoomerAMGSetTol(s, 0.0)
        lib.HYPRE_BoomerAMGSetMaxIter(s, 1)
        pcg = C.c_void_p()
        lib.HYPRE_ParCSRPCGCreate(0, C.byref(pcg))
        lib.HYPRE_PCGSetTol(pcg, opt.tol)
        lib.HYPRE_PCGSetMaxIter(pcg, opt.max_iter)
        lib.HYPRE_PCGSetTwoNorm(pcg, 1)
        lib.HYPRE_PCGSetPrecond(pcg, C.cast(lib.HYPRE_BoomerAMGSolve, C.c_void_p), None, s)
        lib.HYPRE_ParCSRPCGSetup(pcg, A, db, dx)
        lib.HYPRE_ParCSRPCGSolve(pcg, A, db, dx)
        lib.HYPRE_PCGGetNumIterations(pcg, C.byref(its))
        lib.HYPRE_ParCSRPCGDestroy(pcg)
    B.check()
    assert 1 < its.value < 60
    rel = _column_residuals(lib, A, db, dx, n, nv)
    assert np.all(rel < 1e-6), rel
    lib.hypre_ParVectorDestroy(db); lib.hypre_ParVectorDestroy(dx)
    lib.HYPRE_BoomerAMGDestroy(s)


@pytest.mark.parametrize("nc", [4, 5])
def test_driver_replays_fsai_103_on_several_columns(nc):
    """`ij -n 10 10 10 -solver 1 -rlx 7` (fsai.out.103: 22 iterations) with -nc N: identical columns print the closing
    lines of one column, as vector.saved shows for the diagonally scaled PCG."""
    gold = json.load(open(os.path.join(HERE, "golden", "ij_saved.json")))["fsai.out.103"]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "hypre_amd.ij"] + gold["cmd"].split() + ["-nc", str(nc)]
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    exp = gold["expect"]
    assert re.search(r"^Iterations = %d$" % exp["iterations"], p.stdout, re.M), p.stdout
    m = re.search(r"^Final Relative Residual Norm = (\S+)$", p.stdout, re.M)
    assert m and abs(float(m.group(1)) - exp["rel_resid"]) <= 1.5e-6 * exp["rel_resid"], p.stdout


def test_two_ranks_every_column_is_the_single_vector_solve():
    from conftest import free_port
    cases = [{"name": "rlx%d" % t, "options": {"n": [12, 11, 10], "relax_type": t, "coarsen_type": 8}} for t in (18, 11)]
    spec = {"nv": 3, "cases": cases}
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()), os.path.join(HERE, "amg_multivector_worker.py"),
           json.dumps(spec)]
    env = dict(os.environ, OMP_NUM_THREADS="1")
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env)
    res = {}
    for line in r.stdout.splitlines():
        if line.startswith("RESULT "):
            d = json.loads(line[len("RESULT "):])
            res[d["name"]] = d
    assert r.returncode == 0 and len(res) == len(cases), (r.stdout[-2000:], r.stderr[-3000:])
    for name, d in res.items():
        assert d["moved"] == 1 and d["bitwise"] == 1, (name, d)
