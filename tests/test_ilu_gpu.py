"""Block-Jacobi ILU(k) on the device: the level-scheduled triangular solves against the host solve of the same factors, bit for
bit and by kernel form; the reference's saved numbers; ILU as the preconditioner of GMRES, FlexGMRES and BiCGSTAB; repeated
solves and a second Setup.

One object serves both sides of a comparison: Setup factors on the host, a Solve on host vectors runs the host solve, and
after the matrix has moved to the device a Solve on device vectors runs the kernels on the factors of that same Setup.
The Krylov solvers of this library have no host path: their iteration counts are compared with numpy restatements of GMRES and
BiCGSTAB that run on the CPU behind the host ILU application (ilu_krylov_reference.py)."""
import ctypes as C
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

from test_ilu_host import GOLD, RESID_RTOL, _run_worker, csr_i32, difconv_block, grid_5pt, krylov_counts_on_the_cpu, new_ilu
from util import laplace_3d, parcsr

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HOST, DEVICE = 0, 1


def _stats(lib, s):
    v = [C.c_int(-1) for _ in range(6)]
    assert lib.hypre_amd_ILUGetSolveStats(s, *[C.byref(x) for x in v]) == 0
    return dict(zip(("levels_L", "levels_U", "run", "level", "nnz_L", "nnz_U"), (x.value for x in v)))


def _solve(lib, B, s, A, f, u0, location, applications):
    lib.HYPRE_ILUSetMaxIter(s, applications)
    lib.HYPRE_ILUSetTol(s, 0.0)
    fv, uv = B.parvec_from_numpy(f, location=location), B.parvec_from_numpy(u0, location=location)
    assert lib.HYPRE_ILUSolve(s, A, fv, uv) == 0
    B.check()
    u = B.parvec_to_numpy(uv)
    for v in (fv, uv):
        lib.hypre_ParVectorDestroy(v)
    return u


def _apply_chain(lib, B, s, f, u0, location, applications):
    """u_k = u_(k-1) + (L D^-1 U)^-1 (f - 0.3 u_(k-1)) through hypre_amd_ILUApplyFactors; the right-hand sides are formed
    here in numpy, so they have the same bits on both sides as long as the iterates have"""
    u = u0.copy()
    for _ in range(applications):
        fv, uv = B.parvec_from_numpy(f - 0.3 * u, location=location), B.parvec_from_numpy(u, location=location)
        assert lib.hypre_amd_ILUApplyFactors(s, fv, uv) == 0
        B.check()
        u = B.parvec_to_numpy(uv)
        for v in (fv, uv):
            lib.hypre_ParVectorDestroy(v)
    return u


def _parity(lib, M, lfil=0, reordering=1, seed=0):
    """Host and device solve of one Setup's factors, to the bit:
      * the two triangular solves (hypre_amd_ILUApplyFactors) after one and after five applications;
      * one application of HYPRE_ILUSolve from a zero iterate (the residual is then f itself on both sides);
      * five real applications of HYPRE_ILUSolve from a random iterate, one at a time: after each, the host repeats it from
        the iterate the device started from and the residual the device computed (hypre_amd_ILUGetResidual) and must land
        on the device's new iterate.
    The residual product itself is hypre_ParCSRMatrixMatvecOutOfPlace, whose sums run in an order that depends on the kernel
    form its plan chose, so it is held row by row to the rounding of a row sum in any order: (entries + 2) eps
    (|f| + |A| |u|).  Returns the statistics of the last device application."""
    from hypre_amd import binding as B
    assert (B.HYPRE_MEMORY_HOST, B.HYPRE_MEMORY_DEVICE) == (HOST, DEVICE)
    M = csr_i32(M)
    n = M.shape[0]
    rng = np.random.default_rng(100 + seed)
    f, u0 = rng.standard_normal(n), rng.standard_normal(n)
    A = parcsr(lib, B, M, HOST)
    s = new_ilu(lib, lfil=lfil, reordering=reordering)
    assert lib.HYPRE_ILUSetup(s, A, None, None) == 0
    host = {k: _apply_chain(lib, B, s, f, u0, HOST, k) for k in (1, 5)}
    host_first = _solve(lib, B, s, A, f, np.zeros(n), HOST, 1)
    assert _stats(lib, s)["run"] == 0 and _stats(lib, s)["level"] == 0
    lib.hypre_ParCSRMatrixMigrate(A, DEVICE)
    dev_first = _solve(lib, B, s, A, f, np.zeros(n), DEVICE, 1)           # uploads the factors
    st = _stats(lib, s)

    def same_bits(what, dev, ref):
        assert np.all(np.isfinite(dev))
        bad = np.flatnonzero(dev.view(np.int64) != ref.view(np.int64))
        assert bad.size == 0, (what, bad[:5], dev[bad[:5]], ref[bad[:5]])

    same_bits("first Solve", dev_first, host_first)
    for k in (1, 5):
        same_bits("%d applications" % k, _apply_chain(lib, B, s, f, u0, DEVICE, k), host[k])
    assert _stats(lib, s) == st
    absM, rowlen, eps = abs(M), np.diff(M.indptr), np.finfo(float).eps
    u = u0
    for k in range(5):
        u_new = _solve(lib, B, s, A, f, u, DEVICE, 1)
        res = C.c_void_p()
        assert lib.hypre_amd_ILUGetResidual(s, C.byref(res)) == 0 and res.value
        r_dev = B.parvec_to_numpy(C.cast(res, C.POINTER(B.ParVector)))
        r_ref = np.asarray(f.astype(np.longdouble) - M.astype(np.longdouble) @ u.astype(np.longdouble), dtype=np.float64) if n else f
        assert np.all(np.abs(r_dev - r_ref) <= (rowlen + 2) * eps * (np.abs(f) + absM @ np.abs(u))), ("residual", k)
        fv, uv = B.parvec_from_numpy(r_dev, location=HOST), B.parvec_from_numpy(u, location=HOST)
        assert lib.hypre_amd_ILUApplyFactors(s, fv, uv) == 0
        same_bits("application %d of a Solve" % (k + 1), u_new, B.parvec_to_numpy(uv))
        for v in (fv, uv):
            lib.hypre_ParVectorDestroy(v)
        u = u_new
    lib.HYPRE_ILUDestroy(s)
    lib.hypre_ParCSRMatrixDestroy(A)
    return st


def _tridiagonal(n, seed=1):
    rng = np.random.default_rng(seed)
    return sp.diags([rng.uniform(-1, -0.5, n - 1), rng.uniform(3, 4, n), rng.uniform(-1, -0.5, n - 1)], [-1, 0, 1]).tocsr()


def _layers(width, layers=3, seed=2):
    """`layers` levels of `width` rows each, by construction: row i of layer l is coupled to row i of layer l - 1 (and, so
    that rows are longer than one entry, to row i + 1 of it), symmetrically; no reordering keeps the layers as levels"""
    rng = np.random.default_rng(seed)
    n = width * layers
    M = sp.lil_matrix((n, n))
    M.setdiag(rng.uniform(5, 6, n))
    for l in range(1, layers):
        for i in range(width):
            for j in {i, (i + 1) % width}:
                M[l * width + i, (l - 1) * width + j] = rng.uniform(-1, -0.5)
                M[(l - 1) * width + j, l * width + i] = rng.uniform(-1, -0.5)
    return M.tocsr()


def test_tridiagonal_300_rows_is_one_run_per_factor(gpu_lib):
    st = _parity(gpu_lib, _tridiagonal(300), reordering=0)
    assert st == dict(levels_L=300, levels_U=300, run=2, level=0, nnz_L=299, nnz_U=299)


def test_a_chain_longer_than_one_run_is_split(gpu_lib):
    """9000 levels of one row: more than the 8192 whose offsets one run keeps in LDS, so two runs per factor"""
    st = _parity(gpu_lib, _tridiagonal(9000, seed=6), reordering=0)
    assert st == dict(levels_L=9000, levels_U=9000, run=4, level=0, nnz_L=8999, nnz_U=8999)


def test_a_rank_without_rows_on_the_device(gpu_lib):
    """two processes, all 63 rows on the first: the second launches nothing (no level, no entry) but takes part in the
    residual product's exchange and in every global sum; counts agree with the host run, the triangular solves to the bit"""
    _, parts = _run_worker(["empty", "2", "device"], 2)
    print(parts)
    assert [p["rows"] for p in parts] == [63, 0]
    for p in parts:
        assert p["device"]["rc"] == 0 and p["device"]["its"] == p["host"]["its"] == parts[0]["host"]["its"]
        assert p["device"]["close"] and p["device"]["chain_same_bits"]
    assert parts[1]["device"]["stats"] == [0, 0, 0, 0, 0, 0]
    full = parts[0]["device"]["stats"]
    assert full[0] > 1 and full[1] > 1 and (full[2], full[3]) == (2, 0) and full[4] > 0 and full[5] > 0


def test_1025_independent_rows_take_the_level_kernel(gpu_lib):
    """one level, one row wider than the run kernel's workgroup: a grid of five workgroups, the last of them with one row"""
    rng = np.random.default_rng(4)
    st = _parity(gpu_lib, sp.diags(rng.uniform(1, 2, 1025)).tocsr())
    assert st == dict(levels_L=1, levels_U=1, run=0, level=2, nnz_L=0, nnz_U=0)
    st = _parity(gpu_lib, sp.diags(rng.uniform(1, 2, 1024)).tocsr())
    assert (st["run"], st["level"]) == (2, 0)


def test_a_wide_level_followed_by_a_chain_takes_both_forms(gpu_lib):
    """1100 uncoupled rows and a tridiagonal block of 50: the first level of either factor holds 1101 rows (a grid), the
    49 levels behind it one row each (one run)"""
    rng = np.random.default_rng(5)
    M = sp.block_diag([sp.diags(rng.uniform(1, 2, 1100)), _tridiagonal(50)]).tocsr()
    st = _parity(gpu_lib, M, reordering=0)
    assert st == dict(levels_L=50, levels_U=50, run=2, level=2, nnz_L=49, nnz_U=49)


def test_17_by_13_grid(gpu_lib):
    """levels are the grid's anti-diagonals, at most 13 rows wide: 17 + 13 - 1 of them, all inside one run per factor"""
    st = _parity(gpu_lib, grid_5pt(17, 13), reordering=0)
    assert (st["levels_L"], st["levels_U"], st["run"], st["level"]) == (29, 29, 2, 0)
    _parity(gpu_lib, grid_5pt(17, 13), reordering=1)
    _parity(gpu_lib, grid_5pt(17, 13), lfil=1, reordering=1)


@pytest.mark.parametrize("width", [63, 64, 65, 255, 256, 257])
def test_level_widths_around_a_wave_and_around_four(gpu_lib, width):
    st = _parity(gpu_lib, _layers(width), reordering=0, seed=width)
    assert (st["levels_L"], st["levels_U"], st["run"], st["level"]) == (3, 3, 2, 0)


def test_empty_rows_one_row_and_no_row(gpu_lib):
    # row 2 is coupled to nothing: an empty row of L and of U in the middle; the first row of L and the last of U are empty anyway
    M = _tridiagonal(7).tolil()
    M[2, 1] = M[2, 3] = M[1, 2] = M[3, 2] = 0.0
    M = M.tocsr()
    M.eliminate_zeros()
    st = _parity(gpu_lib, M, reordering=0)
    assert (st["nnz_L"], st["nnz_U"]) == (4, 4)
    st = _parity(gpu_lib, sp.csr_matrix(np.array([[2.5]])))
    assert st == dict(levels_L=1, levels_U=1, run=2, level=0, nnz_L=0, nnz_U=0)
    # a rank without rows launches nothing
    st = _parity(gpu_lib, sp.csr_matrix((0, 0)))
    assert st == dict(levels_L=0, levels_U=0, run=0, level=0, nnz_L=0, nnz_U=0)


def test_long_rows_27_point_ilu1(gpu_lib):
    st = _parity(gpu_lib, laplace_3d(6, 6, 6, stencil=27), lfil=1)
    assert st["nnz_L"] > 13 * 216 // 2 and st["level"] == 0


@pytest.mark.parametrize("reordering", [0, 1])
def test_7_point_10_cubed_with_and_without_rcm(gpu_lib, reordering):
    st = _parity(gpu_lib, laplace_3d(10, 10, 10), reordering=reordering)
    if not reordering:
        assert (st["levels_L"], st["levels_U"]) == (28, 28)           # planes x + y + z = const


def test_nonsymmetric_convection_diffusion_block(gpu_lib):
    _parity(gpu_lib, difconv_block(7, 6, 5), lfil=0)
    _parity(gpu_lib, difconv_block(7, 6, 5), lfil=1)


# ---------------------------------------------------------------------------------------------------------------------
# the reference's saved numbers
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ilu.out.300", "ilu.out.301"])
def test_single_rank_golden_lines_on_the_device(gpu_lib, name):
    from hypre_amd import ij
    job = GOLD[name]
    out = io.StringIO()
    its, rel = ij.run(ij.parse_cli(job["cmd"].split()), out=out)
    print(name, its, repr(rel))
    assert its == job["expect"]["iterations"]
    assert abs(rel - job["expect"]["rel_resid"]) <= RESID_RTOL * job["expect"]["rel_resid"]
    assert "hypre_ILU Iterations = %d" % its in out.getvalue()


@pytest.mark.parametrize("name", ["ilu.out.303", "ilu.out.313"])
def test_two_rank_golden_lines_on_the_device(gpu_lib, name):
    """two processes share the GPU; the halo travels over gloo, staged through the host"""
    from conftest import free_port
    job = GOLD[name]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(job["np"]), "--master-addr", "127.0.0.1",
           "--master-port", str(free_port()), os.path.join(HERE, "ilu_worker.py"), "job", name, "device"]
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    its, rel = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][0][len("RESULT "):])
    print(name, its, repr(rel))
    assert its == job["expect"]["iterations"]
    assert abs(rel - job["expect"]["rel_resid"]) <= RESID_RTOL * job["expect"]["rel_resid"]
    assert ("GMRES Iterations = %d" if name == "ilu.out.313" else "hypre_ILU Iterations = %d") % its in p.stdout


# ---------------------------------------------------------------------------------------------------------------------
# as a preconditioner
# ---------------------------------------------------------------------------------------------------------------------
def _krylov(lib, B, name, A, b, ilu, k_dim=5, tol=1e-8, max_iter=500):
    """HYPRE_<name> behind ILU (Setup and Solve handed to SetPrecond) or, with ilu None, behind diagonal scaling"""
    g = C.c_void_p()
    getattr(lib, "HYPRE_ParCSR%sCreate" % name)(0, C.byref(g))
    fn = lambda stem: getattr(lib, "HYPRE_%s%s" % (name, stem))
    if name != "BiCGSTAB":
        fn("SetKDim")(g, k_dim)
    fn("SetMaxIter")(g, max_iter)
    fn("SetTol")(g, tol)
    if ilu is not None:
        fn("SetPrecond")(g, C.cast(lib.HYPRE_ILUSolve, C.c_void_p), C.cast(lib.HYPRE_ILUSetup, C.c_void_p), ilu)
    else:
        fn("SetPrecond")(g, C.cast(lib.HYPRE_ParCSRDiagScale, C.c_void_p), C.cast(lib.HYPRE_ParCSRDiagScaleSetup, C.c_void_p), None)
    x = B.parvec_from_numpy(np.zeros(len(b)))
    bv = B.parvec_from_numpy(b)
    getattr(lib, "HYPRE_ParCSR%sSetup" % name)(g, A, bv, x)
    rc = getattr(lib, "HYPRE_ParCSR%sSolve" % name)(g, A, bv, x)
    B.check()
    its, rel = C.c_int(), C.c_double()
    fn("GetNumIterations")(g, C.byref(its)); fn("GetFinalRelativeResidualNorm")(g, C.byref(rel))
    sol = B.parvec_to_numpy(x)
    getattr(lib, "HYPRE_ParCSR%sDestroy" % name)(g)
    for v in (x, bv):
        lib.hypre_ParVectorDestroy(v)
    return rc, its.value, rel.value, sol


@pytest.fixture(scope="module")
def difconv12(gpu_lib):
    from hypre_amd import binding as B, ij
    opt = ij.IJOptions(problem="difconv", n=(12, 12, 12), a=(10.0, 10.0, 10.0))
    A = ij.build_matrix(opt)
    blk = A.contents.diag.contents
    M = sp.csr_matrix((np.array(np.ctypeslib.as_array(blk.data, shape=(blk.num_nonzeros,))),
                       np.array(np.ctypeslib.as_array(blk.j, shape=(blk.num_nonzeros,))),
                       np.array(np.ctypeslib.as_array(blk.i, shape=(blk.num_rows + 1,)))), shape=(1728, 1728))
    gpu_lib.hypre_ParCSRMatrixMigrate(A, DEVICE)
    yield A, M
    gpu_lib.hypre_ParCSRMatrixDestroy(A)


@pytest.fixture(scope="module")
def cpu_counts(gpu_lib):
    return krylov_counts_on_the_cpu(gpu_lib)


@pytest.mark.parametrize("name", ["GMRES", "FlexGMRES", "BiCGSTAB"])
def test_ilu_preconditions_the_krylov_solvers(gpu_lib, difconv12, cpu_counts, name):
    """12^3 `-difconv -a 10 10 10`: behind ILU(0) every solver meets its tolerance, in fewer iterations than behind diagonal
    scaling (the reference's solvers 81 / 4, 82 / 60 and ILU-BiCGSTAB / 10)"""
    from hypre_amd import binding as B
    lib = gpu_lib
    A, M = difconv12
    b = np.ones(1728)
    ilu = new_ilu(lib, max_iter=1, tol=0.0)
    rc, its, rel, x = _krylov(lib, B, name, A, b, ilu)
    rc_ds, its_ds, rel_ds, _ = _krylov(lib, B, name, A, b, None)
    true_rel = np.linalg.norm(b - M @ x) / np.linalg.norm(b)
    print(name, "ILU", its, rel, "true", true_rel, "diagonal scaling", its_ds, rel_ds)
    assert rc == 0 and rc_ds == 0
    assert rel <= 1e-8 and true_rel <= 1e-7                           # the tolerance, and the residual of x itself near it
    assert rel_ds <= 1e-8
    assert 0 < its < its_ds
    # the counts of the algorithm itself: the numpy restatement with the library's host ILU application and with Jacobi
    assert (its, its_ds) == cpu_counts[name], (name, its, its_ds, cpu_counts[name])
    st = _stats(lib, ilu)
    assert st["run"] + st["level"] >= 2                               # the kernels ran: every application launches L and U
    # the same solve once more with the same object gives the same count
    assert _krylov(lib, B, name, A, b, ilu)[1] == its
    lib.HYPRE_ILUDestroy(ilu)


# ---------------------------------------------------------------------------------------------------------------------
# repeat and re-setup
# ---------------------------------------------------------------------------------------------------------------------
def test_a_second_solve_repeats_and_a_second_setup_leaves_nothing_behind(gpu_lib):
    from hypre_amd import binding as B
    lib = gpu_lib
    rng = np.random.default_rng(9)
    M1, M2 = csr_i32(grid_5pt(17, 13)), csr_i32(sp.block_diag([sp.diags(rng.uniform(1, 2, 1100)), _tridiagonal(50)]).tocsr())
    f1, f2 = rng.standard_normal(M1.shape[0]), rng.standard_normal(M2.shape[0])
    A1, A2 = parcsr(lib, B, M1, DEVICE), parcsr(lib, B, M2, DEVICE)
    s = new_ilu(lib, reordering=0)
    assert lib.HYPRE_ILUSetup(s, A1, None, None) == 0
    a = _solve(lib, B, s, A1, f1, np.zeros(len(f1)), DEVICE, 3)
    b = _solve(lib, B, s, A1, f1, np.zeros(len(f1)), DEVICE, 3)
    assert np.array_equal(a.view(np.int64), b.view(np.int64))
    st1 = _stats(lib, s)
    # another matrix, of another size and with other levels
    assert lib.HYPRE_ILUSetup(s, A2, None, None) == 0
    c = _solve(lib, B, s, A2, f2, np.zeros(len(f2)), DEVICE, 3)
    fresh = new_ilu(lib, reordering=0)
    assert lib.HYPRE_ILUSetup(fresh, A2, None, None) == 0
    d = _solve(lib, B, fresh, A2, f2, np.zeros(len(f2)), DEVICE, 3)
    assert np.array_equal(c.view(np.int64), d.view(np.int64))
    assert _stats(lib, s) == _stats(lib, fresh) and _stats(lib, s) != st1
    # the first matrix with the old object's size is refused now
    fv, uv = B.parvec_from_numpy(f1), B.parvec_from_numpy(np.zeros(len(f1)))
    assert lib.HYPRE_ILUSolve(s, A1, fv, uv) != 0
    lib.HYPRE_ClearAllErrors()
    for v in (fv, uv):
        lib.hypre_ParVectorDestroy(v)
    for o in (s, fresh):
        lib.HYPRE_ILUDestroy(o)
    for m in (A1, A2):
        lib.hypre_ParCSRMatrixDestroy(m)
