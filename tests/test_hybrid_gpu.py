"""The hybrid solver (HYPRE_ParCSRHybrid*; the reference's `ij -solver 20`), the convergence-factor exit of PCG and GMRES it
is written against, and the fused step of diagonally scaled CG, on the device.

1. hypre_amd_ParVectorDiagScaledCGStep fused against the three launches it stands for, bit for bit: x, r, s and both sums;
   also over two ranks;
2. DS-PCG solves with the fused step on and off: the same bits; which path ran; who takes the plain path;
3. the convergence-factor exit of PCG and GMRES against float64 numpy restatements of DS-PCG and DS-GMRES with the rule of
   krylov/pcg.c:893-950 and gmres.c:597-615; with cf_tol = 0 the solves the parent commit computed
   (tests/golden/ij_saved_hybrid.json, "parent");
4. the hybrid solve is the chain it claims to be, for each solver type; it never switches with cf_tol = 0; a second Solve
   for either meaning of the setup type;
5. the reference's four hybrid job lines (tests/golden/ij_saved_hybrid.json, "jobs") on two ranks."""
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
GOLD = json.load(open(os.path.join(HERE, "golden", "ij_saved_hybrid.json")))


def _worker(args, nranks, timeout=600):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    from conftest import free_port
    worker = [os.path.join(HERE, "hybrid_worker.py")] + list(args)
    if nranks == 1:
        cmd = [sys.executable] + worker
    else:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nranks),
               "--master-addr", "127.0.0.1", "--master-port", str(free_port())] + worker
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stderr[-2000:]
    return p.stdout


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _same_double(a, b):
    return np.float64(a).tobytes() == np.float64(b).tobytes()


def _ds(lib):
    return C.cast(lib.HYPRE_ParCSRDiagScale, C.c_void_p), C.cast(lib.HYPRE_ParCSRDiagScaleSetup, C.c_void_p), None


def _operator(lib, **kw):
    """(options, device matrix, scipy copy)"""
    from hypre_amd import binding as B, ij
    opt = ij.IJOptions(**kw)
    A = ij.build_matrix(opt)
    M = B.csr_to_scipy(A.contents.diag)
    lib.hypre_ParCSRMatrixMigrate(A, B.HYPRE_MEMORY_DEVICE)
    B.check()
    return opt, A, M


# ---------------------------------------------------------------------------------------------------------------------
# 1. the kernel
# ---------------------------------------------------------------------------------------------------------------------
def _lengths(lib):
    """1, 255, 256: below one workgroup's 512 elements, tail only / odd / even; 257; 65 537: 129 workgroups and a tail; the
    first length past one trip of the kernel's grid, from the launch shape the library reports"""
    one_pass = int(lib.hypre_amd_DotGridPassElements())
    assert one_pass == 1024 * 256 * 2
    return (1, 255, 256, 257, 65537, one_pass + 1)


@pytest.mark.parametrize("which", range(6))
@pytest.mark.parametrize("alpha", [0.7320508075688772, -3.0e-5])
def test_the_fused_step_has_the_bits_of_the_three_launches(gpu_lib, which, alpha):
    import scipy.sparse as sp
    from hypre_amd import binding as B
    from hybrid_worker import awkward_diagonal
    from util import parcsr
    lib = gpu_lib
    n = _lengths(lib)[which]
    rng = np.random.default_rng(20 + n)
    diag = awkward_diagonal(rng, n)
    assert abs(diag).min() < 1e-100 and (n == 1 or diag.min() < 0 < diag.max())
    A = parcsr(lib, B, sp.diags(diag).tocsr(), B.HYPRE_MEMORY_DEVICE)
    h = {k: rng.standard_normal(n) for k in "psxr"}
    out = {}
    for fused in (1, 0):
        v = {k: B.parvec_from_numpy(h[k]) for k in "psxr"}
        rr, rs = C.c_double(np.nan), C.c_double(np.nan)
        assert lib.hypre_amd_ParVectorDiagScaledCGStep(fused, alpha, A, v["p"], v["s"], v["x"], v["r"], C.byref(rr), C.byref(rs)) == 0
        B.check()
        out[fused] = dict(rr=rr.value, rs=rs.value, **{k: B.parvec_to_numpy(v[k]) for k in "psxr"})
        for w in v.values():
            lib.hypre_ParVectorDestroy(w)
    on, off = out[1], out[0]
    print("n", n, "alpha", alpha, "<r, r>", repr(on["rr"]), repr(off["rr"]), "<r, s>", repr(on["rs"]), repr(off["rs"]))
    for k in "xrs":
        assert np.array_equal(_bits(on[k]), _bits(off[k])), (k, int(np.flatnonzero(_bits(on[k]) != _bits(off[k]))[0]))
    assert np.array_equal(_bits(on["p"]), _bits(h["p"]))
    assert _same_double(on["rr"], off["rr"]) and _same_double(on["rs"], off["rs"])
    # and the three launches do what they say: r - alpha s within one rounding of each term, s the correctly rounded quotient
    assert np.all(np.abs(on["r"] - (h["r"] - alpha * h["s"])) <= 2.0 ** -52 * (np.abs(h["r"]) + abs(alpha) * np.abs(h["s"])))
    assert np.array_equal(on["s"], on["r"] / diag) and np.all(np.isfinite(on["s"]))
    assert abs(on["rr"] - float(np.dot(on["r"], on["r"]))) <= n * np.finfo(np.float64).eps * float(np.dot(on["r"], on["r"]))
    lib.hypre_ParCSRMatrixDestroy(A)


def test_the_fused_step_over_two_ranks():
    """12 x 12 x 9 rows split 5 : 4 in z (720 and 576 rows): the two sums, reduced together, and the vectors of both ranks"""
    parts = json.loads(re.search(r"^RESULT (.*)$", _worker(["step", "9"], 2), re.M).group(1))
    print(parts)
    assert len(parts) == 2 and sum(p["rows"] for p in parts) == 12 * 12 * 9
    for p in parts:
        assert p["rc"] == [0, 0] and p["same"] and p["finite"] and p["fused"] == p["plain"]
    assert parts[0]["fused"] == parts[1]["fused"]


# ---------------------------------------------------------------------------------------------------------------------
# solver helpers
# ---------------------------------------------------------------------------------------------------------------------
def _pcg(lib, A, db, dx, tol=1e-8, max_iter=1000, fused=None, precond="ds", cf_tol=None, two_norm=None, solve=True):
    from hypre_amd import binding as B
    g = C.c_void_p()
    lib.HYPRE_ParCSRPCGCreate(0, C.byref(g))
    lib.HYPRE_PCGSetTol(g, tol)
    lib.HYPRE_PCGSetMaxIter(g, max_iter)
    if two_norm is not None:
        lib.HYPRE_PCGSetTwoNorm(g, two_norm)
    if precond is not None:
        lib.HYPRE_PCGSetPrecond(g, *(_ds(lib) if precond == "ds" else precond))
    if fused is not None:
        assert lib.hypre_amd_PCGSetFusedDiagScale(g, fused) == 0
    if cf_tol is not None:
        assert lib.HYPRE_PCGSetConvergenceFactorTol(g, cf_tol) == 0
    lib.HYPRE_ParCSRPCGSetup(g, A, db, dx)
    used = C.c_int(-1)
    lib.hypre_amd_PCGGetFusedDiagScaleUsed(g, C.byref(used))
    out = dict(used=used.value)
    if solve:
        out["rc"] = lib.HYPRE_ParCSRPCGSolve(g, A, db, dx)
        out["err"] = lib.HYPRE_GetError()
        lib.HYPRE_ClearError(256)
        B.check()
        its, rel, conv = C.c_int(-1), C.c_double(-1.0), C.c_int(-1)
        lib.HYPRE_PCGGetNumIterations(g, C.byref(its))
        lib.HYPRE_PCGGetFinalRelativeResidualNorm(g, C.byref(rel))
        lib.HYPRE_PCGGetConverged(g, C.byref(conv))
        out.update(its=its.value, rel=rel.value, conv=conv.value)
    lib.HYPRE_ParCSRPCGDestroy(g)
    return out


def _gmres(lib, A, db, dx, tol=1e-8, max_iter=1000, precond="ds", cf_tol=None, k_dim=5):
    from hypre_amd import binding as B
    g = C.c_void_p()
    lib.HYPRE_ParCSRGMRESCreate(0, C.byref(g))
    lib.HYPRE_GMRESSetKDim(g, k_dim)
    lib.HYPRE_GMRESSetTol(g, tol)
    lib.HYPRE_GMRESSetMaxIter(g, max_iter)
    lib.HYPRE_GMRESSetPrecond(g, *(_ds(lib) if precond == "ds" else precond))
    if cf_tol is not None:
        assert lib.HYPRE_GMRESSetConvergenceFactorTol(g, cf_tol) == 0
    lib.HYPRE_ParCSRGMRESSetup(g, A, db, dx)
    rc = lib.HYPRE_ParCSRGMRESSolve(g, A, db, dx)
    err = lib.HYPRE_GetError()
    lib.HYPRE_ClearError(256)
    B.check()
    its, rel, conv = C.c_int(-1), C.c_double(-1.0), C.c_int(-1)
    lib.HYPRE_GMRESGetNumIterations(g, C.byref(its))
    lib.HYPRE_GMRESGetFinalRelativeResidualNorm(g, C.byref(rel))
    lib.HYPRE_GMRESGetConverged(g, C.byref(conv))
    lib.HYPRE_ParCSRGMRESDestroy(g)
    return dict(rc=rc, err=err, its=its.value, rel=rel.value, conv=conv.value)


def _bicgstab(lib, A, db, dx, tol=1e-8, max_iter=1000, precond="ds", cf_tol=None):
    from hypre_amd import binding as B
    g = C.c_void_p()
    lib.HYPRE_ParCSRBiCGSTABCreate(0, C.byref(g))
    lib.HYPRE_BiCGSTABSetTol(g, tol)
    lib.HYPRE_BiCGSTABSetMaxIter(g, max_iter)
    lib.HYPRE_BiCGSTABSetPrecond(g, *(_ds(lib) if precond == "ds" else precond))
    if cf_tol is not None:
        lib.HYPRE_BiCGSTABSetConvergenceFactorTol(g, cf_tol)
    lib.HYPRE_BiCGSTABSetup(g, A, db, dx)
    rc = lib.HYPRE_BiCGSTABSolve(g, A, db, dx)
    err = lib.HYPRE_GetError()
    lib.HYPRE_ClearError(256)
    B.check()
    its, rel, conv = C.c_int(-1), C.c_double(-1.0), C.c_int(-1)
    lib.HYPRE_BiCGSTABGetNumIterations(g, C.byref(its))
    lib.HYPRE_BiCGSTABGetFinalRelativeResidualNorm(g, C.byref(rel))
    lib.HYPRE_BiCGSTABGetConverged(g, C.byref(conv))
    lib.HYPRE_ParCSRBiCGSTABDestroy(g)
    return dict(rc=rc, err=err, its=its.value, rel=rel.value, conv=conv.value)


KRYLOV = {1: _pcg, 2: _gmres, 3: _bicgstab}


def _hybrid_amg(lib):
    """a BoomerAMG of the hybrid solver's default options (amg_hybrid.c:131-156, 2110-2155), one cycle per application"""
    from hypre_amd import binding as B
    s = C.c_void_p()
    lib.HYPRE_BoomerAMGCreate(C.byref(s))
    lib.hypre_amd_BoomerAMGSetMemoryLocation(s, B.HYPRE_MEMORY_DEVICE)
    lib.HYPRE_BoomerAMGSetMaxIter(s, 1)
    lib.HYPRE_BoomerAMGSetTol(s, 0.0)
    for name, v in (("CoarsenType", 10), ("InterpType", 6), ("MeasureType", 0), ("PMaxElmts", 4), ("CycleType", 1), ("MaxLevels", 25),
                    ("MaxCoarseSize", 9), ("MinCoarseSize", 1), ("RelaxOrder", 0), ("KeepTranspose", 0)):
        getattr(lib, "HYPRE_BoomerAMGSet" + name)(s, v)
    lib.HYPRE_BoomerAMGSetStrongThreshold(s, 0.25)
    lib.HYPRE_BoomerAMGSetTruncFactor(s, 0.0)
    lib.HYPRE_BoomerAMGSetMaxRowSum(s, 0.9)
    for k, t in ((1, 13), (2, 14), (3, 9)):
        lib.HYPRE_BoomerAMGSetCycleRelaxType(s, t, k)
    B.check()
    return s


def _hybrid(lib, solver_type, cf_tol, setup_type=None, tol=1e-8):
    h = C.c_void_p()
    assert lib.HYPRE_ParCSRHybridCreate(C.byref(h)) == 0
    lib.HYPRE_ParCSRHybridSetTol(h, tol)
    lib.HYPRE_ParCSRHybridSetConvergenceTol(h, cf_tol)
    lib.HYPRE_ParCSRHybridSetSolverType(h, solver_type)
    lib.HYPRE_ParCSRHybridSetLogging(h, 1)
    if setup_type is not None:
        lib.HYPRE_ParCSRHybridSetSetupType(h, setup_type)
    return h


def _hybrid_solve(lib, h, A, db, dx):
    from hypre_amd import binding as B
    assert lib.HYPRE_ParCSRHybridSetup(h, A, db, dx) == 0
    rc = lib.HYPRE_ParCSRHybridSolve(h, A, db, dx)
    err = lib.HYPRE_GetError()
    lib.HYPRE_ClearError(256)
    B.check()
    its, pcg, dscg, rel, amg = C.c_int(-1), C.c_int(-1), C.c_int(-1), C.c_double(-1.0), C.c_void_p()
    lib.HYPRE_ParCSRHybridGetNumIterations(h, C.byref(its))
    lib.HYPRE_ParCSRHybridGetPCGNumIterations(h, C.byref(pcg))
    lib.HYPRE_ParCSRHybridGetDSCGNumIterations(h, C.byref(dscg))
    lib.HYPRE_ParCSRHybridGetFinalRelativeResidualNorm(h, C.byref(rel))
    lib.hypre_amd_ParCSRHybridGetPrecond(h, C.byref(amg))
    return dict(rc=rc, err=err, its=its.value, pcg=pcg.value, dscg=dscg.value, rel=rel.value, amg=amg.value)


@pytest.fixture(scope="module")
def lap12(gpu_lib):
    """7-point 12^3 with the driver's -rhsrand right-hand side: (A on the device, scipy copy, b); nobody changes them"""
    from hypre_amd import ij
    opt, A, M = _operator(gpu_lib, n=(12, 12, 12), rhs="rand")
    b, _ = ij.build_rhs_host(opt, A)
    yield A, M, b
    gpu_lib.hypre_ParCSRMatrixDestroy(A)


# ---------------------------------------------------------------------------------------------------------------------
# 2. fused against plain solves
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["7pt-12", "27pt-9"])
def test_ds_pcg_fused_and_plain_give_the_same_bits(gpu_lib, case):
    from hypre_amd import binding as B, ij
    lib = gpu_lib
    kw = dict(n=(12, 12, 12)) if case == "7pt-12" else dict(n=(9, 9, 9), problem="27pt")
    opt, A, M = _operator(lib, rhs="rand", **kw)
    b, _ = ij.build_rhs_host(opt, A)
    runs = {}
    for fused in (1, 0):
        db, dx = B.parvec_from_numpy(b), B.parvec_from_numpy(np.zeros_like(b))
        runs[fused] = _pcg(lib, A, db, dx, fused=fused)
        runs[fused]["x"] = B.parvec_to_numpy(dx)
        lib.hypre_ParVectorDestroy(db); lib.hypre_ParVectorDestroy(dx)
    on, off = runs[1], runs[0]
    print(case, "fused", on["its"], repr(on["rel"]), "plain", off["its"], repr(off["rel"]))
    assert on["used"] == 1 and off["used"] == 0
    assert on["rc"] == 0 and on["err"] == 0 and on["conv"] == 1 and off["conv"] == 1 and on["its"] >= 10
    assert on["its"] == off["its"] and _same_double(on["rel"], off["rel"])
    assert np.array_equal(_bits(on["x"]), _bits(off["x"]))
    # r = b - A x of the two is then the same too; it meets the tolerance (energy norm of the diagonal scaling)
    r = b - M @ on["x"]
    assert np.sqrt(np.dot(r, r / M.diagonal()) / np.dot(b, b / M.diagonal())) <= 1.01e-8
    lib.hypre_ParCSRMatrixDestroy(A)


def test_who_takes_the_plain_path(gpu_lib, lap12):
    """a multivector, another preconditioner and no preconditioner, with the switch on; a last row without entries: Setup
    alone is looked at (the plain scaling is not run on such a matrix)"""
    import scipy.sparse as sp
    from hypre_amd import binding as B
    from util import parcsr
    lib = gpu_lib
    A, M, b = lap12
    n = len(b)
    db2, dx2 = B.parmultivec_from_numpy(np.column_stack([b, b])), B.parmultivec_from_numpy(np.zeros((n, 2)))
    r = _pcg(lib, A, db2, dx2, fused=1)
    assert r["used"] == 0 and r["conv"] == 1
    db, dx = B.parvec_from_numpy(b), B.parvec_from_numpy(np.zeros(n))
    one = _pcg(lib, A, db, dx, fused=1)
    assert one["used"] == 1 and one["its"] == r["its"]
    amg = _hybrid_amg(lib)
    dx3 = B.parvec_from_numpy(np.zeros(n))
    r = _pcg(lib, A, db, dx3, fused=1, precond=(C.cast(lib.HYPRE_BoomerAMGSolve, C.c_void_p), C.cast(lib.HYPRE_BoomerAMGSetup, C.c_void_p), amg))
    assert r["used"] == 0 and r["conv"] == 1 and r["its"] < one["its"]
    dx4 = B.parvec_from_numpy(np.zeros(n))
    assert _pcg(lib, A, db, dx4, fused=1, precond=None)["used"] == 0
    lib.HYPRE_BoomerAMGDestroy(amg)
    # the last row empty
    T = sp.diags([np.full(9, 2.0), np.full(8, -1.0)], [0, 1]).tolil()
    T[8, :] = 0.0
    T = T.tocsr(); T.eliminate_zeros()
    assert T.indptr[-1] == T.indptr[-2]
    E = parcsr(lib, B, T, B.HYPRE_MEMORY_DEVICE)
    de, dxe = B.parvec_from_numpy(np.ones(9)), B.parvec_from_numpy(np.zeros(9))
    assert _pcg(lib, E, de, dxe, fused=1, solve=False)["used"] == 0
    for v in (db2, dx2, db, dx, dx3, dx4, de, dxe):
        lib.hypre_ParVectorDestroy(v)
    lib.hypre_ParCSRMatrixDestroy(E)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the convergence-factor exit
# ---------------------------------------------------------------------------------------------------------------------
def _rule(cf1, cf0, cf_tol):
    """pcg.c:941-950: weight * cf - cf_tol; the solve leaves when it is positive"""
    weight = 1.0 - abs(cf1 - cf0) / max(cf1, cf0)
    return weight * cf1 - cf_tol


def _numpy_ds_pcg(M, b, tol, cf_tol, max_iter=1000):
    """DS-PCG of krylov/pcg.c from x = 0 in the energy norm of the preconditioner (two_norm = 0) with the exit of :893-950.
    Returns (iterations, converged, the margins weight * cf - cf_tol of every iteration that looked at the rule)."""
    dinv = 1.0 / M.diagonal()
    x = np.zeros(len(b))
    bi_prod = np.dot(dinv * b, b)
    eps = tol * tol
    r = b - M @ x
    p = dinv * r
    gamma = np.dot(r, p)
    i_prod_0, cf0, cf1, margins = gamma, 0.0, 0.0, []
    for i in range(1, max_iter + 1):
        s = M @ p
        alpha = gamma / np.dot(s, p)
        gamma_old = gamma
        x += alpha * p
        r -= alpha * s
        s = dinv * r
        gamma = np.dot(r, s)
        if gamma / bi_prod < eps:
            return i, 1, margins
        cf0, cf1 = cf1, (gamma / i_prod_0) ** (1.0 / (2.0 * i))
        margins.append(_rule(cf1, cf0, cf_tol))
        if margins[-1] > 0:
            return i, 0, margins
        p = s + (gamma / gamma_old) * p
    return max_iter, 0, margins


def _numpy_ds_gmres(M, b, tol, cf_tol, k_dim=5, max_iter=1000):
    """right-preconditioned GMRES(k_dim) of krylov/gmres.c from x = 0 behind the diagonal scaling, modified Gram-Schmidt and
    Givens rotations, with the exit of :597-615 on the norm of the recurrence.  Same return as above."""
    dinv = 1.0 / M.diagonal()
    n = len(b)
    x = np.zeros(n)
    r = b - M @ x
    b_norm = np.linalg.norm(b)
    r_norm = r_norm_0 = np.linalg.norm(r)
    eps, it, cf0, cf1, margins = tol * b_norm, 0, 0.0, 0.0, []
    while it < max_iter:
        p = [r / r_norm]
        H = np.zeros((k_dim + 1, k_dim))
        c, s, rs = np.zeros(k_dim), np.zeros(k_dim), np.zeros(k_dim + 1)
        rs[0] = r_norm
        i = 0
        while i < k_dim and it < max_iter:
            i += 1
            it += 1
            w = M @ (dinv * p[i - 1])
            for j in range(i):
                H[j, i - 1] = np.dot(p[j], w)
                w = w - H[j, i - 1] * p[j]
            t = np.linalg.norm(w)
            H[i, i - 1] = t
            p.append(w / t)
            for j in range(1, i):
                t0 = H[j - 1, i - 1]
                H[j - 1, i - 1] = s[j - 1] * H[j, i - 1] + c[j - 1] * t0
                H[j, i - 1] = -s[j - 1] * t0 + c[j - 1] * H[j, i - 1]
            g = np.hypot(H[i, i - 1], H[i - 1, i - 1])
            c[i - 1], s[i - 1] = H[i - 1, i - 1] / g, H[i, i - 1] / g
            rs[i] = -s[i - 1] * rs[i - 1]
            rs[i - 1] = c[i - 1] * rs[i - 1]
            H[i - 1, i - 1] = s[i - 1] * H[i, i - 1] + c[i - 1] * H[i - 1, i - 1]
            r_norm = abs(rs[i])
            cf0, cf1 = cf1, (r_norm / r_norm_0) ** (1.0 / (2.0 * it))
            margins.append(_rule(cf1, cf0, cf_tol))
            if margins[-1] > 0:
                return it, 0, margins
            if r_norm <= eps:
                break
        y = np.linalg.solve(np.triu(H[:i, :i]), rs[:i])
        x += dinv * (np.column_stack(p[:i]) @ y)
        r = b - M @ x
        r_norm = np.linalg.norm(r)
        if r_norm <= eps:
            return it, 1, margins
    return it, 0, margins


@pytest.mark.parametrize("solver,cf_tol", [("pcg", 0.5), ("pcg", 0.6), ("gmres", 0.5), ("gmres", 0.8)])
def test_the_convergence_factor_exit_against_numpy(gpu_lib, lap12, solver, cf_tol):
    """The iteration at which the library's solve gives up is the one at which the numpy restatement does.  The inputs are
    such that weight * cf stays 1e-6 away from cf_tol at the deciding iteration and at every one before it, so that no order of
    summation can decide the outcome; the test asserts that of its inputs."""
    from hypre_amd import binding as B
    lib = gpu_lib
    A, M, b = lap12
    numpy_solve, lib_solve = (_numpy_ds_pcg, _pcg) if solver == "pcg" else (_numpy_ds_gmres, _gmres)
    its, conv, margins = numpy_solve(M, b, 1e-8, cf_tol)
    print(solver, "cf_tol", cf_tol, "numpy leaves at", its, "margins", margins)
    assert conv == 0 and its >= 2 and margins[-1] > 0
    assert all(abs(m) > 1e-6 for m in margins)
    db, dx = B.parvec_from_numpy(b), B.parvec_from_numpy(np.zeros_like(b))
    r = lib_solve(lib, A, db, dx, cf_tol=cf_tol)
    print("library", r)
    assert r["rc"] == 0 and r["err"] == 0 and r["conv"] == 0 and r["its"] == its and r["rel"] > 1e-8
    # without the exit the same solve goes on to its tolerance and says so
    dx2 = B.parvec_from_numpy(np.zeros_like(b))
    full = lib_solve(lib, A, db, dx2)
    assert full["conv"] == 1 and full["its"] > its and full["rel"] <= 1e-8
    for v in (db, dx, dx2):
        lib.hypre_ParVectorDestroy(v)


@pytest.mark.parametrize("name", ["ds-pcg", "ds-pcg-two-norm", "amg-pcg", "ds-gmres", "amg-gmres"])
def test_with_cf_tol_zero_the_solves_are_the_parent_commits(gpu_lib, lap12, name):
    """iteration count and x, bit for bit, of solves as the existing tests make them, recorded from a build of the parent
    commit; cf_tol is set to 0 explicitly"""
    from hypre_amd import binding as B
    lib = gpu_lib
    A, M, b = lap12
    want = GOLD["parent"][name]
    db, dx = B.parvec_from_numpy(b), B.parvec_from_numpy(np.zeros_like(b))
    amg = _hybrid_amg(lib) if name.startswith("amg") else None
    pc = "ds" if amg is None else (C.cast(lib.HYPRE_BoomerAMGSolve, C.c_void_p), C.cast(lib.HYPRE_BoomerAMGSetup, C.c_void_p), amg)
    if "pcg" in name:
        r = _pcg(lib, A, db, dx, precond=pc, cf_tol=0.0, two_norm=1 if name.endswith("two-norm") else None)
    else:
        r = _gmres(lib, A, db, dx, precond=pc, cf_tol=0.0)
    x = B.parvec_to_numpy(dx)
    print(name, r["its"], repr(r["rel"]), "parent", want["iterations"])
    assert r["conv"] == 1 and r["its"] == want["iterations"]
    assert x.tobytes().hex() == want["x"]
    if amg is not None:
        lib.HYPRE_BoomerAMGDestroy(amg)
    for v in (db, dx):
        lib.hypre_ParVectorDestroy(v)


# ---------------------------------------------------------------------------------------------------------------------
# 4. the hybrid solver
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver_type", [1, 2, 3])
def test_the_hybrid_solve_is_the_chain_it_claims_to_be(gpu_lib, lap12, solver_type):
    """cf_tol 0.5: the diagonally scaled solver with cf_tol by hand, then the same solver behind a BoomerAMG of the same
    options from the x it left; x, both iteration counts and the final norm of the hybrid solve are theirs, bit for bit"""
    from hypre_amd import binding as B
    lib = gpu_lib
    A, M, b = lap12
    solve = KRYLOV[solver_type]
    db, dx = B.parvec_from_numpy(b), B.parvec_from_numpy(np.zeros_like(b))
    first = solve(lib, A, db, dx, cf_tol=0.5)
    assert first["conv"] == 0 and first["err"] == 0 and first["its"] >= 2
    amg = _hybrid_amg(lib)
    second = solve(lib, A, db, dx, max_iter=200, cf_tol=0.0,
                   precond=(C.cast(lib.HYPRE_BoomerAMGSolve, C.c_void_p), C.cast(lib.HYPRE_BoomerAMGSetup, C.c_void_p), amg))
    assert second["conv"] == 1 and second["its"] >= 2
    x_chain = B.parvec_to_numpy(dx)
    h = _hybrid(lib, solver_type, 0.5)
    dxh = B.parvec_from_numpy(np.zeros_like(b))
    r = _hybrid_solve(lib, h, A, db, dxh)
    xh = B.parvec_to_numpy(dxh)
    print("type", solver_type, "by hand", first["its"], second["its"], repr(second["rel"]), "hybrid", r)
    assert r["rc"] == 0 and r["err"] == 0 and r["amg"]
    assert (r["dscg"], r["pcg"], r["its"]) == (first["its"], second["its"], first["its"] + second["its"])
    assert _same_double(r["rel"], second["rel"]) and np.array_equal(_bits(xh), _bits(x_chain))
    assert np.linalg.norm(b - M @ xh) <= 1e-6 * np.linalg.norm(b)
    lib.HYPRE_ParCSRHybridDestroy(h)
    lib.HYPRE_BoomerAMGDestroy(amg)
    for v in (db, dx, dxh):
        lib.hypre_ParVectorDestroy(v)


@pytest.mark.parametrize("solver_type", [1, 2, 3])
def test_a_hybrid_solve_that_never_switches(gpu_lib, lap12, solver_type):
    """cf_tol = 0: the plain diagonally scaled solve, bit for bit; no AMG iteration, no hierarchy"""
    from hypre_amd import binding as B
    lib = gpu_lib
    A, M, b = lap12
    db, dx, dxh = B.parvec_from_numpy(b), B.parvec_from_numpy(np.zeros_like(b)), B.parvec_from_numpy(np.zeros_like(b))
    plain = KRYLOV[solver_type](lib, A, db, dx)
    h = _hybrid(lib, solver_type, 0.0)
    r = _hybrid_solve(lib, h, A, db, dxh)
    print("type", solver_type, "plain", plain, "hybrid", r)
    assert plain["conv"] == 1 and r["rc"] == 0 and r["err"] == 0
    assert (r["dscg"], r["pcg"], r["its"]) == (plain["its"], 0, plain["its"]) and r["amg"] is None
    assert _same_double(r["rel"], plain["rel"])
    assert np.array_equal(_bits(B.parvec_to_numpy(dxh)), _bits(B.parvec_to_numpy(dx)))
    lib.HYPRE_ParCSRHybridDestroy(h)
    for v in (db, dx, dxh):
        lib.hypre_ParVectorDestroy(v)


@pytest.mark.parametrize("setup_type", [1, 0])
def test_a_second_solve_on_the_same_object(gpu_lib, lap12, setup_type):
    """setup_type 1 (the default): the second Solve repeats the first, both phases and a new hierarchy.  setup_type 0: the
    hierarchy of the first Solve is kept and the second starts behind it at once: no diagonally scaled iteration, and
    what the kept hierarchy gives PCG from x = 0 by hand."""
    from hypre_amd import binding as B
    lib = gpu_lib
    A, M, b = lap12
    db, dx1, dx2 = B.parvec_from_numpy(b), B.parvec_from_numpy(np.zeros_like(b)), B.parvec_from_numpy(np.zeros_like(b))
    h = _hybrid(lib, 1, 0.5, setup_type=setup_type)
    one = _hybrid_solve(lib, h, A, db, dx1)
    two = _hybrid_solve(lib, h, A, db, dx2)
    print("setup_type", setup_type, one, two)
    assert one["dscg"] >= 2 and one["pcg"] >= 2 and one["amg"] and two["amg"] and two["err"] == 0
    if setup_type:
        assert (two["dscg"], two["pcg"]) == (one["dscg"], one["pcg"]) and _same_double(two["rel"], one["rel"])
        assert np.array_equal(_bits(B.parvec_to_numpy(dx2)), _bits(B.parvec_to_numpy(dx1)))
    else:
        assert two["amg"] == one["amg"] and two["dscg"] == 0 and two["its"] == two["pcg"]
        dx3 = B.parvec_from_numpy(np.zeros_like(b))
        byhand = _pcg(lib, A, db, dx3, max_iter=200, precond=(C.cast(lib.HYPRE_BoomerAMGSolve, C.c_void_p), None, C.c_void_p(two["amg"])))
        assert byhand["its"] == two["pcg"] and _same_double(byhand["rel"], two["rel"])
        assert np.array_equal(_bits(B.parvec_to_numpy(dx3)), _bits(B.parvec_to_numpy(dx2)))
        lib.hypre_ParVectorDestroy(dx3)
    assert np.linalg.norm(b - M @ B.parvec_to_numpy(dx2)) <= 1e-6 * np.linalg.norm(b)
    lib.HYPRE_ParCSRHybridDestroy(h)
    for v in (db, dx1, dx2):
        lib.hypre_ParVectorDestroy(v)


def test_hybrid_refuses_host_operands_and_multivectors_before_writing(gpu_lib, lap12):
    from hypre_amd import binding as B
    lib = gpu_lib
    A, M, b = lap12
    n = len(b)
    db, dx = B.parvec_from_numpy(b), B.parvec_from_numpy(np.full(n, 3.0))
    hb = lib.hypre_ParVectorCreate(0, n, None)
    lib.hypre_ParVectorInitialize_v2(hb, B.HYPRE_MEMORY_HOST)
    db2, dx2 = B.parmultivec_from_numpy(np.column_stack([b, b])), B.parmultivec_from_numpy(np.full((n, 2), 3.0))
    h = _hybrid(lib, 1, 0.5)
    for rhs, sol, word in ((hb, dx, b"not in device memory"), (db2, dx2, b"multivectors")):
        assert lib.HYPRE_ParCSRHybridSolve(h, A, rhs, sol) != 0
        assert word in lib.hypre_amd_LastErrorMessage()
        lib.HYPRE_ClearAllErrors()
        assert lib.HYPRE_ParCSRHybridSetup(h, A, rhs, sol) != 0
        lib.HYPRE_ClearAllErrors()
    assert np.array_equal(B.parvec_to_numpy(dx), np.full(n, 3.0)) and np.array_equal(B.parmultivec_to_numpy(dx2), np.full((n, 2), 3.0))
    amg = C.c_void_p()
    lib.hypre_amd_ParCSRHybridGetPrecond(h, C.byref(amg))
    assert amg.value is None
    # an option whose other branch is not built reaches the BoomerAMG setter when the hierarchy is needed, and stops there
    assert lib.HYPRE_ParCSRHybridSetAggNumLevels(h, 1) == 0
    assert lib.HYPRE_ParCSRHybridSolve(h, A, db, dx) != 0
    assert b"aggressive coarsening is not built" in lib.hypre_amd_LastErrorMessage()
    lib.HYPRE_ClearAllErrors()
    lib.HYPRE_ParCSRHybridDestroy(h)
    for v in (db, dx, hb, db2, dx2):
        lib.hypre_ParVectorDestroy(v)


# ---------------------------------------------------------------------------------------------------------------------
# 5. reference goldens
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(GOLD["jobs"]))
def test_replay_hybrid_job_on_the_device(name):
    """The three counts exactly; the final relative residual within 1.5e-6 relative (the printed precision), the bar
    test_bicgstab_gpu.py and test_lgmres_gpu.py hold the lines of `.saved` files to."""
    case = GOLD["jobs"][name]
    out = _worker(["job", name], case["np"])
    got = {k: re.search(r"^%s = (\S+)$" % k, out, re.M) for k in ("Iterations", "PCG_Iterations", "DSCG_Iterations", "Final Relative Residual Norm")}
    assert all(got.values()), out
    exp = case["expect"]
    print(name, {k: v.group(1) for k, v in got.items()}, "expected", exp)
    assert int(got["Iterations"].group(1)) == exp["iterations"]
    assert int(got["PCG_Iterations"].group(1)) == exp["pcg_iterations"]
    assert int(got["DSCG_Iterations"].group(1)) == exp["dscg_iterations"]
    assert abs(float(got["Final Relative Residual Norm"].group(1)) - exp["rel_resid"]) <= 1.5e-6 * exp["rel_resid"]
