"""BiCGSTAB (HYPRE_ParCSRBiCGSTAB* / HYPRE_BiCGSTAB*; the reference's `ij -solver 9 | 10`) on the device.

1. the three vector operations it adds (hypre_amd_ParVectorInnerProdWithNorm, hypre_amd_ParVectorTwoAxpysThenInnerProds,
   hypre_amd_ParVectorAxpyScaleAxpy) against the library calls they stand for, bit for bit, outputs and sums alike; the
   sums also over two ranks;
2. a solve with the fused updates against the same solve with the reference's call sequence, bit for bit: behind the
   diagonal scaling on the 8^3 Laplacian, on vectors and on multivectors, and behind BoomerAMG on a non-symmetric
   convection-diffusion operator;
3. against a BiCGSTAB written here in numpy from the recurrence: the iteration count within one, and the residual of the
   library's x computed in numpy under the tolerance (iterates are not compared: the order of the sums differs and
   BiCGSTAB amplifies it);
4. the reference's two BiCGSTAB job lines (tests/golden/ij_saved_bicgstab.json) replayed through the driver's command line;
5. AMG-BiCGSTAB on two ranks against one rank;
6. the edges: a host operand, the zero system, the iteration limit, min_iter, a zero right-hand side with a non-zero guess,
   the convergence-factor exit, and the 0 / 0 step length of an exact half step."""
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
GOLD = json.load(open(os.path.join(HERE, "golden", "ij_saved_bicgstab.json")))

DIFCONV = dict(n=(12, 11, 10), problem="difconv", a=(10.0, 10.0, 10.0))        # `-n 12 11 10 -difconv -a 10 10 10`


def _worker(args, nranks, timeout=600):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    from conftest import free_port
    worker = [os.path.join(HERE, "bicgstab_worker.py")] + list(args)
    if nranks == 1:
        cmd = [sys.executable] + worker
    else:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nranks),
               "--master-addr", "127.0.0.1", "--master-port", str(free_port())] + worker
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stderr[-2000:]
    return p.stdout


def _closing_lines(out):
    its = re.search(r"^BiCGSTAB Iterations = (\d+)$", out, re.M)
    rel = re.search(r"^Final BiCGSTAB Relative Residual Norm = (\S+)$", out, re.M)
    assert its and rel, out
    return int(its.group(1)), float(rel.group(1))


def _result(out):
    return json.loads(re.search(r"^RESULT (.*)$", out, re.M).group(1))


# ---------------------------------------------------------------------------------------------------------------------
# 1. the kernels
# ---------------------------------------------------------------------------------------------------------------------
# the sizes of test_lgmres_gpu.py: 1, 255, 256: below one workgroup's 512 elements, tail only / odd / even; 257: one
# element past 256; 64 * 1024 + 3: 129 workgroups and a tail; 1 060 904: past one pass of the 1024-workgroup grid of a dot
LENGTHS = (1, 255, 256, 257, 64 * 1024 + 3, 1060904)
# 0 and 1 are the shortcuts of hypre_ParVectorScale (set to zero; nothing to do); with -1 equal elements cancel exactly
COEFFS = (0.0, 1.0, -1.0, 0.7320508075688772, -3.0e-5)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _same_double(a, b):
    return np.float64(a).tobytes() == np.float64(b).tobytes()


def _dot_yardstick(want, x, y, count):
    """the library's own dot product against numpy's: any order of summation of `count` products stays within
    count * u * sum |x_i y_i| of the exact sum (u = 2^-53), the library's and numpy's alike: 2 count u = count * eps"""
    x, y = np.ravel(x), np.ravel(y)
    assert abs(want - float(np.dot(x, y))) <= count * np.finfo(np.float64).eps * float(np.sum(np.abs(x * y)))


def _check_three_operations(lib, make, fetch, h, count):
    """h: the host arrays v, x, s, r, r0, q, p; x shares every seventh element with v, r with s, p with q, so that the
    updates with coefficient -1 meet exact zeros"""
    same = lambda dev, host: np.array_equal(_bits(fetch(dev)), _bits(host))
    # <x, y> and <y, y>
    r, s = make(h["r"]), make(h["s"])
    want = lib.hypre_ParVectorInnerProd(r, s), lib.hypre_ParVectorInnerProd(s, s)
    got = C.c_double(np.nan), C.c_double(np.nan)
    assert lib.hypre_amd_ParVectorInnerProdWithNorm(r, s, C.byref(got[0]), C.byref(got[1])) == 0
    print("n", count, "<r, s>", repr(got[0].value), repr(want[0]), "<s, s>", repr(got[1].value), repr(want[1]))
    assert _same_double(got[0].value, want[0]) and _same_double(got[1].value, want[1])
    assert same(r, h["r"]) and same(s, h["s"])
    _dot_yardstick(want[0], h["r"], h["s"], count)
    _dot_yardstick(want[1], h["s"], h["s"], count)
    # the same vector twice: <y, y> both times
    assert lib.hypre_amd_ParVectorInnerProdWithNorm(s, s, C.byref(got[0]), C.byref(got[1])) == 0
    assert _same_double(got[0].value, want[1]) and _same_double(got[1].value, want[1])
    for v in (r, s):
        lib.hypre_ParVectorDestroy(v)
    for k, a in enumerate(COEFFS):
        b = COEFFS[(k + 1) % len(COEFFS)]
        # x += a v, r += b s, <r, r>, <r0, r>
        v, s, r0 = make(h["v"]), make(h["s"]), make(h["r0"])
        x1, r1, x2, r2 = make(h["x"]), make(h["r"]), make(h["x"]), make(h["r"])
        lib.hypre_ParVectorAxpy(a, v, x1)
        lib.hypre_ParVectorAxpy(b, s, r1)
        want = lib.hypre_ParVectorInnerProd(r1, r1), lib.hypre_ParVectorInnerProd(r0, r1)
        got = C.c_double(np.nan), C.c_double(np.nan)
        assert lib.hypre_amd_ParVectorTwoAxpysThenInnerProds(a, v, x2, b, s, r2, r0, C.byref(got[0]), C.byref(got[1])) == 0
        gx, wx, gr, wr = fetch(x2), fetch(x1), fetch(r2), fetch(r1)
        assert np.array_equal(_bits(gx), _bits(wx)), ("x", a, int(np.flatnonzero(_bits(gx) != _bits(wx))[0]))
        assert np.array_equal(_bits(gr), _bits(wr)), ("r", b, int(np.flatnonzero(_bits(gr) != _bits(wr))[0]))
        assert _same_double(got[0].value, want[0]) and _same_double(got[1].value, want[1]), (a, b, got[0].value, want[0], got[1].value, want[1])
        assert same(v, h["v"]) and same(s, h["s"]) and same(r0, h["r0"])
        if a == -1.0:
            assert np.all(gx[::7] == 0.0)
        if b == -1.0:
            assert np.all(gr[::7] == 0.0)
        _dot_yardstick(want[0], wr, wr, count)
        _dot_yardstick(want[1], h["r0"], wr, count)
        for w in (v, s, r0, x1, r1, x2, r2):
            lib.hypre_ParVectorDestroy(w)
        # p = r + c (p + g q)
        g, c = a, COEFFS[(k + 2) % len(COEFFS)]
        q, r, p1, p2 = make(h["q"]), make(h["r"]), make(h["p"]), make(h["p"])
        lib.hypre_ParVectorAxpy(g, q, p1)
        lib.hypre_ParVectorScale(c, p1)
        lib.hypre_ParVectorAxpy(1.0, r, p1)
        assert lib.hypre_amd_ParVectorAxpyScaleAxpy(g, q, c, r, p2) == 0
        gp, wp = fetch(p2), fetch(p1)
        assert np.array_equal(_bits(gp), _bits(wp)), ("p", g, c, int(np.flatnonzero(_bits(gp) != _bits(wp))[0]))
        assert same(q, h["q"]) and same(r, h["r"])
        if g in (0.0, 1.0, -1.0):
            assert np.array_equal(gp, (h["p"] + g * h["q"]) * c + h["r"])           # g q is exact: three roundings, none fused
        for w in (q, r, p1, p2):
            lib.hypre_ParVectorDestroy(w)


def _inputs(rng, shape):
    h = {k: rng.standard_normal(shape) for k in ("v", "x", "s", "r", "r0", "q", "p")}
    for a, b in (("x", "v"), ("r", "s"), ("p", "q")):
        h[a][::7] = h[b][::7]
    return h


@pytest.mark.parametrize("n", LENGTHS)
def test_the_three_operations_have_the_bits_of_the_calls_they_replace(gpu_lib, n):
    from hypre_amd import binding as B
    _check_three_operations(gpu_lib, B.parvec_from_numpy, B.parvec_to_numpy, _inputs(np.random.default_rng(9100000 + n), n), n)
    B.check()


def test_the_three_operations_on_a_multivector_of_odd_flat_length(gpu_lib):
    """3 columns of 693 rows: 2079 elements."""
    from hypre_amd import binding as B
    _check_three_operations(gpu_lib, B.parmultivec_from_numpy, B.parmultivec_to_numpy, _inputs(np.random.default_rng(693), (693, 3)), 2079)
    B.check()


def test_the_operations_refuse_host_operands_aliases_and_other_lengths(gpu_lib):
    from hypre_amd import binding as B
    lib = gpu_lib
    x, y, z = B.parvec_from_numpy(np.ones(10)), B.parvec_from_numpy(np.full(10, 2.0)), B.parvec_from_numpy(np.full(10, 3.0))
    u, w = B.parvec_from_numpy(np.full(10, 4.0)), B.parvec_from_numpy(np.full(10, 5.0))
    short = B.parvec_from_numpy(np.zeros(9))
    h = lib.hypre_ParVectorCreate(0, 10, None)
    lib.hypre_ParVectorInitialize_v2(h, B.HYPRE_MEMORY_HOST)
    r1, r2 = C.c_double(3.0), C.c_double(4.0)
    out = C.byref(r1), C.byref(r2)
    for call in (lambda: lib.hypre_amd_ParVectorInnerProdWithNorm(h, y, *out), lambda: lib.hypre_amd_ParVectorInnerProdWithNorm(x, short, *out),
                 lambda: lib.hypre_amd_ParVectorTwoAxpysThenInnerProds(2.0, x, y, 2.0, z, u, h, *out),
                 lambda: lib.hypre_amd_ParVectorTwoAxpysThenInnerProds(2.0, x, y, 2.0, z, short, w, *out),
                 lambda: lib.hypre_amd_ParVectorTwoAxpysThenInnerProds(2.0, x, y, 2.0, z, y, w, *out),
                 lambda: lib.hypre_amd_ParVectorTwoAxpysThenInnerProds(2.0, x, y, 2.0, z, u, u, *out),
                 lambda: lib.hypre_amd_ParVectorAxpyScaleAxpy(2.0, x, 2.0, y, h), lambda: lib.hypre_amd_ParVectorAxpyScaleAxpy(2.0, x, 2.0, y, short),
                 lambda: lib.hypre_amd_ParVectorAxpyScaleAxpy(2.0, x, 2.0, y, y), lambda: lib.hypre_amd_ParVectorAxpyScaleAxpy(2.0, x, 2.0, x, x)):
        assert call() != 0
        lib.HYPRE_ClearAllErrors()
    assert r1.value == 3.0 and r2.value == 4.0
    for v, val in ((x, 1.0), (y, 2.0), (z, 3.0), (u, 4.0), (w, 5.0)):
        assert np.array_equal(B.parvec_to_numpy(v), np.full(10, val))
    for v in (x, y, z, u, w, short, h):
        lib.hypre_ParVectorDestroy(v)


def test_the_sums_over_two_ranks():
    """1 500 001 elements, three quarters on rank 0 (past one pass of the reduction grid) and the rest on rank 1: the four
    sums, reduced two at a time through dev_global_sums, have the bits of hypre_ParVectorInnerProd on the same two ranks."""
    n = 1500001
    parts = _result(_worker(["dots", str(n)], 2))
    print(parts)
    assert len(parts) == 2 and [p["local"] for p in parts] == [1125000, 375001]
    for p in parts:
        assert p["rc"] == 0 and p["updated"] and p["fused"] == p["separate"]
    assert parts[0]["fused"] == parts[1]["fused"]
    for k in range(4):
        ref = sum(p["numpy_local"][k] for p in parts)
        assert abs(parts[0]["values"][k] - ref) <= 1e-12 * n * max(1.0, abs(ref))


# ---------------------------------------------------------------------------------------------------------------------
# solver helpers
# ---------------------------------------------------------------------------------------------------------------------
def _ds(lib):
    return C.cast(lib.HYPRE_ParCSRDiagScale, C.c_void_p), C.cast(lib.HYPRE_ParCSRDiagScaleSetup, C.c_void_p), None


def _bicgstab(lib, A, db, dx, tol=1e-8, max_iter=1000, fused=None, precond="ds", min_iter=None, cf_tol=None, a_tol=None, stop_crit=None):
    """one solve through the C ABI; returns dict(rc, its, rel, conv, err, norms)"""
    from hypre_amd import binding as B
    g = C.c_void_p()
    lib.HYPRE_ParCSRBiCGSTABCreate(0, C.byref(g))
    lib.HYPRE_BiCGSTABSetTol(g, tol)
    lib.HYPRE_BiCGSTABSetMaxIter(g, max_iter)
    lib.HYPRE_BiCGSTABSetLogging(g, 1)
    if precond is not None:
        lib.HYPRE_BiCGSTABSetPrecond(g, *(_ds(lib) if precond == "ds" else precond))
    for setter, value in ((lib.hypre_amd_BiCGSTABSetFusedUpdates, fused), (lib.HYPRE_BiCGSTABSetMinIter, min_iter),
                          (lib.HYPRE_BiCGSTABSetConvergenceFactorTol, cf_tol), (lib.HYPRE_BiCGSTABSetAbsoluteTol, a_tol),
                          (lib.HYPRE_BiCGSTABSetStopCrit, stop_crit)):
        if value is not None:
            setter(g, value)
    lib.HYPRE_ParCSRBiCGSTABSetup(g, A, db, dx)
    rc = lib.HYPRE_ParCSRBiCGSTABSolve(g, A, db, dx)
    err = lib.HYPRE_GetError()
    lib.HYPRE_ClearError(256)
    B.check()
    its, rel, conv, count, norms = C.c_int(-1), C.c_double(-1.0), C.c_int(-1), C.c_int(-1), C.POINTER(C.c_double)()
    lib.HYPRE_BiCGSTABGetNumIterations(g, C.byref(its))
    lib.HYPRE_BiCGSTABGetFinalRelativeResidualNorm(g, C.byref(rel))
    lib.hypre_amd_BiCGSTABGetConverged(g, C.byref(conv))
    lib.hypre_amd_BiCGSTABGetLoggedNorms(g, C.byref(count), C.byref(norms))
    logged = np.array([norms[i] for i in range(count.value)])
    lib.HYPRE_ParCSRBiCGSTABDestroy(g)
    return dict(rc=rc, its=its.value, rel=rel.value, conv=conv.value, err=err, norms=logged)


def _numpy_bicgstab(M, b, apply_pc, tol, max_iter=1000):
    """Preconditioned BiCGSTAB from x = 0, straight from the recurrence (van der Vorst 1992 with the preconditioner on the
    right, as krylov/bicgstab.c:448-561 runs it), np.dot throughout; it ends when the residual of the recurrence and then
    b - M x meet tol |b|.  Returns (iterations, |b - M x| / |b|)."""
    x = np.zeros(len(b))
    r0 = b - M @ x
    r, p = r0.copy(), r0.copy()
    bn = np.linalg.norm(b)
    res, it = np.dot(r0, r0), 0
    while it < max_iter:
        it += 1
        v = apply_pc(p)
        q = M @ v
        alpha = res / np.dot(r0, q)
        x += alpha * v
        r -= alpha * q
        v = apply_pc(r)
        s = M @ v
        num, den = np.dot(r, s), np.dot(s, s)
        gamma = 0.0 if num == 0.0 and den == 0.0 else num / den
        x += gamma * v
        r -= gamma * s
        if np.sqrt(np.dot(r, r)) <= tol * bn:
            r = b - M @ x
            if np.sqrt(np.dot(r, r)) <= tol * bn:
                break
        beta = 1.0 / res
        res = np.dot(r0, r)
        beta *= res
        p = r + (beta * alpha / gamma) * (p - gamma * q)
    return it, float(np.linalg.norm(b - M @ x) / bn)


def _operator(lib, **kw):
    """(options, device matrix, scipy copy)"""
    from hypre_amd import binding as B, ij
    opt = ij.IJOptions(**kw)
    A = ij.build_matrix(opt)
    M = B.csr_to_scipy(A.contents.diag)
    lib.hypre_ParCSRMatrixMigrate(A, B.HYPRE_MEMORY_DEVICE)
    B.check()
    return opt, A, M


def _amg_difconv(lib):
    """the 12 x 11 x 10 convection-diffusion operator behind the driver's default hierarchy, one cycle per application"""
    from hypre_amd import binding as B, ij
    opt = ij.IJOptions(tol=1e-8, **DIFCONV)
    A = ij.build_matrix(opt)
    M = B.csr_to_scipy(A.contents.diag)
    s = ij.create_amg(opt, memory_location=B.HYPRE_MEMORY_DEVICE)
    lib.HYPRE_BoomerAMGSetup(s, A, None, None)
    B.check()
    lib.hypre_ParCSRMatrixMigrate(A, B.HYPRE_MEMORY_DEVICE)
    lib.HYPRE_BoomerAMGSetTol(s, 0.0)
    lib.HYPRE_BoomerAMGSetMaxIter(s, 1)
    return A, M, s


# ---------------------------------------------------------------------------------------------------------------------
# 2. fusion changes nothing
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["ds", "ds-nc4", "amg-difconv"])
def test_fused_and_plain_updates_give_the_same_bits(gpu_lib, case):
    """x bit for bit, the iteration count, every logged norm and the reported one.  ds: the 8^3 Laplacian with the driver's
    -rhsrand right-hand side; ds-nc4: that and three more random columns as one multivector; amg-difconv: the non-symmetric
    12 x 11 x 10 operator, right-hand side of ones, behind BoomerAMG."""
    from hypre_amd import binding as B, ij
    lib = gpu_lib
    s = None
    if case == "amg-difconv":
        A, M, s = _amg_difconv(lib)
        assert abs(M - M.T).max() > 1.0                                       # non-symmetric
        b = np.ones(M.shape[0])
        precond = (C.cast(lib.HYPRE_BoomerAMGSolve, C.c_void_p), None, s)
    else:
        opt, A, M = _operator(lib, n=(8, 8, 8), rhs="rand")
        b, _ = ij.build_rhs_host(opt, A)
        precond = "ds"
    make, fetch = B.parvec_from_numpy, B.parvec_to_numpy
    if case == "ds-nc4":
        b = np.column_stack([b] + [np.random.default_rng(c).uniform(-1, 1, 512) for c in range(1, 4)])
        make, fetch = B.parmultivec_from_numpy, B.parmultivec_to_numpy
    runs = {}
    for fused in (1, 0):
        db, dx = make(b), make(np.zeros_like(b))
        runs[fused] = _bicgstab(lib, A, db, dx, fused=fused, precond=precond)
        runs[fused]["x"] = fetch(dx)
        lib.hypre_ParVectorDestroy(db); lib.hypre_ParVectorDestroy(dx)
    on, off = runs[1], runs[0]
    print(case, "fused", on["its"], repr(on["rel"]), "plain", off["its"], repr(off["rel"]))
    assert on["rc"] == 0 and on["conv"] == 1 and on["err"] == 0 and on["its"] >= 3 and on["rel"] <= 1e-8
    assert np.array_equal(_bits(on["x"]), _bits(off["x"]))
    assert on["its"] == off["its"] and _same_double(on["rel"], off["rel"]) and on["conv"] == off["conv"]
    assert len(on["norms"]) == on["its"] + 1 and np.array_equal(_bits(on["norms"]), _bits(off["norms"]))
    # the reported norm is that of b - A x computed from x: it and numpy's differ by the rounding of that residual, each
    # row's within (entries + 1) u (|b| + |A| |x|), 8 u for these seven-point rows, for either of the two
    true = np.linalg.norm(b - M @ on["x"])
    assert abs(true - on["rel"] * np.linalg.norm(b)) <= 2 * 8 * 2.0 ** -53 * np.linalg.norm(np.abs(b) + abs(M) @ np.abs(on["x"]))
    if s is not None:
        lib.HYPRE_BoomerAMGDestroy(s)
    lib.hypre_ParCSRMatrixDestroy(A)


# ---------------------------------------------------------------------------------------------------------------------
# 3. an independent yardstick
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["laplacian-one", "laplacian-rand", "difconv-one"])
def test_ds_bicgstab_against_a_numpy_bicgstab(gpu_lib, case):
    """Jacobi preconditioning on both sides, tol 1e-8.  The iteration count within one; |b - A x| / |b| of the library's x,
    computed in numpy, at most 1.01 tol: the exit on the recomputed residual guarantees tol, the 1 % covers numpy's
    other order of summation."""
    from hypre_amd import binding as B, ij
    lib = gpu_lib
    kw = dict(DIFCONV) if case == "difconv-one" else dict(n=(8, 8, 8))
    opt, A, M = _operator(lib, rhs="rand" if case.endswith("rand") else "one", **kw)
    b, _ = ij.build_rhs_host(opt, A)
    n, tol = len(b), 1e-8
    dinv = 1.0 / M.diagonal()
    db, dx = B.parvec_from_numpy(b), B.parvec_from_numpy(np.zeros(n))
    r = _bicgstab(lib, A, db, dx, tol=tol)
    x = B.parvec_to_numpy(dx)
    oits, orel = _numpy_bicgstab(M, b, lambda v: dinv * v, tol)
    true = float(np.linalg.norm(b - M @ x) / np.linalg.norm(b))
    print(case, "iterations", r["its"], oits, "reported", r["rel"], "from x", true, "numpy BiCGSTAB", orel)
    assert r["rc"] == 0 and r["conv"] == 1 and r["err"] == 0
    assert abs(r["its"] - oits) <= 1 and r["its"] >= 10
    assert true <= 1.01 * tol and orel <= 1.01 * tol
    for v in (db, dx):
        lib.hypre_ParVectorDestroy(v)
    lib.hypre_ParCSRMatrixDestroy(A)


# ---------------------------------------------------------------------------------------------------------------------
# 4. reference goldens
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(GOLD))
def test_replay_bicgstab_job_on_the_device(name):
    """The job line as the reference states it, through parse_cli.  Iteration count exactly; final relative residual within
    1.5e-6 relative (the printed precision), the bar test_lgmres_gpu.py holds the lines of the same `.saved` file to."""
    case = GOLD[name]
    its, rel = _closing_lines(_worker(["job", name], case["np"]))
    exp = case["expect"]
    print(name, "iterations", its, "norm", rel, "expected", exp)
    assert its == exp["iterations"]
    assert abs(rel - exp["rel_resid"]) <= 1.5e-6 * exp["rel_resid"]


# ---------------------------------------------------------------------------------------------------------------------
# 5. two ranks
# ---------------------------------------------------------------------------------------------------------------------
def test_amg_bicgstab_on_two_ranks_against_one():
    """The convection-diffusion operator behind the driver's default hierarchy, split in z: the hierarchies differ with the
    partition, so the iteration counts agree within one; |b - A x| / |b| from the gathered x, computed in numpy with the
    operator built on one rank, is under the tolerance (times 1.01, as above) on both."""
    opts = dict(DIFCONV, solver=9, rhs="one", tol=1e-8)
    opts = {k: (list(v) if isinstance(v, tuple) else v) for k, v in opts.items()}
    one = _result(_worker(["solve", json.dumps(opts)], 1))
    two = _result(_worker(["solve", json.dumps(dict(opts, P=[1, 1, 2]))], 2))
    print("one rank", one, "two ranks", two)
    assert one["err"] == 0 and two["err"] == 0
    assert abs(one["iterations"] - two["iterations"]) <= 1 and one["iterations"] >= 2
    assert one["true"] <= 1.01e-8 and two["true"] <= 1.01e-8


# ---------------------------------------------------------------------------------------------------------------------
# 6. edges
# ---------------------------------------------------------------------------------------------------------------------
def test_edges(gpu_lib):
    from hypre_amd import binding as B
    lib = gpu_lib
    _, A, M = _operator(lib, n=(8, 8, 8))
    ones = np.ones(512)
    db = B.parvec_from_numpy(ones)
    # the plain solve: the reference's 12 iterations (vector.saved:47-48 has the same system in every column)
    dx = B.parvec_from_numpy(np.zeros(512))
    full = _bicgstab(lib, A, db, dx)
    assert full["rc"] == 0 and full["conv"] == 1 and full["its"] == 12 and abs(full["rel"] - 6.282586e-09) <= 1.5e-6 * 6.282586e-09
    # the iteration limit: HYPRE_ERROR_CONV (256), count and norm of the last iterate
    dx3 = B.parvec_from_numpy(np.zeros(512))
    r = _bicgstab(lib, A, db, dx3, max_iter=3)
    assert r["err"] & 256 and r["its"] == 3 and r["conv"] == 0 and 1e-8 < r["rel"] < 1.0
    assert _same_double(r["rel"], full["norms"][3] / np.sqrt(512.0)) and np.array_equal(_bits(r["norms"]), _bits(full["norms"][:4]))
    # min_iter: a tolerance the fourth iterate meets is not looked at before the ninth
    dxa, dxb = B.parvec_from_numpy(np.zeros(512)), B.parvec_from_numpy(np.zeros(512))
    loose, held = _bicgstab(lib, A, db, dxa, tol=0.1), _bicgstab(lib, A, db, dxb, tol=0.1, min_iter=9)
    print("tol 0.1:", loose["its"], loose["rel"], "with min_iter 9:", held["its"], held["rel"])
    assert loose["conv"] == 1 and loose["its"] < 9 and held["conv"] == 1 and held["its"] == 9 and held["rel"] < loose["rel"] <= 0.1
    # stop_crit: the absolute test, tol itself when no a_tol is set, else a_tol; |b| = sqrt(512) makes it the stricter one
    dxc, dxd = B.parvec_from_numpy(np.zeros(512)), B.parvec_from_numpy(np.zeros(512))
    ra, rb = _bicgstab(lib, A, db, dxc, tol=0.1, stop_crit=1), _bicgstab(lib, A, db, dxd, tol=0.1, stop_crit=1, a_tol=1e-3)
    print("stop_crit:", ra["its"], ra["rel"], "with a_tol 1e-3:", rb["its"], rb["rel"])
    assert ra["conv"] == 1 and ra["rel"] * np.sqrt(512.0) <= 0.1 and ra["its"] >= loose["its"]
    assert rb["conv"] == 1 and rb["rel"] * np.sqrt(512.0) <= 1e-3 and rb["its"] > ra["its"]
    # the convergence-factor exit: 12 iterations to 1e-8 are an average factor near 0.46 per half step, far above 0.1, so the
    # solve gives up as soon as the estimate has settled (the second iteration), without an error
    dxe = B.parvec_from_numpy(np.zeros(512))
    rc = _bicgstab(lib, A, db, dxe, cf_tol=0.1)
    print("cf_tol 0.1:", rc["its"], rc["rel"])
    assert rc["err"] == 0 and rc["conv"] == 0 and 2 <= rc["its"] < full["its"] and rc["rel"] > 1e-8
    # b = 0, x = 0: the residual is exactly zero, Solve returns at once
    dz, dx0 = B.parvec_from_numpy(np.zeros(512)), B.parvec_from_numpy(np.zeros(512))
    r = _bicgstab(lib, A, dz, dx0)
    assert r["rc"] == 0 and r["err"] == 0 and r["its"] == 0 and r["rel"] == 0.0 and r["conv"] == 0 and list(r["norms"]) == [0.0]
    assert B.parvec_to_numpy(dx0).tobytes() == np.zeros(512).tobytes()
    # b = 0 with a guess: |r_0| = |A x_0| is the denominator of the test, and the norm reported is the residual norm itself
    dx1 = B.parvec_from_numpy(ones)
    r = _bicgstab(lib, A, dz, dx1)
    r0n = float(np.linalg.norm(M @ ones))
    left = float(np.linalg.norm(M @ B.parvec_to_numpy(dx1)))
    print("b = 0:", r["its"], r["rel"], "|A x|", left, "|A x0|", r0n)
    assert r["conv"] == 1 and r["err"] == 0 and r["its"] > 3 and 0.0 < r["rel"] <= 1e-8 * r0n
    assert left <= 1.01e-8 * r0n and abs(left - r["rel"]) <= 1e-6 * left
    assert abs(r["norms"][0] - r0n) <= 1e-12 * r0n
    # a host operand
    hb = lib.hypre_ParVectorCreate(0, 512, None)
    lib.hypre_ParVectorInitialize_v2(hb, B.HYPRE_MEMORY_HOST)
    g = C.c_void_p()
    lib.HYPRE_ParCSRBiCGSTABCreate(0, C.byref(g))
    lib.HYPRE_BiCGSTABSetTol(g, 1e-8)
    lib.HYPRE_BiCGSTABSetPrecond(g, *_ds(lib))
    lib.HYPRE_BiCGSTABSetup(g, A, db, dx)
    before = B.parvec_to_numpy(dx)
    assert lib.HYPRE_BiCGSTABSolve(g, A, hb, dx) != 0
    assert b"not in device memory" in lib.hypre_amd_LastErrorMessage()
    lib.HYPRE_ClearAllErrors()
    assert np.array_equal(B.parvec_to_numpy(dx), before)
    # ... and GetResidual after a solve through the generic names: b - A x of the last check
    dx2 = B.parvec_from_numpy(np.zeros(512))
    assert lib.HYPRE_BiCGSTABSolve(g, A, db, dx2) == 0
    k, rel, res = C.c_int(), C.c_double(), C.c_void_p()
    lib.HYPRE_ParCSRBiCGSTABGetNumIterations(g, C.byref(k))
    lib.HYPRE_ParCSRBiCGSTABGetFinalRelativeResidualNorm(g, C.byref(rel))
    assert k.value == 12 and _same_double(rel.value, full["rel"])
    assert np.array_equal(_bits(B.parvec_to_numpy(dx2)), _bits(B.parvec_to_numpy(dx)))
    lib.HYPRE_ParCSRBiCGSTABGetResidual(g, C.byref(res))
    rv = B.parvec_to_numpy(C.cast(res, C.POINTER(B.ParVector)))
    assert abs(np.linalg.norm(rv) / np.sqrt(512.0) - rel.value) <= 1e-12 * rel.value
    lib.HYPRE_ParCSRBiCGSTABDestroy(g)
    for v in (db, dx, dx3, dxa, dxb, dxc, dxd, dxe, dz, dx0, dx1, dx2, hb):
        lib.hypre_ParVectorDestroy(v)
    lib.hypre_ParCSRMatrixDestroy(A)


@pytest.mark.parametrize("fused", [1, 0])
def test_an_exact_first_half_step_ends_cleanly(gpu_lib, fused):
    """A = I, b = e_1, x = 0, no preconditioner: alpha = 1 and the first half step leaves r = 0 exactly, so s = 0 and the
    step length is 0 / 0, which the reference takes as 0; the convergence test then ends the solve: one iteration, x = b,
    no NaN anywhere."""
    from hypre_amd import binding as B
    lib = gpu_lib
    A = B.laplacian(4, 4, 4, values=np.array([1.0, 0.0, 0.0, 0.0]))
    assert abs(B.csr_to_scipy(A.contents.diag) - np.eye(64)).max() == 0.0
    lib.hypre_ParCSRMatrixMigrate(A, B.HYPRE_MEMORY_DEVICE)
    e1 = np.zeros(64)
    e1[0] = 1.0
    db, dx = B.parvec_from_numpy(e1), B.parvec_from_numpy(np.zeros(64))
    r = _bicgstab(lib, A, db, dx, precond=None, fused=fused)
    x = B.parvec_to_numpy(dx)
    print("fused", fused, r)
    assert r["rc"] == 0 and r["err"] == 0 and r["conv"] == 1 and r["its"] == 1 and r["rel"] == 0.0
    assert list(r["norms"]) == [1.0, 0.0] and not np.any(np.isnan(x)) and np.array_equal(x, e1)
    for v in (db, dx):
        lib.hypre_ParVectorDestroy(v)
    lib.hypre_ParCSRMatrixDestroy(A)
