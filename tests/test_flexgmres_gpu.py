"""FlexGMRES (HYPRE_ParCSRFlexGMRES*; the reference's `ij -solver 60 | 61`) on the device.

1. the reference's four FlexGMRES job lines (tests/golden/ij_saved_flexgmres.json) replayed through the driver (hypre_amd.ij.launch,
   started by tests/flexgmres_worker.py with the options of the job line: the command line keeps refusing the two solver ids);
2. the fused Gram-Schmidt launch (hypre_amd_ParVectorAxpyThenInnerProd, mgs_step_kernel) against hypre_ParVectorAxpy
   followed by hypre_ParVectorInnerProd, bit for bit;
3. a solve with the fused steps against the same solve with the plain InnerProd / Axpy sequence, bit for bit;
4. with a fixed preconditioner FlexGMRES is GMRES: against the oracle's GMRES;
5. with a preconditioner that changes every iteration it is FGMRES: against one written here in numpy;
6. the edges: the iteration limit, a zero right-hand side, SetKDim without Setup, the convergence-factor gate."""
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
GOLD = json.load(open(os.path.join(HERE, "golden", "ij_saved_flexgmres.json")))


# ---------------------------------------------------------------------------------------------------------------------
# 1. reference goldens
# ---------------------------------------------------------------------------------------------------------------------
def _replay(name, case, timeout=600):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    from conftest import free_port
    worker = [os.path.join(HERE, "flexgmres_worker.py"), name]
    if case["np"] == 1:
        cmd = [sys.executable] + worker
    else:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(case["np"]),
               "--master-addr", "127.0.0.1", "--master-port", str(free_port())] + worker
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stderr[-2000:]
    return p.stdout


@pytest.mark.parametrize("name", sorted(GOLD))
def test_replay_flexgmres_job_on_the_device(name):
    """Iteration count exactly; final relative residual within 1.5e-6 relative, the bar test_cogmres_gpu.py holds the
    GMRES-family lines of the same `.saved` files to.  The np 2 and np 4 lines are the multi-rank cases, the vector.jobs
    lines the multivector ones."""
    case = GOLD[name]
    out = _replay(name, case)
    exp = case["expect"]
    m = re.search(r"^Final FlexGMRES Relative Residual Norm = (\S+)$", out, re.M)
    print(name, re.findall(r"^FlexGMRES Iterations = \d+$", out, re.M), m and m.group(1), "expected", exp)
    assert re.search(r"^FlexGMRES Iterations = %d$" % exp["iterations"], out, re.M), out
    assert m and abs(float(m.group(1)) - exp["rel_resid"]) <= 1.5e-6 * exp["rel_resid"], out


# ---------------------------------------------------------------------------------------------------------------------
# 2. the kernel
# ---------------------------------------------------------------------------------------------------------------------
# 1, 255, 256: below one workgroup's 512 elements, tail only / odd / even; 257: one element past 256; 64 * 1024 + 3: 129
# workgroups and a tail; 1 060 904: past one pass of the 1024-workgroup grid of a dot product (test_cogmres_gpu.py's size)
LENGTHS = (1, 255, 256, 257, 64 * 1024 + 3, 1060904)
ALPHAS = (0.0, -1.0, 0.7320508075688772)
_data = {}


def _host_vectors(n):
    if n not in _data:
        rng = np.random.default_rng(60610000 + n)
        _data[n] = tuple(rng.standard_normal(n) for _ in range(3))
        for v in _data[n]:
            v.setflags(write=False)
    return _data[n]


def _fused_against_separate(lib, make, fetch, hx, hy, hz, alpha, z_is_y):
    """one comparison; returns (bits of y equal, fused scalar, separate scalar)"""
    x, y, z = make(hx), make(hy), make(hz)
    lib.hypre_ParVectorAxpy(alpha, x, y)
    want = lib.hypre_ParVectorInnerProd(y if z_is_y else z, y)
    want_y = fetch(y)
    y2 = make(hy)
    got = C.c_double(np.nan)
    assert lib.hypre_amd_ParVectorAxpyThenInnerProd(alpha, x, y2, y2 if z_is_y else z, C.byref(got)) == 0
    got_y = fetch(y2)
    same_inputs = np.array_equal(fetch(x), hx) and np.array_equal(fetch(z), hz)          # x and a separate z are left alone
    for v in (x, y, z, y2):
        lib.hypre_ParVectorDestroy(v)
    return np.array_equal(got_y.view(np.int64), want_y.view(np.int64)) and same_inputs, got.value, want


@pytest.mark.parametrize("n", LENGTHS)
def test_fused_step_has_the_bits_of_axpy_then_inner_prod(gpu_lib, n):
    from hypre_amd import binding as B
    lib = gpu_lib
    hx, hy, hz = _host_vectors(n)
    for alpha in ALPHAS:
        for z_is_y in (False, True):
            same, got, want = _fused_against_separate(lib, B.parvec_from_numpy, B.parvec_to_numpy, hx, hy, hz, alpha, z_is_y)
            print("n", n, "alpha", alpha, "z is y", z_is_y, "fused", repr(got), "separate", repr(want))
            assert same, (n, alpha, z_is_y)
            assert np.float64(got).tobytes() == np.float64(want).tobytes(), (n, alpha, z_is_y, got, want)
            ref = float(np.dot(hy + alpha * hx, (hy + alpha * hx) if z_is_y else hz))
            assert abs(want - ref) <= 1e-12 * n * max(1.0, abs(ref))                 # the yardstick itself is that dot product
    B.check()


def test_fused_step_on_a_multivector_of_odd_flat_length(gpu_lib):
    """3 columns of 693 rows: the flat inner product over all columns, 2079 elements."""
    from hypre_amd import binding as B
    lib = gpu_lib
    rng = np.random.default_rng(693)
    hx, hy, hz = (rng.standard_normal((693, 3)) for _ in range(3))
    for alpha in ALPHAS:
        for z_is_y in (False, True):
            same, got, want = _fused_against_separate(lib, B.parmultivec_from_numpy, B.parmultivec_to_numpy, hx, hy, hz, alpha, z_is_y)
            print("alpha", alpha, "z is y", z_is_y, "fused", repr(got), "separate", repr(want))
            assert same and np.float64(got).tobytes() == np.float64(want).tobytes(), (alpha, z_is_y, got, want)
            ynew = hy + alpha * hx
            assert abs(want - float(np.sum(ynew * (ynew if z_is_y else hz)))) <= 1e-12 * 2079
    B.check()


# ---------------------------------------------------------------------------------------------------------------------
# solver helpers
# ---------------------------------------------------------------------------------------------------------------------
def _ds(lib):
    return C.cast(lib.HYPRE_ParCSRDiagScale, C.c_void_p), C.cast(lib.HYPRE_ParCSRDiagScaleSetup, C.c_void_p), None


def _flexgmres(lib, A, db, dx, k_dim=5, tol=1e-8, max_iter=1000, fused=None, precond=None, modify_pc=None):
    """one solve through the C ABI; returns dict(its, rel, conv, err, stats=(fused_steps, plain_dots, plain_axpys))"""
    g = C.c_void_p()
    lib.HYPRE_ParCSRFlexGMRESCreate(0, C.byref(g))
    lib.HYPRE_FlexGMRESSetKDim(g, k_dim)
    lib.HYPRE_FlexGMRESSetTol(g, tol)
    lib.HYPRE_FlexGMRESSetMaxIter(g, max_iter)
    lib.HYPRE_FlexGMRESSetPrecond(g, *(precond or _ds(lib)))
    if fused is not None:
        lib.hypre_amd_FlexGMRESSetFusedOrthogonalization(g, fused)
    if modify_pc is not None:
        lib.HYPRE_FlexGMRESSetModifyPC(g, C.cast(modify_pc, C.c_void_p))
    lib.HYPRE_ParCSRFlexGMRESSetup(g, A, db, dx)
    lib.HYPRE_ParCSRFlexGMRESSolve(g, A, db, dx)
    err = lib.HYPRE_GetError()
    lib.HYPRE_ClearError(256)
    from hypre_amd import binding as B
    B.check()
    its, rel, conv = C.c_int(), C.c_double(), C.c_int()
    st = [C.c_int(-1) for _ in range(3)]
    lib.HYPRE_FlexGMRESGetNumIterations(g, C.byref(its))
    lib.HYPRE_FlexGMRESGetFinalRelativeResidualNorm(g, C.byref(rel))
    lib.HYPRE_FlexGMRESGetConverged(g, C.byref(conv))
    lib.hypre_amd_FlexGMRESGetLaunchStats(g, *[C.byref(v) for v in st])
    lib.HYPRE_ParCSRFlexGMRESDestroy(g)
    return dict(its=its.value, rel=rel.value, conv=conv.value, err=err, stats=tuple(v.value for v in st))


def _gram_schmidt_steps(its, k_dim):
    """sum of i over the Arnoldi steps of `its` iterations in restart cycles of k_dim"""
    return sum((it - 1) % k_dim + 1 for it in range(1, its + 1))


def _operator(lib, oracle=None, **kw):
    """(options, device matrix, scipy copy, oracle copy or None)"""
    from hypre_amd import binding as B, ij
    opt = ij.IJOptions(**kw)
    A = ij.build_matrix(opt)
    M = B.csr_to_scipy(A.contents.diag)
    Ao = oracle.par_from_handles([A]) if oracle is not None else None
    lib.hypre_ParCSRMatrixMigrate(A, B.HYPRE_MEMORY_DEVICE)
    B.check()
    return opt, A, M, Ao


# ---------------------------------------------------------------------------------------------------------------------
# 3. fusion changes nothing
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nv", [1, 3])
def test_fused_and_plain_orthogonalization_give_the_same_bits_693_rows(gpu_lib, nv):
    """DS-FlexGMRES on the 7 x 9 x 11 Laplacian, the driver's -rhsrand right-hand side (nv 3: that and two more random
    columns as one multivector), k_dim 5, tol 1e-8: x bit for bit, the iteration count and the reported norm."""
    from hypre_amd import binding as B, ij
    lib = gpu_lib
    opt, A, M, _ = _operator(lib, n=(7, 9, 11), rhs="rand")
    b, _ = ij.build_rhs_host(opt, A)
    make, fetch = B.parvec_from_numpy, B.parvec_to_numpy
    if nv > 1:
        b = np.column_stack([b] + [np.random.default_rng(c).uniform(-1, 1, 693) for c in range(1, nv)])
        make, fetch = B.parmultivec_from_numpy, B.parmultivec_to_numpy
    runs = {}
    for fused in (1, 0):
        db, dx = make(b), make(np.zeros_like(b))
        runs[fused] = _flexgmres(lib, A, db, dx, k_dim=5, tol=1e-8, fused=fused)
        runs[fused]["x"] = fetch(dx)
        lib.hypre_ParVectorDestroy(db); lib.hypre_ParVectorDestroy(dx)
    on, off = runs[1], runs[0]
    print("nv", nv, "fused", on["its"], repr(on["rel"]), on["stats"], "plain", off["its"], repr(off["rel"]), off["stats"])
    assert on["conv"] == 1 and on["its"] > 5 and on["rel"] <= 1e-8
    assert np.array_equal(on["x"].view(np.int64), off["x"].view(np.int64))
    assert on["its"] == off["its"] and on["rel"] == off["rel"] and on["conv"] == off["conv"]
    steps = _gram_schmidt_steps(on["its"], 5)
    assert on["stats"] == (steps, on["its"], 0)
    assert off["stats"] == (0, steps + off["its"], steps) and steps > 0
    true = np.linalg.norm(b - M @ on["x"]) / np.linalg.norm(b)
    assert abs(true - on["rel"]) <= 1e-9 * true
    lib.hypre_ParCSRMatrixDestroy(A)


def test_fused_and_plain_orthogonalization_give_the_same_bits_past_one_grid_pass(gpu_lib, oracle):
    """The 104 x 101 x 101 operator (1 060 904 rows: every vector kernel takes a second trip), 3 iterations at tol 0."""
    from hypre_amd import binding as B
    from test_cogmres_gpu import _past_one_grid_pass
    lib = gpu_lib
    h = _past_one_grid_pass(lib, oracle)
    runs = {}
    for fused in (1, 0):
        db, dx = B.parvec_from_numpy(h["b"]), B.parvec_from_numpy(np.zeros(h["n"]))
        runs[fused] = _flexgmres(lib, h["A"], db, dx, k_dim=5, tol=0.0, max_iter=3, fused=fused)
        runs[fused]["x"] = B.parvec_to_numpy(dx)
        lib.hypre_ParVectorDestroy(db); lib.hypre_ParVectorDestroy(dx)
    on, off = runs[1], runs[0]
    print("fused", on["its"], repr(on["rel"]), on["stats"], "plain", off["its"], repr(off["rel"]), off["stats"])
    assert on["its"] == off["its"] == 3 and on["rel"] == off["rel"] and 0.0 < on["rel"] < 1.0
    assert np.array_equal(on["x"].view(np.int64), off["x"].view(np.int64)) and np.any(on["x"] != 0.0)
    assert on["stats"] == (6, 3, 0) and off["stats"] == (0, 9, 6)


# ---------------------------------------------------------------------------------------------------------------------
# 4. fixed preconditioner: GMRES
# ---------------------------------------------------------------------------------------------------------------------
def test_ds_flexgmres_is_the_oracles_ds_gmres(gpu_lib, oracle):
    """8^3 Laplacian, diagonal scaling, k_dim 5, tol 0: after 1, 2, 3 and 7 iterations (7 crosses a restart) the relative
    residual is the oracle's GMRES's to 1e-6 relative and the iterate to 1e-9 of its largest entry."""
    from hypre_amd import binding as B
    lib = gpu_lib
    _, A, _, Ao = _operator(lib, oracle, n=(8, 8, 8))
    b = np.random.default_rng(8).uniform(-1.0, 1.0, 512)
    for k in (1, 2, 3, 7):
        X = np.zeros((512, 1))
        oits, orel, _ = oracle.gmres_ds_multi(Ao, b[:, None], X, tol=0.0, max_iter=k, k_dim=5)
        db, dx = B.parvec_from_numpy(b), B.parvec_from_numpy(np.zeros(512))
        r = _flexgmres(lib, A, db, dx, k_dim=5, tol=0.0, max_iter=k)
        x = B.parvec_to_numpy(dx)
        lib.hypre_ParVectorDestroy(db); lib.hypre_ParVectorDestroy(dx)
        xerr = float(np.max(np.abs(x - X[:, 0])) / np.max(np.abs(X[:, 0])))
        print("iterations", r["its"], oits, "relative residual", r["rel"], orel, "difference", abs(r["rel"] - orel) / orel, "iterate", xerr)
        assert r["its"] == oits == k
        assert 0.0 < orel < 1.0 and abs(r["rel"] - orel) <= 1e-6 * orel
        assert xerr <= 1e-9
    lib.hypre_ParCSRMatrixDestroy(A)


def _amg_problem(lib, oracle):
    """12^3 7-point problem, PMIS / ext+i / l1-Jacobi hierarchy set up once on the device, and the oracle's copy of it"""
    from hypre_amd import binding as B, ij
    opt = ij.IJOptions(n=(12, 12, 12), relax_type=18, coarsen_type=8, tol=1e-8)
    A = ij.build_matrix(opt)
    M = B.csr_to_scipy(A.contents.diag)
    s = ij.create_amg(opt, memory_location=B.HYPRE_MEMORY_DEVICE)
    lib.HYPRE_BoomerAMGSetup(s, A, None, None)
    B.check()
    lib.hypre_ParCSRMatrixMigrate(A, B.HYPRE_MEMORY_DEVICE)
    amg = oracle.amg_from_solvers([s])
    lib.HYPRE_BoomerAMGSetTol(s, 0.0)
    lib.HYPRE_BoomerAMGSetMaxIter(s, 1)
    b = np.random.default_rng(12).uniform(-1.0, 1.0, 12 ** 3)
    return A, M, s, amg, b


def test_amg_flexgmres_is_the_oracles_amg_gmres(gpu_lib, oracle):
    from hypre_amd import binding as B
    lib = gpu_lib
    A, M, s, amg, b = _amg_problem(lib, oracle)
    n = len(b)
    db, dx = B.parvec_from_numpy(b), B.parvec_from_numpy(np.zeros(n))
    r = _flexgmres(lib, A, db, dx, k_dim=5, tol=1e-8, precond=(C.cast(lib.HYPRE_BoomerAMGSolve, C.c_void_p), None, s))
    x = B.parvec_to_numpy(dx)
    xo = np.zeros(n)
    oits, orel, _ = amg.gmres(b, xo, tol=1e-8, max_iter=1000, k_dim=5, precond_cycles=1)
    xerr = float(np.max(np.abs(x - xo)) / np.max(np.abs(xo)))
    print("iterations", r["its"], oits, "relative residual", r["rel"], orel, "iterate", xerr)
    assert r["its"] == oits and r["conv"] == 1
    assert abs(r["rel"] - orel) <= 1e-6 * orel
    assert xerr <= 1e-9
    lib.hypre_ParVectorDestroy(db); lib.hypre_ParVectorDestroy(dx)
    lib.HYPRE_BoomerAMGDestroy(s); lib.hypre_ParCSRMatrixDestroy(A)


# ---------------------------------------------------------------------------------------------------------------------
# 5. changing preconditioner: FGMRES
# ---------------------------------------------------------------------------------------------------------------------
def _numpy_fgmres(M, b, apply_pc, k_dim, tol, max_iter=200):
    """Flexible GMRES(k_dim) from x = 0 (Saad, "A flexible inner-outer preconditioned GMRES algorithm", 1993): modified
    Gram-Schmidt, Givens rotations, x += Z y; apply_pc(iteration, v) is the preconditioner of that iteration.
    Returns (iterations, ||b - M x|| / ||b||, x)."""
    n = len(b)
    x, it, bn = np.zeros(n), 0, np.linalg.norm(b)
    eps = tol * bn
    while it < max_iter:
        r = b - M @ x
        beta = np.linalg.norm(r)
        if beta <= eps:
            break
        V, Z = np.zeros((k_dim + 1, n)), np.zeros((k_dim, n))
        H, g = np.zeros((k_dim + 1, k_dim)), np.zeros(k_dim + 1)
        cs, sn = np.zeros(k_dim), np.zeros(k_dim)
        V[0], g[0], i = r / beta, beta, 0
        while i < k_dim and it < max_iter:
            it += 1
            Z[i] = apply_pc(it, V[i])
            w = M @ Z[i]
            for j in range(i + 1):
                H[j, i] = V[j] @ w
                w = w - H[j, i] * V[j]
            H[i + 1, i] = np.linalg.norm(w)
            V[i + 1] = w / H[i + 1, i]
            for j in range(i):
                H[j, i], H[j + 1, i] = cs[j] * H[j, i] + sn[j] * H[j + 1, i], -sn[j] * H[j, i] + cs[j] * H[j + 1, i]
            d = np.hypot(H[i, i], H[i + 1, i])
            cs[i], sn[i] = H[i, i] / d, H[i + 1, i] / d
            H[i, i], H[i + 1, i] = d, 0.0
            g[i + 1], g[i] = -sn[i] * g[i], cs[i] * g[i]
            i += 1
            if abs(g[i]) <= eps:
                break
        x = x + np.linalg.solve(np.triu(H[:i, :i]), g[:i]) @ Z[:i]
    return it, float(np.linalg.norm(b - M @ x) / bn), x


def test_a_preconditioner_that_changes_every_iteration(gpu_lib, oracle):
    """AMG-FlexGMRES whose modify_pc callback gives the preconditioner one V-cycle on odd and two on even iterations,
    against a numpy FGMRES with the oracle's cycle applied once or twice."""
    from hypre_amd import binding as B
    from hypre_amd.parcsr_ls_binding import MODIFY_PC_FN
    lib = gpu_lib
    A, M, s, amg, b = _amg_problem(lib, oracle)
    n, k_dim, tol = len(b), 5, 1e-8
    calls = []

    def modify(precond_data, iteration, rel_norm):
        calls.append((iteration, rel_norm))
        lib.HYPRE_BoomerAMGSetMaxIter(C.c_void_p(precond_data), 1 if iteration % 2 else 2)
        return 0

    cb = MODIFY_PC_FN(modify)
    db, dx = B.parvec_from_numpy(b), B.parvec_from_numpy(np.zeros(n))
    r = _flexgmres(lib, A, db, dx, k_dim=k_dim, tol=tol, precond=(C.cast(lib.HYPRE_BoomerAMGSolve, C.c_void_p), None, s), modify_pc=cb)
    x = B.parvec_to_numpy(dx)

    def apply_pc(iteration, v):
        u = np.zeros(n)
        amg.cycle(v, u, u_all_zeros=True)
        if iteration % 2 == 0:
            amg.cycle(v, u, u_all_zeros=False)
        return u

    oits, orel, xo = _numpy_fgmres(M, b, apply_pc, k_dim, tol)
    true = float(np.linalg.norm(b - M @ x) / np.linalg.norm(b))
    print("iterations", r["its"], oits, "reported", r["rel"], "numpy from x", true, "numpy FGMRES", orel, "calls", calls)
    assert r["conv"] == 1 and r["its"] == oits and r["its"] > k_dim
    assert abs(r["rel"] - orel) <= 1e-6 * orel
    assert abs(r["rel"] - true) <= 1e-9 * true and r["rel"] <= tol
    assert [c[0] for c in calls] == list(range(1, r["its"] + 1))                  # once per iteration, in order
    for (it, rel), (_, before) in zip(calls[1:], calls[:-1]):
        if (it - 1) % k_dim != 0:                                                  # inside a restart cycle
            assert rel <= before, calls
    assert abs(calls[0][1] - 1.0) <= 1e-14                                         # |r0| / |b| from a zero guess
    # the same solve with the plain Gram-Schmidt sequence: the same bits, also behind this preconditioner
    calls.clear()
    dx2 = B.parvec_from_numpy(np.zeros(n))
    r2 = _flexgmres(lib, A, db, dx2, k_dim=k_dim, tol=tol, fused=0, precond=(C.cast(lib.HYPRE_BoomerAMGSolve, C.c_void_p), None, s), modify_pc=cb)
    assert r2["its"] == r["its"] and r2["rel"] == r["rel"] and B.parvec_to_numpy(dx2).tobytes() == x.tobytes()
    for v in (db, dx, dx2):
        lib.hypre_ParVectorDestroy(v)
    lib.HYPRE_BoomerAMGDestroy(s); lib.hypre_ParCSRMatrixDestroy(A)


# ---------------------------------------------------------------------------------------------------------------------
# 6. edges
# ---------------------------------------------------------------------------------------------------------------------
def test_edges(gpu_lib):
    from hypre_amd import binding as B
    lib = gpu_lib
    _, A, _, _ = _operator(lib, n=(8, 8, 8))
    # the iteration limit: HYPRE_ERROR_CONV (256), three iterations done
    db, dx = B.parvec_from_numpy(np.ones(512)), B.parvec_from_numpy(np.zeros(512))
    r = _flexgmres(lib, A, db, dx, k_dim=5, tol=0.0, max_iter=3)
    assert r["err"] & 256 and r["its"] == 3 and r["conv"] == 0
    # b = 0, x = 0: returns at once
    dz, dx0 = B.parvec_from_numpy(np.zeros(512)), B.parvec_from_numpy(np.zeros(512))
    r = _flexgmres(lib, A, dz, dx0, k_dim=5, tol=1e-8)
    assert r["err"] == 0 and r["its"] == 0 and r["stats"] == (0, 0, 0)
    assert B.parvec_to_numpy(dx0).tobytes() == np.zeros(512).tobytes()
    # SetKDim without a new Setup
    g = C.c_void_p()
    lib.HYPRE_ParCSRFlexGMRESCreate(0, C.byref(g))
    k, p = C.c_int(), C.c_void_p(1)
    lib.HYPRE_FlexGMRESSetPrecond(g, *_ds(lib))
    lib.HYPRE_FlexGMRESGetPrecond(g, C.byref(p))
    assert p.value is None
    lib.HYPRE_ParCSRFlexGMRESSetup(g, A, db, dx0)                # the solver's own default: k_dim 20
    B.check()
    lib.HYPRE_FlexGMRESSetKDim(g, 7)
    assert lib.HYPRE_ParCSRFlexGMRESSolve(g, A, db, dx0) != 0
    assert b"HYPRE_ParCSRFlexGMRESSetup" in lib.hypre_amd_LastErrorMessage()
    lib.HYPRE_ClearAllErrors()
    assert B.parvec_to_numpy(dx0).tobytes() == np.zeros(512).tobytes()          # nothing was solved
    lib.HYPRE_ParCSRFlexGMRESSetup(g, A, db, dx0)
    assert lib.HYPRE_ParCSRFlexGMRESSolve(g, A, db, dx0) == 0
    lib.HYPRE_ParCSRFlexGMRESGetNumIterations(g, C.byref(k))
    assert k.value > 0
    B.check()
    # the convergence-factor exit is not built
    assert lib.HYPRE_FlexGMRESSetConvergenceFactorTol(g, 0.0) == 0
    lib.HYPRE_FlexGMRESSetConvergenceFactorTol(g, 0.5)
    assert lib.HYPRE_GetError() & 4 and lib.HYPRE_GetErrorArg() == 2
    assert b"HYPRE_FlexGMRESSetConvergenceFactorTol" in lib.hypre_amd_LastErrorMessage()
    lib.HYPRE_ClearAllErrors()
    lib.HYPRE_ParCSRFlexGMRESDestroy(g)
    for v in (db, dx, dz, dx0):
        lib.hypre_ParVectorDestroy(v)
    lib.hypre_ParCSRMatrixDestroy(A)
