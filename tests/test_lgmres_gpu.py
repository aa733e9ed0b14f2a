"""LGMRES (HYPRE_ParCSRLGMRES*; the reference's `ij -solver 50 | 51`) on the device.

1. the three vector operations it adds (hypre_amd_ParVectorScaledCopy, hypre_amd_ParVectorCopyThenInnerProd,
   hypre_amd_ParVectorScaledDifference) against the library calls they stand for, bit for bit; the squared norm also
   over two ranks;
2. a solve with the fused updates against the same solve with the reference's call sequence, bit for bit, behind the
   diagonal scaling and behind BoomerAMG, on vectors and on multivectors;
3. against an LGMRES written here in numpy from the algorithm;
4. the reference's four LGMRES job lines (tests/golden/ij_saved_lgmres.json) replayed through the driver
   (tests/lgmres_worker.py: the options of the job line, lgmres = 1);
5. AMG-LGMRES on two ranks against one rank;
6. the edges: a host operand, SetKDim / SetAugDim without Setup, the iteration limit with and without a tolerance, the
   zero residual."""
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
GOLD = json.load(open(os.path.join(HERE, "golden", "ij_saved_lgmres.json")))


def _worker(args, nranks, timeout=600):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    from conftest import free_port
    worker = [os.path.join(HERE, "lgmres_worker.py")] + list(args)
    if nranks == 1:
        cmd = [sys.executable] + worker
    else:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nranks),
               "--master-addr", "127.0.0.1", "--master-port", str(free_port())] + worker
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stderr[-2000:]
    return p.stdout


def _closing_lines(out):
    its = re.search(r"^LGMRES Iterations = (\d+)$", out, re.M)
    rel = re.search(r"^Final LGMRES Relative Residual Norm = (\S+)$", out, re.M)
    assert its and rel, out
    return int(its.group(1)), float(rel.group(1))


# ---------------------------------------------------------------------------------------------------------------------
# 1. the kernels
# ---------------------------------------------------------------------------------------------------------------------
# the sizes of test_flexgmres_gpu.py: 1, 255, 256: below one workgroup's 512 elements, tail only / odd / even; 257: one
# element past 256; 64 * 1024 + 3: 129 workgroups and a tail; 1 060 904: past one pass of the 1024-workgroup grid of a dot
LENGTHS = (1, 255, 256, 257, 64 * 1024 + 3, 1060904)
# 0 and 1 are the shortcuts of hypre_ParVectorScale (set to zero; nothing to do), -1 meets the scale by -1 of the sequence
COEFFS = (0.0, 1.0, -1.0, 0.7320508075688772, -3.0e-5)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _check_three_operations(lib, make, fetch, hx, hy, count):
    """every coefficient through the three operations and through the calls they replace; hx and hy share elements (every
    seventh) so that the difference meets exact zeros"""
    for a in COEFFS:
        # y = a x
        x, y1, y2 = make(hx), make(hy), make(hy)
        lib.hypre_ParVectorCopy(x, y1)
        lib.hypre_ParVectorScale(a, y1)
        assert lib.hypre_amd_ParVectorScaledCopy(a, x, y2) == 0
        assert np.array_equal(_bits(fetch(y2)), _bits(fetch(y1))), ("scaled copy", a)
        assert np.array_equal(_bits(fetch(x)), _bits(hx))
        if a != 0.0:
            assert np.array_equal(fetch(y2), a * hx)                      # one rounding: numpy's product
        # z = a (x - y)
        yd, z1, z2 = make(hy), make(np.full_like(hx, 7.0)), make(np.full_like(hx, 7.0))
        lib.hypre_ParVectorCopy(x, z1)
        lib.hypre_ParVectorScale(-1.0, z1)
        lib.hypre_ParVectorAxpy(1.0, yd, z1)
        lib.hypre_ParVectorScale(-a, z1)
        assert lib.hypre_amd_ParVectorScaledDifference(a, x, yd, z2) == 0
        got, want = fetch(z2), fetch(z1)
        assert np.array_equal(_bits(got), _bits(want)), ("scaled difference", a, int(np.flatnonzero(_bits(got) != _bits(want))[0]))
        assert np.array_equal(_bits(fetch(x)), _bits(hx)) and np.array_equal(_bits(fetch(yd)), _bits(hy))
        if a != 0.0:
            assert np.array_equal(got, (hy - hx) * -a)                    # two roundings, none fused
        for v in (x, y1, y2, yd, z1, z2):
            lib.hypre_ParVectorDestroy(v)
    # y = x with <x, x>
    x, y1, y2 = make(hx), make(hy), make(hy)
    lib.hypre_ParVectorCopy(x, y1)
    want = lib.hypre_ParVectorInnerProd(y1, y1)
    got = C.c_double(np.nan)
    assert lib.hypre_amd_ParVectorCopyThenInnerProd(x, y2, C.byref(got)) == 0
    print("n", count, "fused", repr(got.value), "separate", repr(want))
    assert np.array_equal(_bits(fetch(y2)), _bits(hx)) and np.array_equal(_bits(fetch(x)), _bits(hx))
    assert np.float64(got.value).tobytes() == np.float64(want).tobytes(), (got.value, want)
    ref = float(np.sum(hx * hx))
    assert abs(want - ref) <= 1e-12 * count * max(1.0, ref)                # the yardstick itself is that dot product
    for v in (x, y1, y2):
        lib.hypre_ParVectorDestroy(v)


@pytest.mark.parametrize("n", LENGTHS)
def test_the_three_operations_have_the_bits_of_the_calls_they_replace(gpu_lib, n):
    from hypre_amd import binding as B
    rng = np.random.default_rng(50510000 + n)
    hx, hy = rng.standard_normal(n), rng.standard_normal(n)
    hy[::7] = hx[::7]
    _check_three_operations(gpu_lib, B.parvec_from_numpy, B.parvec_to_numpy, hx, hy, n)
    B.check()


def test_the_three_operations_on_a_multivector_of_odd_flat_length(gpu_lib):
    """3 columns of 693 rows: 2079 elements."""
    from hypre_amd import binding as B
    rng = np.random.default_rng(693)
    hx, hy = rng.standard_normal((693, 3)), rng.standard_normal((693, 3))
    hy[::7] = hx[::7]
    _check_three_operations(gpu_lib, B.parmultivec_from_numpy, B.parmultivec_to_numpy, hx, hy, 2079)
    B.check()


def test_the_operations_refuse_host_operands_and_aliases(gpu_lib):
    from hypre_amd import binding as B
    lib = gpu_lib
    x, y = B.parvec_from_numpy(np.ones(10)), B.parvec_from_numpy(np.zeros(10))
    short = B.parvec_from_numpy(np.zeros(9))
    h = lib.hypre_ParVectorCreate(0, 10, None)
    lib.hypre_ParVectorInitialize_v2(h, B.HYPRE_MEMORY_HOST)
    r = C.c_double(3.0)
    for call in (lambda: lib.hypre_amd_ParVectorScaledCopy(2.0, x, h), lambda: lib.hypre_amd_ParVectorCopyThenInnerProd(h, y, C.byref(r)),
                 lambda: lib.hypre_amd_ParVectorScaledDifference(2.0, x, y, h), lambda: lib.hypre_amd_ParVectorScaledCopy(2.0, x, short),
                 lambda: lib.hypre_amd_ParVectorScaledCopy(2.0, x, x), lambda: lib.hypre_amd_ParVectorScaledDifference(2.0, x, y, y)):
        assert call() != 0
        lib.HYPRE_ClearAllErrors()
    assert r.value == 3.0 and np.array_equal(B.parvec_to_numpy(y), np.zeros(10))
    for v in (x, y, short, h):
        lib.hypre_ParVectorDestroy(v)


def test_the_squared_norm_over_two_ranks(gpu_lib):
    """1 500 001 elements, three quarters on rank 0 (past one pass of the reduction grid) and the rest on rank 1: the sum
    over the ranks through dev_global_sums has the bits of hypre_ParVectorInnerProd after the copy, on both ranks."""
    n = 1500001
    out = _worker(["norm2", str(n)], 2)
    parts = json.loads(re.search(r"^RESULT (.*)$", out, re.M).group(1))
    print(parts)
    assert len(parts) == 2 and [p["local"] for p in parts] == [1125000, 375001]
    for p in parts:
        assert p["rc"] == 0 and p["copied"] and p["fused"] == p["separate"]
    assert parts[0]["fused"] == parts[1]["fused"]
    ref = sum(p["numpy_local"] for p in parts)
    assert abs(parts[0]["value"] - ref) <= 1e-12 * n * ref


# ---------------------------------------------------------------------------------------------------------------------
# solver helpers
# ---------------------------------------------------------------------------------------------------------------------
def _lgmres(lib, A, db, dx, k_dim=5, aug_dim=2, tol=1e-8, max_iter=1000, fused=None, precond=None, approx=None):
    """one solve through the C ABI; returns dict(its, rel, conv, err, stats=(fused_steps, plain_dots, plain_axpys,
    fused_updates, plain_updates))"""
    from hypre_amd import binding as B
    from test_flexgmres_gpu import _ds
    g = C.c_void_p()
    lib.HYPRE_ParCSRLGMRESCreate(0, C.byref(g))
    lib.HYPRE_LGMRESSetKDim(g, k_dim)
    lib.HYPRE_LGMRESSetAugDim(g, aug_dim)
    lib.HYPRE_LGMRESSetTol(g, tol)
    lib.HYPRE_LGMRESSetMaxIter(g, max_iter)
    lib.HYPRE_LGMRESSetPrecond(g, *(precond or _ds(lib)))
    if fused is not None:
        lib.hypre_amd_LGMRESSetFusedUpdates(g, fused)
    if approx is not None:
        lib.hypre_amd_LGMRESSetApproxConstant(g, approx)
    lib.HYPRE_ParCSRLGMRESSetup(g, A, db, dx)
    lib.HYPRE_ParCSRLGMRESSolve(g, A, db, dx)
    err = lib.HYPRE_GetError()
    lib.HYPRE_ClearError(256)
    B.check()
    its, rel, conv = C.c_int(-1), C.c_double(-1.0), C.c_int(-1)
    st = [C.c_int(-1) for _ in range(5)]
    lib.HYPRE_LGMRESGetNumIterations(g, C.byref(its))
    lib.HYPRE_LGMRESGetFinalRelativeResidualNorm(g, C.byref(rel))
    lib.HYPRE_LGMRESGetConverged(g, C.byref(conv))
    lib.hypre_amd_LGMRESGetLaunchStats(g, *[C.byref(v) for v in st])
    lib.HYPRE_ParCSRLGMRESDestroy(g)
    return dict(its=its.value, rel=rel.value, conv=conv.value, err=err, stats=tuple(v.value for v in st))


def _numpy_lgmres(M, b, apply_pc, k_dim, aug_dim, tol, max_iter=1000):
    """LGMRES(k_dim - aug_dim, aug_dim) from x = 0 (Baker, Jessup, Manteuffel 2005, algorithm 2, right-preconditioned): a
    cycle of k_dim steps whose last ones, as many as there are error approximations z (aug_dim at most, the newest first),
    extend the Krylov basis by A M^-1 z instead of A M^-1 v; the correction is w = [V Z] y, x += M^-1 w, and w / |w| is the
    next z.  Dense operations throughout: A M^-1 z is computed, not recovered from residuals.  A cycle ends when the
    recurrence's residual meets the tolerance; the solve ends when the recomputed one does.
    Returns (iterations, ||b - M x|| / ||b||, x)."""
    n = len(b)
    x, it, bn = np.zeros(n), 0, np.linalg.norm(b)
    eps = tol * bn
    zs = []                                               # newest first
    op = lambda v: M @ apply_pc(v)
    while it < max_iter:
        r = b - M @ x
        beta = np.linalg.norm(r)
        if beta <= eps:
            break
        m = k_dim - len(zs)                               # Arnoldi steps of this cycle
        V, W = np.zeros((k_dim + 1, n)), np.zeros((k_dim, n))
        H, g = np.zeros((k_dim + 1, k_dim)), np.zeros(k_dim + 1)
        cs, sn = np.zeros(k_dim), np.zeros(k_dim)
        V[0], g[0], i = r / beta, beta, 0
        while i < k_dim and it < max_iter:
            it += 1
            W[i] = V[i] if i < m else zs[i - m]
            u = op(W[i])
            for j in range(i + 1):
                H[j, i] = V[j] @ u
                u = u - H[j, i] * V[j]
            H[i + 1, i] = np.linalg.norm(u)
            V[i + 1] = u / H[i + 1, i]
            for j in range(i):
                H[j, i], H[j + 1, i] = cs[j] * H[j, i] + sn[j] * H[j + 1, i], -sn[j] * H[j, i] + cs[j] * H[j + 1, i]
            d = np.hypot(H[i, i], H[i + 1, i])
            cs[i], sn[i] = H[i, i] / d, H[i + 1, i] / d
            H[i, i], H[i + 1, i] = d, 0.0
            g[i + 1], g[i] = -sn[i] * g[i], cs[i] * g[i]
            i += 1
            if abs(g[i]) <= eps:
                break
        w = np.linalg.solve(np.triu(H[:i, :i]), g[:i]) @ W[:i]
        x = x + apply_pc(w)
        if aug_dim > 0:
            zs = ([w / np.linalg.norm(w)] + zs)[:aug_dim]
    return it, float(np.linalg.norm(b - M @ x) / bn), x


def _expected_stats(its, k_dim, fused):
    """a converged solve with approx_constant 1 and aug_dim > 0: cycles of k_dim steps, the last one cut short"""
    from test_flexgmres_gpu import _gram_schmidt_steps
    steps, cycles = _gram_schmidt_steps(its, k_dim), -(-its // k_dim)
    if fused:
        return (steps, its, 0, 5 * (cycles - 1) + 2, 0)
    return (0, steps + its, steps, 0, 12 * (cycles - 1) + 3)


def _amg_693(lib, oracle=None):
    """the 7 x 9 x 11 operator with a PMIS / ext+i / l1-Jacobi hierarchy (serves multivectors), one cycle per application"""
    from hypre_amd import binding as B, ij
    opt = ij.IJOptions(n=(7, 9, 11), relax_type=18, coarsen_type=8, tol=1e-8, rhs="rand")
    A = ij.build_matrix(opt)
    M = B.csr_to_scipy(A.contents.diag)
    s = ij.create_amg(opt, memory_location=B.HYPRE_MEMORY_DEVICE)
    lib.HYPRE_BoomerAMGSetup(s, A, None, None)
    B.check()
    lib.hypre_ParCSRMatrixMigrate(A, B.HYPRE_MEMORY_DEVICE)
    amg = oracle.amg_from_solvers([s]) if oracle is not None else None
    lib.HYPRE_BoomerAMGSetTol(s, 0.0)
    lib.HYPRE_BoomerAMGSetMaxIter(s, 1)
    b, _ = ij.build_rhs_host(opt, A)
    return A, M, s, amg, b


# ---------------------------------------------------------------------------------------------------------------------
# 2. fusion changes nothing
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nv", [1, 3])
@pytest.mark.parametrize("pc", ["ds", "amg"])
def test_fused_and_plain_updates_give_the_same_bits_693_rows(gpu_lib, pc, nv):
    """The 7 x 9 x 11 Laplacian, the driver's -rhsrand right-hand side (nv 3: that and two more random columns as one
    multivector), k_dim 5, aug_dim 2, tol 1e-8: x bit for bit, the iteration count, the reported norm, and counters that
    say which path ran."""
    from hypre_amd import binding as B
    lib = gpu_lib
    A, M, s, _, b = _amg_693(lib)
    precond = (C.cast(lib.HYPRE_BoomerAMGSolve, C.c_void_p), None, s) if pc == "amg" else None
    make, fetch = B.parvec_from_numpy, B.parvec_to_numpy
    if nv > 1:
        b = np.column_stack([b] + [np.random.default_rng(c).uniform(-1, 1, 693) for c in range(1, nv)])
        make, fetch = B.parmultivec_from_numpy, B.parmultivec_to_numpy
    runs = {}
    for fused in (1, 0):
        db, dx = make(b), make(np.zeros_like(b))
        runs[fused] = _lgmres(lib, A, db, dx, fused=fused, precond=precond)
        runs[fused]["x"] = fetch(dx)
        lib.hypre_ParVectorDestroy(db); lib.hypre_ParVectorDestroy(dx)
    on, off = runs[1], runs[0]
    print(pc, "nv", nv, "fused", on["its"], repr(on["rel"]), on["stats"], "plain", off["its"], repr(off["rel"]), off["stats"])
    assert on["conv"] == 1 and on["err"] == 0 and on["its"] > 5 and on["rel"] <= 1e-8
    assert np.array_equal(_bits(on["x"]), _bits(off["x"]))
    assert on["its"] == off["its"] and on["rel"] == off["rel"] and on["conv"] == off["conv"]
    assert on["stats"] == _expected_stats(on["its"], 5, True)
    assert off["stats"] == _expected_stats(off["its"], 5, False)
    true = np.linalg.norm(b - M @ on["x"]) / np.linalg.norm(b)
    assert abs(true - on["rel"]) <= 1e-9 * true
    lib.HYPRE_BoomerAMGDestroy(s); lib.hypre_ParCSRMatrixDestroy(A)


# ---------------------------------------------------------------------------------------------------------------------
# 3. an independent yardstick
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k_dim,aug_dim", [(5, 2), (2, 1), (8, 3)])
def test_ds_lgmres_against_a_numpy_lgmres(gpu_lib, k_dim, aug_dim):
    """693 rows, diagonal scaling: several dozen cycles, so the fill phase and many truncations."""
    from hypre_amd import binding as B
    lib = gpu_lib
    A, M, s, _, b = _amg_693(lib)
    dinv = 1.0 / M.diagonal()
    db, dx = B.parvec_from_numpy(b), B.parvec_from_numpy(np.zeros(693))
    r = _lgmres(lib, A, db, dx, k_dim=k_dim, aug_dim=aug_dim, tol=1e-8)
    x = B.parvec_to_numpy(dx)
    oits, orel, xo = _numpy_lgmres(M, b, lambda v: dinv * v, k_dim, aug_dim, 1e-8)
    true = float(np.linalg.norm(b - M @ x) / np.linalg.norm(b))
    print("k_dim", k_dim, "aug_dim", aug_dim, "iterations", r["its"], oits, "reported", r["rel"], "from x", true, "numpy LGMRES", orel)
    assert r["conv"] == 1 and r["err"] == 0 and r["its"] == oits and r["its"] > 3 * k_dim
    assert abs(r["rel"] - orel) <= 1e-6 * orel
    assert abs(r["rel"] - true) <= 1e-9 * true and r["rel"] <= 1e-8
    for v in (db, dx):
        lib.hypre_ParVectorDestroy(v)
    lib.HYPRE_BoomerAMGDestroy(s); lib.hypre_ParCSRMatrixDestroy(A)


def test_amg_lgmres_against_a_numpy_lgmres(gpu_lib, oracle):
    """12^3 rows behind one V-cycle (the oracle's cycle in the numpy solver), k_dim 3 and aug_dim 1 so that the few
    iterations BoomerAMG leaves still cross restarts."""
    from hypre_amd import binding as B
    from test_flexgmres_gpu import _amg_problem
    lib = gpu_lib
    A, M, s, amg, b = _amg_problem(lib, oracle)
    n, k_dim, aug_dim, tol = len(b), 3, 1, 1e-8
    db, dx = B.parvec_from_numpy(b), B.parvec_from_numpy(np.zeros(n))
    r = _lgmres(lib, A, db, dx, k_dim=k_dim, aug_dim=aug_dim, tol=tol, precond=(C.cast(lib.HYPRE_BoomerAMGSolve, C.c_void_p), None, s))
    x = B.parvec_to_numpy(dx)

    def apply_pc(v):
        u = np.zeros(n)
        amg.cycle(np.ascontiguousarray(v), u, u_all_zeros=True)
        return u

    oits, orel, xo = _numpy_lgmres(M, b, apply_pc, k_dim, aug_dim, tol)
    true = float(np.linalg.norm(b - M @ x) / np.linalg.norm(b))
    print("iterations", r["its"], oits, "reported", r["rel"], "from x", true, "numpy LGMRES", orel)
    assert r["conv"] == 1 and r["its"] == oits and r["its"] > k_dim
    assert abs(r["rel"] - orel) <= 1e-6 * orel
    assert abs(r["rel"] - true) <= 1e-9 * true and r["rel"] <= tol
    for v in (db, dx):
        lib.hypre_ParVectorDestroy(v)
    lib.HYPRE_BoomerAMGDestroy(s); lib.hypre_ParCSRMatrixDestroy(A)


# ---------------------------------------------------------------------------------------------------------------------
# 4. reference goldens
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(GOLD))
def test_replay_lgmres_job_on_the_device(name):
    """Iteration count exactly; final relative residual within 1.5e-6 relative (the printed precision), the bar
    test_flexgmres_gpu.py holds the lines of the same `.saved` files to.  np 2 and np 4 are the multi-rank cases, the
    vector.jobs lines the multivector ones."""
    case = GOLD[name]
    its, rel = _closing_lines(_worker(["job", name], case["np"]))
    exp = case["expect"]
    print(name, "iterations", its, "norm", rel, "expected", exp)
    assert its == exp["iterations"]
    assert abs(rel - exp["rel_resid"]) <= 1.5e-6 * exp["rel_resid"]


# ---------------------------------------------------------------------------------------------------------------------
# 5. two ranks
# ---------------------------------------------------------------------------------------------------------------------
def test_amg_lgmres_on_two_ranks_is_the_one_rank_solve():
    """A hierarchy that does not depend on the partition (the sequential random numbers of -pmis1, direct interpolation
    without truncation, three levels, Jacobi with the plain diagonal; slabs in z keep the row numbering: see
    test_dist_golden.py), so the two solves differ in the order of their sums alone.  k_dim 3, aug_dim 1."""
    opts = dict(n=[14, 13, 12], solver=3, lgmres=1, k_dim=3, aug_dim=1, coarsen_type=9, interp_type=3, relax_type=7, relax_wt=0.8,
                max_levels=3, P_max_elmts=0, rhs="one")
    one = _closing_lines(_worker(["options", json.dumps(opts)], 1))
    two = _closing_lines(_worker(["options", json.dumps(dict(opts, P=[1, 1, 2]))], 2))
    print("one rank", one, "two ranks", two)
    assert one[0] == two[0] and one[0] > 3
    assert abs(one[1] - two[1]) <= 1.5e-6 * one[1] and one[1] <= 1e-8


# ---------------------------------------------------------------------------------------------------------------------
# 6. edges
# ---------------------------------------------------------------------------------------------------------------------
def test_edges(gpu_lib):
    from hypre_amd import binding as B
    from test_flexgmres_gpu import _ds, _operator
    lib = gpu_lib
    _, A, _, _ = _operator(lib, n=(8, 8, 8))
    db, dx = B.parvec_from_numpy(np.ones(512)), B.parvec_from_numpy(np.zeros(512))
    # the iteration limit inside the first augmentation step of the third cycle (5 | 4 + 1 | 3 + 2): HYPRE_ERROR_CONV (256) ...
    r = _lgmres(lib, A, db, dx, tol=1e-30, max_iter=14)
    assert r["err"] & 256 and r["its"] == 14 and r["conv"] == 0 and 0.0 < r["rel"] < 1.0
    x14 = B.parvec_to_numpy(dx)
    # ... but only when a tolerance is set (lgmres.c:918); the iterate is the same
    dx2 = B.parvec_from_numpy(np.zeros(512))
    r0 = _lgmres(lib, A, db, dx2, tol=0.0, max_iter=14)
    assert r0["err"] == 0 and r0["its"] == 14 and r0["rel"] == r["rel"]
    assert np.array_equal(_bits(B.parvec_to_numpy(dx2)), _bits(x14)) and np.any(x14 != 0.0)
    # b = 0, x = 0: the residual is exactly zero, Solve returns at once and stores nothing
    dz, dx0 = B.parvec_from_numpy(np.zeros(512)), B.parvec_from_numpy(np.zeros(512))
    r = _lgmres(lib, A, dz, dx0)
    assert r["err"] == 0 and r["its"] == 0 and r["rel"] == 0.0 and r["conv"] == 0 and r["stats"] == (0, 0, 0, 0, 0)
    assert B.parvec_to_numpy(dx0).tobytes() == np.zeros(512).tobytes()
    # ... also after a solve that stored something: count and norm stay those of that solve
    g = C.c_void_p()
    lib.HYPRE_ParCSRLGMRESCreate(0, C.byref(g))
    lib.HYPRE_LGMRESSetKDim(g, 5)
    lib.HYPRE_LGMRESSetAugDim(g, 2)
    lib.HYPRE_LGMRESSetTol(g, 1e-8)
    lib.HYPRE_LGMRESSetPrecond(g, *_ds(lib))
    lib.HYPRE_ParCSRLGMRESSetup(g, A, db, dx0)
    assert lib.HYPRE_ParCSRLGMRESSolve(g, A, db, dx0) == 0
    k, rel, rel2, res = C.c_int(), C.c_double(), C.c_double(), C.c_void_p()
    lib.HYPRE_LGMRESGetNumIterations(g, C.byref(k))
    lib.HYPRE_LGMRESGetFinalRelativeResidualNorm(g, C.byref(rel))
    first = k.value
    assert first > 5 and 0.0 < rel.value <= 1e-8
    # GetResidual: the work vector that holds b - A x of the last check
    lib.HYPRE_ParCSRLGMRESGetResidual(g, C.byref(res))
    rv = B.parvec_to_numpy(C.cast(res, C.POINTER(B.ParVector)))
    assert abs(np.linalg.norm(rv) / np.sqrt(512.0) - rel.value) <= 1e-12 * rel.value
    dx1 = B.parvec_from_numpy(np.zeros(512))
    assert lib.HYPRE_LGMRESSolve(g, A, dz, dx1) == 0
    lib.HYPRE_ParCSRLGMRESGetNumIterations(g, C.byref(k))
    lib.HYPRE_ParCSRLGMRESGetFinalRelativeResidualNorm(g, C.byref(rel2))
    assert k.value == first and rel2.value == rel.value
    # SetKDim, then SetAugDim, without a new Setup
    lib.HYPRE_LGMRESSetKDim(g, 7)
    assert lib.HYPRE_ParCSRLGMRESSolve(g, A, db, dx1) != 0
    assert b"HYPRE_ParCSRLGMRESSetup after HYPRE_LGMRESSetKDim" in lib.hypre_amd_LastErrorMessage()
    lib.HYPRE_ClearAllErrors()
    lib.HYPRE_LGMRESSetKDim(g, 5)
    lib.HYPRE_LGMRESSetAugDim(g, 3)
    assert lib.HYPRE_ParCSRLGMRESSolve(g, A, db, dx1) != 0
    assert b"HYPRE_ParCSRLGMRESSetup after HYPRE_LGMRESSetAugDim" in lib.hypre_amd_LastErrorMessage()
    lib.HYPRE_ClearAllErrors()
    assert B.parvec_to_numpy(dx1).tobytes() == np.zeros(512).tobytes()          # nothing was solved
    lib.HYPRE_ParCSRLGMRESSetup(g, A, db, dx1)
    assert lib.HYPRE_ParCSRLGMRESSolve(g, A, db, dx1) == 0
    # a host operand
    hb = lib.hypre_ParVectorCreate(0, 512, None)
    lib.hypre_ParVectorInitialize_v2(hb, B.HYPRE_MEMORY_HOST)
    before = B.parvec_to_numpy(dx1)
    assert lib.HYPRE_ParCSRLGMRESSolve(g, A, hb, dx1) != 0
    assert b"not in device memory" in lib.hypre_amd_LastErrorMessage()
    lib.HYPRE_ClearAllErrors()
    assert np.array_equal(B.parvec_to_numpy(dx1), before)
    # the switches take 0 and 1
    for setter in (lib.hypre_amd_LGMRESSetFusedUpdates, lib.hypre_amd_LGMRESSetApproxConstant):
        assert setter(g, 0) == 0 and setter(g, 1) == 0
        setter(g, 2)
        assert lib.HYPRE_GetError() & 4 and lib.HYPRE_GetErrorArg() == 2
        lib.HYPRE_ClearAllErrors()
    lib.HYPRE_ParCSRLGMRESDestroy(g)
    for v in (db, dx, dx2, dz, dx0, dx1, hb):
        lib.hypre_ParVectorDestroy(v)
    lib.hypre_ParCSRMatrixDestroy(A)


def test_approx_constant_off_and_aug_dim_zero(gpu_lib):
    """aug_dim 0 is GMRES: the iteration count, the norm and the iterate of HYPRE_ParCSRGMRES on the same system.
    approx_constant 0 (k_dim - aug_dim Arnoldi steps from the first cycle on): fused and plain agree bit for bit there
    too, and the reported norm is that of the iterate."""
    from hypre_amd import binding as B, ij
    from test_flexgmres_gpu import _operator
    lib = gpu_lib
    opt, A, M, _ = _operator(lib, n=(7, 9, 11), rhs="rand")
    b, _ = ij.build_rhs_host(opt, A)
    db, dx = B.parvec_from_numpy(b), B.parvec_from_numpy(np.zeros(693))
    r = _lgmres(lib, A, db, dx, k_dim=5, aug_dim=0, tol=1e-8)
    dx2 = B.parvec_from_numpy(np.zeros(693))
    gits, grel = ij.solve_ds_gmres(ij.IJOptions(k_dim=5, tol=1e-8), A, db, dx2)
    print("aug_dim 0:", r["its"], r["rel"], "GMRES:", gits, grel)
    assert r["conv"] == 1 and r["its"] == gits and r["rel"] == grel
    assert np.array_equal(_bits(B.parvec_to_numpy(dx)), _bits(B.parvec_to_numpy(dx2)))
    runs = []
    for fused in (1, 0):
        dx3 = B.parvec_from_numpy(np.zeros(693))
        runs.append(_lgmres(lib, A, db, dx3, k_dim=5, aug_dim=2, tol=1e-8, approx=0, fused=fused))
        runs[-1]["x"] = B.parvec_to_numpy(dx3)
        lib.hypre_ParVectorDestroy(dx3)
    true = float(np.linalg.norm(b - M @ runs[0]["x"]) / np.linalg.norm(b))
    print("approx_constant 0:", runs[0]["its"], runs[0]["rel"], true)
    assert runs[0]["conv"] == 1 and runs[0]["its"] == runs[1]["its"] and runs[0]["rel"] == runs[1]["rel"]
    assert np.array_equal(_bits(runs[0]["x"]), _bits(runs[1]["x"]))
    assert abs(runs[0]["rel"] - true) <= 1e-9 * true and runs[0]["rel"] <= 1e-8
    for v in (db, dx, dx2):
        lib.hypre_ParVectorDestroy(v)
    lib.hypre_ParCSRMatrixDestroy(A)
