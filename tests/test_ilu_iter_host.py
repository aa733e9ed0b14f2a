"""Iterative triangular solves of ILU (the reference's tri_solve 0, hypre_ILUSolveLUIter) as far as no GPU is needed: the host
path (ilu::solve_iter, reached through HYPRE_MEMORY_HOST operands) against a restatement of the specification written here
in plain float64 Python loops, bit for bit; nilpotency; the C interface; the driver's options; and the stand-alone host
program under the sanitizers.

The specification, in the permuted index space of the factors, r the right-hand side:
    y^0 = 0;  y^k_i = r_i - sum_j L_ij y^(k-1)_j          k = 1 .. lower
    z^0 = 0;  z^k_i = Dinv_i (y_i - sum_j U_ij z^(k-1)_j)  k = 1 .. upper
    u += z
with every sum started at +0.0, the products added one by one in stored order, each product and each sum rounded; without a
lower or without an upper sweep u stays as it is."""
import ctypes as C
import io

import numpy as np
import pytest
import scipy.sparse as sp

from test_ilu_host import _parameters, csr_i32, difconv_block, grid_5pt, library_factors, new_ilu
from util import laplace_3d, parcsr, run_host_program

PAIRS = [(0, 0), (0, 3), (3, 0), (1, 1), (1, 2), (2, 1), (5, 5), (3, 7)]


# ---------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------
def _rows(T):
    """[(columns, values)] of a csr matrix in stored order, as Python ints and floats"""
    return [(T.indices[T.indptr[i]:T.indptr[i + 1]].tolist(), T.data[T.indptr[i]:T.indptr[i + 1]].tolist()) for i in range(T.shape[0])]


def sweeps_reference(perm, Lm, dinv, Um, r, lower, upper):
    """z, in the numbering of the vectors, by the specification above: Python floats are IEEE doubles, `s + a * x` rounds the
    product and then the sum"""
    n = len(perm)
    z_out = np.zeros(n)
    if lower == 0 or upper == 0:
        return z_out
    perm, dinv, rp = [int(p) for p in perm], [float(d) for d in dinv], [float(r[int(p)]) for p in perm]
    Lr, Ur = _rows(Lm), _rows(Um)
    y = [0.0] * n
    for _ in range(lower):
        new = [0.0] * n
        for i in range(n):
            s = 0.0
            for c, a in zip(*Lr[i]):
                s = s + a * y[c]
            new[i] = rp[i] - s
        y = new
    z = [0.0] * n
    for _ in range(upper):
        new = [0.0] * n
        for i in range(n):
            s = 0.0
            for c, a in zip(*Ur[i]):
                s = s + a * z[c]
            new[i] = dinv[i] * (y[i] - s)
        z = new
    for i in range(n):
        z_out[perm[i]] = z[i]
    return z_out


def substitution_reference(perm, Lm, dinv, Um, r):
    """forward and backward substitution in the same association: the sum from +0.0, then r_i - sum and Dinv_i (y_i - sum)"""
    n = len(perm)
    perm, dinv = [int(p) for p in perm], [float(d) for d in dinv]
    Lr, Ur = _rows(Lm), _rows(Um)
    y, z = [0.0] * n, [0.0] * n
    for i in range(n):
        s = 0.0
        for c, a in zip(*Lr[i]):
            s = s + a * y[c]
        y[i] = float(r[perm[i]]) - s
    for i in range(n - 1, -1, -1):
        s = 0.0
        for c, a in zip(*Ur[i]):
            s = s + a * z[c]
        z[i] = dinv[i] * (y[i] - s)
    out = np.zeros(n)
    for i in range(n):
        out[perm[i]] = z[i]
    return out


def same_bits(what, got, want):
    assert got.shape == want.shape, what
    bad = np.flatnonzero(got.view(np.int64) != want.view(np.int64))
    assert bad.size == 0, (what, bad[:5], got[bad[:5]], want[bad[:5]])


def set_sweeps(lib, s, lower, upper, on=1):
    assert lib.hypre_amd_ILUSetIterativeTriSolve(s, on) == 0
    assert lib.HYPRE_ILUSetLowerJacobiIters(s, lower) == 0
    assert lib.HYPRE_ILUSetUpperJacobiIters(s, upper) == 0


def iterative_stats(lib, s):
    i = [C.c_int(-9) for _ in range(4)]
    p = [C.c_longlong(-9) for _ in range(2)]
    assert lib.hypre_amd_ILUGetIterativeStats(s, *[C.byref(v) for v in i + p]) == 0
    return dict(zip(("on", "lower", "upper", "launches", "padded_L", "padded_U"), (v.value for v in i + p)))


def apply_factors(lib, B, s, f, u0, location):
    fv, uv = B.parvec_from_numpy(f, location=location), B.parvec_from_numpy(u0, location=location)
    assert lib.hypre_amd_ILUApplyFactors(s, fv, uv) == 0
    B.check()
    u = B.parvec_to_numpy(uv)
    for v in (fv, uv):
        lib.hypre_ParVectorDestroy(v)
    return u


def solve_once(lib, B, s, A, f, u0, location):
    lib.HYPRE_ILUSetMaxIter(s, 1)
    lib.HYPRE_ILUSetTol(s, 0.0)
    fv, uv = B.parvec_from_numpy(f, location=location), B.parvec_from_numpy(u0, location=location)
    assert lib.HYPRE_ILUSolve(s, A, fv, uv) == 0
    B.check()
    u = B.parvec_to_numpy(uv)
    for v in (fv, uv):
        lib.hypre_ParVectorDestroy(v)
    return u


def cases():
    return {"17x13 ilu0": (grid_5pt(17, 13), 0, 0), "17x13 ilu0 rcm": (grid_5pt(17, 13), 0, 1), "17x13 ilu1": (grid_5pt(17, 13), 1, 0),
            "17x13 ilu1 rcm": (grid_5pt(17, 13), 1, 1), "6^3 27-point ilu1": (laplace_3d(6, 6, 6, stencil=27), 1, 1),
            "convection-diffusion": (difconv_block(7, 6, 5), 0, 1), "diagonal": (sp.diags(np.linspace(1.5, 3.0, 70)).tocsr(), 0, 1),
            "one row": (sp.csr_matrix(np.array([[2.5]])), 0, 1), "no row": (sp.csr_matrix((0, 0)), 0, 1)}


_reference_cache = {}


def references(lib, name):
    """(matrix, lfil, reordering, f, u0, {(lower, upper): z of the restatement}) of a case, computed once from the library's
    own factors (held to a dense restatement by test_ilu_host.py) and shared by the host and the device tests"""
    if name not in _reference_cache:
        from hypre_amd import binding as B
        M, lfil, reordering = cases()[name]
        M = csr_i32(M)
        n = M.shape[0]
        rng = np.random.default_rng(len(name) + 31 * n)
        f, u0 = rng.standard_normal(n), rng.standard_normal(n)
        A = parcsr(lib, B, M, B.HYPRE_MEMORY_HOST)
        s = new_ilu(lib, lfil=lfil, reordering=reordering)
        assert lib.HYPRE_ILUSetup(s, A, None, None) == 0
        perm, Lm, dinv, Um = library_factors(lib, s)
        z = {p: sweeps_reference(perm, Lm, dinv, Um, f, *p) for p in PAIRS}
        lib.HYPRE_ILUDestroy(s)
        lib.hypre_ParCSRMatrixDestroy(A)
        _reference_cache[name] = (M, lfil, reordering, f, u0, z)
    return _reference_cache[name]


# ---------------------------------------------------------------------------------------------------------------------
# the host path against the restatement
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases()))
def test_host_sweeps_are_the_restatement_bit_for_bit(lib, name):
    from hypre_amd import binding as B
    HOST = B.HYPRE_MEMORY_HOST
    M, lfil, reordering, f, u0, want = references(lib, name)
    n = M.shape[0]
    A = parcsr(lib, B, M, HOST)
    s = new_ilu(lib, lfil=lfil, reordering=reordering)
    set_sweeps(lib, s, 5, 5)
    assert lib.HYPRE_ILUSetup(s, A, None, None) == 0
    for lower, upper in PAIRS:
        set_sweeps(lib, s, lower, upper)
        same_bits((name, lower, upper, "ApplyFactors"), apply_factors(lib, B, s, f, u0, HOST), u0 + want[(lower, upper)])
        # a Solve of one application from a zero iterate: the host residual f - A 0 is f itself
        same_bits((name, lower, upper, "Solve"), solve_once(lib, B, s, A, f, np.zeros(n), HOST), np.zeros(n) + want[(lower, upper)])
        if lower == 0 or upper == 0:
            same_bits((name, lower, upper, "u untouched"), apply_factors(lib, B, s, f, u0, HOST), u0)
        assert iterative_stats(lib, s)["launches"] == 0
    if n > 1 and name != "diagonal":
        # the sweeps are not the direct solve: (1, 1) is Dinv r alone
        assert not np.array_equal(want[(1, 1)], want[(5, 5)])
    lib.HYPRE_ILUDestroy(s)
    lib.hypre_ParCSRMatrixDestroy(A)


def tridiagonal_300():
    rng = np.random.default_rng(1)
    n = 300
    return csr_i32(sp.diags([rng.uniform(-1, -0.5, n - 1), rng.uniform(3, 4, n), rng.uniform(-1, -0.5, n - 1)], [-1, 0, 1]).tocsr())


def nilpotency(lib, location, migrate=False):
    """300 levels per factor: L and U are nilpotent of index 300, so 300 sweeps are the exact solve and three more change
    nothing — identical bits, no tolerance — and both are substitution written in the sweeps' association"""
    from hypre_amd import binding as B
    M = tridiagonal_300()
    rng = np.random.default_rng(2)
    f, u0 = rng.standard_normal(300), rng.standard_normal(300)
    A = parcsr(lib, B, M, B.HYPRE_MEMORY_HOST)
    s = new_ilu(lib, reordering=0)
    assert lib.HYPRE_ILUSetup(s, A, None, None) == 0
    st = [C.c_int() for _ in range(6)]
    lib.hypre_amd_ILUGetSolveStats(s, *[C.byref(v) for v in st])
    assert (st[0].value, st[1].value) == (300, 300)
    perm, Lm, dinv, Um = library_factors(lib, s)
    want = u0 + substitution_reference(perm, Lm, dinv, Um, f)
    if migrate:
        lib.hypre_ParCSRMatrixMigrate(A, location)
        solve_once(lib, B, s, A, f, u0, location)                     # brings the factors to the device
    out = {}
    for k in (300, 303):
        set_sweeps(lib, s, k, k)
        out[k] = apply_factors(lib, B, s, f, u0, location)
    stats = iterative_stats(lib, s)
    same_bits("300 against 303 sweeps", out[300], out[303])
    same_bits("300 sweeps against substitution", out[300], want)
    set_sweeps(lib, s, 5, 5)
    assert not np.array_equal(apply_factors(lib, B, s, f, u0, location), want)
    lib.HYPRE_ILUDestroy(s)
    lib.hypre_ParCSRMatrixDestroy(A)
    return stats


def test_sweeps_past_the_nilpotency_index_are_the_exact_solve(lib):
    from hypre_amd import binding as B
    nilpotency(lib, B.HYPRE_MEMORY_HOST)


# ---------------------------------------------------------------------------------------------------------------------
# C interface and driver
# ---------------------------------------------------------------------------------------------------------------------
def test_setters_getters_defaults_and_refusals(lib):
    lib.HYPRE_ClearAllErrors()
    s = C.c_void_p()
    assert lib.HYPRE_ILUCreate(C.byref(s)) == 0
    assert iterative_stats(lib, s) == dict(on=0, lower=5, upper=5, launches=0, padded_L=0, padded_U=0)
    assert _parameters(lib, s)["tri_solve"] == 1
    assert lib.HYPRE_ILUSetLowerJacobiIters(s, 3) == 0 and lib.HYPRE_ILUSetUpperJacobiIters(s, 7) == 0
    assert _parameters(lib, s)["tri_solve"] == 1                      # the counts alone switch nothing
    assert lib.hypre_amd_ILUSetIterativeTriSolve(s, 1) == 0
    assert iterative_stats(lib, s) == dict(on=1, lower=3, upper=7, launches=0, padded_L=0, padded_U=0)
    assert _parameters(lib, s)["tri_solve"] == 0
    assert lib.HYPRE_ILUSetLowerJacobiIters(s, 0) == 0 and lib.HYPRE_ILUSetUpperJacobiIters(s, 0) == 0
    assert (iterative_stats(lib, s)["lower"], iterative_stats(lib, s)["upper"]) == (0, 0)
    assert lib.HYPRE_GetError() == 0
    for call in (lambda: lib.HYPRE_ILUSetLowerJacobiIters(s, -1), lambda: lib.HYPRE_ILUSetUpperJacobiIters(s, -1),
                 lambda: lib.hypre_amd_ILUSetIterativeTriSolve(s, 2), lambda: lib.hypre_amd_ILUSetIterativeTriSolve(s, -1)):
        assert call() != 0
        assert lib.HYPRE_GetError() & 4 and lib.HYPRE_GetErrorArg() == 2
        lib.HYPRE_ClearAllErrors()
    assert iterative_stats(lib, s) == dict(on=1, lower=0, upper=0, launches=0, padded_L=0, padded_U=0)
    # HYPRE_ILUSetTriSolve goes on refusing 0 and says where the capability lives; accepting 1 does not switch the sweeps off
    assert lib.HYPRE_ILUSetTriSolve(s, 0) != 0 and b"hypre_amd_ILUSetIterativeTriSolve" in lib.hypre_amd_LastErrorMessage()
    lib.HYPRE_ClearAllErrors()
    assert lib.hypre_amd_ILUSetIterativeTriSolve(s, 0) == 0
    assert _parameters(lib, s)["tri_solve"] == 1 and iterative_stats(lib, s)["on"] == 0
    for fn in (lib.HYPRE_ILUSetLowerJacobiIters, lib.HYPRE_ILUSetUpperJacobiIters, lib.hypre_amd_ILUSetIterativeTriSolve):
        assert fn(None, 1) != 0 and lib.HYPRE_GetErrorArg() == 1
        lib.HYPRE_ClearAllErrors()
    assert lib.hypre_amd_ILUGetIterativeStats(None, None, None, None, None, None, None) != 0
    lib.HYPRE_ClearAllErrors()
    assert lib.hypre_amd_ILUGetIterativeStats(s, None, None, None, None, None, None) == 0
    lib.HYPRE_ILUDestroy(s)
    assert lib.HYPRE_GetError() == 0


def test_padded_entries_are_counted_at_setup(lib):
    """every slice of 64 rows of the level order is as long as its longest row: the count from the library's own factors and
    levels, restated here"""
    from hypre_amd import binding as B
    M = csr_i32(sp.block_diag([sp.diags(np.linspace(1.0, 2.0, 70)), laplace_3d(6, 6, 6, stencil=27)]).tocsr())
    A = parcsr(lib, B, M, B.HYPRE_MEMORY_HOST)
    s = new_ilu(lib, lfil=1, reordering=0)
    assert lib.HYPRE_ILUSetup(s, A, None, None) == 0
    perm, Lm, dinv, Um = library_factors(lib, s)
    n = M.shape[0]

    def padded(T, forward):
        level = np.zeros(n, dtype=np.int64)
        for i in (range(n) if forward else range(n - 1, -1, -1)):
            cols = T.indices[T.indptr[i]:T.indptr[i + 1]]
            level[i] = level[cols].max() + 1 if len(cols) else 0
        order = np.argsort(level, kind="stable")
        lens = np.diff(T.indptr)[order]
        return int(sum(64 * lens[k:k + 64].max() for k in range(0, n, 64)))

    st = iterative_stats(lib, s)
    assert (st["padded_L"], st["padded_U"]) == (padded(Lm, True), padded(Um, False))
    assert st["padded_L"] >= Lm.nnz and st["padded_U"] >= Um.nnz and st["padded_L"] % 64 == 0
    assert np.diff(Lm.indptr).max() >= 30 and np.diff(Lm.indptr).min() == 0       # empty, short and long rows (31 at the most)
    lib.HYPRE_ILUDestroy(s)
    lib.hypre_ParCSRMatrixDestroy(A)


def test_the_switch_flips_between_two_solves_of_one_setup(lib):
    from hypre_amd import binding as B
    HOST = B.HYPRE_MEMORY_HOST
    M, lfil, reordering, f, u0, want = references(lib, "17x13 ilu1 rcm")
    A = parcsr(lib, B, M, HOST)
    s = new_ilu(lib, lfil=lfil, reordering=reordering)
    assert lib.HYPRE_ILUSetup(s, A, None, None) == 0
    direct = apply_factors(lib, B, s, f, u0, HOST)
    direct_solve = solve_once(lib, B, s, A, f, u0, HOST)
    set_sweeps(lib, s, 3, 7)
    same_bits("sweeps after a direct solve", apply_factors(lib, B, s, f, u0, HOST), u0 + want[(3, 7)])
    assert lib.hypre_amd_ILUSetIterativeTriSolve(s, 0) == 0
    same_bits("direct again", apply_factors(lib, B, s, f, u0, HOST), direct)
    same_bits("direct Solve again", solve_once(lib, B, s, A, f, u0, HOST), direct_solve)
    assert not np.array_equal(direct, u0 + want[(3, 7)])
    lib.HYPRE_ILUDestroy(s)
    lib.hypre_ParCSRMatrixDestroy(A)


def test_the_drivers_options_reach_the_solver(lib):
    from hypre_amd import binding as B, ij
    d = ij.IJOptions()
    assert (d.ilu_iterative, d.ilu_ljac_iters, d.ilu_ujac_iters) == (0, 5, 5)
    for sid in (80, 81, 82):
        opt = ij.check_options(ij.IJOptions(solver=sid, ilu_iterative=1, ilu_ljac_iters=3, ilu_ujac_iters=4))
        s = ij.create_ilu(opt, preconditioner=sid != 80)
        st = iterative_stats(lib, s)
        assert (st["on"], st["lower"], st["upper"]) == (1, 3, 4) and _parameters(lib, s)["tri_solve"] == 0
        lib.HYPRE_ILUDestroy(s)
    s = ij.create_ilu(ij.IJOptions(solver=80))
    assert iterative_stats(lib, s)["on"] == 0 and _parameters(lib, s)["tri_solve"] == 1
    lib.HYPRE_ILUDestroy(s)
    for bad in (dict(ilu_iterative=2), dict(ilu_iterative=1, ilu_ljac_iters=-1), dict(ilu_iterative=1, ilu_ujac_iters=-1)):
        with pytest.raises(SystemExit):
            ij.check_options(ij.IJOptions(solver=80, **bad))
    # solver 80 in host memory, 8^3 7-point: both ways reach 1e-8; five sweeps a factor are the weaker preconditioner
    counts = {}
    for it in (0, 1):
        opt = ij.check_options(ij.IJOptions(solver=80, n=(8, 8, 8), tol=1e-8, max_iter=200, ilu_iterative=it))
        out = io.StringIO()
        its, rel = ij.run_ilu(opt, ij.build_matrix(opt), out=out, memory_location=B.HYPRE_MEMORY_HOST)
        assert rel <= 1e-8 and "hypre_ILU Iterations = %d" % its in out.getvalue()
        counts[it] = its
    print(counts)
    assert 0 < counts[0] <= counts[1] < 200


# ---------------------------------------------------------------------------------------------------------------------
# the host code alone, under the address and undefined-behaviour sanitizers
# ---------------------------------------------------------------------------------------------------------------------
def test_sweeps_and_slices_run_clean_under_the_sanitizers(tmp_path):
    out = run_host_program("host/ilu_iter_host_check.cpp", tmp_path)
    assert "ilu iter host check ok" in out
