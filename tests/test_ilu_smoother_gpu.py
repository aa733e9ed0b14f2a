"""ILU as a BoomerAMG level smoother on the device (smooth_type 5, and 15 with the conjugate-gradient acceleration around it).

One cycle and whole solves are compared with the numpy restatement of ilu_smoother_reference.py, built on the device solver's
own hierarchy with stand-alone host ILU objects as the level smoothers.  The yardstick of a cycle is the rounding of a float64
cycle itself: max|u_dev - u_ld| <= 16 max|u_64 - u_ld|, u_ld the long-double restatement and u_64 the float64 one (16: a device
row sum in another order on each of at most six levels).  The fused acceleration is held to the unfused call sequence bit for
bit and to zero read-backs, its vector kernels to numpy with the spelled-out roundings bit for bit."""
import contextlib
import ctypes as C

import numpy as np
import pytest

from ilu_smoother_reference import LD, Restatement, clear_of_tolerance, fma

pytestmark = pytest.mark.gpu

HOST, DEVICE = 0, 1
OPERATORS = {
    "7pt": dict(problem="laplacian", n=(12, 11, 10)),
    "27pt": dict(problem="27pt", n=(9, 8, 7)),
    "difconv": dict(problem="difconv", n=(10, 10, 10), a=(10.0, 10.0, 10.0)),
}


def _case(name, op, smooth_type, levels, sweeps=1, iterative=0, lower=5, upper=5, lfil=0, mu=1, ns=1, solver=0, **kw):
    return dict(name=name, op=op, smooth_type=smooth_type, smooth_num_levels=levels, smooth_num_sweeps=sweeps, iterative=iterative,
                lower=lower, upper=upper, lfil=lfil, mu=mu, ns=ns, solver=solver, **kw)


# every value of the issue's list appears at least once
CYCLE_CASES = [
    _case("7pt-5-L1", "7pt", 5, 1),
    _case("7pt-5-L2-s2-iter33", "7pt", 5, 2, sweeps=2, iterative=1, lower=3, upper=3),
    _case("7pt-5-all-lfil1", "7pt", 5, 25, lfil=1),
    _case("7pt-15-L1", "7pt", 15, 1),
    _case("7pt-15-L2-s2", "7pt", 15, 2, sweeps=2),
    _case("7pt-15-all-s2-iter11", "7pt", 15, 25, sweeps=2, iterative=1, lower=1, upper=1),
    _case("7pt-15-L2-s2-ns2", "7pt", 15, 2, sweeps=2, ns=2),
    _case("7pt-15-L2-s2-W", "7pt", 15, 2, sweeps=2, mu=2),
    _case("27pt-5-L2-iter11", "27pt", 5, 2, iterative=1, lower=1, upper=1),
    _case("27pt-15-all-s2-lfil1", "27pt", 15, 25, sweeps=2, lfil=1),
    _case("27pt-15-L1-s2-iter33", "27pt", 15, 1, sweeps=2, iterative=1, lower=3, upper=3),
    _case("difconv-5-L1", "difconv", 5, 1),
    _case("difconv-5-all-s2-lfil1", "difconv", 5, 25, sweeps=2, lfil=1),
    _case("difconv-5-L2-iter33", "difconv", 5, 2, iterative=1, lower=3, upper=3),
]
SOLVE_CASES = [
    _case("solve-7pt-5-L2", "7pt", 5, 2, seed=1),
    _case("solve-7pt-15-all-s2", "7pt", 15, 25, sweeps=2, seed=2),
    _case("solve-27pt-15-L1-iter33", "27pt", 15, 1, sweeps=2, iterative=1, lower=3, upper=3, seed=1),
    _case("solve-difconv-5-all", "difconv", 5, 25, seed=7, beats_jacobi=True),
    _case("pcg-7pt-5-L2", "7pt", 5, 2, solver=1, seed=1),
    _case("pcg-27pt-15-all", "27pt", 15, 25, solver=1, seed=1),
]


def options_of(case):
    from hypre_amd import ij
    kw = dict(OPERATORS[case["op"]])
    kw.update(coarsen_type=8, relax_type=18, cycle_type=case["mu"], num_sweeps=case["ns"], solver=case["solver"], tol=1e-8,
              smooth_type=case["smooth_type"], smooth_num_levels=case["smooth_num_levels"], smooth_num_sweeps=case["smooth_num_sweeps"],
              ilu_lfil=case["lfil"], ilu_iterative=case["iterative"], ilu_ljac_iters=case["lower"], ilu_ujac_iters=case["upper"])
    if case["smooth_num_levels"] == 0:
        kw.update(smooth_type=6)
    return ij.check_options(ij.IJOptions(**kw))


def restatement_of(lib, oracle, s, case, levels=None):
    from hypre_amd import binding as B
    return Restatement(lib, B, oracle, s, case["smooth_type"], case["smooth_num_levels"] if levels is None else levels,
                       smooth_num_sweeps=case["smooth_num_sweeps"], lfil=case["lfil"], iterative=case["iterative"], lower=case["lower"],
                       upper=case["upper"])


def rhs_of(case, n):
    return np.random.default_rng(case.get("seed", 1)).standard_normal(n)


@contextlib.contextmanager
def host_hierarchy(lib, oracle, case):
    """the case's hierarchy set up in host memory and its restatement (no GPU): (restatement, rows)"""
    from hypre_amd import ij
    opt = options_of(case)
    A = ij.build_matrix(opt)
    s = ij.create_amg(opt, memory_location=HOST)
    assert lib.HYPRE_BoomerAMGSetup(s, A, None, None) == 0
    R = restatement_of(lib, oracle, s, case)
    try:
        yield R, int(A.contents.diag.contents.num_rows)
    finally:
        R.close()
        lib.HYPRE_BoomerAMGDestroy(s)
        lib.hypre_ParCSRMatrixDestroy(A)


@contextlib.contextmanager
def device_hierarchy(lib, case):
    from hypre_amd import binding as B, ij
    opt = options_of(case)
    A = ij.build_matrix(opt)
    s = ij.create_amg(opt, memory_location=DEVICE)
    assert lib.HYPRE_BoomerAMGSetup(s, A, None, None) == 0
    B.check()
    lib.hypre_ParCSRMatrixMigrate(A, DEVICE)
    try:
        yield opt, s, A, int(A.contents.diag.contents.num_rows)
    finally:
        lib.HYPRE_BoomerAMGDestroy(s)
        lib.hypre_ParCSRMatrixDestroy(A)
        lib.hypre_amd_SetSmootherFusion(1)
        lib.HYPRE_ClearAllErrors()


def one_cycle(lib, s, A, f, u0, zero):
    from hypre_amd import binding as B
    df, du = B.parvec_from_numpy(f), B.parvec_from_numpy(u0)
    if zero:
        lib.hypre_ParVectorSetZeros(du)
    lib.HYPRE_BoomerAMGSetTol(s, 0.0)
    lib.HYPRE_BoomerAMGSetMaxIter(s, 1)
    lib.HYPRE_BoomerAMGSolve(s, A, df, du)
    B.check()
    u = B.parvec_to_numpy(du)
    for v in (df, du):
        lib.hypre_ParVectorDestroy(v)
    assert np.all(np.isfinite(u))
    return u


def smoother_stats(lib, s):
    v = [C.c_int(-7) for _ in range(5)]
    assert lib.hypre_amd_BoomerAMGGetSmootherStats(s, *[C.byref(x) for x in v]) == 0
    return dict(zip(("type", "levels", "sweeps", "visits", "readbacks"), (x.value for x in v)))


def error_ratio(u_dev, R, f, u0, zero):
    u_64 = R.cycle(f, u0, zero)
    u_ld = R.cycle(f, u0, zero, dt=LD)
    yard = float(np.max(np.abs(u_64.astype(LD) - u_ld)))
    err = float(np.max(np.abs(u_dev.astype(LD) - u_ld)))
    assert yard > 0.0 and float(np.max(np.abs(u_ld))) > 0.0
    return err / yard, err, yard


@pytest.mark.parametrize("case", CYCLE_CASES, ids=[c["name"] for c in CYCLE_CASES])
def test_one_cycle_against_the_restatement(gpu_lib, oracle, case):
    """From a random iterate and from zero.  Every type-15 case runs fused and unfused as well: the same bits, no read-back in
    the fused visits, two per sweep in the unfused ones."""
    lib = gpu_lib
    with device_hierarchy(lib, case) as (opt, s, A, n):
        R = restatement_of(lib, oracle, s, case)
        try:
            rng = np.random.default_rng(7)
            f, u0 = rng.standard_normal(n), rng.standard_normal(n)
            for zero in (False, True):
                start = np.zeros(n) if zero else u0
                u_dev = one_cycle(lib, s, A, f, start, zero)
                st = smoother_stats(lib, s)
                ratio, err, yard = error_ratio(u_dev, R, f, start, zero)
                print("%s %s: max|u_dev - u_ld| = %.3e, max|u_64 - u_ld| = %.3e, ratio %.2f, visits %d, readbacks %d"
                      % (case["name"], "zero" if zero else "random", err, yard, ratio, st["visits"], st["readbacks"]))
                assert ratio <= 16.0, (case["name"], zero, ratio)
                nl = lib.hypre_amd_BoomerAMGGetNumLevels(s)
                levels = min(case["smooth_num_levels"], nl)
                v_cycle_visits = 2 * levels - (1 if levels == nl else 0)      # down and up; the coarsest level once
                assert st["visits"] == v_cycle_visits if case["mu"] == 1 else st["visits"] > v_cycle_visits
                if case["smooth_type"] == 15:
                    assert st["readbacks"] == 0
                    assert lib.hypre_amd_SetSmootherFusion(0) == 0
                    u_plain = one_cycle(lib, s, A, f, start, zero)
                    plain = smoother_stats(lib, s)
                    assert lib.hypre_amd_SetSmootherFusion(1) == 1
                    assert np.array_equal(u_plain.view(np.int64), u_dev.view(np.int64)), np.max(np.abs(u_plain - u_dev))
                    assert plain["visits"] == st["visits"] and plain["readbacks"] == 2 * case["smooth_num_sweeps"] * plain["visits"]
                else:
                    assert st["readbacks"] == 0
        finally:
            R.close()


def test_a_zero_right_hand_side_leaves_the_iterate(gpu_lib):
    """gamma = <R, Z> is exactly 0: the visit ends, on the device by the flag in the scalar block, and U stays (the reference
    divides 0 by 0); fused and unfused alike"""
    lib = gpu_lib
    case = _case("zero-rhs", "7pt", 15, 25, sweeps=2)
    with device_hierarchy(lib, case) as (opt, s, A, n):
        for fusion in (1, 0):
            lib.hypre_amd_SetSmootherFusion(fusion)
            u = one_cycle(lib, s, A, np.zeros(n), np.zeros(n), True)
            assert np.all(u == 0.0)


@pytest.mark.parametrize("case", SOLVE_CASES, ids=[c["name"] for c in SOLVE_CASES])
def test_solves_reach_the_restatements_count(gpu_lib, oracle, case):
    from hypre_amd import binding as B, ij
    lib = gpu_lib
    with device_hierarchy(lib, case) as (opt, s, A, n):
        R = restatement_of(lib, oracle, s, case)
        try:
            f = rhs_of(case, n)
            its_ref, hist = R.solve(f, tol=1e-8) if case["solver"] == 0 else R.pcg(f, tol=1e-8)
            assert clear_of_tolerance(hist, 1e-8), hist[-2:]
            db, dx = B.parvec_from_numpy(f), B.parvec_from_numpy(np.zeros(n))
            if case["solver"] == 0:
                lib.HYPRE_BoomerAMGSetTol(s, 1e-8)
                lib.HYPRE_BoomerAMGSetMaxIter(s, 100)
                lib.HYPRE_BoomerAMGSolve(s, A, db, dx)
                B.check()
                its = C.c_int()
                lib.HYPRE_BoomerAMGGetNumIterations(s, C.byref(its))
                its = its.value
            else:
                its, rel = ij.solve_pcg(opt, A, db, dx, amg=s)
                lib.HYPRE_ClearError(256)
                B.check()
            x = B.parvec_to_numpy(dx)
            for v in (db, dx):
                lib.hypre_ParVectorDestroy(v)
            print("%s: %d iterations, the restatement %d (last residuals %.2e %.2e)" % (case["name"], its, its_ref, hist[-2] if len(hist) > 1 else 1, hist[-1]))
            assert its == its_ref
            assert np.linalg.norm(R._Ax(0, x, np.float64) - f) <= 1e-8 * np.linalg.norm(f)
            if case.get("beats_jacobi"):
                J = restatement_of(lib, oracle, s, case, levels=0)
                its_j, _ = J.solve(f, tol=1e-8)
                J.close()
                assert its < its_j, (its, its_j)
        finally:
            R.close()


def _kernel_test(lib, n, scalars, first, zero_z, with_dots, U, R, P, Z, V):
    sc = np.array(scalars, dtype=np.float64)
    out = [np.array(v, dtype=np.float64) for v in (U, R, P, Z)]
    ptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.hypre_amd_ILUSmootherKernelTest(n, ptr(sc), first, zero_z, with_dots, *[ptr(a) for a in out], ptr(np.ascontiguousarray(V))) == 0
    return sc, out


def _bits(a, b):
    return np.array_equal(np.asarray(a).view(np.int64), np.asarray(b).view(np.int64))


def _device_dot(lib, x, y):
    from hypre_amd import binding as B
    dx, dy = B.parvec_from_numpy(x), B.parvec_from_numpy(y)
    lib.hypre_ParVectorInnerProd.restype = C.c_double
    v = lib.hypre_ParVectorInnerProd(dx, dy)
    for w in (dx, dy):
        lib.hypre_ParVectorDestroy(w)
    return v


def test_the_vector_kernels_alone(gpu_lib):
    """Direction and update through their launchers against numpy with the spelled-out rounding (one fused multiply-add each,
    the quotients rounded once), bit for bit: n = 1, 2, 63, 64, 65, 1025 and one n past a single pass of the vector grid; the first
    sweep (P is Z exactly); a raised flag and a sum of exactly 0 (U, R, P untouched); the two sums with the bits of the
    library's dot product."""
    lib = gpu_lib
    past_one_pass = 2048 * 256 * 2 + 3
    for n in (1, 2, 63, 64, 65, 1025, past_one_pass):
        rng = np.random.default_rng(n)
        U, R, P, Z, V = (rng.standard_normal(n) for _ in range(5))
        gamma, gammaold, pv = 0.7310585786300049, 1.9371, -2.4142135623730951
        # a later sweep: P = Z + (gamma / gammaold) P, then U += alfa P, R -= alfa V, Z = 0
        sc, (u, r, p, z) = _kernel_test(lib, n, [gamma, gammaold, pv, 0.0], 0, 1, 0, U, R, P, Z, V)
        beta, alfa = gamma / gammaold, gamma / pv
        p_ref = fma(beta, P, Z)
        assert _bits(p, p_ref) and _bits(u, fma(alfa, p_ref, U)) and _bits(r, fma(-alfa, V, R)) and np.all(z == 0.0)
        assert _bits(sc, [gamma, gammaold, pv, 0.0])
        # the first sweep: P = Z exactly, Z kept
        sc, (u, r, p, z) = _kernel_test(lib, n, [gamma, 0.0, pv, 0.0], 1, 0, 0, U, R, P, Z, V)
        assert _bits(p, Z) and _bits(z, Z) and _bits(u, fma(alfa, Z, U)) and _bits(r, fma(-alfa, V, R))
        # a raised flag: nothing moves
        sc, (u, r, p, z) = _kernel_test(lib, n, [gamma, gammaold, pv, 1.0], 0, 1, 0, U, R, P, Z, V)
        assert _bits(u, U) and _bits(r, R) and _bits(p, P) and _bits(z, Z)
        # with the sums: gamma = <R, Z> and <P, V> as the library's dot product leaves them, gamma moved to gammaold
        sc, (u, r, p, z) = _kernel_test(lib, n, [gamma, gammaold, pv, 0.0], 0, 0, 1, U, R, P, Z, V)
        g = _device_dot(lib, R, Z)
        p_ref = fma(g / gamma, P, Z)
        dpv = _device_dot(lib, p_ref, V)
        assert _bits(sc, [g, gamma, dpv, 0.0]) and _bits(p, p_ref)
        assert _bits(u, fma(g / dpv, p_ref, U)) and _bits(r, fma(-(g / dpv), V, R)) and _bits(z, Z)
        # gamma == 0 (R is zero): the flag goes up on the device, U, R and P stay
        sc, (u, r, p, z) = _kernel_test(lib, n, [gamma, gammaold, pv, 0.0], 0, 1, 1, U, np.zeros(n), P, Z, V)
        assert sc[3] == 1.0 and sc[0] == 0.0 and sc[1] == gamma and _bits(u, U) and np.all(r == 0.0) and _bits(p, P) and _bits(z, Z)


def test_a_zero_iterate_skips_the_product_with_the_same_result(gpu_lib):
    """HYPRE_ILUSolve with u->all_zeros set uses f as it is: == the full path's result (f - A 0 is f as a number)"""
    from hypre_amd import binding as B, ij
    from test_ilu_host import new_ilu
    lib = gpu_lib
    for iterative in (0, 1):
        opt = ij.IJOptions(**OPERATORS["difconv"])
        A = ij.build_matrix(opt)
        n = int(A.contents.diag.contents.num_rows)
        s = new_ilu(lib, lfil=1)
        lib.hypre_amd_ILUSetIterativeTriSolve(s, iterative)
        lib.HYPRE_ILUSetMaxIter(s, 2)
        lib.HYPRE_ILUSetTol(s, 0.0)
        assert lib.HYPRE_ILUSetup(s, A, None, None) == 0
        lib.hypre_ParCSRMatrixMigrate(A, DEVICE)
        f = np.random.default_rng(3).standard_normal(n)
        out = []
        for flagged in (False, True):
            df, du = B.parvec_from_numpy(f), B.parvec_from_numpy(np.zeros(n))
            if flagged:
                lib.hypre_ParVectorSetZeros(du)
            assert du.contents.all_zeros == (1 if flagged else 0)
            assert lib.HYPRE_ILUSolve(s, A, df, du) == 0
            B.check()
            assert du.contents.all_zeros == 0
            out.append(B.parvec_to_numpy(du))
            for v in (df, du):
                lib.hypre_ParVectorDestroy(v)
        assert np.all(np.isfinite(out[0])) and np.any(out[0] != 0.0) and np.all(out[0] == out[1])
        lib.HYPRE_ILUDestroy(s)
        lib.hypre_ParCSRMatrixDestroy(A)


@pytest.mark.parametrize("levels", [1, 25])
def test_where_the_tail_and_the_graph_start(gpu_lib, oracle, levels):
    """smooth_num_levels 1 on a hierarchy of at least four levels: the one-workgroup tail and the recorded graph start at a
    level >= 1 and the cycle (the third: the graph is replayed by then) still matches the restatement; 25: both are off"""
    lib = gpu_lib
    case = _case("placement", "7pt", 15, levels, sweeps=2)
    with device_hierarchy(lib, case) as (opt, s, A, n):
        assert lib.hypre_amd_BoomerAMGGetNumLevels(s) >= 4
        rng = np.random.default_rng(9)
        f, u0 = rng.standard_normal(n), rng.standard_normal(n)
        for _ in range(3):
            u = one_cycle(lib, s, A, f, u0, False)
        gl, nodes = C.c_int(-5), C.c_int(-5)
        lib.hypre_amd_BoomerAMGGetGraphInfo(s, C.byref(gl), C.byref(nodes))
        tail = lib.hypre_amd_BoomerAMGGetSmallTailLevel(s)
        if levels == 1:
            assert tail >= 1 and gl.value >= 1 and nodes.value > 0
        else:
            assert tail == -1 and gl.value == -1
        R = restatement_of(lib, oracle, s, case)
        try:
            ratio, err, yard = error_ratio(u, R, f, u0, False)
            print("placement, %d levels: tail %d, graph %d, ratio %.2f" % (levels, tail, gl.value, ratio))
            assert ratio <= 16.0
        finally:
            R.close()


def test_a_second_setup_uses_the_new_factors(gpu_lib, oracle):
    """Setup, solve, new matrix values, Setup again, solve, Destroy: the second solve runs on the factors of the new values"""
    from hypre_amd import binding as B
    lib = gpu_lib
    case = _case("lifetime", "7pt", 5, 25, iterative=1, lower=3, upper=3)
    with device_hierarchy(lib, case) as (opt, s, A, n):
        rng = np.random.default_rng(21)
        f, u0 = rng.standard_normal(n), rng.standard_normal(n)
        first = one_cycle(lib, s, A, f, u0, False)
        lib.hypre_ParCSRMatrixMigrate(A, HOST)
        blk = A.contents.diag.contents
        np.ctypeslib.as_array(blk.data, shape=(blk.num_nonzeros,))[:] *= 3.0
        assert lib.HYPRE_BoomerAMGSetup(s, A, None, None) == 0
        B.check()
        lib.hypre_ParCSRMatrixMigrate(A, DEVICE)
        second = one_cycle(lib, s, A, f, u0, False)
        R = restatement_of(lib, oracle, s, case)
        try:
            ratio, err, yard = error_ratio(second, R, f, u0, False)
            assert ratio <= 16.0, ratio
        finally:
            R.close()
        assert np.max(np.abs(second - first)) > 1e-3 * np.max(np.abs(first))
