"""The V-cycle over several columns with its large matrix passes fused (par_solve.cpp: amg_cycle_columns): on the levels above
the one-workgroup tail every pass over an operator is one launch for a group of 2 - 4 columns, below it each column runs the
single-column cycle.  Every column of such a solve is, byte for byte, the single-vector solve of that column on the same
solver with the same switches; the fused passes are really taken and stream fewer bytes than the column loop; configurations
the fused cycle does not serve keep the column loop."""
import ctypes as C

import numpy as np
import pytest

from test_amg_multivector_gpu import PROBLEMS, _columns, _setup, _solve_multi, _solve_single

pytestmark = pytest.mark.gpu

CASES = dict(PROBLEMS)
CASES["7pt_large"] = dict(n=(24, 23, 22))


def _bits(lib, s, A, n, nv, k, seed, guesses=(True, False)):
    """Every column of the fused solve against the single-vector solve of that column and against the column loop."""
    F, U0 = _columns(n, nv, seed), _columns(n, nv, seed + 1)
    lib.HYPRE_BoomerAMGSetTol(s, 0.0)
    lib.HYPRE_BoomerAMGSetMaxIter(s, k)
    for zero in guesses:
        start = np.zeros_like(U0) if zero else U0
        assert lib.hypre_amd_SetMultivectorCycle(1) == 1
        U = _solve_multi(lib, s, A, F, start, zero)
        assert not np.array_equal(U, start)
        for v in range(nv):
            u = _solve_single(lib, s, A, F[:, v], start[:, v], zero)
            assert U[:, v].tobytes() == u.tobytes(), (v, zero, float(np.max(np.abs(U[:, v] - u))))
        assert lib.hypre_amd_SetMultivectorCycle(0) == 0
        Uc = _solve_multi(lib, s, A, F, start, zero)
        lib.hypre_amd_SetMultivectorCycle(1)
        assert Uc.tobytes() == U.tobytes(), zero


@pytest.fixture(autouse=True)
def _switch_restored(gpu_lib):
    before = gpu_lib.hypre_amd_SetMultivectorCycle(-1)
    yield
    gpu_lib.hypre_amd_SetMultivectorCycle(before)


@pytest.mark.parametrize("relax", [18, 7])
@pytest.mark.parametrize("problem,nvs", [("7pt", (2, 5)), ("7pt_large", (3, 4, 8)), ("27pt", (4, 5)), ("difconv", (2, 3, 8))])
def test_every_column_of_the_fused_cycle_is_the_single_vector_solve(gpu_lib, problem, relax, nvs):
    lib = gpu_lib
    opt, A, s, n = _setup(lib, relax_type=relax, **CASES[problem])
    for nv in nvs:
        _bits(lib, s, A, n, nv, 2, 11 + nv)
    lib.HYPRE_BoomerAMGDestroy(s)


@pytest.mark.parametrize("relax", [18, 7])
def test_every_column_with_every_switch(gpu_lib, relax):
    """Cycle fusion, the one-workgroup tail, the fused multivector passes and the coarse-tail graph each on and off."""
    lib = gpu_lib
    opt, A, s, n = _setup(lib, relax_type=relax, n=(24, 23, 22))
    try:
        for fused, tail, fusion in ((1, 1, 1), (0, 1, 1), (1, 0, 1), (1, 1, 0), (1, 0, 0)):
            lib.hypre_amd_SpmvSetFusedMultivectors(fused)
            lib.hypre_amd_SetSmallTail(tail)
            lib.hypre_amd_SetCycleFusion(fusion)
            _bits(lib, s, A, n, 4, 3, 21)
        for rows in (200, 0):                                  # a recorded tail from the first level of at most 200 rows; none
            lib.hypre_amd_BoomerAMGSetGraphThreshold(s, rows)
            _bits(lib, s, A, n, 5, 3, 31)
            _bits(lib, s, A, n, 3, 3, 33, guesses=(False,))   # (the graph is recorded by now: replayed)
    finally:
        lib.hypre_amd_SpmvSetFusedMultivectors(1)
        lib.hypre_amd_SetSmallTail(1)
        lib.hypre_amd_SetCycleFusion(1)
    lib.HYPRE_BoomerAMGDestroy(s)


def _streamed(lib):
    csr, streamed = C.c_double(), C.c_double()
    lib.hypre_amd_ByteCounters(C.byref(csr), C.byref(streamed), 0)
    return streamed.value


def test_the_fused_passes_are_taken_and_stream_fewer_bytes(gpu_lib):
    """48 x 48 x 48: the finest operator takes the slice multivector form, level 1 the row slices.  One NV = 4 cycle (tol = 0,
    max_iter = 1: no outer residual) launches at least the four matrix passes of level 0 as multivector passes and streams
    strictly fewer bytes than four single-column cycles."""
    lib = gpu_lib
    opt, A, s, n = _setup(lib, relax_type=18, n=(48, 48, 48))
    nv = 4
    F, U0 = _columns(n, nv, 3), _columns(n, nv, 4)
    lib.HYPRE_BoomerAMGSetTol(s, 0.0)
    lib.HYPRE_BoomerAMGSetMaxIter(s, 1)
    _solve_single(lib, s, A, F[:, 0], U0[:, 0], False)            # plans and scratch exist from here on
    b0 = _streamed(lib)
    _solve_single(lib, s, A, F[:, 0], U0[:, 0], False)
    single = _streamed(lib) - b0
    assert single > 0
    from hypre_amd import binding as B
    assert lib.hypre_amd_CSRMatrixPlanForm(A.contents.diag) == 4                              # slice form on the finest level
    A1 = C.cast(lib.hypre_amd_BoomerAMGGetA(s, 1), C.POINTER(B.ParCSRMatrix))
    assert lib.hypre_amd_CSRMatrixPlanForm(A1.contents.diag) == 5                             # row slices on level 1
    lib.hypre_amd_SetMultivectorCycle(1)
    _solve_multi(lib, s, A, F, U0, False)                          # level vectors exist from here on
    before, b0 = lib.hypre_amd_SpmvFusedMultivectorLaunches(), _streamed(lib)
    U = _solve_multi(lib, s, A, F, U0, False)
    launches, fused = lib.hypre_amd_SpmvFusedMultivectorLaunches() - before, _streamed(lib) - b0
    print("fused launches %d, streamed bytes: fused cycle %.0f, 4 single cycles %.0f" % (launches, fused, nv * single))
    assert launches >= 4
    assert fused < nv * single
    lib.hypre_amd_SetMultivectorCycle(0)
    before, b0 = lib.hypre_amd_SpmvFusedMultivectorLaunches(), _streamed(lib)
    Uc = _solve_multi(lib, s, A, F, U0, False)
    assert lib.hypre_amd_SpmvFusedMultivectorLaunches() == before
    loop = _streamed(lib) - b0
    print("column loop %.0f" % loop)
    assert fused < loop
    assert U.tobytes() == Uc.tobytes()
    _bits(lib, s, A, n, 4, 2, 41)
    _bits(lib, s, A, n, 3, 1, 43, guesses=(True,))
    lib.HYPRE_BoomerAMGDestroy(s)


@pytest.mark.parametrize("relax", [18, 7])
def test_one_fused_cycle_matches_oracle(gpu_lib, oracle, relax):
    lib = gpu_lib
    opt, A, s, n = _setup(lib, relax_type=relax, n=(12, 11, 10))
    amg = oracle.amg_from_solvers([s], num_threads=opt.num_threads)
    nv = 3
    F, U0 = _columns(n, nv, 5), _columns(n, nv, 6)
    lib.HYPRE_BoomerAMGSetTol(s, 0.0)
    lib.HYPRE_BoomerAMGSetMaxIter(s, 1)
    lib.hypre_amd_SetMultivectorCycle(1)
    before = lib.hypre_amd_SpmvFusedMultivectorLaunches()
    U = _solve_multi(lib, s, A, F, U0, False)
    assert lib.hypre_amd_SpmvFusedMultivectorLaunches() > before
    for v in range(nv):
        ur = U0[:, v].copy()
        amg.cycle(F[:, v].copy(), ur, u_all_zeros=False)
        assert np.max(np.abs(U[:, v] - ur)) <= 1e-11 * np.max(np.abs(ur)), v
    lib.HYPRE_BoomerAMGDestroy(s)


@pytest.mark.parametrize("kw", [dict(relax_type=11), dict(relax_type=12), dict(relax_type=18, cycle_type=2)])
def test_unserved_cycles_keep_the_column_loop(gpu_lib, kw):
    """Two-stage Gauss-Seidel sweeps and a W-cycle: solved, with the bits of the column loop, by the column loop."""
    lib = gpu_lib
    opt, A, s, n = _setup(lib, n=(12, 11, 10), **kw)
    if "cycle_type" in kw:
        lib.HYPRE_BoomerAMGSetCycleType(s, kw["cycle_type"])
    nv = 3
    F, U0 = _columns(n, nv, 7), _columns(n, nv, 8)
    lib.HYPRE_BoomerAMGSetTol(s, 0.0)
    lib.HYPRE_BoomerAMGSetMaxIter(s, 2)
    out = {}
    for on in (1, 0):
        lib.hypre_amd_SetMultivectorCycle(on)
        before = lib.hypre_amd_SpmvFusedMultivectorLaunches()
        out[on] = _solve_multi(lib, s, A, F, U0, False)
        assert lib.hypre_amd_SpmvFusedMultivectorLaunches() == before
    assert out[1].tobytes() == out[0].tobytes()
    assert not np.array_equal(out[1], U0)
    for v in range(nv):
        u = _solve_single(lib, s, A, F[:, v], U0[:, v], False)
        assert out[1][:, v].tobytes() == u.tobytes(), v
    lib.HYPRE_BoomerAMGDestroy(s)


@pytest.mark.parametrize("nth", [1, 2, 4])
def test_a_failed_level_vector_allocation_falls_back_to_the_column_loop(gpu_lib, nth):
    """Site 7 of hypre_amd_PlanTestFailAlloc: the level vectors of the fused cycle.  The nth of them fails: nothing is raised,
    the cycle runs column by column (no fused pass), the bits are the same, and the next solve gets its vectors."""
    from hypre_amd import binding as B
    lib = gpu_lib
    opt, A, s, n = _setup(lib, relax_type=18, n=(12, 11, 10))
    nv = 3
    F, U0 = _columns(n, nv, 7), _columns(n, nv, 8)
    lib.HYPRE_BoomerAMGSetTol(s, 0.0)
    lib.HYPRE_BoomerAMGSetMaxIter(s, 1)
    lib.hypre_amd_SetMultivectorCycle(1)
    try:
        lib.hypre_amd_PlanTestFailAlloc(7, nth)
        before = lib.hypre_amd_SpmvFusedMultivectorLaunches()
        U = _solve_multi(lib, s, A, F, U0, False)               # (B.check() inside: the error flag is clean)
        assert lib.hypre_amd_PlanTestFailAlloc(0, 0) == 0       # it happened
        assert lib.hypre_amd_SpmvFusedMultivectorLaunches() == before
    finally:
        lib.hypre_amd_PlanTestFailAlloc(0, 0)
    before = lib.hypre_amd_SpmvFusedMultivectorLaunches()
    U2 = _solve_multi(lib, s, A, F, U0, False)
    assert lib.hypre_amd_SpmvFusedMultivectorLaunches() > before
    assert U.tobytes() == U2.tobytes()
    lib.HYPRE_BoomerAMGDestroy(s)
