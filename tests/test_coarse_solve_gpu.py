"""The dense solve of the coarsest level above the default 9 unknowns: its three copies (coarse_solve_wave_kernel up to 32
unknowns, coarse_solve_kernel above, the copy inside the one-workgroup tail) against the oracle's hypre_gselim loop as raw
bytes through hypre_amd_CoarseSolveTest, zero pivots and zero multipliers included, and through the cycle on hierarchies
whose coarsest level has 10 - 32, 33 - 64 and more than 64 rows (HYPRE_BoomerAMGSetMaxCoarseSize): eager, in the
one-workgroup tail, recorded in the coarse-tail graph and under the fused multi-column cycle."""
import ctypes as C

import numpy as np
import pytest

from util import rand_vector

gpu = pytest.mark.gpu

WAVE_SIZES = (1, 2, 3, 9, 10, 31, 32)              # one wave (form 0) and one lane (form 1)
LANE_SIZES = (33, 63, 64, 65, 100)                 # one lane either way
KINDS = ("dominant", "dominant_half_zero")


def _dominant(n, kind):
    """Strictly diagonally dominant by rows (|a_ii| = 1 + sum of the row's other magnitudes), both signs off the diagonal and
    on it; `dominant_half_zero`: about half of the off-diagonal entries exactly zero (the zero-multiplier skip)."""
    rng = np.random.default_rng(7000 + n + (500 if kind == "dominant_half_zero" else 0))
    M = rng.uniform(-1.0, 1.0, (n, n))
    if kind == "dominant_half_zero":
        M[rng.random((n, n)) < 0.5] = 0.0
    np.fill_diagonal(M, 0.0)
    d = 1.0 + np.abs(M).sum(axis=1)
    np.fill_diagonal(M, np.where(rng.random(n) < 0.5, -d, d))
    return np.ascontiguousarray(M), rng.uniform(-1.0, 1.0, n)


def _oracle_solve(oracle, M, b):
    A, x = np.ascontiguousarray(M, dtype=np.float64).copy().ravel(), np.array(b, dtype=np.float64)
    oracle.load().oracle_gselim(A.ctypes.data_as(oracle.RealP), x.ctypes.data_as(oracle.RealP), len(x))
    return x


def _device_solve(lib, M, b, form):
    from hypre_amd import binding as B
    a, rhs = np.ascontiguousarray(M, dtype=np.float64).copy(), np.array(b, dtype=np.float64)
    x = np.full(len(rhs), np.nan)
    assert lib.hypre_amd_CoarseSolveTest(B._rp(a), len(rhs), B._rp(rhs), form, B._rp(x)) == 0
    B.check()
    assert a.tobytes() == np.ascontiguousarray(M, dtype=np.float64).tobytes() and rhs.tobytes() == np.asarray(b, dtype=np.float64).tobytes()
    return x


def _same_bytes(lib, oracle, M, b, what):
    """form 0 (and form 1 where it is another kernel: n <= 32) against the oracle, and against each other"""
    n = len(b)
    ref = _oracle_solve(oracle, M, b)
    assert np.all(np.isfinite(ref)), what
    got = {form: _device_solve(lib, M, b, form) for form in ((0, 1) if n <= 32 else (0,))}
    for form, x in got.items():
        print(what, "n", n, "form", form, "max |device - oracle|", float(np.max(np.abs(x - ref))))
        assert x.tobytes() == ref.tobytes(), (what, n, form, float(np.max(np.abs(x - ref))))
    if n <= 32:
        assert got[0].tobytes() == got[1].tobytes(), (what, n)


@pytest.mark.parametrize("kind", KINDS)
def test_the_oracle_solves_the_dominant_systems(oracle, kind):
    """The yardstick is not vacuous: on the diagonally dominant inputs of the parity test the oracle's elimination agrees
    with numpy.linalg.solve to 1e-12 max|x| (CPU only).  Observed: between 0 (n = 1, 2) and 1.1e-15 max|x| (n = 100) over
    the twelve orders and both kinds, growing slowly with n."""
    worst = 0.0
    for n in WAVE_SIZES + LANE_SIZES:
        M, b = _dominant(n, kind)
        x, ref = _oracle_solve(oracle, M, b), np.linalg.solve(M, b)
        err = float(np.max(np.abs(x - ref)) / np.max(np.abs(ref)))
        print(kind, "n", n, "oracle against numpy.linalg.solve", err)
        worst = max(worst, err)
        assert err <= 1e-12, (kind, n, err)
    print(kind, "worst", worst)


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", WAVE_SIZES + LANE_SIZES)
def test_device_solve_has_the_bytes_of_the_host_loop(gpu_lib, oracle, n, kind):
    """(This is the test that found the kernels fusing x - factor * x_k into one multiply-add through __dsub_rn(x,
    __dmul_rn(..)): from n = 3 on an entry or two differed from the host loop in the last bit, up to 5.6e-17.)"""
    M, b = _dominant(n, kind)
    _same_bytes(gpu_lib, oracle, M, b, kind)


def _zero_pivot_steps(M):
    """The oracle's elimination restated (same operations, same order): the steps whose pivot is exactly zero, the last
    one (which only the back substitution meets) included, and whether every intermediate stayed an exact small number."""
    A = np.array(M, dtype=np.float64)
    n = A.shape[0]
    steps = []
    for k in range(n - 1):
        if A[k, k] == 0.0:
            steps.append(k)
            continue
        div = 1.0 / A[k, k]
        for j in range(k + 1, n):
            if A[j, k] != 0.0:
                factor = A[j, k] * div
                A[j, k + 1:] -= factor * A[k, k + 1:]
    if A[n - 1, n - 1] == 0.0:
        steps.append(n - 1)
    exact = bool(np.all(A * 64.0 == np.round(A * 64.0)) and np.max(np.abs(A)) < 1024.0)
    return steps, exact


# small integers, pivots that are powers of two: every intermediate is a multiple of 1/64 well below 2^53, so the zero
# pivots below are exact zeros and not the leftovers of a cancellation
ZERO_PIVOTS = {
    "step 0": ([[0, 1, 2], [1, 2, 2], [2, 1, 5]], [0]),
    "a middle step": ([[2, 1, 1, 0, 1], [2, 1, 3, 1, 0], [4, 2, 4, 1, 1], [0, 1, 2, 5, 1], [2, 3, 1, 1, 2]], [1]),
    "the last step (two equal rows)": ([[2, 1, 0, 1], [0, 4, 1, 2], [2, 1, 2, 3], [2, 1, 2, 3]], [3]),
    "the last two steps (three equal rows)": ([[2, 1, 0, 1, 1], [0, 4, 1, 2, 0], [2, 1, 2, 3, 1], [2, 1, 2, 3, 1], [2, 1, 2, 3, 1]], [3, 4]),
    "every step": ([[0, 1, 2], [3, 0, 1], [2, 5, 0]], [0, 1, 2]),
}


def _embedded(Z, n):
    """The small matrix as the trailing block of an n x n one: the leading unknowns have the pivot 4; the even ones feed
    the block's rows in the elimination (multipliers 1/4 .. 2), the odd ones take the block's unknowns in the back
    substitution.  No fill reaches the block, so its zero pivots move to the steps n - len(Z) + k."""
    Z = np.array(Z, dtype=np.float64)
    m, z = n - len(Z), len(Z)
    M = np.zeros((n, n))
    M[m:, m:] = Z
    for i in range(m):
        M[i, i] = 4.0
        if i % 2 == 0:
            M[m + i % z, i] = (1.0, -2.0, 4.0, -8.0)[(i // 2) % 4]
        else:
            M[i, m + i % z] = (3.0, -1.0, 2.0)[(i // 2) % 3]
    return M


@gpu
@pytest.mark.parametrize("name", sorted(ZERO_PIVOTS))
def test_zero_pivots_skip_their_step_as_the_host_loop_does(gpu_lib, oracle, name):
    """A zero pivot skips its elimination step and its back substitution (utilities/gselim.h); all three copies guard
    the division, so only finite numbers appear.  The matrix on its own (both kernels), and as the trailing block of a
    system of 32 (both kernels again, every lane of the wave's half in use) and of 40 unknowns (one lane)."""
    Z, steps = ZERO_PIVOTS[name]
    Z = np.array(Z, dtype=np.float64)
    found, exact = _zero_pivot_steps(Z)
    assert found == steps and exact, (name, found, exact)
    for n in (len(Z), 32, 40):
        M = Z if n == len(Z) else _embedded(Z, n)
        found, exact = _zero_pivot_steps(M)
        assert found == [n - len(Z) + k for k in steps] and exact, (name, n, found, exact)
        b = np.arange(1.0, n + 1.0) * np.where(np.arange(n) % 3 == 1, -1.0, 1.0)
        _same_bytes(gpu_lib, oracle, M, b, name)


@gpu
def test_one_by_one_zero_matrix_leaves_the_right_hand_side(gpu_lib, oracle):
    M, b = np.zeros((1, 1)), np.array([3.0])
    _same_bytes(gpu_lib, oracle, M, b, "[0]")
    assert _device_solve(gpu_lib, M, b, 0)[0] == 3.0


# ---------------------------------------------------------------------------
# through the cycle
# ---------------------------------------------------------------------------
# Grid, HYPRE_BoomerAMGSetMaxCoarseSize and the rows the coarsest level must then have; found with the host setup (PMIS,
# ext+i): 16 x 15 x 14 -> 3360, 1101, 170, 26; 20 x 19 x 18 -> 6840, 2277, 345, 54; 12 x 11 x 10 -> 1320, 452, 72.  In all
# three the one-workgroup tail would begin at a level above the coarsest one (operators of at most 20 000 entries), so in
# the second and third it is the limit of 32 unknowns alone that keeps it out.
RANGES = {
    "10 to 32 rows": dict(n=(16, 15, 14), coarse_threshold=32, lo=10, hi=32),
    "33 to 64 rows": dict(n=(20, 19, 18), coarse_threshold=64, lo=33, hi=64),
    "more than 64 rows": dict(n=(12, 11, 10), coarse_threshold=100, lo=65, hi=100),
}


def _setup(lib, which, relax_type):
    """the hierarchy of one range; the range is asserted from the last level's actual row count"""
    from hypre_amd import binding as B, ij
    r = RANGES[which]
    opt = ij.IJOptions(n=r["n"], coarsen_type=8, relax_type=relax_type, coarse_threshold=r["coarse_threshold"])
    A = ij.build_matrix(opt)
    s = ij.create_amg(opt, memory_location=B.HYPRE_MEMORY_DEVICE)
    lib.HYPRE_BoomerAMGSetup(s, A, None, None)
    B.check()
    lib.hypre_ParCSRMatrixMigrate(A, B.HYPRE_MEMORY_DEVICE)
    nl = lib.hypre_amd_BoomerAMGGetNumLevels(s)
    Ac = C.cast(lib.hypre_amd_BoomerAMGGetA(s, nl - 1), C.POINTER(B.ParCSRMatrix)).contents
    nc = int(Ac.global_num_rows)
    print(which, "relax", relax_type, "levels", nl, "coarsest rows", nc)
    assert r["lo"] <= nc <= r["hi"], (which, nl, nc)
    assert nl >= 3
    lib.HYPRE_BoomerAMGSetTol(s, 0.0)
    lib.HYPRE_BoomerAMGSetMaxIter(s, 1)
    return opt, A, s, nl, nc, int(np.prod(r["n"]))


def _one_cycle(lib, s, A, f, u0, zero):
    from hypre_amd import binding as B
    du, df = B.parvec_from_numpy(u0), B.parvec_from_numpy(f)
    if zero:
        lib.hypre_ParVectorSetZeros(du)
    lib.HYPRE_BoomerAMGSolve(s, A, df, du)
    B.check()
    u = B.parvec_to_numpy(du)
    lib.hypre_ParVectorDestroy(du); lib.hypre_ParVectorDestroy(df)
    return u


@gpu
@pytest.mark.parametrize("which", sorted(RANGES))
def test_densified_coarsest_operator_has_the_bytes_of_the_host_loop(gpu_lib, oracle, which):
    """the coarsest operator of a real hierarchy (hypre_amd_BoomerAMGGetA at the last level) as a dense matrix"""
    from hypre_amd import binding as B
    lib = gpu_lib
    opt, A, s, nl, nc, n = _setup(lib, which, 18)
    Ac = C.cast(lib.hypre_amd_BoomerAMGGetA(s, nl - 1), C.POINTER(B.ParCSRMatrix)).contents
    M = np.ascontiguousarray(B.csr_to_scipy(Ac.diag).toarray())
    assert M.shape == (nc, nc) and np.count_nonzero(M) > nc
    _same_bytes(lib, oracle, M, rand_vector(nc, 3), which)
    lib.HYPRE_BoomerAMGDestroy(s)
    B.check()


@gpu
@pytest.mark.parametrize("relax_type", [18, 11])
@pytest.mark.parametrize("which", sorted(RANGES))
def test_cycle_with_a_larger_coarsest_level(gpu_lib, oracle, which, relax_type):
    """One cycle from zero and one from a random iterate are the oracle's (1e-11, as test_one_cycle_matches_oracle).
    10 - 32 rows: the one-workgroup tail is in use, its three image forms give the same bits, and with it the cycle is
    the cycle without it up to the order of a row's sum (1e-13).  Above 32 rows the tail stays out (-1) and switching it
    on or off changes no bit."""
    from hypre_amd import binding as B
    lib = gpu_lib
    opt, A, s, nl, nc, n = _setup(lib, which, relax_type)
    amg = oracle.amg_from_solvers([s], num_threads=opt.num_threads)
    f = rand_vector(n, 5)
    fits = nc <= 32
    try:
        for zero in (True, False):
            u0 = np.zeros(n) if zero else rand_vector(n, 6)
            ur = u0.copy()
            amg.cycle(f, ur, u_all_zeros=zero)
            scale = np.max(np.abs(ur))
            out, used, by_form = {}, {}, {}
            for on in (1, 0):
                lib.hypre_amd_SetSmallTailForm(-1)
                assert lib.hypre_amd_SetSmallTail(on) == on
                out[on] = _one_cycle(lib, s, A, f, u0, zero)
                used[on] = lib.hypre_amd_BoomerAMGGetSmallTailLevel(s)
                err = float(np.max(np.abs(out[on] - ur)) / scale)
                print(which, "relax", relax_type, "zero", zero, "tail", on, "level", used[on], "against the oracle", err)
                assert err <= 1e-11, (which, relax_type, zero, on)
            assert used[0] == -1
            if fits:
                assert 1 <= used[1] <= nl - 2, (used, nl)
                lib.hypre_amd_SetSmallTail(1)
                for form in (0, 1, 2):
                    lib.hypre_amd_SetSmallTailForm(form)
                    by_form[form] = _one_cycle(lib, s, A, f, u0, zero)
                    assert 1 <= lib.hypre_amd_BoomerAMGGetSmallTailLevel(s) <= nl - 2, form
                for form in (1, 2):
                    assert by_form[form].tobytes() == by_form[0].tobytes(), (form, float(np.max(np.abs(by_form[form] - by_form[0]))))
                assert by_form[0].tobytes() == out[1].tobytes()
                d = float(np.max(np.abs(out[1] - out[0])) / scale)
                print(which, "relax", relax_type, "zero", zero, "tail on against off", d)
                assert d <= 1e-13
            else:
                assert used[1] == -1, (used, nc)
                assert out[1].tobytes() == out[0].tobytes()
    finally:
        lib.hypre_amd_SetSmallTail(1)
        lib.hypre_amd_SetSmallTailForm(-1)
    lib.HYPRE_BoomerAMGDestroy(s)
    B.check()


@gpu
@pytest.mark.parametrize("which", ["10 to 32 rows", "33 to 64 rows"])
def test_recorded_graph_and_fused_columns_with_a_larger_coarsest_level(gpu_lib, oracle, which):
    """The coarse-tail graph (recorded on the second cycle, replayed from the third) gives the bits of the eager first
    cycle, and every column of a 3-column solve with the fused multi-column cycle the bits of its single-column solve."""
    from hypre_amd import binding as B
    from test_amg_fused_columns_gpu import _bits
    lib = gpu_lib
    opt, A, s, nl, nc, n = _setup(lib, which, 18)
    f = rand_vector(n, 5)
    lev, nodes = C.c_int(), C.c_int()
    for zero in (True, False):
        u0 = np.zeros(n) if zero else rand_vector(n, 6)
        lib.hypre_amd_BoomerAMGSetGraphThreshold(s, 0)
        eager = _one_cycle(lib, s, A, f, u0, zero)
        lib.hypre_amd_BoomerAMGGetGraphInfo(s, C.byref(lev), C.byref(nodes))
        assert lev.value == -1
        lib.hypre_amd_BoomerAMGSetGraphThreshold(s, 100000)
        us = [_one_cycle(lib, s, A, f, u0, zero) for _ in range(4)]        # eager, recorded, replayed twice
        lib.hypre_amd_BoomerAMGGetGraphInfo(s, C.byref(lev), C.byref(nodes))
        print(which, "zero", zero, "graph from level", lev.value, "nodes", nodes.value)
        assert lev.value >= 1 and nodes.value > 0
        for k, u in enumerate(us):
            assert u.tobytes() == eager.tobytes(), (which, zero, k, float(np.max(np.abs(u - eager))))
    before = lib.hypre_amd_SetMultivectorCycle(-1)
    try:
        launches = lib.hypre_amd_SpmvFusedMultivectorLaunches()
        _bits(lib, s, A, n, 3, 2, 51)
        assert lib.hypre_amd_SpmvFusedMultivectorLaunches() > launches
    finally:
        lib.hypre_amd_SetMultivectorCycle(before)
    lib.HYPRE_BoomerAMGDestroy(s)
    B.check()
