"""Parity of the device solve phase (relaxation, V/W/F cycle, solve, PCG) against
the CPU oracle on the SAME hierarchy (built once by the library's host setup and
handed to both).  fp64.  Tolerances: one sweep / one cycle agree to 1e-12
relative in the max norm (different summation association only); complete
solves must take the identical number of iterations and agree on the final
relative residual to 1e-6 relative (hard part 5)."""
import ctypes as C

import numpy as np
import pytest

from util import rand_vector

pytestmark = pytest.mark.gpu


def _setup(lib, **kw):
    from hypre_amd import binding as B, ij
    opt = ij.IJOptions(**kw)
    A = ij.build_matrix(opt)
    s = ij.create_amg(opt, memory_location=B.HYPRE_MEMORY_DEVICE)
    lib.HYPRE_BoomerAMGSetup(s, A, None, None)
    B.check()
    lib.hypre_ParCSRMatrixMigrate(A, B.HYPRE_MEMORY_DEVICE)
    return opt, A, s


def _level(lib, s, l):
    from hypre_amd import binding as B
    A = C.cast(lib.hypre_amd_BoomerAMGGetA(s, l), C.POINTER(B.ParCSRMatrix))
    cfp = lib.hypre_amd_BoomerAMGGetCFMarker(s, l)
    l1p = lib.hypre_amd_BoomerAMGGetL1Norms(s, l)
    cf = C.cast(cfp, C.POINTER(B.IntArray)).contents.data if cfp else None
    l1 = C.cast(l1p, C.POINTER(B.Vector)).contents.data if l1p else None
    return A, cf, l1


@pytest.mark.parametrize("relax_type,relax_points,w,zero", [
    (18, 0, 1.0, False), (18, 0, 0.8, True), (18, 1, 1.0, False), (18, -1, 0.9, False), (18, 1, 1.0, True),
    (7, 0, 0.7, False), (7, 0, 1.0, True), (0, 0, 0.6, False), (0, 1, 1.0, False), (0, -1, 0.5, False),
    (11, 0, 1.0, False), (12, 0, 0.9, False)])
@pytest.mark.parametrize("level", [0, 1])
def test_single_sweep(gpu_lib, oracle, relax_type, relax_points, w, zero, level):
    from hypre_amd import binding as B
    lib = gpu_lib
    # relax_order=1 makes the setup keep CF-restricted l1 norms like the reference does
    opt, A0, s = _setup(lib, n=(9, 8, 7), relax_type=relax_type if relax_type != 0 else 18, coarsen_type=8,
                        relax_order=1 if relax_points else 0)
    A, cf, l1 = _level(lib, s, level)
    amg = oracle.amg_from_solvers([s])
    n = amg.A_levels[level].nrows
    f = rand_vector(n, 3)
    u0 = np.zeros(n) if zero else rand_vector(n, 4)
    du = B.parvec_from_numpy(u0)
    df = B.parvec_from_numpy(f)
    dv = B.parvec_from_numpy(np.zeros(n))
    dz = B.parvec_from_numpy(np.zeros(n))
    if zero:
        lib.hypre_ParVectorSetZeros(du)
    l1_arg = l1 if relax_type in (7, 18, 11, 12) else None
    err = lib.hypre_BoomerAMGRelax(A, df, cf, relax_type, relax_points, w, 1.0, l1_arg, du, dv, dz)
    B.check()
    assert err == 0 and du.contents.all_zeros == 0
    u = B.parvec_to_numpy(du)
    ur = u0.copy()
    l1_np = amg.l1[level] if relax_type in (7, 18, 11, 12) else None
    oracle.relax(amg.A_levels[level], f, amg.cf[level], relax_type, relax_points, w, 1.0, l1_np, ur, all_zeros=zero)
    assert np.max(np.abs(u - ur)) <= 1e-12 * max(1.0, np.max(np.abs(ur)))
    lib.HYPRE_BoomerAMGDestroy(s)


@pytest.mark.parametrize("level", [0, 1])
def test_two_stage_gs_tends_to_the_gauss_seidel_sweep(gpu_lib, level):
    """The reference's regression set has no job with relax 11 / 12, so beside the oracle comparison the
    two-stage sweep is tied to the golden-pinned hybrid Gauss-Seidel through the identity it is built on
    (par_relax.c:1506-1588): u + sum_{j<=k} (-D^-1 L)^j D^-1 (f - A u)  ->  u + (D + L)^-1 (f - A u), the forward
    Gauss-Seidel sweep, as the number of inner iterations k grows (here rho(D^-1 L) <= 1/2 and k = 60)."""
    from hypre_amd import binding as B
    lib = gpu_lib
    opt, A0, s = _setup(lib, n=(11, 10, 9), relax_type=11, coarsen_type=8)
    A, cf, l1 = _level(lib, s, level)                      # relax 11/12: l1 holds the diagonal (ams.c:695-726, option 5)
    n = A.contents.diag.contents.num_rows
    f, u0 = rand_vector(n, 7), rand_vector(n, 8)
    du, df = B.parvec_from_numpy(u0), B.parvec_from_numpy(f)
    dr, dz = B.parvec_from_numpy(np.zeros(n)), B.parvec_from_numpy(np.zeros(n))
    lib.hypre_BoomerAMGRelaxTwoStageGaussSeidelDevice(A, df, 1.0, 1.0, l1, du, dr, dz, 60)
    B.check()
    u_ts = B.parvec_to_numpy(du)
    dg, dv, dw = B.parvec_from_numpy(u0), B.parvec_from_numpy(np.zeros(n)), B.parvec_from_numpy(np.zeros(n))
    lib.hypre_BoomerAMGRelax(A, df, None, 3, 0, 1.0, 1.0, None, dg, dv, dw)          # forward Gauss-Seidel on one rank
    B.check()
    u_gs = B.parvec_to_numpy(dg)
    assert np.max(np.abs(u_ts - u_gs)) <= 1e-12 * np.max(np.abs(u_gs))
    # and the sweeps the cycle uses are the first partial sums of that series
    for k, relax_type in ((1, 11), (2, 12)):
        da, db = B.parvec_from_numpy(u0), B.parvec_from_numpy(u0)
        lib.hypre_BoomerAMGRelaxTwoStageGaussSeidelDevice(A, df, 1.0, 1.0, l1, da, dr, dz, k)
        lib.hypre_BoomerAMGRelax(A, df, None, relax_type, 0, 1.0, 1.0, l1, db, dv, dw)
        B.check()
        assert np.array_equal(B.parvec_to_numpy(da), B.parvec_to_numpy(db))
    # the sweep in two or three passes (hypre_amd_SetCycleFusion: residual already scaled by the diagonal, "u += z" folded into
    # the first inner step) is the sweep in four or five, bit for bit — from a non-zero and from a zero iterate
    try:
        for k in (1, 2, 3):
            for zero in (False, True):
                res = []
                for on in (1, 0):
                    lib.hypre_amd_SetCycleFusion(on)
                    da = B.parvec_from_numpy(np.zeros(n) if zero else u0)
                    if zero:
                        lib.hypre_ParVectorSetZeros(da)
                    lib.hypre_BoomerAMGRelaxTwoStageGaussSeidelDevice(A, df, 0.9, 1.0, l1, da, dr, dz, k)
                    B.check()
                    res.append(B.parvec_to_numpy(da))
                assert np.array_equal(res[0].view(np.int64), res[1].view(np.int64)), (k, zero)
    finally:
        lib.hypre_amd_SetCycleFusion(1)
    lib.HYPRE_BoomerAMGDestroy(s)


@pytest.mark.parametrize("relax_type", [3, 4, 6, 8, 13, 14, 88, 89])
@pytest.mark.parametrize("relax_points,w,omega", [(0, 1.0, 1.0), (1, 1.0, 1.0), (-1, 1.0, 1.0), (0, 0.8, 1.2), (1, 0.9, 1.0)])
@pytest.mark.parametrize("level", [0, 1])
def test_hybrid_gauss_seidel_sweep_is_the_sequential_sweep(gpu_lib, oracle, relax_type, relax_points, w, omega, level):
    """Level-scheduled device sweep == the oracle's in-order row loop, bit for bit (same row
    sums in stored order, no fused multiply-add), for every member of the hybrid GS/SOR family."""
    from hypre_amd import binding as B
    lib = gpu_lib
    opt, A0, s = _setup(lib, n=(9, 8, 7), relax_type=relax_type, coarsen_type=8, relax_order=1 if relax_points else 0)
    A, cf, l1 = _level(lib, s, level)
    amg = oracle.amg_from_solvers([s])
    n = amg.A_levels[level].nrows
    f = rand_vector(n, 3)
    u0 = rand_vector(n, 4)
    du, df = B.parvec_from_numpy(u0), B.parvec_from_numpy(f)
    dv, dz = B.parvec_from_numpy(np.zeros(n)), B.parvec_from_numpy(np.zeros(n))
    uses_l1 = relax_type in (8, 13, 14, 88, 89)
    err = lib.hypre_BoomerAMGRelax(A, df, cf, relax_type, relax_points, w, omega, l1 if uses_l1 else None, du, dv, dz)
    B.check()
    assert err == 0
    u = B.parvec_to_numpy(du)
    ur = u0.copy()
    oracle.relax(amg.A_levels[level], f, amg.cf[level], relax_type, relax_points, w, omega,
                 amg.l1[level] if uses_l1 else None, ur)
    assert np.array_equal(u, ur), float(np.max(np.abs(u - ur)))
    lib.HYPRE_BoomerAMGDestroy(s)


@pytest.mark.parametrize("kw", [
    dict(relax_type=18, coarsen_type=8),
    dict(relax_type=18, coarsen_type=8, relax_order=1),
    dict(relax_type=18, coarsen_type=10, num_sweeps=2),
    dict(relax_type=7, coarsen_type=8, relax_wt=0.8),
    dict(relax_type=0, coarsen_type=9, P_max_elmts=0, relax_wt=0.7),
    dict(relax_type=18, coarsen_type=8, cycle_type=2),
    dict(relax_type=18, coarsen_type=8, fcycle=1),
    dict(relax_type=11, coarsen_type=8),
    dict(relax_type=12, coarsen_type=8),
    dict(relax_type=18, coarsen_type=8, problem="27pt"),
    dict(relax_type=6, coarsen_type=8),
    dict(relax_type=17, coarsen_type=10, relax_wt=0.9),
    dict(relax_type=15, coarsen_type=8, num_sweeps=2),
    dict(relax_type=17, coarsen_type=8, relax_coarse=17),
    dict(relax_type=3, coarsen_type=10, relax_order=1),
    dict(relax_type=8, coarsen_type=8),
    dict(relax_type=13, coarsen_type=10, num_threads=3),
    dict(relax_type=6, coarsen_type=8, num_threads=4),
    dict(relax_type=89, coarsen_type=8, problem="27pt"),
    dict(relax_type=-1, coarsen_type=10),
    dict(relax_type=16, coarsen_type=8),
    dict(relax_type=16, coarsen_type=8, cheby_order=4, cheby_fraction=0.2),
    dict(relax_type=16, coarsen_type=10, cheby_order=3, cheby_variant=1),
    dict(relax_type=16, coarsen_type=8, cheby_scale=0, problem="27pt"),
    dict(relax_type=16, coarsen_type=8, cheby_eig_est=0, cheby_order=1, num_sweeps=2),
    dict(relax_type=16, coarsen_type=8, cheby_eig_est=0, cheby_scale=0, cycle_type=2),
])
def test_one_cycle_matches_oracle(gpu_lib, oracle, kw):
    from hypre_amd import binding as B
    lib = gpu_lib
    opt, A, s = _setup(lib, n=(12, 11, 10), **kw)
    amg = oracle.amg_from_solvers([s], num_threads=opt.num_threads)
    n = amg.A_levels[0].nrows
    f = rand_vector(n, 5)
    for zero in (True, False):
        u0 = np.zeros(n) if zero else rand_vector(n, 6)
        du, df = B.parvec_from_numpy(u0), B.parvec_from_numpy(f)
        if zero:
            lib.hypre_ParVectorSetZeros(du)
        lib.HYPRE_BoomerAMGSetTol(s, 0.0)
        lib.HYPRE_BoomerAMGSetMaxIter(s, 1)
        lib.HYPRE_BoomerAMGSolve(s, A, df, du)
        B.check()
        u = B.parvec_to_numpy(du)
        ur = u0.copy()
        amg.cycle(f, ur, u_all_zeros=zero)
        assert np.max(np.abs(u - ur)) <= 1e-11 * np.max(np.abs(ur)), (kw, zero)
    lib.HYPRE_BoomerAMGDestroy(s)


@pytest.mark.parametrize("kw", [
    dict(relax_type=18, coarsen_type=8),
    dict(relax_type=18, coarsen_type=10, relax_order=1),
    dict(relax_type=0, coarsen_type=9, P_max_elmts=0, rhs="xisone"),
    dict(relax_type=12, coarsen_type=8),
])
def test_amg_solve_iterations_match_oracle(gpu_lib, oracle, kw):
    from hypre_amd import binding as B, ij
    lib = gpu_lib
    opt, A, s = _setup(lib, n=(16, 16, 16), **kw)
    amg = oracle.amg_from_solvers([s])
    n = amg.A_levels[0].nrows
    b, x0 = ij.build_rhs_host(opt, A)
    if b is None:
        b = np.zeros(n)
        oracle.par_matvec(1.0, amg.A_levels[0], np.ones(n), 0.0, b, b)
    its_r, rel_r, conv_r, hist = amg.solve(b, x0.copy(), tol=opt.tol, max_iter=opt.mg_max_iter)
    dx, db = B.parvec_from_numpy(x0), B.parvec_from_numpy(b)
    lib.HYPRE_BoomerAMGSolve(s, A, db, dx)
    its, rel = C.c_int(), C.c_double()
    lib.HYPRE_BoomerAMGGetNumIterations(s, C.byref(its))
    lib.HYPRE_BoomerAMGGetFinalRelativeResidualNorm(s, C.byref(rel))
    B.check()
    assert its.value == its_r
    assert abs(rel.value - rel_r) <= 1e-6 * rel_r
    lib.HYPRE_BoomerAMGDestroy(s)


@pytest.mark.parametrize("kw", [
    dict(relax_type=18, coarsen_type=8),
    dict(relax_type=18, coarsen_type=8, relax_order=1),
    dict(relax_type=7, coarsen_type=10, relax_wt=0.8),
    dict(relax_type=18, coarsen_type=8, problem="difconv", c=(1.0, 1.0, 0.001), a=(0.0, 0.0, 0.0)),
    dict(relax_type=18, coarsen_type=8, problem="27pt", cycle_type=2),
])
def test_mixed_precision_cycle(gpu_lib, oracle, kw):
    """BASELINE config C5's arithmetic: matrix values streamed as fp32, vectors, accumulation,
    smoother diagonals and the coarse solve in fp64.  That is the fp64 cycle of the hierarchy whose
    operator / interpolation values are rounded to fp32, so the oracle on that hierarchy is matched to
    1e-11 (summation association only); against the unrounded fp64 cycle the difference is fp32-sized."""
    from hypre_amd import binding as B
    lib = gpu_lib
    opt, A, s = _setup(lib, n=(12, 11, 10), **kw)
    lib.hypre_amd_BoomerAMGSetMixedPrecision(s, 1)
    amg32 = oracle.amg_from_solvers([s], mixed_precision=True)
    amg64 = oracle.amg_from_solvers([s])
    n = amg64.A_levels[0].nrows
    f = rand_vector(n, 5)
    for zero in (True, False):
        u0 = np.zeros(n) if zero else rand_vector(n, 6)
        du, df = B.parvec_from_numpy(u0), B.parvec_from_numpy(f)
        if zero:
            lib.hypre_ParVectorSetZeros(du)
        lib.HYPRE_BoomerAMGSetTol(s, 0.0)
        lib.HYPRE_BoomerAMGSetMaxIter(s, 1)
        lib.HYPRE_BoomerAMGSolve(s, A, df, du)
        B.check()
        u = B.parvec_to_numpy(du)
        u32, u64 = u0.copy(), u0.copy()
        # one pass of the solve loop: from a non-zero guess the mixed cycle works on the error equation (fp64 residual
        # with the exact operator, cycle from zero, fp64 correction)
        amg32.solve(f, u32, tol=0.0, max_iter=1, u_all_zeros=zero)
        amg64.cycle(f, u64, u_all_zeros=zero)
        scale = np.max(np.abs(u64))
        assert np.max(np.abs(u - u32)) <= 1e-11 * scale, (kw, zero)
        d64 = np.max(np.abs(u - u64)) / scale
        assert 0.0 < d64 <= 1e-5, (kw, zero, d64)
    lib.HYPRE_BoomerAMGDestroy(s)


def test_mixed_precision_preconditioner_keeps_pcg_convergence(gpu_lib, oracle):
    """Anisotropic diffusion (ij -difconv -c 1 1 0.001), AMG in mixed precision as the PCG
    preconditioner: PCG itself is fp64, converges to the same tolerance within one iteration of the
    all-fp64 run."""
    kw = dict(n=(20, 20, 20), problem="difconv", c=(1.0, 1.0, 0.001), a=(0.0, 0.0, 0.0), relax_type=18, coarsen_type=8)
    its64, rel64 = _pcg_on_device(gpu_lib, **kw)
    its32, rel32 = _pcg_on_device(gpu_lib, mixed=True, **kw)
    assert abs(its32 - its64) <= 1
    assert rel32 < 1e-8 and rel64 < 1e-8


def _pcg_on_device(lib, mixed=False, **kw):
    from hypre_amd import binding as B, ij
    opt, A, s = _setup(lib, solver=1, **kw)
    if mixed:
        lib.hypre_amd_BoomerAMGSetMixedPrecision(s, 1)
    lib.HYPRE_BoomerAMGSetTol(s, 0.0)
    lib.HYPRE_BoomerAMGSetMaxIter(s, 1)
    b, x0 = ij.build_rhs_host(opt, A)
    dx, db = B.parvec_from_numpy(x0), B.parvec_from_numpy(b)
    pcg = C.c_void_p()
    lib.HYPRE_ParCSRPCGCreate(0, C.byref(pcg))
    lib.HYPRE_PCGSetTol(pcg, opt.tol)
    lib.HYPRE_PCGSetMaxIter(pcg, opt.max_iter)
    lib.HYPRE_PCGSetTwoNorm(pcg, 1)
    lib.HYPRE_PCGSetPrecond(pcg, C.cast(lib.HYPRE_BoomerAMGSolve, C.c_void_p), None, s)
    lib.HYPRE_ParCSRPCGSetup(pcg, A, db, dx)
    lib.HYPRE_ParCSRPCGSolve(pcg, A, db, dx)
    its, rel = C.c_int(), C.c_double()
    lib.HYPRE_PCGGetNumIterations(pcg, C.byref(its))
    lib.HYPRE_PCGGetFinalRelativeResidualNorm(pcg, C.byref(rel))
    B.check()
    lib.HYPRE_ParCSRPCGDestroy(pcg)
    lib.HYPRE_BoomerAMGDestroy(s)
    return its.value, rel.value


@pytest.mark.parametrize("kw", [dict(n=(12, 11, 10), relax_type=18, coarsen_type=8),
                                dict(n=(12, 11, 10), relax_type=18, coarsen_type=8, k_dim=3, precon_cycles=2),
                                dict(n=(10, 10, 10)),
                                dict(n=(9, 9, 9), problem="difconv", a=(10.0, 10.0, 10.0), relax_type=7, tol=1e-10)])
def test_gmres_on_device_matches_oracle(gpu_lib, oracle, kw):
    """AMG-GMRES (krylov/gmres.c:274-1000) on the device against the oracle's restatement: same iteration
    count (restarts included: k_dim 3 / 5), same final residual, same solution — also on a nonsymmetric
    convection-diffusion operator, where PCG does not apply."""
    from hypre_amd import binding as B, ij
    lib = gpu_lib
    opt, A, s = _setup(lib, solver=3, **kw)
    amg = oracle.amg_from_solvers([s])
    b, x0 = ij.build_rhs_host(opt, A)
    dx, db = B.parvec_from_numpy(x0), B.parvec_from_numpy(b)
    its, rel = ij.solve_gmres(opt, s, A, db, dx)
    B.check()
    xo = x0.copy()
    oits, orel, _ = amg.gmres(b, xo, tol=opt.tol, max_iter=opt.max_iter, k_dim=opt.k_dim, precond_cycles=opt.precon_cycles)
    assert its == oits and its > opt.k_dim - 2
    assert abs(rel - orel) <= 1e-6 * orel + 5e-15        # relative residuals near 1e-10 carry the rounding of |b|-sized sums
    xd = B.parvec_to_numpy(dx)
    assert np.max(np.abs(xd - xo)) <= 1e-9 * np.max(np.abs(xo))
    lib.HYPRE_BoomerAMGDestroy(s)


def test_gmres_reports_non_convergence(gpu_lib):
    """gmres.c:982-985: HYPRE_ERROR_CONV when max_iter is hit above the tolerance."""
    from hypre_amd import binding as B, ij
    lib = gpu_lib
    opt, A, s = _setup(lib, solver=3, n=(10, 10, 10), relax_type=18, coarsen_type=8, max_iter=2)
    b, x0 = ij.build_rhs_host(opt, A)
    dx, db = B.parvec_from_numpy(x0), B.parvec_from_numpy(b)
    its, rel = ij.solve_gmres(opt, s, A, db, dx)
    assert its == 2 and rel > opt.tol
    assert lib.HYPRE_GetError() & 256
    lib.HYPRE_ClearAllErrors()
    lib.HYPRE_BoomerAMGDestroy(s)


def test_golden_fsai103_pcg_relax7_on_device(gpu_lib):
    """TEST_ij/fsai.saved:89-91 — `ij -n 10 10 10 -solver 1 -rlx 7`: 22 iterations, 7.480945e-09."""
    its, rel = _pcg_on_device(gpu_lib, n=(10, 10, 10), relax_type=7)
    assert its == 22
    assert abs(rel - 7.480945e-09) <= 1e-6 * 7.480945e-09


def test_survey_c1_default_smoothers_on_device(gpu_lib):
    """BASELINE config C1: `ij -laplacian -n 64 64 64 -solver 1` with the CPU defaults
    (HMIS, ext+i, hybrid l1-GS 13 down / 14 up in the 8 thread blocks of the reference's OpenMP run):
    8 PCG iterations, final relative residual 7.176874e-09 — here with every sweep on the GPU."""
    its, rel = _pcg_on_device(gpu_lib, n=(64, 64, 64), num_threads=8)
    assert its == 8
    assert abs(rel - 7.176874e-09) <= 5e-7 * 7.176874e-09


def test_golden_default0_relax0_on_device(gpu_lib):
    """TEST_ij/default.saved:1-6 — `ij -pmis1 -Pmx 0 -rlx 0 -xisone`: average convergence
    factor 0.678738, grid complexity 1.407000, operator complexity 3.252344."""
    from hypre_amd import binding as B, ij
    lib = gpu_lib
    opt, A, s = _setup(lib, coarsen_type=9, P_max_elmts=0, relax_type=0, rhs="xisone")
    g, o = C.c_double(), C.c_double()
    lib.hypre_amd_BoomerAMGGetComplexities(s, C.byref(g), C.byref(o))
    assert round(g.value, 6) == 1.407000 and round(o.value, 6) == 3.252344
    n = 1000
    dx = B.parvec_from_numpy(np.ones(n))
    db = B.parvec_from_numpy(np.zeros(n))
    lib.hypre_ParCSRMatrixMatvec(1.0, A, dx, 0.0, db)
    lib.hypre_ParVectorSetConstantValues(dx, 0.0)
    r0 = np.linalg.norm(B.parvec_to_numpy(db))
    lib.HYPRE_BoomerAMGSolve(s, A, db, dx)
    its, rel = C.c_int(), C.c_double()
    lib.HYPRE_BoomerAMGGetNumIterations(s, C.byref(its))
    lib.HYPRE_BoomerAMGGetFinalRelativeResidualNorm(s, C.byref(rel))
    B.check()
    cf = rel.value ** (1.0 / its.value)
    assert its.value == 48 and abs(cf - 0.678738) < 5e-7
    lib.HYPRE_BoomerAMGDestroy(s)


def test_host_hierarchy_fails_loudly(gpu_lib):
    from hypre_amd import binding as B, ij
    lib = gpu_lib
    opt = ij.IJOptions(relax_type=18, coarsen_type=8)
    A = ij.build_matrix(opt)
    s = ij.create_amg(opt, memory_location=B.HYPRE_MEMORY_HOST)
    lib.HYPRE_BoomerAMGSetup(s, A, None, None)
    B.check()
    hx = B.parvec_from_numpy(np.zeros(1000), location=B.HYPRE_MEMORY_HOST)
    hb = B.parvec_from_numpy(np.ones(1000), location=B.HYPRE_MEMORY_HOST)
    lib.HYPRE_BoomerAMGSolve(s, A, hb, hx)
    with pytest.raises(B.HypreAmdError, match="host execution is not part of this library"):
        B.check()


def test_solver_life_cycle_leaves_no_error(gpu_lib, oracle):
    """Set up, solve, set up again on another matrix with another smoother, solve, destroy everything: every free must
    happen in the memory space the object lives in (the sticky error flag stays clear), and the second hierarchy is
    not contaminated by the first."""
    from hypre_amd import binding as B, ij
    lib = gpu_lib
    lib.HYPRE_ClearAllErrors()
    opt1 = ij.IJOptions(n=(10, 9, 8), relax_type=16, coarsen_type=8)           # scaled Chebyshev: per-level vectors
    opt2 = ij.IJOptions(n=(7, 7, 7), relax_type=13, coarsen_type=10, problem="27pt")
    A1, A2 = ij.build_matrix(opt1), ij.build_matrix(opt2)
    s = ij.create_amg(opt1, memory_location=B.HYPRE_MEMORY_DEVICE)
    lib.HYPRE_BoomerAMGSetup(s, A1, None, None)
    lib.hypre_ParCSRMatrixMigrate(A1, B.HYPRE_MEMORY_DEVICE)
    b1, x1 = B.parvec_from_numpy(np.ones(720)), B.parvec_from_numpy(np.zeros(720))
    lib.HYPRE_BoomerAMGSolve(s, A1, b1, x1)
    B.check()
    # same solver object, new problem, new smoother family
    lib.HYPRE_BoomerAMGSetRelaxType(s, 13)
    lib.HYPRE_BoomerAMGSetCycleRelaxType(s, 14, 2)
    lib.HYPRE_BoomerAMGSetCoarsenType(s, 10)
    lib.HYPRE_BoomerAMGSetup(s, A2, None, None)
    lib.hypre_ParCSRMatrixMigrate(A2, B.HYPRE_MEMORY_DEVICE)
    b2, x2 = B.parvec_from_numpy(np.ones(343)), B.parvec_from_numpy(np.zeros(343))
    lib.HYPRE_BoomerAMGSolve(s, A2, b2, x2)
    B.check()
    its, rel = C.c_int(), C.c_double()
    lib.HYPRE_BoomerAMGGetNumIterations(s, C.byref(its))
    lib.HYPRE_BoomerAMGGetFinalRelativeResidualNorm(s, C.byref(rel))
    amg = oracle.amg_from_solvers([s])
    xo = np.zeros(343)
    oits, orel, _, _ = amg.solve(np.ones(343), xo, tol=opt2.tol, max_iter=opt2.mg_max_iter)
    assert its.value == oits and abs(rel.value - orel) <= 1e-6 * orel
    lib.hypre_ParCSRMatrixDestroy(A1)          # the first matrix may go while the solver lives on the second
    B.check()
    lib.HYPRE_BoomerAMGDestroy(s)
    B.check()
    lib.hypre_ParCSRMatrixDestroy(A2)
    for v in (b1, x1, b2, x2):
        lib.hypre_ParVectorDestroy(v)
    B.check()


@pytest.mark.parametrize("kw", [
    dict(relax_type=18), dict(relax_type=18, relax_order=1), dict(relax_type=11), dict(relax_type=12, problem="27pt"),
    dict(relax_down=21, relax_up=22), dict(relax_type=16), dict(relax_type=7, relax_wt=0.8), dict(relax_type=18, mixed=True),
])
def test_coarse_tail_graph_replays_the_same_cycle(gpu_lib, oracle, kw):
    """The coarse tail of the V-cycle is recorded as a HIP graph on the second cycle and replayed afterwards: cycles 1
    (eager), 2 (recorded and launched) and 3, 4 (replayed) give the same result — the oracle's — from a zero and from a
    non-zero guess; changing a smoother weight invalidates the recording and the new cycles follow the new weight."""
    from hypre_amd import binding as B
    lib = gpu_lib
    kw = dict(kw)
    mixed = kw.pop("mixed", False)
    opt, A, s = _setup(lib, n=(30, 29, 28), coarsen_type=8, **kw)
    if mixed:
        lib.hypre_amd_BoomerAMGSetMixedPrecision(s, 1)
    lib.HYPRE_BoomerAMGSetTol(s, 0.0)
    lib.HYPRE_BoomerAMGSetMaxIter(s, 1)
    n = 30 * 29 * 28
    f = rand_vector(n, 5)
    lev, nodes = C.c_int(), C.c_int()

    def check(rounds):
        amg = oracle.amg_from_solvers([s], mixed_precision=mixed)
        for k in range(rounds):
            zero = k % 2 == 0
            u0 = np.zeros(n) if zero else rand_vector(n, 6 + k)
            du, df = B.parvec_from_numpy(u0), B.parvec_from_numpy(f)
            if zero:
                lib.hypre_ParVectorSetZeros(du)
            lib.HYPRE_BoomerAMGSolve(s, A, df, du)
            B.check()
            ur = u0.copy()
            amg.solve(f, ur, tol=0.0, max_iter=1, u_all_zeros=zero)
            assert np.max(np.abs(B.parvec_to_numpy(du) - ur)) <= 1e-11 * np.max(np.abs(ur)), (kw, k)

    check(4)
    lib.hypre_amd_BoomerAMGGetGraphInfo(s, C.byref(lev), C.byref(nodes))
    assert lev.value >= 1 and nodes.value > 5
    # a different weight on every level: the recording must not survive it
    view = C.cast(s, C.POINTER(oracle.AmgDataView)).contents
    for l in range(lib.hypre_amd_BoomerAMGGetNumLevels(s)):
        view.relax_weight[l] = 0.9
    check(4)
    # and switched off
    lib.hypre_amd_BoomerAMGSetGraphThreshold(s, 0)
    check(2)
    lib.hypre_amd_BoomerAMGGetGraphInfo(s, C.byref(lev), C.byref(nodes))
    assert lev.value == -1
    lib.HYPRE_BoomerAMGDestroy(s)


@pytest.mark.parametrize("kw", [dict(n=(40, 39, 38)), dict(n=(30, 30, 30), problem="27pt"),
                                dict(n=(36, 35, 34), problem="difconv", c=(1.0, 1.0, 0.001), a=(0.0, 0.0, 0.0)),
                                dict(n=(40, 40, 40), coarsen_type=10, P_max_elmts=0)])
def test_device_galerkin_product_is_the_host_product(gpu_lib, kw):
    """Setup with the Galerkin products formed on the device (one wave per coarse row, the host loop's order) and on the
    host: every level's operator identical array for array — row pointers, column order, values bit for bit — and so
    are the stored transposes of the interpolation operators (device transpose vs host counting sort)."""
    from hypre_amd import binding as B, ij
    lib = gpu_lib
    hier = []
    for on in (0, 1):
        lib.hypre_amd_SetSetupDeviceRAP(on, 50)
        lib.hypre_amd_SetSetupDeviceInterp(0)
        opt = ij.IJOptions(relax_type=18, **dict(dict(coarsen_type=8), **kw))
        A = ij.build_matrix(opt)
        s = ij.create_amg(opt, memory_location=B.HYPRE_MEMORY_DEVICE)
        lib.HYPRE_BoomerAMGSetup(s, A, None, None)
        B.check()
        formed = lib.hypre_amd_SetSetupDeviceRAP(-1, -1)
        nl = lib.hypre_amd_BoomerAMGGetNumLevels(s)
        assert (formed >= 2) if on else (formed == 0), (on, formed, nl)
        lv = []
        for l in range(nl):
            Al = C.cast(lib.hypre_amd_BoomerAMGGetA(s, l), C.POINTER(B.ParCSRMatrix))
            lv.append(B.csr_to_arrays(Al.contents.diag))
            if l < nl - 1:
                Pl = C.cast(lib.hypre_amd_BoomerAMGGetP(s, l), C.POINTER(B.ParCSRMatrix))
                lv.append(B.csr_to_arrays(Pl.contents.diagT))
        hier.append(lv)
        lib.HYPRE_BoomerAMGDestroy(s)
    lib.hypre_amd_SetSetupDeviceRAP(1, 20000)
    lib.hypre_amd_SetSetupDeviceInterp(1)
    assert len(hier[0]) == len(hier[1])
    for m0, m1 in zip(hier[0], hier[1]):
        for a, b in zip(m0, m1):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("kw", [dict(n=(40, 39, 38)), dict(n=(30, 30, 30), problem="27pt"),
                                dict(n=(36, 35, 34), problem="difconv", c=(1.0, 1.0, 0.001), a=(0.0, 0.0, 0.0)),
                                dict(n=(34, 33, 32), coarsen_type=10, P_max_elmts=0),
                                dict(n=(30, 30, 30), problem="27pt", P_max_elmts=6, trunc_factor=0.1),
                                dict(n=(40, 40, 20), P_max_elmts=2),
                                dict(n=(32, 32, 32), problem="difconv", c=(1.0, 0.01, 1.0), a=(3.0, 2.0, 1.0), P_max_elmts=0)])
@pytest.mark.parametrize("rung", [0, 2])
def test_device_interpolation_is_the_host_interpolation(gpu_lib, kw, rung):
    """Setup with the extended+i interpolation (and its truncation) computed on the device — one wave per row, the host
    loop's statement order — and on the host: every interpolation operator and every coarse operator identical array
    for array (column order included: the truncated rows keep the order the reference's quicksort leaves them in)."""
    from hypre_amd import binding as B, ij
    lib = gpu_lib
    hier = []
    for on in (0, 1):
        lib.hypre_amd_SetSetupDeviceRAP(0, 50)
        lib.hypre_amd_SetSetupDeviceInterp(on * (1 + rung))          # first rung of the kernel's table sizes
        opt = ij.IJOptions(relax_type=18, **dict(dict(coarsen_type=8), **kw))
        A = ij.build_matrix(opt)
        s = ij.create_amg(opt, memory_location=B.HYPRE_MEMORY_DEVICE)
        lib.HYPRE_BoomerAMGSetup(s, A, None, None)
        B.check()
        built = lib.hypre_amd_SetSetupDeviceInterp(-1)
        nl = lib.hypre_amd_BoomerAMGGetNumLevels(s)
        assert (built >= 2) if on else (built == 0), (on, built, nl)
        lv = []
        for l in range(nl):
            Al = C.cast(lib.hypre_amd_BoomerAMGGetA(s, l), C.POINTER(B.ParCSRMatrix))
            lv.append(B.csr_to_arrays(Al.contents.diag))
            if l < nl - 1:
                Pl = C.cast(lib.hypre_amd_BoomerAMGGetP(s, l), C.POINTER(B.ParCSRMatrix))
                lv.append(B.csr_to_arrays(Pl.contents.diag))
        hier.append(lv)
        lib.HYPRE_BoomerAMGDestroy(s)
    lib.hypre_amd_SetSetupDeviceRAP(1, 20000)
    lib.hypre_amd_SetSetupDeviceInterp(1)
    assert len(hier[0]) == len(hier[1])
    for m0, m1 in zip(hier[0], hier[1]):
        for a, b in zip(m0, m1):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("kw", [dict(n=(40, 39, 38)), dict(n=(30, 30, 30), problem="27pt"),
                                dict(n=(36, 35, 34), problem="difconv", c=(1.0, 1.0, 0.001), a=(0.0, 0.0, 0.0)),
                                dict(n=(40, 39, 38), relax_type=8), dict(n=(34, 33, 32), relax_type=7),
                                dict(n=(34, 33, 32), relax_type=18, relax_order=1),
                                dict(n=(30, 30, 30), problem="27pt", coarsen_type=9, P_max_elmts=6, trunc_factor=0.1),
                                dict(n=(32, 32, 32), problem="difconv", c=(1.0, 0.01, 1.0), a=(3.0, 2.0, 1.0), max_row_sum=0.8),
                                dict(n=(40, 40, 20), strong_threshold=0.6),
                                dict(n=(40, 39, 38), matrix_on_device=True),
                                # other generators of the reference driver: rotated anisotropy (2-D, 9-point), jumping coefficients
                                dict(n=(150, 140, 1), problem="rotate", alpha=60.0, eps=0.1),
                                dict(n=(34, 33, 32), problem="vardifconv", eps=0.1),
                                dict(n=(36, 35, 34), problem="difconv", c=(1.0, 1.0, 1.0), a=(10.0, 10.0, 10.0)),
                                # the device interpolation declines these (truncation by threshold alone): host loop on fetched copies
                                dict(n=(30, 30, 30), P_max_elmts=0, trunc_factor=0.2),
                                dict(n=(30, 30, 30), P_max_elmts=0, trunc_factor=0.2, matrix_on_device=True),
                                dict(n=(20, 20, 20), max_levels=2, matrix_on_device=True)])
def test_device_coarsening_is_the_host_coarsening(gpu_lib, kw):
    """Setup with strength of connection, PMIS, interpolation, Galerkin product and smoother diagonals all on the device
    (nothing fetched between levels; with matrix_on_device the caller's matrix is not copied to the host either) and the
    host setup: C/F markers, interpolation operators, coarse operators and smoother diagonals identical array for array."""
    from hypre_amd import binding as B, ij
    lib = gpu_lib
    kw = dict(kw)
    on_device = kw.pop("matrix_on_device", False)
    hier = []
    for on in (0, 1):
        lib.hypre_amd_SetSetupDeviceRAP(on, 50)
        lib.hypre_amd_SetSetupDeviceInterp(on)
        lib.hypre_amd_SetSetupDeviceCoarsen(on)
        opt = ij.IJOptions(**dict(dict(coarsen_type=8, relax_type=18), **kw))
        A = ij.build_matrix(opt)
        if on and on_device:
            lib.hypre_ParCSRMatrixMigrate(A, B.HYPRE_MEMORY_DEVICE)
        s = ij.create_amg(opt, memory_location=B.HYPRE_MEMORY_DEVICE)
        lib.HYPRE_BoomerAMGSetup(s, A, None, None)
        B.check()
        levels = lib.hypre_amd_SetSetupDeviceCoarsen(-1)
        nl = lib.hypre_amd_BoomerAMGGetNumLevels(s)
        assert (levels >= min(2, nl - 1)) if on else (levels == 0), (on, levels, nl)
        if on and on_device:
            assert A.contents.diag.contents.memory_location == B.HYPRE_MEMORY_DEVICE
        lv = []
        for l in range(nl):
            Al = C.cast(lib.hypre_amd_BoomerAMGGetA(s, l), C.POINTER(B.ParCSRMatrix))
            if l > 0:
                assert Al.contents.diag.contents.memory_location == B.HYPRE_MEMORY_DEVICE
                lv.append(B.csr_to_arrays(Al.contents.diag))
            if l < nl - 1:
                Pl = C.cast(lib.hypre_amd_BoomerAMGGetP(s, l), C.POINTER(B.ParCSRMatrix))
                lv.append(B.csr_to_arrays(Pl.contents.diag))
                lv.append(B.csr_to_arrays(Pl.contents.diagT))
                cf = C.cast(lib.hypre_amd_BoomerAMGGetCFMarker(s, l), C.POINTER(B.IntArray)).contents
                lv.append((B.fetch(cf.data, cf.size, np.int32, cf.memory_location),))
            l1p = lib.hypre_amd_BoomerAMGGetL1Norms(s, l)
            if l1p:
                lv.append((B.vec_to_numpy(C.cast(l1p, C.POINTER(B.Vector))),))
        hier.append(lv)
        lib.HYPRE_BoomerAMGDestroy(s)
    lib.hypre_amd_SetSetupDeviceRAP(1, 20000)
    lib.hypre_amd_SetSetupDeviceInterp(1)
    lib.hypre_amd_SetSetupDeviceCoarsen(1)
    assert len(hier[0]) == len(hier[1])
    for m0, m1 in zip(hier[0], hier[1]):
        assert len(m0) == len(m1)
        for a, b in zip(m0, m1):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("relax_type", [18, 8])
def test_device_setup_on_an_unstructured_matrix(gpu_lib, tmp_path, relax_type):
    """The reference's own unstructured test matrix (test/TEST_ij/data/tucker21935, four IJ files merged into one rank's):
    irregular rows, rows without strong couplings, positive off-diagonal entries.  Device setup == host setup, array for
    array, and the hierarchy solves the system."""
    import os
    from hypre_amd import binding as B, ij
    lib = gpu_lib
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ij_files", "data", "tucker21935")
    rows, n = [], 0
    for r in range(4):
        with open(os.path.join(src, "IJ.A.%05d" % r)) as fh:
            head = fh.readline().split()
            n = max(n, int(head[1]) + 1)
            rows.append(fh.read())
    merged = tmp_path / "IJ.A.00000"
    merged.write_text("0 %d 0 %d\n" % (n - 1, n - 1) + "".join(rows))
    hier, solves = [], []
    for on in (0, 1):
        lib.hypre_amd_SetSetupDeviceRAP(on, -1)
        lib.hypre_amd_SetSetupDeviceInterp(on)
        lib.hypre_amd_SetSetupDeviceCoarsen(on)
        opt = ij.IJOptions(fromfile=str(tmp_path / "IJ.A"), coarsen_type=8, interp_type=6, P_max_elmts=4, relax_type=relax_type)
        A = ij.build_matrix(opt)
        assert A.contents.diag.contents.num_rows == n and n > 20000          # large enough for the device path by default
        s = ij.create_amg(opt, memory_location=B.HYPRE_MEMORY_DEVICE)
        lib.HYPRE_BoomerAMGSetup(s, A, None, None)
        B.check()
        levels = lib.hypre_amd_SetSetupDeviceCoarsen(-1)
        assert (levels >= 1) if on else (levels == 0)
        nl = lib.hypre_amd_BoomerAMGGetNumLevels(s)
        lv = []
        for l in range(nl):
            Al = C.cast(lib.hypre_amd_BoomerAMGGetA(s, l), C.POINTER(B.ParCSRMatrix))
            if l > 0:
                lv.append(B.csr_to_arrays(Al.contents.diag))
            if l < nl - 1:
                Pl = C.cast(lib.hypre_amd_BoomerAMGGetP(s, l), C.POINTER(B.ParCSRMatrix))
                lv.append(B.csr_to_arrays(Pl.contents.diag))
                cf = C.cast(lib.hypre_amd_BoomerAMGGetCFMarker(s, l), C.POINTER(B.IntArray)).contents
                lv.append((B.fetch(cf.data, cf.size, np.int32, cf.memory_location),))
            l1p = lib.hypre_amd_BoomerAMGGetL1Norms(s, l)
            if l1p:
                lv.append((B.vec_to_numpy(C.cast(l1p, C.POINTER(B.Vector))),))
        hier.append(lv)
        lib.hypre_ParCSRMatrixMigrate(A, B.HYPRE_MEMORY_DEVICE)
        b, u = B.parvec_from_numpy(np.ones(n)), B.parvec_from_numpy(np.zeros(n))
        lib.HYPRE_BoomerAMGSetTol(s, 0.0)
        lib.HYPRE_BoomerAMGSetMaxIter(s, 10)                 # ten cycles (the reference solves this one with PCG)
        lib.HYPRE_BoomerAMGSolve(s, A, b, u)
        lib.HYPRE_ClearAllErrors()                           # "not converged within max_iter": expected
        rel = C.c_double()
        lib.HYPRE_BoomerAMGGetFinalRelativeResidualNorm(s, C.byref(rel))
        solves.append((rel.value, B.parvec_to_numpy(u)))
        lib.HYPRE_BoomerAMGDestroy(s)
    lib.hypre_amd_SetSetupDeviceRAP(1, 20000)
    lib.hypre_amd_SetSetupDeviceInterp(1)
    lib.hypre_amd_SetSetupDeviceCoarsen(1)
    assert len(hier[0]) == len(hier[1])
    for m0, m1 in zip(hier[0], hier[1]):
        for a, b in zip(m0, m1):
            assert np.array_equal(a, b)
    assert solves[0][0] == solves[1][0] < 0.5
    assert np.array_equal(solves[0][1], solves[1][1])


def test_graphs_of_two_hierarchies_keep_their_own_diagonal_buffers(gpu_lib, oracle):
    """Weighted Jacobi (relax 0) divides by a diagonal the sweep extracts into a work buffer.  That buffer used to be one
    process-wide, grow-only scratch: a second, larger hierarchy reallocated it under the first one's recorded coarse-tail
    graph.  Now every solver owns a buffer per level: cycles of a small and of a large hierarchy, interleaved, with both
    graphs recorded, each give the oracle's result."""
    from hypre_amd import binding as B
    lib = gpu_lib
    sets = []
    for n in ((24, 24, 24), (44, 43, 42)):
        opt, A, s = _setup(lib, n=n, coarsen_type=8, relax_type=0, relax_wt=0.7)
        lib.HYPRE_BoomerAMGSetTol(s, 0.0)
        lib.HYPRE_BoomerAMGSetMaxIter(s, 1)
        lib.hypre_amd_BoomerAMGSetGraphThreshold(s, 1000000)        # every level below the finest belongs to the tail
        sets.append((n[0] * n[1] * n[2], A, s, oracle.amg_from_solvers([s])))
    lev, nodes = C.c_int(), C.c_int()
    for k in range(5):
        for nn, A, s, amg in sets:                       # small, large, small, large ...
            f = rand_vector(nn, 3 + k)
            du, df = B.parvec_from_numpy(np.zeros(nn)), B.parvec_from_numpy(f)
            lib.hypre_ParVectorSetZeros(du)
            lib.HYPRE_BoomerAMGSolve(s, A, df, du)
            B.check()
            ur = np.zeros(nn)
            amg.solve(f, ur, tol=0.0, max_iter=1, u_all_zeros=True)
            assert np.max(np.abs(B.parvec_to_numpy(du) - ur)) <= 1e-11 * np.max(np.abs(ur)), (nn, k)
    for nn, A, s, amg in sets:
        lib.hypre_amd_BoomerAMGGetGraphInfo(s, C.byref(lev), C.byref(nodes))
        assert lev.value >= 1 and nodes.value > 5
        lib.HYPRE_BoomerAMGDestroy(s)
    B.check()


def test_values_changed_under_a_mixed_precision_hierarchy_are_noticed(gpu_lib):
    """Mixed precision multiplies by an fp32 copy (or an fp32-rounded table) of the matrix values kept in the plan.  Values
    changed in place without hypre_amd_CSRMatrixInvalidatePlan leave that copy behind.  A stand-alone solve (more than one
    cycle allowed) verifies the fine-level plans against the caller's arrays where it begins — the stale plan is replaced
    silently and the solve is the new matrix's; a preconditioner call (one cycle, no verification) is found out by the
    kernels' rotating value check: HYPRE_ERROR_GENERIC instead of silently preconditioning with the old operator."""
    from hypre_amd import binding as B
    lib = gpu_lib
    opt, A, s = _setup(lib, n=(30, 30, 30), coarsen_type=8, relax_type=18)
    lib.hypre_amd_BoomerAMGSetMixedPrecision(s, 1)
    lib.HYPRE_BoomerAMGSetTol(s, 0.0)
    lib.HYPRE_BoomerAMGSetMaxIter(s, 2)
    n = 27000
    du, df = B.parvec_from_numpy(np.zeros(n)), B.parvec_from_numpy(np.ones(n))
    lib.HYPRE_BoomerAMGSolve(s, A, df, du)
    lib.HYPRE_ClearAllErrors()                            # (max_iter reached: expected)
    u_old = B.parvec_to_numpy(du)
    d = A.contents.diag.contents
    vals = B.fetch(d.data, d.num_nonzeros, np.float64, d.memory_location) * 3.0
    lib.hypre_Memcpy(C.cast(d.data, C.c_void_p), vals.ctypes.data_as(C.c_void_p), vals.nbytes, B.HYPRE_MEMORY_DEVICE, B.HYPRE_MEMORY_HOST)
    # stand-alone solve: verified where it begins, nothing raised, and the fine-level operator is the new one (3 A: the
    # hierarchy below is the old one's, so the iterate is not u_old / 3 exactly — but the residual it reports is 3 A's)
    lib.hypre_ParVectorSetZeros(du)
    lib.HYPRE_BoomerAMGSolve(s, A, df, du)
    lib.hypre_SyncComputeStream()
    assert not (lib.HYPRE_GetError() & 1)
    lib.HYPRE_ClearAllErrors()
    assert lib.hypre_amd_CSRMatrixVerifyPlan(A.contents.diag) == 1
    assert np.max(np.abs(B.parvec_to_numpy(du) - u_old)) > 1e-3 * np.max(np.abs(u_old))
    # preconditioner call (one cycle): the kernels notice
    vals = vals / 3.0
    lib.hypre_Memcpy(C.cast(d.data, C.c_void_p), vals.ctypes.data_as(C.c_void_p), vals.nbytes, B.HYPRE_MEMORY_DEVICE, B.HYPRE_MEMORY_HOST)
    lib.HYPRE_BoomerAMGSetMaxIter(s, 1)
    lib.hypre_ParVectorSetZeros(du)
    lib.HYPRE_BoomerAMGSolve(s, A, df, du)
    lib.hypre_SyncComputeStream()
    lib.hypre_ParVectorSetZeros(du)
    lib.HYPRE_BoomerAMGSolve(s, A, df, du)                # (the flag is read when the plan is next asked for)
    assert lib.HYPRE_GetError() & 1           # HYPRE_ERROR_GENERIC: "a kernel found its SpMV plan out of date"
    lib.HYPRE_BoomerAMGDestroy(s)
    lib.HYPRE_ClearAllErrors()


@pytest.mark.parametrize("edit", ["one coefficient in the middle of a tile", "one row scaled"])
@pytest.mark.parametrize("relax_type", [18, 11])
def test_a_new_setup_after_an_in_place_edit_works_on_the_new_values(gpu_lib, oracle, edit, relax_type):
    """The hypre idiom: change some coefficients of the matrix in place (HYPRE_IJMatrixSetValues on the same pattern), call
    HYPRE_BoomerAMGSetup again, solve.  The fine-level operator of these stencils is multiplied from value codes in slice
    form — a private copy of the values — and the setup drops the plans of the matrix it is handed before anything else: with
    NO call to hypre_amd_CSRMatrixInvalidatePlan, one cycle after the new setup is the oracle's cycle on the new matrix
    (hierarchy and fine level alike), and nothing is raised."""
    from hypre_amd import binding as B, ij
    lib = gpu_lib
    opt = ij.IJOptions(n=(24, 22, 20), coarsen_type=8, relax_type=relax_type)
    A = ij.build_matrix(opt)
    lib.hypre_ParCSRMatrixMigrate(A, B.HYPRE_MEMORY_DEVICE)
    s = ij.create_amg(opt, memory_location=B.HYPRE_MEMORY_DEVICE)
    lib.HYPRE_BoomerAMGSetTol(s, 0.0)
    lib.HYPRE_BoomerAMGSetMaxIter(s, 1)
    n = 24 * 22 * 20
    f = rand_vector(n, 5)
    df, du = B.parvec_from_numpy(f), B.parvec_from_numpy(np.zeros(n))

    def one_cycle():
        lib.HYPRE_BoomerAMGSetup(s, A, None, None)
        B.check()
        lib.hypre_ParVectorSetZeros(du)
        lib.HYPRE_BoomerAMGSolve(s, A, df, du)
        B.check()
        u = B.parvec_to_numpy(du)
        amg = oracle.amg_from_solvers([s])
        ur = np.zeros(n)
        amg.cycle(f, ur, u_all_zeros=True)
        return u, ur

    u, ur = one_cycle()
    assert np.max(np.abs(u - ur)) <= 1e-11 * np.max(np.abs(ur))
    d = A.contents.diag.contents
    assert lib.hypre_amd_CSRMatrixPlanForm(A.contents.diag) == 4          # coded, slice form: the values are a private copy
    vals = B.fetch(d.data, d.num_nonzeros, np.float64, d.memory_location).copy()
    rowptr = B.fetch(d.i, d.num_rows + 1, np.int32, d.memory_location)
    if edit.startswith("one coefficient"):
        vals[2048 * 7 + 1001] *= 1.25
    else:
        r = n // 2 + 3
        vals[rowptr[r]:rowptr[r + 1]] *= 1.5
    lib.hypre_Memcpy(C.cast(d.data, C.c_void_p), vals.ctypes.data_as(C.c_void_p), vals.nbytes, B.HYPRE_MEMORY_DEVICE, B.HYPRE_MEMORY_HOST)
    u2, ur2 = one_cycle()
    assert np.max(np.abs(ur2 - ur)) > 1e-6 * np.max(np.abs(ur))            # the edit matters ...
    assert np.max(np.abs(u2 - ur2)) <= 1e-11 * np.max(np.abs(ur2))         # ... and the device cycle is the new matrix's
    lib.HYPRE_BoomerAMGDestroy(s)
    B.check()


@pytest.mark.parametrize("kw", [dict(relax_type=18), dict(relax_type=7, relax_wt=0.8), dict(relax_type=18, cycle_type=2),
                                dict(relax_type=18, mixed=True), dict(relax_type=18, relax_order=1), dict(relax_type=11),
                                dict(relax_type=12, problem="27pt"), dict(relax_type=11, mixed=True)])
def test_the_fusions_across_the_steps_of_a_cycle_change_no_bit(gpu_lib, oracle, kw):
    """hypre_amd_SetCycleFusion.  On one rank the restriction f_c = P^T r also writes the coarse level's first Jacobi-type sweep from
    zero, u_c = (w f_c) ./ d_c (an epilogue of the SpMV kernels instead of a kernel of its own), and a two-stage Gauss-Seidel
    sweep runs in two or three passes instead of four or five (the residual already scaled by the diagonal, "u += z" folded into
    the first inner step).  The cycle is the same BIT FOR BIT with the fusions on and off — eager, recorded as a graph and
    replayed, V- and W-cycles, fp32 matrix values; switching them invalidates a recorded coarse tail (the recording leaves out
    what a fused restriction into it did); CF-ordered sweeps are untouched — and it is the oracle's cycle."""
    from hypre_amd import binding as B
    lib = gpu_lib
    kw = dict(kw)
    mixed = kw.pop("mixed", False)
    opt, A, s = _setup(lib, n=(30, 29, 28), coarsen_type=8, **kw)
    if mixed:
        lib.hypre_amd_BoomerAMGSetMixedPrecision(s, 1)
    lib.HYPRE_BoomerAMGSetTol(s, 0.0)
    lib.HYPRE_BoomerAMGSetMaxIter(s, 1)
    n = 30 * 29 * 28
    f = rand_vector(n, 5)
    amg = oracle.amg_from_solvers([s], mixed_precision=mixed)
    ur = np.zeros(n)
    amg.solve(f, ur, tol=0.0, max_iter=1, u_all_zeros=True)
    out = []
    try:
        for on in (1, 1, 1, 0, 0, 0, 1, 1):                # (three cycles each: eager, recorded, replayed)
            assert lib.hypre_amd_SetCycleFusion(on) == on
            du, df = B.parvec_from_numpy(np.zeros(n)), B.parvec_from_numpy(f)
            lib.hypre_ParVectorSetZeros(du)
            lib.HYPRE_BoomerAMGSolve(s, A, df, du)
            B.check()
            out.append(B.parvec_to_numpy(du))
            lib.hypre_ParVectorDestroy(du); lib.hypre_ParVectorDestroy(df)
    finally:
        lib.hypre_amd_SetCycleFusion(1)
    for u in out:
        assert np.array_equal(u.view(np.int64), out[0].view(np.int64))
    assert np.max(np.abs(out[0] - ur)) <= 1e-11 * np.max(np.abs(ur))
    lib.HYPRE_BoomerAMGDestroy(s)
    B.check()


@pytest.mark.parametrize("kw", [dict(relax_type=18), dict(relax_type=7, relax_wt=0.8), dict(relax_type=18, mixed=True),
                                dict(relax_type=18, problem="27pt"), dict(relax_type=18, n=(40, 12, 9)),
                                dict(relax_type=18, cycle_type=2), dict(relax_type=18, relax_order=1), dict(relax_type=11),
                                dict(relax_type=12, problem="27pt"), dict(relax_type=11, mixed=True), dict(relax_type=18, relax_up=12),
                                dict(relax_type=16)])
def test_the_smallest_levels_in_one_kernel(gpu_lib, oracle, kw):
    """hypre_amd_SetSmallTail.  From the first level whose operators hold at most 20 000 entries down to the direct solve and
    back up, a V(1,1) cycle with Jacobi / l1-Jacobi or two-stage Gauss-Seidel smoothing runs as ONE kernel of one workgroup instead of a dozen launches
    (tail_kernels.hip).  The cycle with it is the cycle without it up to the order of a row's sum (1e-13), the same bits
    eager, recorded in the coarse-tail graph and replayed, it is the oracle's cycle, and configurations it does not serve
    (W-cycles, C/F-ordered sweeps, other smoothers) leave it out."""
    from hypre_amd import binding as B
    lib = gpu_lib
    kw = dict(kw)
    mixed = kw.pop("mixed", False)
    dims = kw.pop("n", (30, 29, 28))
    served = kw.get("cycle_type", 1) == 1 and kw.get("relax_order", 0) == 0 and kw["relax_type"] in (7, 18, 11, 12)
    opt, A, s = _setup(lib, n=dims, coarsen_type=8, **kw)
    if mixed:
        lib.hypre_amd_BoomerAMGSetMixedPrecision(s, 1)
    lib.HYPRE_BoomerAMGSetTol(s, 0.0)
    lib.HYPRE_BoomerAMGSetMaxIter(s, 1)
    n = dims[0] * dims[1] * dims[2]
    f = rand_vector(n, 6)
    amg = oracle.amg_from_solvers([s], mixed_precision=mixed)
    ur = np.zeros(n)
    amg.solve(f, ur, tol=0.0, max_iter=1, u_all_zeros=True)
    nl = lib.hypre_amd_BoomerAMGGetNumLevels(s)
    out, used, by_form = {1: [], 0: []}, {}, {}
    try:
        # (three cycles each: eager, recorded, replayed; then the two other forms of the kernel's image: the first level's
        # operator in the lanes' registers, and streamed from global memory)
        for on, form in ((1, -1), (1, -1), (1, -1), (0, -1), (0, -1), (0, -1), (1, 1), (1, 1), (1, 2), (1, 2), (1, 0)):
            lib.hypre_amd_SetSmallTailForm(form)
            assert lib.hypre_amd_SetSmallTail(on) == on
            du, df = B.parvec_from_numpy(np.zeros(n)), B.parvec_from_numpy(f)
            lib.hypre_ParVectorSetZeros(du)
            lib.HYPRE_BoomerAMGSolve(s, A, df, du)
            B.check()
            if form < 0:
                out[on].append(B.parvec_to_numpy(du))
                used[on] = lib.hypre_amd_BoomerAMGGetSmallTailLevel(s)
            else:
                by_form.setdefault(form, []).append(B.parvec_to_numpy(du))
            lib.hypre_ParVectorDestroy(du); lib.hypre_ParVectorDestroy(df)
    finally:
        lib.hypre_amd_SetSmallTail(1)
        lib.hypre_amd_SetSmallTailForm(-1)
    assert used[0] == -1
    assert (1 <= used[1] <= nl - 2) if served else used[1] == -1, (used, nl)
    for on in (0, 1):
        for u in out[on]:
            assert np.array_equal(u.view(np.int64), out[on][0].view(np.int64))
    scale = np.max(np.abs(ur))
    assert np.max(np.abs(out[1][0] - out[0][0])) <= 1e-13 * scale
    for form, us in by_form.items():
        for u in us:
            assert np.array_equal(u.view(np.int64), us[0].view(np.int64))
            assert np.max(np.abs(u - out[0][0])) <= 1e-13 * scale, form
    assert np.max(np.abs(out[1][0] - ur)) <= 1e-11 * scale
    if not served:
        assert np.array_equal(out[1][0].view(np.int64), out[0][0].view(np.int64))
    lib.HYPRE_BoomerAMGDestroy(s)
    B.check()
