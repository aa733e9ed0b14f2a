"""hypre_SetSyncCudaCompute survives every way out of a solve.  Inside HYPRE_ParCSRPCGSolve, HYPRE_ParCSRGMRESSolve,
HYPRE_ParCSRLGMRESSolve and HYPRE_BoomerAMGSolve the synchronisation after each inner call is switched off by a scope
guard (QuietSync, hypre_amd/csrc/internal.hpp); after the call, whether it ran to its end or left by an early return,
hypre_GetSyncCudaCompute reports what the caller had set.  The 6 x 6 x 6 seven-point problem is the smallest whose
hierarchy has two levels, which is all the test needs of its size; the early returns are ordinary refusals and error
returns of host code."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 216


def _sync(lib):
    v = C.c_int(-1)
    lib.hypre_GetSyncCudaCompute(C.byref(v))
    return v.value


def _krylov(lib, name, A, db, dx):
    """(solver, solve function) of PCG / GMRES / LGMRES behind the diagonal scaling, set up on (db, dx)"""
    from test_flexgmres_gpu import _ds
    create = getattr(lib, "HYPRE_ParCSR%sCreate" % name)
    g = C.c_void_p()
    create(0, C.byref(g))
    getattr(lib, "HYPRE_%sSetTol" % name)(g, 1e-8)
    getattr(lib, "HYPRE_%sSetPrecond" % name)(g, *_ds(lib))
    if name != "PCG":
        getattr(lib, "HYPRE_%sSetKDim" % name)(g, 5)
    getattr(lib, "HYPRE_ParCSR%sSetup" % name)(g, A, db, dx)
    return g, getattr(lib, "HYPRE_ParCSR%sSolve" % name)


@pytest.mark.parametrize("setting", [1, 0])
def test_the_callers_setting_survives_every_way_out_of_a_solve(gpu_lib, setting):
    from hypre_amd import binding as B, ij
    lib = gpu_lib
    opt = ij.IJOptions(n=(6, 6, 6), relax_type=18, coarsen_type=8)
    A = ij.build_matrix(opt)
    amg = ij.create_amg(opt, memory_location=B.HYPRE_MEMORY_DEVICE)
    lib.HYPRE_BoomerAMGSetup(amg, A, None, None)
    B.check()
    assert lib.hypre_amd_BoomerAMGGetNumLevels(amg) >= 2
    lib.hypre_ParCSRMatrixMigrate(A, B.HYPRE_MEMORY_DEVICE)
    ones, zeros, bad = np.ones(N), np.zeros(N), np.ones(N)
    bad[3] = np.nan
    made = []

    def vec(values):
        made.append(B.parmultivec_from_numpy(values) if values.ndim == 2 else B.parvec_from_numpy(values))
        return made[-1]

    before = _sync(lib)
    lib.hypre_SetSyncCudaCompute(setting)
    try:
        def after(ret, ok):
            assert (ret == 0) == ok, lib.hypre_amd_LastErrorMessage()
            lib.HYPRE_ClearAllErrors()
            assert _sync(lib) == setting

        # PCG: to the end; b = 0 (x = b, no iteration); a NaN in b
        g, solve = _krylov(lib, "PCG", A, vec(ones), vec(zeros))
        dx = vec(zeros)
        after(solve(g, A, vec(ones), dx), True)
        assert np.all(np.abs(B.parvec_to_numpy(dx) - np.linalg.solve(B.csr_to_scipy(A.contents.diag).toarray(), ones)) < 1e-6)
        k = C.c_int(-1)
        after(solve(g, A, vec(zeros), vec(ones)), True)
        lib.HYPRE_PCGGetNumIterations(g, C.byref(k))
        assert k.value == 0
        after(solve(g, A, vec(bad), vec(zeros)), False)
        lib.HYPRE_ParCSRPCGDestroy(g)

        # GMRES: to the end; a NaN in b
        g, solve = _krylov(lib, "GMRES", A, vec(ones), vec(zeros))
        after(solve(g, A, vec(ones), vec(zeros)), True)
        lib.HYPRE_GMRESGetNumIterations(g, C.byref(k))
        assert k.value > 0
        after(solve(g, A, vec(bad), vec(zeros)), False)
        lib.HYPRE_ParCSRGMRESDestroy(g)

        # LGMRES: to the end; work vectors of another k_dim
        g, solve = _krylov(lib, "LGMRES", A, vec(ones), vec(zeros))
        after(solve(g, A, vec(ones), vec(zeros)), True)
        lib.HYPRE_LGMRESGetNumIterations(g, C.byref(k))
        assert k.value > 0
        lib.HYPRE_LGMRESSetKDim(g, 7)
        ret = solve(g, A, vec(ones), vec(zeros))
        assert b"HYPRE_ParCSRLGMRESSetup after HYPRE_LGMRESSetKDim" in lib.hypre_amd_LastErrorMessage()
        after(ret, False)
        lib.HYPRE_ParCSRLGMRESDestroy(g)

        # BoomerAMG: to the end; a NaN in f; a multivector with a smoother that does not serve one
        lib.HYPRE_BoomerAMGSetMaxIter(amg, 200)
        after(lib.HYPRE_BoomerAMGSolve(amg, A, vec(ones), vec(zeros)), True)
        after(lib.HYPRE_BoomerAMGSolve(amg, A, vec(bad), vec(zeros)), False)
        lib.HYPRE_BoomerAMGDestroy(amg)
        gs = ij.create_amg(ij.IJOptions(n=(6, 6, 6), relax_type=3, coarsen_type=8), memory_location=B.HYPRE_MEMORY_DEVICE)
        Ah = ij.build_matrix(opt)
        lib.HYPRE_BoomerAMGSetup(gs, Ah, None, None)
        lib.hypre_ParCSRMatrixMigrate(Ah, B.HYPRE_MEMORY_DEVICE)
        ret = lib.HYPRE_BoomerAMGSolve(gs, Ah, vec(np.ones((N, 2))), vec(np.zeros((N, 2))))
        assert b"doesn't support multicomponent vectors" in lib.hypre_amd_LastErrorMessage()
        after(ret, False)
        lib.HYPRE_BoomerAMGDestroy(gs)
    finally:
        for v in made:
            lib.hypre_ParVectorDestroy(v)
        lib.HYPRE_ClearAllErrors()
        lib.hypre_SetSyncCudaCompute(before)
