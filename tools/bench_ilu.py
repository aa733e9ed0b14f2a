"""Time of one ILU application on the device:
`python tools/bench_ilu.py [--n 256] [--lfil 0] [--reordering 1] [--reps 20] [--iterative --ljac 5 --ujac 5] [--gmres]`.

The 7-point operator on an n^3 grid (the operator of `bench.py --problem 7pt`), one rank.  Setup (host: ordering,
factorisation, levels; upload) is timed once.  An application — HYPRE_ILUSolve with max_iter 1 and tol 0: the product with A,
the L solve, the U solve with the update of u — is timed over `--reps` calls after `--warmup`, each closed by a device
synchronisation.  Prints one JSON line: milliseconds per application, levels and entries of L and U, launches per
application by kernel form, the bytes an application must move (factors, row and level tables, vectors, and the product's
CSR bytes) and that over the time.

With `--iterative` the triangular solves are `--ljac` / `--ujac` Jacobi sweeps on the factors in row slices
(hypre_amd_ILUSetIterativeTriSolve): the line then also carries the sweep launches per application, the padded entries of
the slice form beside the stored ones, and the bytes are those of the sweeps (per product with a factor 12 bytes a padded
entry, per row the slot tables and the vectors the pass reads and writes: DESIGN.md section 6, ILU).  With `--gmres` the
same object then preconditions GMRES (`ij -solver 81`, restart `--kdim`) on a right-hand side of ones to 1e-8: iterations and
seconds of the solve.

`--amg-smoother 5|15` times something else: one V-cycle of BoomerAMG (PMIS, ext+i) on the same operator with ILU as the smoother
of ALL levels (smooth_num_levels 25, `--sm-sweeps` sweeps, iterative triangular solves of `--ljac` / `--ujac` sweeps), the
accelerated smoother fused (hypre_amd_SetSmootherFusion 1) and unfused (0), and beside them the l1-Jacobi V(1,1) cycle of the
same hierarchy settings.  One JSON line: milliseconds per cycle of the three, smoother visits and read-backs per cycle."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def amg_smoother_cycles(a, L, B, ij):
    """one V-cycle with ILU on all levels, fused and unfused, and the l1-Jacobi cycle: median milliseconds of each"""
    n = a.n ** 3
    f = np.ones(n)

    def cycle_ms(opt, fusion):
        A = ij.build_matrix(opt)
        s = ij.create_amg(ij.check_options(opt), memory_location=B.HYPRE_MEMORY_DEVICE)
        L.HYPRE_BoomerAMGSetup(s, A, None, None)
        B.check()
        L.hypre_ParCSRMatrixMigrate(A, B.HYPRE_MEMORY_DEVICE)
        L.HYPRE_BoomerAMGSetTol(s, 0.0)
        L.HYPRE_BoomerAMGSetMaxIter(s, 1)
        L.hypre_amd_SetSmootherFusion(fusion)
        df, du = B.parvec_from_numpy(f), B.parvec_from_numpy(np.zeros(n))
        times = []
        for k in range(a.warmup + a.reps):
            L.hypre_ParVectorSetZeros(du)
            t0 = time.perf_counter()
            L.HYPRE_BoomerAMGSolve(s, A, df, du)         # ends in a synchronisation of the compute stream
            if k >= a.warmup:
                times.append(time.perf_counter() - t0)
        B.check()
        st = [C.c_int() for _ in range(5)]
        L.hypre_amd_BoomerAMGGetSmootherStats(s, *[C.byref(v) for v in st])
        levels = L.hypre_amd_BoomerAMGGetNumLevels(s)
        L.hypre_amd_SetSmootherFusion(1)
        L.HYPRE_BoomerAMGDestroy(s)
        for v in (df, du):
            L.hypre_ParVectorDestroy(v)
        L.hypre_ParCSRMatrixDestroy(A)
        return 1e3 * float(np.median(times)), 1e3 * min(times), levels, st[3].value, st[4].value

    base = dict(n=(a.n, a.n, a.n), coarsen_type=8, relax_type=18)
    smooth = dict(base, smooth_type=a.amg_smoother, smooth_num_levels=25, smooth_num_sweeps=a.sm_sweeps, ilu_lfil=a.lfil, ilu_reordering=a.reordering,
                  ilu_iterative=1, ilu_ljac_iters=a.ljac, ilu_ujac_iters=a.ujac)
    out = dict(tool="bench_ilu", mode="amg-smoother", n=a.n, rows=n, smooth_type=a.amg_smoother, smooth_num_sweeps=a.sm_sweeps, lfil=a.lfil,
               ljac=a.ljac, ujac=a.ujac)
    for name, opt, fusion in (("fused", smooth, 1), ("unfused", smooth, 0), ("l1_jacobi", base, 1)):
        ms, ms_min, levels, visits, readbacks = cycle_ms(ij.IJOptions(**opt), fusion)
        out.update({"ms_per_cycle_" + name: round(ms, 4), "ms_min_" + name: round(ms_min, 4), "levels": levels})
        if name != "l1_jacobi":
            out.update({"visits_" + name: visits, "readbacks_" + name: readbacks})
    print(json.dumps(out))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--amg-smoother", type=int, choices=(5, 15), default=0, help="time a V-cycle with ILU smoothing on all levels instead")
    ap.add_argument("--sm-sweeps", type=int, default=1, help="smooth_num_sweeps of --amg-smoother")
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--lfil", type=int, default=0)
    ap.add_argument("--reordering", type=int, default=1)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iterative", action="store_true", help="triangular solves as Jacobi sweeps")
    ap.add_argument("--ljac", type=int, default=5)
    ap.add_argument("--ujac", type=int, default=5)
    ap.add_argument("--gmres", action="store_true", help="then ILU-GMRES to 1e-8 with the same object")
    ap.add_argument("--kdim", type=int, default=5)
    a = ap.parse_args()
    from hypre_amd import binding as B, ij
    L = B.load_library(build_if_missing=True)
    if not L.hypre_amd_DeviceAvailable():
        raise SystemExit("bench_ilu: no HIP device")
    if a.amg_smoother:
        return amg_smoother_cycles(a, L, B, ij)
    opt = ij.IJOptions(n=(a.n, a.n, a.n))
    A = ij.build_matrix(opt)
    n = a.n ** 3
    nnzA = int(A.contents.diag.contents.num_nonzeros)
    L.hypre_ParCSRMatrixMigrate(A, B.HYPRE_MEMORY_DEVICE)
    s = C.c_void_p()
    L.HYPRE_ILUCreate(C.byref(s))
    L.HYPRE_ILUSetLevelOfFill(s, a.lfil)
    L.HYPRE_ILUSetLocalReordering(s, a.reordering)
    L.HYPRE_ILUSetMaxIter(s, 1)
    L.HYPRE_ILUSetTol(s, 0.0)
    L.hypre_amd_ILUSetIterativeTriSolve(s, 1 if a.iterative else 0)
    L.HYPRE_ILUSetLowerJacobiIters(s, a.ljac)
    L.HYPRE_ILUSetUpperJacobiIters(s, a.ujac)
    t0 = time.perf_counter()
    L.HYPRE_ILUSetup(s, A, None, None)             # host work and blocking copies
    setup_s = time.perf_counter() - t0
    B.check()
    f, u = B.parvec_from_numpy(np.ones(n)), B.parvec_from_numpy(np.zeros(n))
    times = []
    for k in range(a.warmup + a.reps):
        t0 = time.perf_counter()
        L.HYPRE_ILUSolve(s, A, f, u)                 # ends in a synchronisation of the compute stream (the library's default)
        if k >= a.warmup:
            times.append(time.perf_counter() - t0)
    B.check()
    st = [C.c_int() for _ in range(6)]
    L.hypre_amd_ILUGetSolveStats(s, *[C.byref(v) for v in st])
    levels_L, levels_U, runs, grids, nnzL, nnzU = (v.value for v in st)
    tri_bytes = 12.0 * (nnzL + nnzU) + 64.0 * n + 4.0 * (levels_L + levels_U)
    extra = {}
    if a.iterative:
        it = [C.c_int() for _ in range(4)]
        pad = [C.c_longlong() for _ in range(2)]
        L.hypre_amd_ILUGetIterativeStats(s, *[C.byref(v) for v in it + pad])
        padL, padU = pad[0].value, pad[1].value
        lo, up, slices = a.ljac, a.ujac, (n + 63) // 64
        # (lo - 1) products with L, the last storing Dinv y as well; (up - 1) with U, the last updating u; lo, up >= 2
        # (ILU; the library's own count of one application is printed beside it)
        tri_bytes = (lo - 1) * (12.0 * padL + 32.0 * n) + 16.0 * n + (up - 1) * (12.0 * padU + 40.0 * n) + 8.0 * n + 8.0 * slices * (lo + up - 2) \
            if lo >= 2 and up >= 2 else float("nan")
        L.hypre_amd_ByteCounters(None, None, 1)
        L.HYPRE_ILUSolve(s, A, f, u)
        counted = C.c_double()
        L.hypre_amd_ByteCounters(None, C.byref(counted), 1)
        extra = dict(iterative=1, ljac=lo, ujac=up, sweep_launches=it[3].value, padded_nnz_L=padL, padded_nnz_U=padU,
                     padding_L=round(padL / max(nnzL, 1), 4), padding_U=round(padU / max(nnzU, 1), 4),
                     counted_bytes_per_application=counted.value)
    if a.gmres:
        g = C.c_void_p()
        L.HYPRE_ParCSRGMRESCreate(0, C.byref(g))
        L.HYPRE_GMRESSetKDim(g, a.kdim)
        L.HYPRE_GMRESSetMaxIter(g, 5000)
        L.HYPRE_GMRESSetTol(g, 1e-8)
        L.HYPRE_GMRESSetPrecond(g, C.cast(L.HYPRE_ILUSolve, C.c_void_p), C.cast(L.HYPRE_ILUSetup, C.c_void_p), s)
        x = B.parvec_from_numpy(np.zeros(n))
        t0 = time.perf_counter()
        L.HYPRE_ParCSRGMRESSetup(g, A, f, x)           # factors again (host work)
        gsetup = time.perf_counter() - t0
        solves = []
        for _ in range(2):                             # the second run is the one reported
            L.hypre_ParVectorSetConstantValues(x, 0.0)
            t0 = time.perf_counter()
            L.HYPRE_ParCSRGMRESSolve(g, A, f, x)
            solves.append(time.perf_counter() - t0)
        gits, grel = C.c_int(), C.c_double()
        L.HYPRE_GMRESGetNumIterations(g, C.byref(gits)); L.HYPRE_GMRESGetFinalRelativeResidualNorm(g, C.byref(grel))
        L.HYPRE_ClearError(256)
        B.check()
        extra.update(gmres_kdim=a.kdim, gmres_iterations=gits.value, gmres_rel_resid=grel.value, gmres_solve_s=round(solves[-1], 4),
                     gmres_setup_s=round(gsetup, 3))
        L.HYPRE_ParCSRGMRESDestroy(g)
        L.hypre_ParVectorDestroy(x)
    spmv_bytes = 12.0 * nnzA + 4.0 * n + 3 * 8.0 * n
    ms = 1e3 * float(np.median(times))
    print(json.dumps(dict(tool="bench_ilu", n=a.n, rows=n, lfil=a.lfil, reordering=a.reordering, setup_s=round(setup_s, 3),
                          ms_per_application=round(ms, 4), ms_min=round(1e3 * min(times), 4), levels_L=levels_L, levels_U=levels_U,
                          run_launches=runs, level_launches=grids, nnz_L=nnzL, nnz_U=nnzU,
                          us_per_level=round(1e3 * ms / max(levels_L + levels_U, 1), 3),
                          triangular_bytes=tri_bytes, product_bytes=spmv_bytes,
                          tb_per_s=round((tri_bytes + spmv_bytes) / (ms * 1e-3) / 1e12, 4), **extra)))
    L.HYPRE_ILUDestroy(s)
    for v in (f, u):
        L.hypre_ParVectorDestroy(v)
    L.hypre_ParCSRMatrixDestroy(A)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
