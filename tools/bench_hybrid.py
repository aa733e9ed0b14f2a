"""Time per iteration of diagonally scaled PCG (HYPRE_ParCSRPCG* behind HYPRE_ParCSRDiagScale, `ij -solver 2`) on one GPU
with the fused step (hypre_amd_PCGSetFusedDiagScale) and with the three launches it stands for, on the 7-point operator of
`bench.py`; then, once each, the hybrid solver (HYPRE_ParCSRHybrid*) to 1e-8 against AMG-PCG with its setup, on that
operator and on the anisotropic one of `bench.py --problem difconv`.

    python tools/bench_hybrid.py --grid 256 --iters 50 --reps 3 --out profiles/hybrid_dscg_ab.json

Every timed DS-PCG solve runs with tol 0 and a fixed iteration count, so both legs take the same steps; the legs are timed in
turn `--reps` times after one untimed solve each, with events on the compute stream around HYPRE_ParCSRPCGSolve (the solve
begins with one residual, two preconditioner applications and two inner products, which the figure per iteration
includes).  The results are printed as one JSON document and written to --out."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from hypre_amd import binding as B, ij  # noqa: E402


def _ds_pcg(L, A, b, n, tol, max_iter, fused):
    """(ms of the Solve, iterations, reported norm, whether the fused step ran)"""
    db, dx = B.parvec_from_numpy(b), B.parvec_from_numpy(np.zeros(n))
    g = C.c_void_p()
    L.HYPRE_ParCSRPCGCreate(0, C.byref(g))
    L.HYPRE_PCGSetTol(g, tol)
    L.HYPRE_PCGSetMaxIter(g, max_iter)
    L.HYPRE_PCGSetTwoNorm(g, 1)
    L.HYPRE_PCGSetPrecond(g, C.cast(L.HYPRE_ParCSRDiagScale, C.c_void_p), C.cast(L.HYPRE_ParCSRDiagScaleSetup, C.c_void_p), None)
    L.hypre_amd_PCGSetFusedDiagScale(g, fused)
    L.HYPRE_ParCSRPCGSetup(g, A, db, dx)
    used = C.c_int()
    L.hypre_amd_PCGGetFusedDiagScaleUsed(g, C.byref(used))
    L.hypre_SyncComputeStream()
    L.hypre_amd_EventTimerStart()
    L.HYPRE_ParCSRPCGSolve(g, A, db, dx)
    ms = L.hypre_amd_EventTimerStopMs()
    L.HYPRE_ClearError(256)                   # tol 0: the solve ends at max_iter
    B.check()
    its, rel = C.c_int(), C.c_double()
    L.HYPRE_PCGGetNumIterations(g, C.byref(its))
    L.HYPRE_PCGGetFinalRelativeResidualNorm(g, C.byref(rel))
    L.HYPRE_ParCSRPCGDestroy(g)
    L.hypre_ParVectorDestroy(db); L.hypre_ParVectorDestroy(dx)
    return ms, its.value, rel.value, used.value


def _to_1e_8(L, opt, cf_tol):
    """wall-clock seconds, synchronised, of a hybrid solve and of AMG-PCG with its setup, both from x = 0 to 1e-8"""
    n = opt.n[0] * opt.n[1] * opt.n[2]
    A = ij.build_matrix(opt)
    L.hypre_ParCSRMatrixMigrate(A, B.HYPRE_MEMORY_DEVICE)
    b = np.ones(n)
    out = {}
    # hybrid: everything, the setup of the hierarchy included if it comes to that, is inside Solve
    db, dx = B.parvec_from_numpy(b), B.parvec_from_numpy(np.zeros(n))
    h = ij.create_hybrid(ij.IJOptions(**dict(vars(opt), hybrid=1, cf_tol=cf_tol)))
    L.hypre_SyncComputeStream()
    t0 = time.perf_counter()
    L.HYPRE_ParCSRHybridSetup(h, A, db, dx)
    L.HYPRE_ParCSRHybridSolve(h, A, db, dx)
    L.hypre_SyncComputeStream()
    t1 = time.perf_counter()
    L.HYPRE_ClearError(256)
    B.check()
    its, pcg, dscg, rel = C.c_int(), C.c_int(), C.c_int(), C.c_double()
    L.HYPRE_ParCSRHybridGetNumIterations(h, C.byref(its))
    L.HYPRE_ParCSRHybridGetPCGNumIterations(h, C.byref(pcg))
    L.HYPRE_ParCSRHybridGetDSCGNumIterations(h, C.byref(dscg))
    L.HYPRE_ParCSRHybridGetFinalRelativeResidualNorm(h, C.byref(rel))
    times = (C.c_double * 4)()
    L.HYPRE_ParCSRHybridGetSetupSolveTime(h, times)
    out["hybrid"] = dict(seconds=round(t1 - t0, 4), iterations=its.value, amg_iterations=pcg.value, ds_iterations=dscg.value, rel_resid=rel.value,
                         cf_tol=cf_tol, setup1_solve1_setup2_solve2_s=[round(t, 4) for t in times])
    L.HYPRE_ParCSRHybridDestroy(h)
    L.hypre_ParVectorDestroy(db); L.hypre_ParVectorDestroy(dx)
    # AMG-PCG: setup of the same hierarchy, then the solve
    db, dx = B.parvec_from_numpy(b), B.parvec_from_numpy(np.zeros(n))
    L.hypre_SyncComputeStream()
    t0 = time.perf_counter()
    amg = ij.create_amg(opt, memory_location=B.HYPRE_MEMORY_DEVICE)
    L.HYPRE_BoomerAMGSetup(amg, A, None, None)
    L.HYPRE_BoomerAMGSetTol(amg, 0.0)
    L.HYPRE_BoomerAMGSetMaxIter(amg, 1)
    L.hypre_SyncComputeStream()
    t1 = time.perf_counter()
    g = C.c_void_p()
    L.HYPRE_ParCSRPCGCreate(0, C.byref(g))
    L.HYPRE_PCGSetTol(g, opt.tol)
    L.HYPRE_PCGSetMaxIter(g, opt.mg_max_iter)
    L.HYPRE_PCGSetPrecond(g, C.cast(L.HYPRE_BoomerAMGSolve, C.c_void_p), None, amg)
    L.HYPRE_ParCSRPCGSetup(g, A, db, dx)
    L.HYPRE_ParCSRPCGSolve(g, A, db, dx)
    L.hypre_SyncComputeStream()
    t2 = time.perf_counter()
    L.HYPRE_ClearError(256)
    B.check()
    k, rel = C.c_int(), C.c_double()
    L.HYPRE_PCGGetNumIterations(g, C.byref(k))
    L.HYPRE_PCGGetFinalRelativeResidualNorm(g, C.byref(rel))
    out["amg_pcg"] = dict(seconds=round(t2 - t0, 4), setup_s=round(t1 - t0, 4), solve_s=round(t2 - t1, 4), iterations=k.value, rel_resid=rel.value)
    L.HYPRE_ParCSRPCGDestroy(g)
    L.HYPRE_BoomerAMGDestroy(amg)
    L.hypre_ParVectorDestroy(db); L.hypre_ParVectorDestroy(dx)
    L.hypre_ParCSRMatrixDestroy(A)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=256, help="grid points per dimension (the default of bench.py)")
    ap.add_argument("--iters", type=int, default=50, help="iterations of a timed solve")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cf-tol", type=float, default=0.9, help="cf_tol of the hybrid solves (the reference's default)")
    ap.add_argument("--skip-to-1e-8", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    L = B.load_library()
    if not L.hypre_amd_DeviceAvailable():
        raise SystemExit("bench_hybrid: no HIP device — nothing is timed without one")
    g = args.grid
    n = g ** 3
    opt = ij.IJOptions(n=(g, g, g), P=(1, 1, 1))
    A = ij.build_matrix(opt)
    L.hypre_ParCSRMatrixMigrate(A, B.HYPRE_MEMORY_DEVICE)
    b = np.ones(n)
    times = {1: [], 0: []}
    for rep in range(args.reps + 1):                       # the first round is the warm-up
        for fused in (1, 0):
            ms, its, _, used = _ds_pcg(L, A, b, n, 0.0, args.iters, fused)
            assert its == args.iters and used == fused, (fused, its, used)
            if rep:
                times[fused].append(ms / its)
    L.hypre_ParCSRMatrixDestroy(A)
    rng3 = lambda v: [round(min(v), 4), round(max(v), 4)]
    doc = dict(what="DS-PCG, the fused step against the three launches it stands for, one MI355X",
               operator="bench.py: 7-point Laplacian, %d^3 rows" % g, iterations_timed=args.iters, runs=args.reps,
               timing="events on the compute stream around Solve, after one untimed solve per leg; the legs taken in turn",
               bytes_per_element=dict(fused=64, plain=92),
               ms_per_iteration=dict(fused=rng3(times[1]), plain=rng3(times[0]), fused_all=[round(t, 4) for t in times[1]],
                                     plain_all=[round(t, 4) for t in times[0]]),
               fused_is_the_default=bool(max(times[1]) <= min(times[0])))
    if not args.skip_to_1e_8:
        amg_opts = dict(coarsen_type=8, interp_type=6, P_max_elmts=4, relax_type=18, num_sweeps=1, tol=1e-8)      # the hierarchy of bench.py
        doc["to_1e_8"] = dict(note="measured once; wall clock with the device synchronised, hierarchy setup included on both sides",
                              laplacian=_to_1e_8(L, ij.IJOptions(n=(g, g, g), P=(1, 1, 1), **amg_opts), args.cf_tol),
                              difconv=_to_1e_8(L, ij.IJOptions(n=(g, g, g), P=(1, 1, 1), problem="difconv", c=(1.0, 1.0, 0.001), a=(0.0, 0.0, 0.0),
                                                               **amg_opts), args.cf_tol))
    text = json.dumps(doc, indent=1)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
