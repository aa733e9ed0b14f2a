"""Time per iteration of AMG-BiCGSTAB (HYPRE_ParCSRBiCGSTAB*, `ij -solver 9`) on one GPU with the fused vector updates and
with the reference's call sequence, on the operator and the hierarchy of `bench.py --problem difconv`.

    python tools/bench_bicgstab.py --grid 256 --iters 20 --reps 3 --out profiles/bicgstab_ab.json

Every timed solve runs with tol 0 and a fixed iteration count, so both legs take the same steps; the legs are timed in turn
`--reps` times after one untimed solve each, with events on the compute stream around HYPRE_ParCSRBiCGSTABSolve (the solve
begins with one residual and two inner products, which the figure per iteration includes).  The two preconditioner
applications and the two products with A of an iteration are timed the same way on their own; what is left of an
iteration is the vector work the switch changes.  Last, one AMG-BiCGSTAB and one AMG-GMRES solve to 1e-8.  The results
are printed as one JSON document and written to --out."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from hypre_amd import binding as B, ij  # noqa: E402


def _bicgstab(L, A, amg, b, n, tol, max_iter, fused):
    """(ms of the Solve, iterations, reported norm)"""
    db, dx = B.parvec_from_numpy(b), B.parvec_from_numpy(np.zeros(n))
    g = C.c_void_p()
    L.HYPRE_ParCSRBiCGSTABCreate(0, C.byref(g))
    L.HYPRE_BiCGSTABSetTol(g, tol)
    L.HYPRE_BiCGSTABSetMaxIter(g, max_iter)
    L.HYPRE_BiCGSTABSetPrecond(g, C.cast(L.HYPRE_BoomerAMGSolve, C.c_void_p), None, amg)
    L.hypre_amd_BiCGSTABSetFusedUpdates(g, fused)
    L.HYPRE_ParCSRBiCGSTABSetup(g, A, db, dx)
    L.hypre_SyncComputeStream()
    L.hypre_amd_EventTimerStart()
    L.HYPRE_ParCSRBiCGSTABSolve(g, A, db, dx)
    ms = L.hypre_amd_EventTimerStopMs()
    L.HYPRE_ClearError(256)                   # tol 0: the solve ends at max_iter
    B.check()
    its, rel = C.c_int(), C.c_double()
    L.HYPRE_BiCGSTABGetNumIterations(g, C.byref(its))
    L.HYPRE_BiCGSTABGetFinalRelativeResidualNorm(g, C.byref(rel))
    L.HYPRE_ParCSRBiCGSTABDestroy(g)
    L.hypre_ParVectorDestroy(db); L.hypre_ParVectorDestroy(dx)
    return ms, its.value, rel.value


def _gmres(L, A, amg, b, n, tol, k_dim):
    db, dx = B.parvec_from_numpy(b), B.parvec_from_numpy(np.zeros(n))
    g = C.c_void_p()
    L.HYPRE_ParCSRGMRESCreate(0, C.byref(g))
    L.HYPRE_GMRESSetKDim(g, k_dim)
    L.HYPRE_GMRESSetTol(g, tol)
    L.HYPRE_GMRESSetMaxIter(g, 1000)
    L.HYPRE_GMRESSetPrecond(g, C.cast(L.HYPRE_BoomerAMGSolve, C.c_void_p), None, amg)
    L.HYPRE_ParCSRGMRESSetup(g, A, db, dx)
    L.hypre_SyncComputeStream()
    L.hypre_amd_EventTimerStart()
    L.HYPRE_ParCSRGMRESSolve(g, A, db, dx)
    ms = L.hypre_amd_EventTimerStopMs()
    B.check()
    its, rel = C.c_int(), C.c_double()
    L.HYPRE_GMRESGetNumIterations(g, C.byref(its))
    L.HYPRE_GMRESGetFinalRelativeResidualNorm(g, C.byref(rel))
    L.HYPRE_ParCSRGMRESDestroy(g)
    L.hypre_ParVectorDestroy(db); L.hypre_ParVectorDestroy(dx)
    return ms, its.value, rel.value


def _operators_alone(L, A, amg, b, n, iters):
    """ms of what an iteration spends in M^-1 and A: two cycles from a zero guess and two products, `iters` times"""
    rng = np.random.default_rng(9)
    f, u, w = B.parvec_from_numpy(rng.uniform(-1, 1, n)), B.parvec_from_numpy(np.zeros(n)), B.parvec_from_numpy(np.zeros(n))

    def once():
        for _ in range(2):
            L.hypre_ParVectorSetZeros(u)
            L.HYPRE_BoomerAMGSolve(amg, A, f, u)
            L.hypre_ParCSRMatrixMatvec(1.0, A, u, 0.0, w)
    once()
    L.hypre_SyncComputeStream()
    L.hypre_amd_EventTimerStart()
    for _ in range(iters):
        once()
    ms = L.hypre_amd_EventTimerStopMs() / iters
    B.check()
    for v in (f, u, w):
        L.hypre_ParVectorDestroy(v)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=256, help="grid points per dimension (the default of bench.py)")
    ap.add_argument("--iters", type=int, default=20, help="iterations of a timed solve")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    L = B.load_library()
    if not L.hypre_amd_DeviceAvailable():
        raise SystemExit("bench_bicgstab: no HIP device — nothing is timed without one")
    g = args.grid
    n = g ** 3
    # bench.py --problem difconv: anisotropic diffusion (1, 1, 0.001), PMIS, ext+i(4), l1-Jacobi, setup on the device
    opt = ij.IJOptions(n=(g, g, g), P=(1, 1, 1), coarsen_type=8, interp_type=6, P_max_elmts=4, relax_type=18, num_sweeps=1,
                       problem="difconv", c=(1.0, 1.0, 0.001), a=(0.0, 0.0, 0.0))
    A = ij.build_matrix(opt)
    amg = ij.create_amg(opt, memory_location=B.HYPRE_MEMORY_DEVICE)
    L.hypre_ParCSRMatrixMigrate(A, B.HYPRE_MEMORY_DEVICE)
    L.HYPRE_BoomerAMGSetup(amg, A, None, None)
    B.check()
    L.HYPRE_BoomerAMGSetTol(amg, 0.0)
    L.HYPRE_BoomerAMGSetMaxIter(amg, 1)
    b = np.ones(n)
    times = {1: [], 0: []}
    for rep in range(args.reps + 1):                       # the first round is the warm-up
        for fused in (1, 0):
            ms, its, _ = _bicgstab(L, A, amg, b, n, 0.0, args.iters, fused)
            assert its == args.iters, (fused, its)
            if rep:
                times[fused].append(ms / its)
    ops = [_operators_alone(L, A, amg, b, n, args.iters) for _ in range(args.reps)]
    ops_ms = float(np.median(ops))
    bms, bits, brel = _bicgstab(L, A, amg, b, n, 1e-8, 1000, 1)
    gms, gits, grel = _gmres(L, A, amg, b, n, 1e-8, 5)
    rng3 = lambda v: [round(min(v), 4), round(max(v), 4)]
    doc = dict(what="AMG-BiCGSTAB, fused vector updates against the reference's call sequence, one MI355X",
               operator="bench.py --problem difconv: 7-point anisotropic diffusion (1, 1, 0.001), %d^3 rows" % g,
               hierarchy="PMIS, ext+i (4 per row), l1-Jacobi, one V-cycle per application", iterations_timed=args.iters, runs=args.reps,
               timing="events on the compute stream around Solve, after one untimed solve per leg; the legs taken in turn",
               ms_per_iteration=dict(fused=rng3(times[1]), plain=rng3(times[0]), fused_all=[round(t, 4) for t in times[1]],
                                     plain_all=[round(t, 4) for t in times[0]]),
               two_preconditioner_applications_and_two_products_ms=dict(range=rng3(ops), median=round(ops_ms, 4)),
               share_outside_preconditioner_and_products=dict(fused=[round(1.0 - ops_ms / t, 4) for t in rng3(times[1])],
                                                              plain=[round(1.0 - ops_ms / t, 4) for t in rng3(times[0])]),
               to_1e_8=dict(note="measured once", bicgstab=dict(iterations=bits, preconditioner_applications=2 * bits, ms=round(bms, 2), rel_resid=brel),
                            gmres_k5=dict(iterations=gits, preconditioner_applications=gits, ms=round(gms, 2), rel_resid=grel)))
    text = json.dumps(doc, indent=1)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    L.HYPRE_BoomerAMGDestroy(amg)
    L.hypre_ParCSRMatrixDestroy(A)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
