"""Time per iteration of the GMRES callers on one GPU: COGMRES (batched Gram-Schmidt, `ij -solver 17 | 16`) against GMRES
(modified Gram-Schmidt, `-solver 4 | 3`), and the batched vector kernels alone.

    python tools/bench_krylov.py --grid 256 --k 5 30 --iters 60 --amg-iters 30 --reps 3

Every solve runs with tol 0 and a fixed iteration count, so both solvers of a pair take the same number of steps; a pair is
timed alternately `--reps` times after one untimed solve each, and the median wall time (the solve ends in a stream
synchronisation) over the iterations is reported.  Step i of a restart cycle streams 5 i vectors in GMRES (i dots, i
axpys) and 2 i + 3 in COGMRES; averaged over a cycle of k steps that is 5 (k + 1) / 2 against k + 4 passes, which the
output lists beside the times.  The kernel section times hypre_SeqVectorMassInnerProd / MassAxpy on 8 vectors against the
8 single calls they replace, host clock around calls that end in a synchronisation, and turns the times into bytes per
second of the K + 1 (K + 2) vectors a batched call moves.  One JSON line per result.

    python tools/bench_krylov.py --solver lgmres --grid 256 --k 5 --aug 2 --iters 60 --amg-iters 15 --reps 3

times LGMRES (HYPRE_ParCSRLGMRES*) with the reference's call sequence and with the fused updates beside GMRES and FlexGMRES
on the same problem, and lists the vector launches per iteration the library counted (bench_lgmres).
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from hypre_amd import binding as B, ij  # noqa: E402


def _solve(opt, A, b, n, amg):
    db, dx = B.parvec_from_numpy(b), B.parvec_from_numpy(np.zeros(n))
    L = B.load_library()
    t0 = time.perf_counter()
    if opt.solver == 17:
        its, _ = ij.solve_cogmres(opt, A, db, dx)
    elif opt.solver == 16:
        its, _ = ij.solve_cogmres(opt, A, db, dx, amg=amg)
    elif opt.solver == 4:
        its, _ = ij.solve_ds_gmres(opt, A, db, dx)
    else:
        its, _ = ij.solve_gmres(opt, amg, A, db, dx)
    el = time.perf_counter() - t0
    L.HYPRE_ClearAllErrors()                  # tol 0: every solve ends at max_iter
    L.hypre_ParVectorDestroy(db); L.hypre_ParVectorDestroy(dx)
    return el, its


def bench_pairs(args):
    L = B.load_library()
    g = args.grid
    n = g ** 3
    base = ij.IJOptions(n=(g, g, g), relax_type=18, coarsen_type=8, tol=0.0)
    A = ij.build_matrix(base)
    amg = None
    if not args.no_amg:
        amg = ij.create_amg(base, memory_location=B.HYPRE_MEMORY_DEVICE)
        t0 = time.perf_counter()
        L.HYPRE_BoomerAMGSetup(amg, A, None, None)
        B.check()
        print(json.dumps(dict(what="amg_setup_s", grid=g, value=round(time.perf_counter() - t0, 2))), flush=True)
    L.hypre_ParCSRMatrixMigrate(A, B.HYPRE_MEMORY_DEVICE)
    b = np.ones(n)
    pairs = [(17, 4, args.iters)] + ([] if args.no_amg else [(16, 3, args.amg_iters)])
    for new, old, iters in pairs:
        for k in args.k:
            times = {new: [], old: []}
            for rep in range(args.reps + 1):              # the first round is the warm-up
                for solver in (new, old):
                    opt = ij.IJOptions(n=(g, g, g), solver=solver, k_dim=k, tol=0.0, max_iter=iters, mg_max_iter=iters)
                    el, its = _solve(opt, A, b, n, amg)
                    assert its == iters, (solver, its, iters)
                    if rep:
                        times[solver].append(1e3 * el / iters)
            med = {s: statistics.median(t) for s, t in times.items()}
            print(json.dumps(dict(what="ms_per_iteration", grid=g, k=k, iterations=iters, cogmres_solver=new, gmres_solver=old,
                                  cogmres_ms=round(med[new], 4), gmres_ms=round(med[old], 4),
                                  cogmres_all=[round(t, 4) for t in times[new]], gmres_all=[round(t, 4) for t in times[old]],
                                  passes_per_step_cogmres=k + 4, passes_per_step_gmres=2.5 * (k + 1),
                                  speedup=round(med[old] / med[new], 3))), flush=True)
    if amg is not None:
        L.HYPRE_BoomerAMGDestroy(amg)
    L.hypre_ParCSRMatrixDestroy(A)


def _gram_schmidt_launches(its, k, fused):
    """inner products + updates of modified Gram-Schmidt over `its` iterations in cycles of k: step i is i + 1 dots and i
    axpys, fused one dot and i launches (what hypre_amd_FlexGMRESGetLaunchStats counts)"""
    steps = sum((it - 1) % k + 1 for it in range(1, its + 1))
    return steps + its if fused else 2 * steps + its


def _solve_family(name, A, b, n, k, iters, precond, aug=None, fused=None):
    """one solve of HYPRE_ParCSR<name> at tol 0 for `iters` iterations; (seconds, iterations, launch counters or None)"""
    L = B.load_library()
    fn = lambda stem: getattr(L, "HYPRE_%s%s" % (name, stem))
    db, dx = B.parvec_from_numpy(b), B.parvec_from_numpy(np.zeros(n))
    g = C.c_void_p()
    getattr(L, "HYPRE_ParCSR%sCreate" % name)(0, C.byref(g))
    fn("SetKDim")(g, k)
    if aug is not None:
        L.HYPRE_LGMRESSetAugDim(g, aug)
        L.hypre_amd_LGMRESSetFusedUpdates(g, fused)
    fn("SetMaxIter")(g, iters)
    fn("SetTol")(g, 0.0)
    fn("SetPrecond")(g, *precond)
    getattr(L, "HYPRE_ParCSR%sSetup" % name)(g, A, db, dx)
    t0 = time.perf_counter()
    getattr(L, "HYPRE_ParCSR%sSolve" % name)(g, A, db, dx)
    el = time.perf_counter() - t0
    L.HYPRE_ClearAllErrors()                  # tol 0: the solve ends at max_iter
    its = C.c_int()
    fn("GetNumIterations")(g, C.byref(its))
    stats = None
    if name == "LGMRES":
        st = [C.c_int() for _ in range(5)]
        L.hypre_amd_LGMRESGetLaunchStats(g, *[C.byref(v) for v in st])
        stats = [v.value for v in st]
    elif name == "FlexGMRES":
        st = [C.c_int() for _ in range(3)]
        L.hypre_amd_FlexGMRESGetLaunchStats(g, *[C.byref(v) for v in st])
        stats = [v.value for v in st]
    getattr(L, "HYPRE_ParCSR%sDestroy" % name)(g)
    L.hypre_ParVectorDestroy(db); L.hypre_ParVectorDestroy(dx)
    return el, its.value, stats


def bench_lgmres(args):
    """LGMRES with the reference's call sequence and with the fused updates beside GMRES and FlexGMRES: the same problem,
    the same restart length, tol 0 and a fixed iteration count, behind the diagonal scaling and behind BoomerAMG.  Per
    iteration: wall time (median of --reps solves after a warm-up round, the four taken in turn) and launches of the
    Gram-Schmidt steps plus, for LGMRES, of what forms the correction and ends a cycle (the library's own counters;
    GMRES keeps none, its figure is the formula they follow)."""
    L = B.load_library()
    g, n, aug = args.grid, args.grid ** 3, args.aug
    base = ij.IJOptions(n=(g, g, g), relax_type=18, coarsen_type=8, tol=0.0)
    A = ij.build_matrix(base)
    preconds = [("ds", (C.cast(L.HYPRE_ParCSRDiagScale, C.c_void_p), C.cast(L.HYPRE_ParCSRDiagScaleSetup, C.c_void_p), None), args.iters)]
    amg = None
    if not args.no_amg:
        amg = ij.create_amg(base, memory_location=B.HYPRE_MEMORY_DEVICE)
        L.HYPRE_BoomerAMGSetup(amg, A, None, None)
        B.check()
        L.HYPRE_BoomerAMGSetTol(amg, 0.0)
        L.HYPRE_BoomerAMGSetMaxIter(amg, 1)
        preconds.append(("amg", (C.cast(L.HYPRE_BoomerAMGSolve, C.c_void_p), None, amg), args.amg_iters))
    L.hypre_ParCSRMatrixMigrate(A, B.HYPRE_MEMORY_DEVICE)
    b = np.ones(n)
    variants = [("gmres", "GMRES", None, None), ("flexgmres", "FlexGMRES", None, None),
                ("lgmres_plain", "LGMRES", aug, 0), ("lgmres_fused", "LGMRES", aug, 1)]
    for pname, precond, iters in preconds:
        for k in args.k:
            times, stats = {v[0]: [] for v in variants}, {}
            for rep in range(args.reps + 1):              # the first round is the warm-up
                for label, name, a, fused in variants:
                    el, its, st = _solve_family(name, A, b, n, k, iters, precond, aug=a, fused=fused)
                    assert its == iters, (label, its, iters)
                    stats[label] = st
                    if rep:
                        times[label].append(1e3 * el / iters)
            launches = {"gmres": _gram_schmidt_launches(iters, k, False), "flexgmres": sum(stats["flexgmres"]),
                        "lgmres_plain": sum(stats["lgmres_plain"]), "lgmres_fused": sum(stats["lgmres_fused"])}
            print(json.dumps(dict(what="lgmres_ms_per_iteration", grid=g, precond=pname, k=k, aug=aug, iterations=iters,
                                  ms={v: round(statistics.median(t), 4) for v, t in times.items()},
                                  ms_all={v: [round(x, 4) for x in t] for v, t in times.items()},
                                  launches_per_iteration={v: round(c / iters, 3) for v, c in launches.items()},
                                  lgmres_counters=dict(plain=stats["lgmres_plain"], fused=stats["lgmres_fused"]))), flush=True)
    if amg is not None:
        L.HYPRE_BoomerAMGDestroy(amg)
    L.hypre_ParCSRMatrixDestroy(A)


def bench_kernels(args):
    L = B.load_library()
    n = args.grid ** 3
    K = 8
    rng = np.random.default_rng(1)
    x = B.vec_from_numpy(rng.standard_normal(n))
    y = B.vec_from_numpy(rng.standard_normal(n))
    z = [B.vec_from_numpy(rng.standard_normal(n)) for _ in range(K)]
    zs = (C.POINTER(B.Vector) * K)(*z)
    alpha = np.full(K, 1e-3)
    r = np.zeros(K)

    def timed(fn):
        fn()                                               # warm-up
        ts = []
        for _ in range(args.kernel_reps):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        return statistics.median(ts)

    def single_dots():
        for j in range(K):
            L.hypre_SeqVectorInnerProd(x, z[j])

    def single_axpys():
        for j in range(K):
            L.hypre_SeqVectorAxpy(1e-3, z[j], y)

    vec = 8.0 * n
    t = timed(lambda: L.hypre_SeqVectorMassInnerProd(x, zs, K, 0, B._rp(r)))
    t1 = timed(single_dots)
    print(json.dumps(dict(what="mass_dot_kernel<8>", n=n, call_ms=round(1e3 * t, 4), TBps=round((K + 1) * vec / t / 1e12, 3),
                          eight_single_dots_ms=round(1e3 * t1, 4), single_TBps=round(2 * K * vec / t1 / 1e12, 3))), flush=True)
    t = timed(lambda: L.hypre_SeqVectorMassAxpy(B._rp(alpha), zs, y, K, 0))
    t1 = timed(single_axpys)
    print(json.dumps(dict(what="mass_axpy_kernel<8>", n=n, call_ms=round(1e3 * t, 4), TBps=round((K + 2) * vec / t / 1e12, 3),
                          eight_single_axpys_ms=round(1e3 * t1, 4), single_TBps=round(3 * K * vec / t1 / 1e12, 3))), flush=True)
    t = timed(lambda: L.hypre_SeqVectorMassDotpTwo(x, y, zs, K, 0, B._rp(r), B._rp(np.zeros(K))))
    print(json.dumps(dict(what="mass_dot_two_kernel<8>", n=n, call_ms=round(1e3 * t, 4), TBps=round((K + 2) * vec / t / 1e12, 3))), flush=True)
    B.check()
    for v in [x, y] + z:
        L.hypre_SeqVectorDestroy(v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=256, help="grid points per dimension of the 7-point problem")
    ap.add_argument("--k", type=int, nargs="+", default=[5, 30], help="restart lengths")
    ap.add_argument("--iters", type=int, default=60, help="iterations of a diagonally scaled solve")
    ap.add_argument("--amg-iters", type=int, default=30, help="iterations of a solve with BoomerAMG in front")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kernel-reps", type=int, default=20)
    ap.add_argument("--no-amg", action="store_true", help="skip the pairs that need a hierarchy")
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--solver", choices=["cogmres", "lgmres"], default="cogmres",
                    help="cogmres: COGMRES against GMRES and the batched kernels; lgmres: LGMRES plain and fused beside GMRES and FlexGMRES")
    ap.add_argument("--aug", type=int, default=2, help="augmentation vectors of LGMRES")
    args = ap.parse_args()
    L = B.load_library()
    if not L.hypre_amd_DeviceAvailable():
        raise SystemExit("bench_krylov: no HIP device — nothing is timed without one")
    if args.solver == "lgmres":
        bench_lgmres(args)
        return 0
    if not args.no_kernels:
        bench_kernels(args)
    bench_pairs(args)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
