"""Time of one ILU application on the device: `python tools/bench_ilu.py [--n 256] [--lfil 0] [--reordering 1] [--reps 20]`.

The 7-point operator on an n^3 grid (the operator of `bench.py --problem 7pt`), one rank.  Setup (host: ordering,
factorisation, levels; upload) is timed once.  An application — HYPRE_ILUSolve with max_iter 1 and tol 0: the product with A,
the L solve, the U solve with the update of u — is timed over `--reps` calls after `--warmup`, each closed by a device
synchronisation.  Prints one JSON line: milliseconds per application, levels and entries of L and U, launches per
application by kernel form, the bytes an application must move (factors, row and level tables, vectors, and the product's
CSR bytes) and that over the time."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--lfil", type=int, default=0)
    ap.add_argument("--reordering", type=int, default=1)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    from hypre_amd import binding as B, ij
    L = B.load_library(build_if_missing=True)
    if not L.hypre_amd_DeviceAvailable():
        raise SystemExit("bench_ilu: no HIP device")
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
    spmv_bytes = 12.0 * nnzA + 4.0 * n + 3 * 8.0 * n
    ms = 1e3 * float(np.median(times))
    print(json.dumps(dict(tool="bench_ilu", n=a.n, rows=n, lfil=a.lfil, reordering=a.reordering, setup_s=round(setup_s, 3),
                          ms_per_application=round(ms, 4), ms_min=round(1e3 * min(times), 4), levels_L=levels_L, levels_U=levels_U,
                          run_launches=runs, level_launches=grids, nnz_L=nnzL, nnz_U=nnzU,
                          us_per_level=round(1e3 * ms / max(levels_L + levels_U, 1), 3),
                          triangular_bytes=tri_bytes, product_bytes=spmv_bytes,
                          tb_per_s=round((tri_bytes + spmv_bytes) / (ms * 1e-3) / 1e12, 4))))
    L.HYPRE_ILUDestroy(s)
    for v in (f, u):
        L.hypre_ParVectorDestroy(v)
    L.hypre_ParCSRMatrixDestroy(A)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
