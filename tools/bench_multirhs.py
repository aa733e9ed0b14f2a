"""BoomerAMG cycles on several right-hand sides at once (hypre_BoomerAMGSolve with num_vectors = NV columns) against NV
single-vector cycles, on the benchmark's C2 problem: 7-point Laplacian, PMIS, ext+i(4), l1-Jacobi V(1,1), fp64, one GPU.

    python tools/bench_multirhs.py [--grid 256] [--nv 1 2 4 8] [--cycles 10] [--warmup 3] [--pause-ms 0] [--fused 0 1]

One JSON line per NV and path: ms per NV-column cycle, ms per column, NV single-vector cycles for comparison and their
ratio, and the bytes one cycle streams (hypre_amd_ByteCounters).  --fused 0: the column loop — the single-column cycle once
per column, its matrix bytes NV times those of one cycle; --fused 1: the large levels cycled for all columns at once
(hypre_amd_SetMultivectorCycle), each operator read once per group of columns.  Both (the default) are measured alternately in
one process, on the same solver; each column is bit for bit the single-vector cycle either way.

--pause-ms P leaves the GPU idle for P ms before every timed loop, so that a kernel trace of the run can be cut there:
tools/multirhs_trace_stats.py takes the launches after the last such gap, the timed cycles of the last NV."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--nv", type=int, nargs="+", default=[1, 2, 4, 8])
    ap.add_argument("--cycles", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--pause-ms", type=float, default=0.0)
    ap.add_argument("--fused", type=int, nargs="+", default=[0, 1], choices=[0, 1])
    args = ap.parse_args()
    from hypre_amd import binding as B, ij
    L = B.load_library()
    if not L.hypre_amd_DeviceAvailable():
        raise SystemExit("bench_multirhs.py needs a HIP device")
    n1 = args.grid
    opt = ij.IJOptions(n=(n1, n1, n1), coarsen_type=8, interp_type=6, P_max_elmts=4, relax_type=18, num_sweeps=1)
    A = ij.build_matrix(opt)
    s = ij.create_amg(opt, memory_location=B.HYPRE_MEMORY_DEVICE)
    L.hypre_ParCSRMatrixMigrate(A, B.HYPRE_MEMORY_DEVICE)
    L.HYPRE_BoomerAMGSetup(s, A, None, None)
    B.check()
    L.hypre_ParCSRMatrixMigrate(A, B.HYPRE_MEMORY_DEVICE)
    n = A.contents.diag.contents.num_rows
    L.HYPRE_BoomerAMGSetTol(s, 0.0)
    L.HYPRE_BoomerAMGSetMaxIter(s, 1)
    L.hypre_SetSyncCudaCompute(0)

    def timed(b, u):
        def step():
            L.hypre_ParVectorSetZeros(u)
            L.HYPRE_BoomerAMGSolve(s, A, b, u)
        for _ in range(max(args.warmup, 2)):
            step()
        L.hypre_SyncComputeStream()
        B.check()
        if args.pause_ms > 0:
            time.sleep(args.pause_ms / 1e3)
        t0 = time.perf_counter()
        for _ in range(args.cycles):
            step()
        L.hypre_SyncComputeStream()
        ms = 1e3 * (time.perf_counter() - t0) / args.cycles
        csr, streamed = C.c_double(), C.c_double()
        L.hypre_amd_ByteCounters(C.byref(csr), C.byref(streamed), 1)
        step()
        L.hypre_SyncComputeStream()
        L.hypre_amd_ByteCounters(C.byref(csr), C.byref(streamed), 0)
        return ms, streamed.value

    b1 = B.parvec_from_numpy(np.ones(n))
    u1 = B.parvec_from_numpy(np.zeros(n))
    ms1, bytes1 = timed(b1, u1)
    before = L.hypre_amd_SetMultivectorCycle(-1)
    for nv in args.nv:
        for fused in ([0] if nv == 1 else args.fused):
            L.hypre_amd_SetMultivectorCycle(fused)
            if nv == 1:
                ms, streamed = ms1, bytes1
            else:
                bm = B.parmultivec_from_numpy(np.repeat(np.ones(n)[:, None], nv, axis=1))
                um = B.parmultivec_from_numpy(np.zeros((n, nv)))
                ms, streamed = timed(bm, um)
                L.hypre_ParVectorDestroy(bm); L.hypre_ParVectorDestroy(um)
            print(json.dumps({
                "metric": "BoomerAMG cycle on NV right-hand sides (%d^3 7-pt, PMIS / ext+i(4) / l1-Jacobi V(1,1), fp64)" % n1,
                "nv": nv, "fused": fused, "ms_per_cycle": round(ms, 4), "ms_per_column": round(ms / nv, 4),
                "ms_nv_single_cycles": round(nv * ms1, 4), "ratio_to_nv_single": round(ms / (nv * ms1), 4),
                "gb_streamed_per_cycle": round(streamed / 1e9, 3),
                "cycles": args.cycles, "levels": L.hypre_amd_BoomerAMGGetNumLevels(s),
                "column_path": "large levels for all columns at once, the tail per column" if fused else
                               "single-column cycle per column",
                "bits": "every column bitwise the single-vector cycle"}), flush=True)
    L.hypre_amd_SetMultivectorCycle(before)
    L.hypre_ParVectorDestroy(b1); L.hypre_ParVectorDestroy(u1)
    L.HYPRE_BoomerAMGDestroy(s)


if __name__ == "__main__":
    main()
