"""Worker of the two-rank multivector test (test_amg_multivector_gpu.py): run under torch.distributed.run.
On one distributed hierarchy per case, hypre_BoomerAMGSolve on NV columns at once must give, on every rank, the bytes of
the single-vector solves of the columns one by one.  Prints one RESULT line per case on rank 0."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch
    import torch.distributed as dist
    from hypre_amd import binding as B, ij, distributed

    spec = json.loads(sys.argv[1])
    import faulthandler
    faulthandler.dump_traceback_later(int(os.environ.get("HYPRE_AMD_TEST_WATCHDOG", "300")), exit=True)
    dist.init_process_group(backend="gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    L = B.load_library()
    comm = distributed.create_stream_staged_comm(dist, rank, world)
    if L.hypre_amd_CommSelfTest(comm, 4099) != 0:
        raise SystemExit("communicator self-test failed on rank %d" % rank)
    nv = int(spec["nv"])
    for case in spec["cases"]:
        opt = ij.IJOptions(**{k: (tuple(v) if isinstance(v, list) else v) for k, v in case["options"].items()})
        A = ij.build_matrix(opt, comm=comm, rank=rank, nprocs=world)
        s = ij.create_amg(opt, memory_location=B.HYPRE_MEMORY_DEVICE)
        L.hypre_ParCSRMatrixMigrate(A, B.HYPRE_MEMORY_DEVICE)
        L.HYPRE_BoomerAMGSetup(s, A, None, None)
        B.check()
        L.hypre_ParCSRMatrixMigrate(A, B.HYPRE_MEMORY_DEVICE)
        Am = A.contents
        n, first, nglob = Am.diag.contents.num_rows, int(Am.row_starts[0]), int(Am.global_num_rows)
        rng = np.random.default_rng(100 + rank)
        F, U0 = rng.uniform(-1, 1, (n, nv)), rng.uniform(-1, 1, (n, nv))
        L.HYPRE_BoomerAMGSetTol(s, 0.0)
        L.HYPRE_BoomerAMGSetMaxIter(s, 2)
        single = np.zeros((n, nv))
        for v in range(nv):
            df = B.parvec_from_numpy(F[:, v], comm=comm, global_size=nglob, first=first)
            du = B.parvec_from_numpy(U0[:, v], comm=comm, global_size=nglob, first=first)
            L.HYPRE_BoomerAMGSolve(s, A, df, du)
            B.check()
            single[:, v] = B.parvec_to_numpy(du)
            L.hypre_ParVectorDestroy(df); L.hypre_ParVectorDestroy(du)
        df = B.parmultivec_from_numpy(F, comm=comm, global_size=nglob, first=first)
        du = B.parmultivec_from_numpy(U0, comm=comm, global_size=nglob, first=first)
        L.HYPRE_BoomerAMGSolve(s, A, df, du)
        B.check()
        multi = B.parmultivec_to_numpy(du)
        L.hypre_ParVectorDestroy(df); L.hypre_ParVectorDestroy(du)
        same = int(multi.tobytes() == single.tobytes())
        moved = int(not np.array_equal(multi, U0))
        flags = torch.tensor([same, moved], dtype=torch.int32)
        dist.all_reduce(flags, op=dist.ReduceOp.MIN)
        diff = torch.tensor([float(np.max(np.abs(multi - single))) if n else 0.0], dtype=torch.float64)
        dist.all_reduce(diff, op=dist.ReduceOp.MAX)
        tail = C.c_int(L.hypre_amd_BoomerAMGGetNumLevels(s))
        L.HYPRE_BoomerAMGDestroy(s)
        if rank == 0:
            print("RESULT " + json.dumps({"name": case["name"], "bitwise": int(flags[0]), "moved": int(flags[1]),
                                          "max_diff": float(diff[0]), "levels": tail.value}), flush=True)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
