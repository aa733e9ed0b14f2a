"""Worker of tests/test_hybrid_gpu.py.  Run alone or as the ranks of a torch.distributed.run job.

    python tests/hybrid_worker.py job <name>     one hybrid job line of tests/golden/ij_saved_hybrid.json: its options, set in code
                                                 (the command line keeps refusing -solver 20), through hypre_amd.ij.launch
    python tests/hybrid_worker.py step <nz>      hypre_amd_ParVectorDiagScaledCGStep fused against plain on the rows of a
                                                 12 x 12 x nz Laplacian spread over the ranks, its diagonal replaced by entries of
                                                 both signs and tiny ones: prints "RESULT <json>" with the bits of both sums and
                                                 whether x, r and s agree
"""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))


def _world():
    """(dist or None, rank, world, comm)"""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world == 1:
        return None, 0, 1, 0
    import torch.distributed as dist
    from hypre_amd import distributed
    dist.init_process_group(backend="gloo")
    rank = dist.get_rank()
    return dist, rank, world, distributed.create_callback_comm(dist, rank, world)


def awkward_diagonal(rng, n):
    """entries of both signs, every seventh one tiny (the quotients stay finite)"""
    d = rng.uniform(0.5, 4.0, n) * rng.choice([-1.0, 1.0], n)
    d[::7] = 3.0e-150
    return d


def step(nz):
    import numpy as np
    from hypre_amd import binding as B, ij
    dist, rank, world, comm = _world()
    L = B.load_library()
    opt = ij.IJOptions(n=(12, 12, nz), P=(1, 1, world))
    A = ij.build_matrix(opt, comm=comm, rank=rank, nprocs=world)
    blk = A.contents.diag.contents
    n = blk.num_rows
    rng = np.random.default_rng(77 + rank)
    ai = np.ctypeslib.as_array(blk.i, shape=(n + 1,))
    np.ctypeslib.as_array(blk.data, shape=(blk.num_nonzeros,))[ai[:-1]] = awkward_diagonal(rng, n)
    L.hypre_ParCSRMatrixMigrate(A, B.HYPRE_MEMORY_DEVICE)
    first, nglob = int(A.contents.row_starts[0]), int(A.contents.global_num_rows)
    h = {k: rng.standard_normal(n) for k in "psxr"}
    make = lambda a: B.parvec_from_numpy(a, comm=comm, global_size=nglob, first=first)
    got = {}
    for fused in (1, 0):
        v = {k: make(h[k]) for k in "psxr"}
        rr, rs = C.c_double(float("nan")), C.c_double(float("nan"))
        rc = L.hypre_amd_ParVectorDiagScaledCGStep(fused, -0.8125, A, v["p"], v["s"], v["x"], v["r"], C.byref(rr), C.byref(rs))
        B.check()
        got[fused] = dict(rc=rc, sums=[np.float64(rr.value).tobytes().hex(), np.float64(rs.value).tobytes().hex()],
                          vecs={k: B.parvec_to_numpy(v[k]).tobytes() for k in "sxr"})
        for w in v.values():
            L.hypre_ParVectorDestroy(w)
    mine = dict(rows=n, rc=[got[1]["rc"], got[0]["rc"]], fused=got[1]["sums"], plain=got[0]["sums"],
                same=all(got[1]["vecs"][k] == got[0]["vecs"][k] for k in "sxr"),
                finite=bool(np.all(np.isfinite(np.frombuffer(got[1]["vecs"]["s"])))))
    parts = [mine]
    if dist is not None:
        parts = [None] * world if rank == 0 else None
        dist.gather_object(mine, parts, dst=0)
    if rank == 0:
        print("RESULT " + json.dumps(parts), flush=True)
    L.hypre_ParCSRMatrixDestroy(A)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    return 0


def main():
    from hypre_amd import ij
    mode, arg = sys.argv[1], sys.argv[2]
    if mode == "step":
        return step(int(arg))
    if mode == "job":
        case = json.load(open(os.path.join(HERE, "golden", "ij_saved_hybrid.json")))["jobs"][arg]
        return ij.launch(ij.check_options(ij.IJOptions(**case["options"])))
    raise SystemExit("hybrid_worker: unknown mode %r" % mode)


if __name__ == "__main__":
    raise SystemExit(main())
