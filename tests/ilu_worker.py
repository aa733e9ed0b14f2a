"""Worker of tests/test_ilu_host.py and tests/test_ilu_gpu.py.  Run alone or as the ranks of a torch.distributed.run job.

    python tests/ilu_worker.py job <name> <host|device>    one line of tests/golden/ij_saved_ilu.json: its command, parsed as the
                                                           driver parses it, run in host or in device memory; rank 0 prints the
                                                           driver's closing lines and "RESULT <json>"
    python tests/ilu_worker.py krylov <name> host          a GMRES line of the golden file (solver 81) on the CPU: the numpy
                                                           restatement of GMRES (ilu_krylov_reference.py) over the ranks'
                                                           pieces, preconditioned by every rank's host ILU application
    python tests/ilu_worker.py empty <nranks> <host|device>  a 9 x 7 5-point operator whose rows all lie on rank 0 of <nranks>
                                                           (the others own none): ILU alone to 1e-8 in host memory, and with
                                                           `device` again on the device, where the triangular solves are
                                                           compared with the host's bit for bit; "RESULT <json>", one entry
                                                           per rank
"""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def _world():
    """(dist or None, rank, world, comm, allsum)"""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world == 1:
        return None, 0, 1, 0, None
    import torch
    import torch.distributed as dist
    from hypre_amd import distributed
    dist.init_process_group(backend="gloo")
    rank = dist.get_rank()

    def allsum(v):
        t = torch.tensor([v], dtype=torch.float64)
        dist.all_reduce(t)
        return float(t.item())

    return dist, rank, world, distributed.create_callback_comm(dist, rank, world), allsum


def _finish(dist):
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    return 0


def job(name, where):
    from hypre_amd import binding as B, ij
    case = json.load(open(os.path.join(HERE, "golden", "ij_saved_ilu.json")))[name]
    opt = ij.parse_cli(case["cmd"].split())
    loc = B.HYPRE_MEMORY_HOST if where == "host" else B.HYPRE_MEMORY_DEVICE
    dist, rank, world, comm, allsum = _world()
    A = ij.build_matrix(opt, comm=comm, rank=rank, nprocs=world)
    its, rel = ij.run_ilu(opt, A, comm=comm, rank=rank, allreduce=allsum, memory_location=loc)
    if rank == 0:
        print("RESULT " + json.dumps([its, rel]), flush=True)
    return _finish(dist)


def _local_blocks(A):
    """(diagonal block, ghost block with global columns) of this rank as scipy matrices, stored order kept"""
    import numpy as np
    import scipy.sparse as sp
    Am = A.contents
    out = []
    for blk in (Am.diag.contents, Am.offd.contents):
        n, nnz = blk.num_rows, blk.num_nonzeros
        take = lambda p, k, t: np.array(np.ctypeslib.as_array(p, shape=(k,)), dtype=t) if k else np.zeros(0, dtype=t)
        out.append((take(blk.data, nnz, np.float64), take(blk.j, nnz, np.int64), take(blk.i, n + 1, np.int64) if n else np.zeros(1, dtype=np.int64), n))
    (da, dj, di, n), (oa, oj, oi, _) = out
    ncols_offd = Am.offd.contents.num_cols
    cmap = np.array(np.ctypeslib.as_array(Am.col_map_offd, shape=(ncols_offd,)), dtype=np.int64) if ncols_offd else np.zeros(0, dtype=np.int64)
    nglob = int(Am.global_num_rows)
    return sp.csr_matrix((da, dj, di), shape=(n, n)), sp.csr_matrix((oa, cmap[oj], oi), shape=(n, nglob))


def krylov(name):
    """the GMRES of `ij -solver 81` on host memory: the operator as every rank's rows (the iterate gathered over the ranks for
    the ghost columns), inner products summed over the ranks, the preconditioner every rank's own HYPRE_ILUSetup factors"""
    import numpy as np
    import torch
    from hypre_amd import binding as B, ij
    import ilu_krylov_reference as K
    case = json.load(open(os.path.join(HERE, "golden", "ij_saved_ilu.json")))[name]
    opt = ij.parse_cli(case["cmd"].split())
    assert opt.solver == 81
    dist, rank, world, comm, allsum = _world()
    L = B.load_library()
    A = ij.build_matrix(opt, comm=comm, rank=rank, nprocs=world)
    Dm, Om = _local_blocks(A)
    n = Dm.shape[0]
    b, _ = ij.build_rhs_host(opt, A, rank=rank, allreduce=allsum)
    ilu = ij.create_ilu(opt, preconditioner=True)
    assert L.HYPRE_ILUSetup(ilu, A, None, None) == 0

    def gather(x):
        if dist is None:
            return x
        parts = [None] * world
        dist.all_gather_object(parts, x)
        return np.concatenate(parts)

    matvec = lambda x: Dm @ x + Om @ gather(x)
    dot = lambda u, v: (allsum(float(np.dot(u, v))) if allsum else float(np.dot(u, v)))
    its, rel, _ = K.gmres(matvec, K.host_ilu_preconditioner(L, B, ilu, n), dot, b, k_dim=opt.k_dim, tol=opt.tol, max_iter=opt.max_iter)
    if rank == 0:
        print("GMRES Iterations = %d\nFinal GMRES Relative Residual Norm = %e" % (its, rel))
        print("RESULT " + json.dumps([its, rel]), flush=True)
    L.HYPRE_ILUDestroy(ilu)
    return _finish(dist)


def empty(where):
    import hashlib
    import numpy as np
    from hypre_amd import binding as B, ij
    dist, rank, world, comm, allsum = _world()
    L = B.load_library()
    HOST, DEVICE = B.HYPRE_MEMORY_HOST, B.HYPRE_MEMORY_DEVICE
    opt = ij.IJOptions(n=(9, 7, 1), P=(1, 1, world))              # one plane: rank 0 takes it, the others nothing
    A = ij.build_matrix(opt, comm=comm, rank=rank, nprocs=world)
    Am = A.contents
    n, first, nglob = Am.diag.contents.num_rows, int(Am.row_starts[0]), int(Am.global_num_rows)
    rng = np.random.default_rng(41)
    f = rng.standard_normal(nglob)[first:first + n]
    s = C.c_void_p()
    L.HYPRE_ILUCreate(C.byref(s))
    assert L.HYPRE_ILUSetup(s, A, None, None) == 0
    mine = dict(rows=n)

    def solve(loc):
        L.HYPRE_ILUSetTol(s, 1e-8)
        L.HYPRE_ILUSetMaxIter(s, 200)
        fv = B.parvec_from_numpy(f, comm=comm, global_size=nglob, first=first, location=loc)
        uv = B.parvec_from_numpy(np.zeros(n), comm=comm, global_size=nglob, first=first, location=loc)
        rc = L.HYPRE_ILUSolve(s, A, fv, uv)
        B.check()
        its, rel = C.c_int(), C.c_double()
        L.HYPRE_ILUGetNumIterations(s, C.byref(its)); L.HYPRE_ILUGetFinalRelativeResidualNorm(s, C.byref(rel))
        u = B.parvec_to_numpy(uv)
        for v in (fv, uv):
            L.hypre_ParVectorDestroy(v)
        return rc, its.value, rel.value, u

    def chain(loc, k):
        u = np.zeros(n)
        for _ in range(k):
            fv, uv = B.parvec_from_numpy(f - 0.3 * u, location=loc), B.parvec_from_numpy(u, location=loc)
            assert L.hypre_amd_ILUApplyFactors(s, fv, uv) == 0
            B.check()
            u = B.parvec_to_numpy(uv)
            for v in (fv, uv):
                L.hypre_ParVectorDestroy(v)
        return u

    def stats():
        v = [C.c_int(-1) for _ in range(6)]
        L.hypre_amd_ILUGetSolveStats(s, *[C.byref(x) for x in v])
        return [x.value for x in v]

    rc, its, rel, u = solve(HOST)
    mine.update(host=dict(rc=rc, its=its, rel=rel, u=hashlib.sha256(u.tobytes()).hexdigest()))
    host_chain = chain(HOST, 5)
    if where == "device":
        L.hypre_ParCSRMatrixMigrate(A, DEVICE)
        rc, its, rel, ud = solve(DEVICE)
        mine.update(device=dict(rc=rc, its=its, rel=rel, stats=stats(), close=bool(n == 0 or np.max(np.abs(ud - u)) <= 1e-10 * np.max(np.abs(u))),
                                chain_same_bits=bool(np.array_equal(chain(DEVICE, 5).view(np.int64), host_chain.view(np.int64)))))
    parts = [mine]
    if dist is not None:
        parts = [None] * world if rank == 0 else None
        dist.gather_object(mine, parts, dst=0)
    if rank == 0:
        print("RESULT " + json.dumps(parts), flush=True)
    L.HYPRE_ILUDestroy(s)
    L.hypre_ParCSRMatrixDestroy(A)
    return _finish(dist)


def main():
    mode = sys.argv[1]
    if mode == "job" and sys.argv[3] in ("host", "device"):
        return job(sys.argv[2], sys.argv[3])
    if mode == "krylov" and sys.argv[3] == "host":
        return krylov(sys.argv[2])
    if mode == "empty" and sys.argv[3] in ("host", "device"):
        return empty(sys.argv[3])
    raise SystemExit("ilu_worker: job <name> <host|device> | krylov <name> host | empty <nranks> <host|device>")


if __name__ == "__main__":
    raise SystemExit(main())
