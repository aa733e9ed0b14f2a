"""Worker of tests/test_bicgstab_gpu.py.  Run alone or as the ranks of a torch.distributed.run job.

    python tests/bicgstab_worker.py job <name>       one BiCGSTAB job line of tests/golden/ij_saved_bicgstab.json through the
                                                     command line of the driver (hypre_amd.ij.parse_cli, launch)
    python tests/bicgstab_worker.py solve <json>     AMG-BiCGSTAB (solver 9) with these driver options; rank 0 gathers x and
                                                     prints "RESULT <json>": iterations, the reported norm and
                                                     |b - A x| / |b| computed in numpy with the operator built on one rank
    python tests/bicgstab_worker.py dots <n>         hypre_amd_ParVectorInnerProdWithNorm and
                                                     hypre_amd_ParVectorTwoAxpysThenInnerProds against the library calls they
                                                     stand for, on vectors of n elements spread over the ranks: prints
                                                     "RESULT <json>" with the bits of every sum
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


def _finish(dist, rank, mine):
    parts = [mine]
    if dist is not None:
        parts = [None] * dist.get_world_size() if rank == 0 else None
        dist.gather_object(mine, parts, dst=0)
    return parts


def _hex(v):
    import numpy as np
    return np.float64(v).tobytes().hex()


def dots(n):
    import numpy as np
    from hypre_amd import binding as B
    dist, rank, world, comm = _world()
    L = B.load_library()
    # an uneven split: the ranks fold different numbers of workgroup partials
    first = [0] + [(n * (2 * r + 1)) // (2 * world) for r in range(1, world)] + [n]
    lo, hi = first[rank], first[rank + 1]
    rng = np.random.default_rng(910)
    h = {k: rng.standard_normal(n)[lo:hi] for k in ("v", "x", "s", "r", "r0")}
    make = lambda a: B.parvec_from_numpy(a, comm=comm, global_size=n, first=lo)
    a, b = 0.7320508075688772, -3.0e-5
    # the separate calls
    v, s, r0, x1, r1 = make(h["v"]), make(h["s"]), make(h["r0"]), make(h["x"]), make(h["r"])
    want_rs, want_ss = L.hypre_ParVectorInnerProd(r1, s), L.hypre_ParVectorInnerProd(s, s)
    L.hypre_ParVectorAxpy(a, v, x1)
    L.hypre_ParVectorAxpy(b, s, r1)
    want_rr, want_r0r = L.hypre_ParVectorInnerProd(r1, r1), L.hypre_ParVectorInnerProd(r0, r1)
    # the fused ones
    x2, r2 = make(h["x"]), make(h["r"])
    got = [C.c_double(float("nan")) for _ in range(4)]
    rc = L.hypre_amd_ParVectorInnerProdWithNorm(r2, s, C.byref(got[0]), C.byref(got[1]))
    rc |= L.hypre_amd_ParVectorTwoAxpysThenInnerProds(a, v, x2, b, s, r2, r0, C.byref(got[2]), C.byref(got[3]))
    B.check()
    same = all(np.array_equal(B.parvec_to_numpy(p).view(np.int64), B.parvec_to_numpy(q).view(np.int64)) for p, q in ((x1, x2), (r1, r2)))
    rn = B.parvec_to_numpy(r1)
    mine = dict(rc=rc, local=hi - lo, updated=bool(same), fused=[_hex(g.value) for g in got],
                separate=[_hex(w) for w in (want_rs, want_ss, want_rr, want_r0r)], values=[g.value for g in got],
                numpy_local=[float(np.dot(h["r"], h["s"])), float(np.dot(h["s"], h["s"])), float(np.dot(rn, rn)), float(np.dot(h["r0"], rn))])
    for p in (v, s, r0, x1, r1, x2, r2):
        L.hypre_ParVectorDestroy(p)
    parts = _finish(dist, rank, mine)
    if rank == 0:
        print("RESULT " + json.dumps(parts), flush=True)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    return 0


def solve(options):
    import numpy as np
    from hypre_amd import binding as B, ij
    dist, rank, world, comm = _world()
    L = B.load_library()
    opt = ij.check_options(ij.IJOptions(**{k: (tuple(v) if isinstance(v, list) else v) for k, v in options.items()}))
    assert opt.solver == 9
    A = ij.build_matrix(opt, comm=comm, rank=rank, nprocs=world)
    s = ij.create_amg(opt, memory_location=B.HYPRE_MEMORY_DEVICE)
    L.HYPRE_BoomerAMGSetup(s, A, None, None)
    B.check()
    L.hypre_ParCSRMatrixMigrate(A, B.HYPRE_MEMORY_DEVICE)
    first, nglob = int(A.contents.row_starts[0]), int(A.contents.global_num_rows)
    b, x0 = ij.build_rhs_host(opt, A, rank=rank)
    db = B.parvec_from_numpy(b, comm=comm, global_size=nglob, first=first)
    dx = B.parvec_from_numpy(x0, comm=comm, global_size=nglob, first=first)
    its, rel = ij.solve_bicgstab(opt, A, db, dx, comm=comm, amg=s)
    err = L.HYPRE_GetError()
    L.HYPRE_ClearError(256)
    B.check()
    parts = _finish(dist, rank, (first, B.parvec_to_numpy(dx).tolist()))
    if rank == 0:
        x = np.zeros(nglob)
        for lo, vals in parts:
            x[lo:lo + len(vals)] = vals
        # slabs in z keep the row numbering of the one-rank operator
        one = dict(options)
        one.pop("P", None)
        A1 = ij.build_matrix(ij.IJOptions(**{k: (tuple(v) if isinstance(v, list) else v) for k, v in one.items()}))
        M = B.csr_to_scipy(A1.contents.diag)
        bg = np.ones(nglob)
        true = float(np.linalg.norm(bg - M @ x) / np.linalg.norm(bg))
        print("RESULT " + json.dumps(dict(iterations=its, reported=rel, true=true, err=err)), flush=True)
        L.hypre_ParCSRMatrixDestroy(A1)
    L.hypre_ParVectorDestroy(db); L.hypre_ParVectorDestroy(dx)
    L.HYPRE_BoomerAMGDestroy(s)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    return 0


def main():
    from hypre_amd import ij
    mode, arg = sys.argv[1], sys.argv[2]
    if mode == "dots":
        return dots(int(arg))
    if mode == "solve":
        return solve(json.loads(arg))
    if mode == "job":
        return ij.launch(ij.parse_cli(json.load(open(os.path.join(HERE, "golden", "ij_saved_bicgstab.json")))[arg]["cmd"].split()))
    raise SystemExit("bicgstab_worker: unknown mode %r" % mode)


if __name__ == "__main__":
    raise SystemExit(main())
