"""Worker of tests/test_lgmres_gpu.py.  Run alone or as the ranks of a torch.distributed.run job.

    python tests/lgmres_worker.py job <name>        one LGMRES job of tests/golden/ij_saved_lgmres.json through the driver
                                                    (hypre_amd.ij.launch) with the options the golden file states for it
    python tests/lgmres_worker.py options <json>    the driver with these options
    python tests/lgmres_worker.py norm2 <n>         hypre_amd_ParVectorCopyThenInnerProd against hypre_ParVectorCopy and
                                                    hypre_ParVectorInnerProd on a vector of n elements spread over the
                                                    ranks: prints "RESULT <json>" with the bits of both sums
"""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))


def _options(d):
    from hypre_amd import ij
    return ij.check_options(ij.IJOptions(**{k: (tuple(v) if isinstance(v, list) else v) for k, v in d.items()}))


def norm2(n):
    import numpy as np
    import torch.distributed as dist
    from hypre_amd import binding as B, distributed
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank, comm = 0, 0
    if world > 1:
        dist.init_process_group(backend="gloo")
        rank = dist.get_rank()
        comm = distributed.create_callback_comm(dist, rank, world)
    L = B.load_library()
    # an uneven split: the ranks fold different numbers of workgroup partials
    first = [0] + [(n * (2 * r + 1)) // (2 * world) for r in range(1, world)] + [n]
    lo, hi = first[rank], first[rank + 1]
    h = np.random.default_rng(5051).standard_normal(n)[lo:hi]
    x = B.parvec_from_numpy(h, comm=comm, global_size=n, first=lo)
    y1 = B.parvec_from_numpy(np.zeros(hi - lo), comm=comm, global_size=n, first=lo)
    y2 = B.parvec_from_numpy(np.zeros(hi - lo), comm=comm, global_size=n, first=lo)
    L.hypre_ParVectorCopy(x, y1)
    want = L.hypre_ParVectorInnerProd(y1, y1)
    got = C.c_double(float("nan"))
    rc = L.hypre_amd_ParVectorCopyThenInnerProd(x, y2, C.byref(got))
    B.check()
    same = bool(np.array_equal(B.parvec_to_numpy(y2).view(np.int64), h.view(np.int64)))
    mine = dict(rc=rc, local=hi - lo, copied=same, fused=np.float64(got.value).tobytes().hex(), separate=np.float64(want).tobytes().hex(),
                value=got.value, numpy_local=float(np.dot(h, h)))
    for v in (x, y1, y2):
        L.hypre_ParVectorDestroy(v)
    parts = [mine]
    if world > 1:
        parts = [None] * world if rank == 0 else None
        dist.gather_object(mine, parts, dst=0)
    if rank == 0:
        print("RESULT " + json.dumps(parts), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    return 0


def main():
    from hypre_amd import ij
    mode, arg = sys.argv[1], sys.argv[2]
    if mode == "norm2":
        return norm2(int(arg))
    if mode == "job":
        return ij.launch(_options(json.load(open(os.path.join(HERE, "golden", "ij_saved_lgmres.json")))[arg]["options"]))
    if mode == "options":
        return ij.launch(_options(json.loads(arg)))
    raise SystemExit("lgmres_worker: unknown mode %r" % mode)


if __name__ == "__main__":
    raise SystemExit(main())
