"""CPU: the HOST setup pinned array for array.  tests/golden/setup_hierarchy_digests.json holds one sha256 per rank
and level over A_l, P_l (both blocks, column counts, ghost column maps), the C/F marker and the smoother diagonal
(dist_worker.hierarchy_digests), recorded once with `python tests/test_setup_digests.py --record`.  Every host builder
(strength, PMIS / HMIS, ext+i and direct interpolation, function filter, Galerkin product; single-rank and distributed)
is on the path of at least one case.  The device builders are compared with the host builders array for array by the
GPU tests, so these digests pin them as well.  A mismatch means the setup computes something else: the file is not
re-recorded to make a change pass."""
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "setup_hierarchy_digests.json")
sys.path.insert(0, HERE)

PMIS = {"coarsen_type": 8, "relax_type": 18}
SINGLE = {
    "7pt_extpi": dict(PMIS, n=(14, 13, 12), interp_type=6, P_max_elmts=4),
    "7pt_extpi_trunc": dict(PMIS, n=(14, 13, 12), interp_type=6, P_max_elmts=4, trunc_factor=0.3),
    "27pt_extpi": dict(PMIS, n=(12, 11, 10), problem="27pt"),
    "7pt_direct": dict(PMIS, n=(14, 13, 12), interp_type=3),
    "7pt_hmis": dict(n=(14, 13, 12), coarsen_type=10, relax_type=18),
    "sys2": dict(PMIS, n=(8, 8, 8), sys_num_fun=2, num_functions=2),
    "sys2_filtered": dict(PMIS, n=(8, 8, 8), sys_num_fun=2, num_functions=2, filter_functions=1),
    # above the row counts at which the host builders split their rows over threads
    "7pt_threads": dict(PMIS, n=(64, 60, 56)),
}
# name -> (ranks, options).  A 2 x 2 x 1 process grid needs four ranks; two and three ranks split x.  The 27-point
# cases must put new off-rank nodes (ghosts of ghosts) into P: the recorder and the test check that they do.
GRID = {2: [2, 1, 1], 3: [3, 1, 1], 4: [2, 2, 1]}
MULTI = {}
for _r, _P in GRID.items():
    MULTI["7pt_r%d" % _r] = (_r, dict(PMIS, n=[14, 13, 12], P=_P))
    MULTI["27pt_r%d" % _r] = (_r, dict(PMIS, n=[12, 11, 10], problem="27pt", P=_P))
MULTI["7pt_direct_r4"] = (4, dict(n=[14, 13, 12], coarsen_type=9, interp_type=3, relax_type=18, P=[1, 1, 4], P_max_elmts=0))
MULTI["rank_without_rows_r4"] = (4, dict(PMIS, n=[3, 5, 4], P=[4, 1, 1]))
THREADED = "solvers.out.19"        # 3 ranks with 3 OpenMP threads each: the threaded distributed row loops


def single_digest(lib, options, threads=None):
    from hypre_amd import binding as B, ij
    from dist_worker import hierarchy_digests
    if threads:
        lib.hypre_amd_SetHostThreads(threads)
    opt = ij.IJOptions(**options)
    A = ij.build_matrix(opt)
    s = ij.create_amg(opt, memory_location=B.HYPRE_MEMORY_HOST)
    lib.HYPRE_BoomerAMGSetup(s, A, None, None)
    B.check()
    d = hierarchy_digests(lib, B, s)
    lib.HYPRE_BoomerAMGDestroy(s)
    lib.hypre_ParCSRMatrixDestroy(A)
    if threads:
        lib.hypre_amd_SetHostThreads(lib.hypre_amd_HostCpuShare())
    return [d]                       # one list of levels per rank


def launch(nranks, cases, omp):
    """One launch of dist_worker.py for all `cases` ({name: options}) of one rank count."""
    from conftest import free_port
    spec = {"batch": [{"name": k, "options": v, "digest": 1} for k, v in cases.items()]}
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nranks),
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()), os.path.join(HERE, "dist_worker.py"),
           json.dumps(spec)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=dict(os.environ, OMP_NUM_THREADS=str(omp)))
    res = {}
    for line in r.stdout.splitlines():
        if line.startswith("RESULT "):
            d = json.loads(line[len("RESULT "):])
            res[d["name"]] = d
    return r.returncode, res, r.stdout[-1500:] + "\n--- stderr tail ---\n" + r.stderr[-3000:]


_launches = {}


def multi_result(name):
    nranks = MULTI[name][0]
    if nranks not in _launches:
        _launches[nranks] = launch(nranks, {k: v[1] for k, v in MULTI.items() if v[0] == nranks}, omp=1)
    rc, res, tail = _launches[nranks]
    assert name in res, "no result for %s (worker exit code %d)\n%s" % (name, rc, tail)
    return res[name]


def threaded_result():
    case = json.load(open(os.path.join(HERE, "golden", "ij_saved.json")))[THREADED]
    rc, res, tail = launch(case["ranks"], {THREADED: case["options"]}, omp=3)
    assert THREADED in res, "no result (worker exit code %d)\n%s" % (rc, tail)
    return res[THREADED]


def golden():
    return json.load(open(GOLDEN))


@pytest.mark.parametrize("name", sorted(k for k in SINGLE if k != "7pt_threads"))
def test_single_rank_hierarchy(lib, name):
    assert single_digest(lib, SINGLE[name]) == golden()[name]


@pytest.mark.parametrize("threads", [1, 8])
def test_hierarchy_does_not_depend_on_the_row_partition(lib, threads):
    """One recorded digest for one and for eight host threads: the per-thread row blocks leave no trace."""
    assert single_digest(lib, SINGLE["7pt_threads"], threads=threads) == golden()["7pt_threads"]


@pytest.mark.parametrize("name", sorted(MULTI))
def test_distributed_hierarchy(name):
    out = multi_result(name)
    if name.startswith("27pt"):
        assert sum(out["new_nodes"]) > 0, "no new off-rank node in any P: the extra comm package is not exercised"
    assert out["digest"] == golden()[name]


def test_threaded_distributed_hierarchy():
    assert threaded_result()["digest"] == golden()[THREADED + "_omp3"]


def record():
    assert not os.path.exists(GOLDEN), "%s exists: the digests are recorded once and never again" % GOLDEN
    from hypre_amd import binding as B
    lib = B.load_library(build_if_missing=True)
    out = {}
    for name, options in SINGLE.items():
        out[name] = single_digest(lib, options, threads=1 if name == "7pt_threads" else None)
    assert single_digest(lib, SINGLE["7pt_threads"], threads=8) == out["7pt_threads"]
    for name in sorted(MULTI):
        res = multi_result(name)
        if name.startswith("27pt"):
            assert sum(res["new_nodes"]) > 0, name
        out[name] = res["digest"]
    out[THREADED + "_omp3"] = threaded_result()["digest"]
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("recorded %d cases in %s" % (len(out), GOLDEN))


if __name__ == "__main__":
    if "--record" in sys.argv:
        sys.path.insert(0, os.path.dirname(HERE))
        record()
