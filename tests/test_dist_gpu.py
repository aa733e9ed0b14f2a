"""GPU, two to four ranks sharing the card: the distributed DEVICE path — pack kernel, overlapped interior
product, ghost product, transpose product with scatter-add, distributed cycle, coarse gather, replicated tail —
against the CPU oracle running the same hierarchy as virtual ranks.

Transport: the stream-staged device-buffer communicator (hypre_amd_CommCreateStreamStaged over gloo).  The library
drives it exactly as it drives RCCL — send buffer packed on the compute stream, event, exchange enqueued on the
communication stream, event, compute stream waits; all-reduces of device buffers — so the production branch of
hypre_ParCSRCommHandleCreate_v2 / Destroy, dev_allreduce_sum and the event pool run between real ranks here.  (RCCL
itself refuses two ranks on one device; its provider is covered by the size-1 self-test below and by bench.py
--gpus N.)  A few cases also run over the blocking host-staged branch (device_buffers = 0)."""
import pytest

import json
import os
import subprocess
import sys

from test_dist_golden import GOLD, HERE, run_ranks, _tail

pytestmark = pytest.mark.gpu

DEVICE_CASES = ["smoother.out.10", "smoother.out.9", "solvers.out.21", "default.out.1",
                "smoother.out.0", "smoother.out.3", "smoother.out.11", "smoother.out.11.2",
                "smoother.out.12", "smoother.out.16", "smoother.out.17", "smoother.out.23",
                "matrix.out.11", "solvers.out.404", "solvers.out.405",
                "solvers.out.2", "solvers.out.20", "solvers.out.22", "elast.out.7",
                "solvers.out.sysu", "solvers.out.29", "solvers.out.30", "smoother.out.18", "smoother.out.19",
                "smoother.out.20", "smoother.out.14", "smoother.out.15", "solvers.out.25"]
_batches = {}


def device_batch_result(name):
    """The device cases of one rank count share a launch: one process per rank solves them one after the other (which
    also exercises create / solve / destroy cycles inside one process), ranks share the card."""
    nranks = GOLD[name]["ranks"]
    if nranks not in _batches:
        from conftest import free_port
        names = [k for k in DEVICE_CASES if GOLD[k]["ranks"] == nranks]
        spec = {"batch": [{"name": k, "options": GOLD[k]["options"], "device": 1} for k in names], "transport": "staged"}
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nranks),
               "--master-addr", "127.0.0.1", "--master-port", str(free_port()), os.path.join(HERE, "dist_worker.py"),
               json.dumps(spec)]
        env = dict(os.environ, OMP_NUM_THREADS="1", HYPRE_AMD_TEST_WATCHDOG="900")
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=1200, env=env)
        res = {}
        for line in r.stdout.splitlines():
            if line.startswith("RESULT "):
                d = json.loads(line[len("RESULT "):])
                res[d["name"]] = d
        _batches[nranks] = (r.returncode, res, _tail(r))
    rc, res, tail = _batches[nranks]
    assert name in res, "no result for %s (worker exit code %d)\n%s" % (name, rc, tail)
    return res[name]


@pytest.mark.parametrize("name", DEVICE_CASES)
def test_two_or_three_ranks_on_device(name):
    case = dict(GOLD[name])
    out = device_batch_result(name)
    exp = case["expect"]
    assert out["matvec_err"] < 1e-13 and out["matvecT_err"] < 1e-13 and out["dot_err"] < 1e-12
    assert out["mv_err"] < 1e-13 and out["matvecT_repeats"]
    assert out["dev_iterations"] == out["iterations"]
    assert abs(out["dev_rel_resid"] - out["rel_resid"]) <= 1e-6 * out["rel_resid"]
    assert out["x_err"] < 1e-9
    # the overlap diagnosis (hypre_amd_CommExposedTimes): the solve's exchanges were timed, level by level; what the compute
    # stream waited for an exchange cannot exceed what the exchange took
    t = out["timed"]
    assert t["exchanges"] > 0 and t["in_cycle"] > 0 and t["transfer_us"] > 0.0 and t["exposed_us"] >= 0.0 and t["worst"] <= 50.0 and t["host_us"] > 0.0
    if "iterations" in exp:
        assert out["dev_iterations"] == exp["iterations"]
        assert abs(out["dev_rel_resid"] - exp["rel_resid"]) <= 5e-7 * exp["rel_resid"]
    if "conv_factor" in exp:
        # same iteration count and final residual as the oracle, whose factor is pinned on the CPU side
        assert abs(out["conv_factor"] - exp["conv_factor"]) < 5.1e-7


HOST_STAGED_CASES = ["smoother.out.10", "solvers.out.21", "smoother.out.0"]


@pytest.mark.parametrize("name", HOST_STAGED_CASES)
def test_blocking_host_staged_branch(name):
    """device_buffers = 0: hypre_ParCSRCommHandleCreate_v2 copies the halo buffers through host memory around a
    blocking exchange (what the reference's device path does).  Same goldens."""
    case = dict(GOLD[name])
    out = run_ranks(case["ranks"], {"options": case["options"]}, timeout=600, extra={"device": 1})
    exp = case["expect"]
    assert out["matvec_err"] < 1e-13 and out["matvecT_err"] < 1e-13 and out["dot_err"] < 1e-12
    assert out["dev_iterations"] == out["iterations"]
    if "iterations" in exp:
        assert out["dev_iterations"] == exp["iterations"]
        assert abs(out["dev_rel_resid"] - exp["rel_resid"]) <= 5e-7 * exp["rel_resid"]


# The three multi-rank BASELINE configurations at sizes the oracle solves in seconds, ranks in the reference's
# P x Q x R box layout: C3 (7-point, l1-Jacobi, replicated tail), C4 (27-point, two-stage Gauss-Seidel: every level
# stays distributed), C5 (anisotropic diffusion, fp32 matrix values in the cycle).  AMG alone and under PCG.
BASELINE_CASES = {
    "c3_pcg_4ranks": (4, dict(n=[24, 24, 12], P=[2, 2, 1], relax_type=18, coarsen_type=8, solver=1), {}),
    "c3_amg_4ranks": (4, dict(n=[24, 24, 12], P=[2, 2, 1], relax_type=18, coarsen_type=8), {}),
    "c3_amg_4ranks_no_tail": (4, dict(n=[24, 24, 12], P=[2, 2, 1], relax_type=18, coarsen_type=8), {"replicate": 0}),
    "c4_amg_relax11_2ranks": (2, dict(n=[16, 16, 16], P=[2, 1, 1], problem="27pt", relax_type=11, coarsen_type=8), {}),
    "c4_pcg_relax11_4ranks": (4, dict(n=[20, 20, 10], P=[2, 2, 1], problem="27pt", relax_type=11, coarsen_type=8, solver=1), {}),
    "c4_pcg_relax12_4ranks": (4, dict(n=[20, 20, 10], P=[2, 2, 1], problem="27pt", relax_type=12, coarsen_type=8, solver=1), {}),
    "c4_pcg_relax11_4ranks_no_tail": (4, dict(n=[20, 20, 10], P=[2, 2, 1], problem="27pt", relax_type=11, coarsen_type=8, solver=1),
                                      {"replicate": 0}),
    "c4_amg_relax12_2ranks_no_tail": (2, dict(n=[16, 16, 16], P=[2, 1, 1], problem="27pt", relax_type=12, coarsen_type=8),
                                      {"replicate": 0}),
    "c5_amg_mixed_2ranks": (2, dict(n=[20, 20, 20], P=[1, 1, 2], problem="difconv", c=[1.0, 1.0, 0.001], a=[0.0, 0.0, 0.0],
                                    relax_type=18, coarsen_type=8), {"mixed": 1}),
    "c5_pcg_mixed_4ranks": (4, dict(n=[20, 20, 20], P=[2, 2, 1], problem="difconv", c=[1.0, 1.0, 0.001], a=[0.0, 0.0, 0.0],
                                    relax_type=18, coarsen_type=8, solver=1), {"mixed": 1}),
    "c5_pcg_mixed_relax11_4ranks": (4, dict(n=[16, 16, 16], P=[2, 2, 1], problem="27pt", relax_type=11, coarsen_type=8, solver=1),
                                    {"mixed": 1}),
    "c5_amg_mixed_2ranks_no_tail": (2, dict(n=[20, 20, 20], P=[1, 1, 2], problem="difconv", c=[1.0, 1.0, 0.001], a=[0.0, 0.0, 0.0],
                                            relax_type=18, coarsen_type=8), {"mixed": 1, "replicate": 0}),
    # -coarse_th 40: the dense solve of the coarsest level on more than the default 9 unknowns, its right-hand side
    # gathered from every rank's slice (zero-fill, own slice, all-reduce: hypre_GaussElimSolve).  Coarsest level and the
    # ranks' slices with the host setup: 25 rows (15, 10; the one-wave kernel), 39 rows (14, 12, 13; the one-lane kernel)
    # and 10 rows of which the middle rank owns a single one (5, 1, 4).
    "coarse40_amg_2ranks_no_tail": (2, dict(n=[16, 15, 14], P=[2, 1, 1], relax_type=18, coarsen_type=8, coarse_threshold=40),
                                    {"replicate": 0}),
    "coarse40_amg_3ranks_no_tail": (3, dict(n=[18, 15, 21], P=[1, 1, 3], relax_type=18, coarsen_type=8, coarse_threshold=40),
                                    {"replicate": 0}),
    "coarse40_amg_3ranks_one_row_slice_no_tail": (3, dict(n=[21, 19, 18], P=[3, 1, 1], relax_type=18, coarsen_type=8,
                                                          coarse_threshold=40), {"replicate": 0}),
}
# rows the coarsest level of the coarse40 cases must have (lower bound, upper bound, smallest slice of a rank)
COARSE40_ROWS = {"coarse40_amg_2ranks_no_tail": (10, 32, 2), "coarse40_amg_3ranks_no_tail": (33, 40, 2),
                 "coarse40_amg_3ranks_one_row_slice_no_tail": (10, 32, 1)}
_baseline = {}


def _baseline_result(name):
    nranks = BASELINE_CASES[name][0]
    if nranks not in _baseline:
        from conftest import free_port
        names = [k for k, v in BASELINE_CASES.items() if v[0] == nranks]
        spec = {"batch": [dict({"name": k, "options": BASELINE_CASES[k][1], "device": 1}, **BASELINE_CASES[k][2])
                          for k in names], "transport": "staged"}
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nranks),
               "--master-addr", "127.0.0.1", "--master-port", str(free_port()), os.path.join(HERE, "dist_worker.py"),
               json.dumps(spec)]
        env = dict(os.environ, OMP_NUM_THREADS="1", HYPRE_AMD_TEST_WATCHDOG="900")
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=1200, env=env)
        res = {}
        for line in r.stdout.splitlines():
            if line.startswith("RESULT "):
                d = json.loads(line[len("RESULT "):])
                res[d["name"]] = d
        _baseline[nranks] = (r.returncode, res, _tail(r))
    rc, res, tail = _baseline[nranks]
    assert name in res, "no result for %s (worker exit code %d)\n%s" % (name, rc, tail)
    return res[name]


@pytest.mark.parametrize("name", sorted(BASELINE_CASES))
def test_baseline_multi_rank_configs_on_device(name):
    out = _baseline_result(name)
    assert out["matvec_err"] < 1e-13 and out["matvecT_err"] < 1e-13 and out["dot_err"] < 1e-12
    assert out["mv_err"] < 1e-13 and out["matvecT_repeats"]
    assert out["dev_iterations"] == out["iterations"] and out["iterations"] > 3
    assert abs(out["dev_rel_resid"] - out["rel_resid"]) <= 1e-6 * out["rel_resid"]
    assert out["x_err"] < 1e-9
    # the small levels run on every rank's replica (one all-reduce per cycle instead of four halo exchanges per
    # level) for all three configurations: two-stage GS keeps the triangles of the ranks' diagonal blocks there,
    # mixed precision the fp32-rounded values
    assert (out["replicated_level"] == -1) == ("no_tail" in name)
    if name in COARSE40_ROWS:
        # every rank owns part of a coarsest level of the intended size
        lo, hi, smallest = COARSE40_ROWS[name]
        rows = out["coarse_local_rows"]
        assert lo <= out["sizes"][-1] == sum(rows) <= hi and min(rows) >= 1 and (smallest > 1 or min(rows) == 1), (out["sizes"], rows)


# The distributed SETUP on the device (par_amg_setup_dist.cpp, the device half: the single-rank kernels on the extended
# numbering [local points | ghost points]) against the host routines of the same library, which the reference's 2-8-rank
# regression files pin: every array of every level identical on every rank.  Levels of at least min_rows rows per rank go to
# the device (default 20000: the test lowers it so that three or four levels of these small problems do).  Rank counts:
# the GPU box admits six processes on its card at once — the test runner, the launcher and FOUR ranks — so the 2 x 2 x 2
# boxes of the eight-GPU configurations cannot share it; 2 x 2 x 1 gives the 27-point operator faces and an edge (three
# neighbours), 1 x 2 x 2 and 4 x 1 x 1 the other orientations.  (Eight ranks run through the same routines on the host
# transport in tests/test_dist_golden.py; the eight-GPU run is the driver's.)
SETUP_CASES = {
    "c3_7pt_2ranks": (2, dict(n=[40, 20, 20], P=[2, 1, 1], relax_type=18, coarsen_type=8), {}),
    "c3_7pt_4ranks": (4, dict(n=[40, 40, 20], P=[2, 2, 1], relax_type=18, coarsen_type=8), {}),
    "c3_7pt_4ranks_matrix_on_device": (4, dict(n=[36, 36, 18], P=[2, 2, 1], relax_type=18, coarsen_type=8), {"matrix_on_device": 1}),
    "c3_7pt_4ranks_1x1x4": (4, dict(n=[20, 20, 48], P=[1, 1, 4], relax_type=18, coarsen_type=8), {"rung": 2}),
    "c3_7pt_4ranks_4x1x1": (4, dict(n=[64, 14, 14], P=[4, 1, 1], relax_type=18, coarsen_type=8), {}),
    "c4_27pt_2ranks_relax11": (2, dict(n=[32, 16, 16], P=[2, 1, 1], problem="27pt", relax_type=11, coarsen_type=8), {}),
    "c4_27pt_4ranks_relax12": (4, dict(n=[28, 28, 14], P=[2, 2, 1], problem="27pt", relax_type=12, coarsen_type=8), {}),
    "c4_27pt_4ranks_1x2x2_relax11": (4, dict(n=[14, 26, 26], P=[1, 2, 2], problem="27pt", relax_type=11, coarsen_type=8), {}),
    "c5_difconv_4ranks": (4, dict(n=[32, 32, 16], P=[2, 2, 1], problem="difconv", c=[1.0, 1.0, 0.001], a=[0.0, 0.0, 0.0],
                                  relax_type=18, coarsen_type=8), {}),
    "c5_difconv_convection_2ranks": (2, dict(n=[24, 24, 24], P=[1, 1, 2], problem="difconv", c=[1.0, 0.01, 1.0], a=[3.0, 2.0, 1.0],
                                             relax_type=18, coarsen_type=8), {}),
    "pmis1_trunc_4ranks": (4, dict(n=[28, 28, 14], P=[2, 2, 1], problem="27pt", relax_type=18, coarsen_type=9, P_max_elmts=6,
                                   trunc_factor=0.1), {}),
    "no_pmax_2ranks": (2, dict(n=[32, 16, 16], P=[2, 1, 1], relax_type=18, coarsen_type=8, P_max_elmts=0), {}),
    "pmax2_3ranks": (3, dict(n=[45, 16, 16], P=[3, 1, 1], relax_type=7, coarsen_type=8, P_max_elmts=2), {}),
    "cf_relax_l1_4ranks": (4, dict(n=[32, 32, 16], P=[2, 2, 1], relax_type=18, relax_order=1, coarsen_type=8), {}),
    "l1_gs_3ranks": (3, dict(n=[42, 18, 18], P=[3, 1, 1], relax_type=8, coarsen_type=8), {}),
    # a rank's device kernel declines a step (tables too small for a row: here on request): every rank repeats the step
    # with the host routine and the level's remaining steps follow on the host copies
    "decline_interp_rank1_4ranks": (4, dict(n=[32, 32, 16], P=[2, 2, 1], relax_type=18, coarsen_type=8), {"decline": [1, 1]}),
    "decline_product_rows_rank0_4ranks": (4, dict(n=[28, 28, 14], P=[2, 2, 1], problem="27pt", relax_type=11, coarsen_type=8), {"decline": [2, 0]}),
    "decline_product_rank2_3ranks": (3, dict(n=[45, 16, 16], P=[3, 1, 1], relax_type=18, coarsen_type=8), {"decline": [3, 2]}),
    "strong_threshold_4ranks": (4, dict(n=[32, 32, 16], P=[2, 2, 1], relax_type=18, coarsen_type=8, strong_threshold=0.6, max_row_sum=0.8), {}),
}
# the device product's retry ladder (first tables forced small) and its budget of strided scratch (0: every product of
# the distributed levels goes to the host routine) on two of the cases above
for _base in ("c3_7pt_2ranks", "c4_27pt_2ranks_relax11"):
    SETUP_CASES[_base + "_rap_small_tables"] = (2, SETUP_CASES[_base][1], {"rap_tables": [16, 8, -1]})
    SETUP_CASES[_base + "_rap_no_scratch"] = (2, SETUP_CASES[_base][1], {"rap_tables": [-1, -1, 0]})
_setup = {}


def _setup_result(name):
    nranks = SETUP_CASES[name][0]
    if nranks not in _setup:
        from conftest import free_port
        names = [k for k, v in SETUP_CASES.items() if v[0] == nranks]
        spec = {"batch": [dict({"name": k, "options": SETUP_CASES[k][1], "device": 1, "compare_setup": 1}, **SETUP_CASES[k][2])
                          for k in names], "transport": "staged"}
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nranks),
               "--master-addr", "127.0.0.1", "--master-port", str(free_port()), os.path.join(HERE, "dist_worker.py"),
               json.dumps(spec)]
        env = dict(os.environ, OMP_NUM_THREADS="1", HYPRE_AMD_TEST_WATCHDOG="900")
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=1200, env=env)
        res = {}
        for line in r.stdout.splitlines():
            if line.startswith("RESULT "):
                d = json.loads(line[len("RESULT "):])
                res[d["name"]] = d
        _setup[nranks] = (r.returncode, res, _tail(r))
    rc, res, tail = _setup[nranks]
    assert name in res, "no result for %s (worker exit code %d)\n%s" % (name, rc, tail)
    return res[name]


@pytest.mark.parametrize("name", sorted(SETUP_CASES))
def test_distributed_device_setup_is_the_host_setup(name):
    out = _setup_result(name)
    assert out["setup_equal"], out["mismatch"]
    # the host run coarsened nothing on the device, the device run at least two levels on every rank, interpolation and
    # Galerkin product included
    assert all(c[0] == 0 for c in out["host_counts"]), out["host_counts"]
    if name.endswith("_rap_no_scratch"):
        # no product fits the scratch budget: all of them on the host, coarsening and interpolation still on the device
        assert all(min(c[:2]) >= 2 and c[2] == 0 for c in out["device_counts"]), out["device_counts"]
    else:
        assert all(min(c) >= (1 if "decline" in name else 2) for c in out["device_counts"]), out["device_counts"]


@pytest.mark.parametrize("name", sorted(k for k in SETUP_CASES if "_rap_" in k))
def test_distributed_device_product_takes_the_forced_path(name):
    """the path report of every rank's last device product: no pilot and a second attempt or more with the small first
    tables, the host routine without scratch"""
    paths = _setup_result(name)["rap_paths"]
    for pilot, attempts, two_walks, fell_back in paths:
        if name.endswith("_rap_small_tables"):
            assert pilot == 0 and attempts >= 2 and two_walks == 0 and fell_back == 0, paths
        else:
            assert attempts == 0 and fell_back == 1, paths


# ... and the solve phase on hierarchies the device built (communication packages, row lists of the ghost blocks, stored
# transposes made there): the BASELINE configurations again, AMG and AMG-PCG against the oracle on the exported hierarchy
DEVICE_BUILT_CASES = {
    "c3_pcg_4ranks": (4, dict(n=[32, 32, 16], P=[2, 2, 1], relax_type=18, coarsen_type=8, solver=1), {"min_rows": 40}),
    "c3_amg_4ranks_no_tail": (4, dict(n=[32, 32, 16], P=[2, 2, 1], relax_type=18, coarsen_type=8), {"min_rows": 40, "replicate": 0}),
    "c3_amg_4ranks_matrix_on_device": (4, dict(n=[32, 32, 16], P=[2, 2, 1], relax_type=18, coarsen_type=8),
                                       {"min_rows": 40, "matrix_on_device": 1}),
    "c4_pcg_relax11_4ranks": (4, dict(n=[24, 24, 12], P=[2, 2, 1], problem="27pt", relax_type=11, coarsen_type=8, solver=1), {"min_rows": 40}),
    "c4_amg_relax12_4ranks_no_tail": (4, dict(n=[12, 24, 24], P=[1, 2, 2], problem="27pt", relax_type=12, coarsen_type=8),
                                      {"min_rows": 40, "replicate": 0}),
    "c5_pcg_mixed_4ranks": (4, dict(n=[24, 24, 24], P=[2, 2, 1], problem="difconv", c=[1.0, 1.0, 0.001], a=[0.0, 0.0, 0.0],
                                    relax_type=18, coarsen_type=8, solver=1), {"min_rows": 40, "mixed": 1}),
    "c3_amg_3ranks": (3, dict(n=[36, 20, 20], P=[3, 1, 1], relax_type=18, coarsen_type=8), {"min_rows": 40}),
}
_built = {}


def _built_result(name):
    nranks = DEVICE_BUILT_CASES[name][0]
    if nranks not in _built:
        from conftest import free_port
        names = [k for k, v in DEVICE_BUILT_CASES.items() if v[0] == nranks]
        spec = {"batch": [dict({"name": k, "options": DEVICE_BUILT_CASES[k][1], "device": 1}, **DEVICE_BUILT_CASES[k][2])
                          for k in names], "transport": "staged"}
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nranks),
               "--master-addr", "127.0.0.1", "--master-port", str(free_port()), os.path.join(HERE, "dist_worker.py"),
               json.dumps(spec)]
        env = dict(os.environ, OMP_NUM_THREADS="1", HYPRE_AMD_TEST_WATCHDOG="900")
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=1200, env=env)
        res = {}
        for line in r.stdout.splitlines():
            if line.startswith("RESULT "):
                d = json.loads(line[len("RESULT "):])
                res[d["name"]] = d
        _built[nranks] = (r.returncode, res, _tail(r))
    rc, res, tail = _built[nranks]
    assert name in res, "no result for %s (worker exit code %d)\n%s" % (name, rc, tail)
    return res[name]


@pytest.mark.parametrize("name", sorted(DEVICE_BUILT_CASES))
def test_solves_on_device_built_distributed_hierarchies(name):
    out = _built_result(name)
    assert out["device_levels"] >= 2
    assert out["matvec_err"] < 1e-13 and out["matvecT_err"] < 1e-13 and out["dot_err"] < 1e-12
    assert out["dev_iterations"] == out["iterations"] and out["iterations"] > 3
    assert abs(out["dev_rel_resid"] - out["rel_resid"]) <= 1e-6 * out["rel_resid"]
    assert out["x_err"] < 1e-9
    assert (out["replicated_level"] == -1) == ("no_tail" in name)


def test_replicated_tail_is_used_and_optional():
    """Jacobi-type V-cycles on several ranks run their small levels on a replicated copy (one all-reduce instead of
    four halo exchanges per level); switched off, the same solve goes through the distributed levels.  Both
    reproduce the reference's golden (smoother.out.9: relax 18 with CF ordering, 3 ranks)."""
    case = dict(GOLD["smoother.out.9"])
    on = run_ranks(3, {"options": case["options"], "device": 1}, timeout=600, extra={"device": 1, "transport": "staged"})
    off = run_ranks(3, {"options": case["options"]}, timeout=600, extra={"device": 1, "replicate": 0, "transport": "staged"})
    assert on["replicated_level"] >= 1 and off["replicated_level"] == -1
    for out in (on, off):
        assert out["dev_iterations"] == case["expect"]["iterations"]
        assert abs(out["dev_rel_resid"] - case["expect"]["rel_resid"]) <= 5e-7 * case["expect"]["rel_resid"]
    # same operators, same sweeps; only the association of the row sums differs (one piece vs diag + ghost block)
    assert abs(on["dev_rel_resid"] - off["dev_rel_resid"]) <= 1e-6 * off["dev_rel_resid"]


@pytest.mark.parametrize("name", ["vector.out.B100", "vector.out.B107", "vector.out.B101", "solvers.out.1", "solvers.out.3"])
def test_ds_pcg_on_multivectors_four_ranks_on_device(name):
    """test/TEST_ij/vector.jobs (and solvers.jobs:34,36: the single-vector lines on 2 ranks): PCG (B101, solvers.out.3:
    GMRES(5)) with diagonal scaling on a multivector of 6 / 7 columns over 4 ranks — the multivector
    products (one halo exchange for all columns, the local block fused over the columns), inner products, updates and
    the diagonal scaling on the device — against the reference's saved lines and the oracle's iterate."""
    case = dict(GOLD[name])
    out = run_ranks(case["ranks"], {"options": case["options"]}, timeout=600, extra={"device": 1, "transport": "staged"})
    assert out["dev_iterations"] == case["expect"]["iterations"] == out["iterations"]
    assert abs(out["dev_rel_resid"] - case["expect"]["rel_resid"]) <= 5e-7 * case["expect"]["rel_resid"]
    assert out["x_err"] < (1e-7 if case["options"]["solver"] == 4 else 1e-9)      # (54 Arnoldi steps amplify the last bits)
    if case["options"].get("num_components", 1) > 1:
        assert all(f > 0 for f in out["fused"])          # the fused kernel served the local blocks' products


@pytest.mark.parametrize("name", ["posneg.out.400", "posneg.out.402", "posneg.out.403"])
def test_negated_operator_solves_alike_on_device(name):
    """test/TEST_ij/posneg.jobs on the device path: with -A the distributed device solve (AMG, Chebyshev smoothing,
    GMRES) takes the iterations and reaches the residual it does with A, and both are the oracle's."""
    from test_dist_golden import posneg_pair
    pos, neg = posneg_pair(name, extra={"device": 1, "transport": "staged"})
    for out in (pos, neg):
        assert out["dev_iterations"] == out["iterations"]
        assert abs(out["dev_rel_resid"] - out["rel_resid"]) <= 1e-6 * out["rel_resid"]
    assert pos["dev_iterations"] == neg["dev_iterations"]
    assert abs(pos["dev_rel_resid"] - neg["dev_rel_resid"]) <= 5e-7 * pos["dev_rel_resid"]


def test_pcg_three_ranks_on_device():
    case = dict(GOLD["solvers.out.19"])
    out = run_ranks(3, {"options": case["options"]}, timeout=600, extra={"device": 1, "transport": "staged"})
    assert out["dev_iterations"] == case["expect"]["iterations"] == out["iterations"]
    assert abs(out["dev_rel_resid"] - case["expect"]["rel_resid"]) <= 5e-7 * case["expect"]["rel_resid"]


def test_rccl_provider_single_rank_round_trip():
    """The RCCL provider on the one GPU a test box has: a size-1 communicator whose ring shift is a
    send-to-self / recv-from-self pair inside one ncclGroup, plus all-reduce and all-gather, with
    host-staged and device buffers (hypre_amd_CommSelfTest)."""
    import ctypes as C
    from hypre_amd import binding as B
    L = B.load_library()
    ident = (C.c_ubyte * 128)()
    L.hypre_amd_RCCLGetUniqueId(C.cast(ident, C.c_void_p))
    B.check()
    comm = L.hypre_amd_CommCreateRCCL(C.cast(ident, C.c_void_p), 0, 1)
    B.check()
    assert comm > 0
    assert L.hypre_amd_CommSelfTest(comm, 1 << 16) == 0
    assert L.hypre_amd_CommSelfTest(comm, 24) == 0
    B.check()
    L.hypre_amd_CommDestroy(comm)


def test_rank_without_rows_on_device():
    """Three grid points across four ranks: one rank owns nothing on any level.  Empty blocks, empty halos and empty
    device arrays must go through setup, migration, the distributed solve and destruction without an error."""
    opts = {"n": [3, 5, 4], "P": [4, 1, 1], "relax_type": 18, "coarsen_type": 8}
    out = run_ranks(4, {"options": opts, "device": 1}, timeout=600, extra={"device": 1, "transport": "staged"})
    assert out["sizes"][0] == 60
    assert out["dev_iterations"] == out["iterations"]
    assert abs(out["dev_rel_resid"] - out["rel_resid"]) <= 1e-6 * out["rel_resid"]
    assert out["x_err"] < 1e-9
