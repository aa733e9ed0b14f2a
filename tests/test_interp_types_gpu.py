"""GPU: extended (interp_type 14) and extended+i "if no common C point" (7) interpolation built by the device kernel
(interp_kernels.hip, extpi_rows_kernel<MODE, TYPE>) against the host builders, which tests/test_interp_types.py pins: the
same arrays on every path the kernel takes (rungs of the table ladder, batches of 64 strong neighbours, truncation, many
rows per wave, rows that do not fit the smallest tables or any), the whole setup on the device, the solve on such a
hierarchy against the oracle, and two ranks."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
TYPES = [7, 14]
P27 = dict(n=(30, 30, 30), problem="27pt", P_max_elmts=6, trunc_factor=0.1)


def _restore(lib):
    lib.hypre_amd_SetSetupDeviceRAP(1, 20000)
    lib.hypre_amd_SetSetupDeviceInterp(1)
    lib.hypre_amd_SetSetupDeviceCoarsen(1)
    lib.hypre_amd_SetDeviceInterpWaves(0)


def _hierarchy(lib, opt, everything=False, matrix_on_device=False):
    """set up with the switches the caller chose; ([arrays], interpolations built on the device, levels coarsened there, path)"""
    from hypre_amd import binding as B, ij
    A = ij.build_matrix(opt)
    if matrix_on_device:
        lib.hypre_ParCSRMatrixMigrate(A, B.HYPRE_MEMORY_DEVICE)
    s = ij.create_amg(opt, memory_location=B.HYPRE_MEMORY_DEVICE)
    try:
        lib.HYPRE_BoomerAMGSetup(s, A, None, None)
        B.check()
        built, coarsened = lib.hypre_amd_SetSetupDeviceInterp(-1), lib.hypre_amd_SetSetupDeviceCoarsen(-1)
        rep = (C.c_int * 5)(-9, -9, -9, -9, -9)
        lib.hypre_amd_GetDeviceInterpPath(rep)
        path = dict(zip(("first", "rung", "attempts", "count_then_write", "declined"), list(rep)))
        nl = lib.hypre_amd_BoomerAMGGetNumLevels(s)
        lv = []
        for l in range(nl):
            Al = C.cast(lib.hypre_amd_BoomerAMGGetA(s, l), C.POINTER(B.ParCSRMatrix))
            if l > 0 or not matrix_on_device:
                lv.append(B.csr_to_arrays(Al.contents.diag))
            if l < nl - 1:
                Pl = C.cast(lib.hypre_amd_BoomerAMGGetP(s, l), C.POINTER(B.ParCSRMatrix))
                lv.append(B.csr_to_arrays(Pl.contents.diag))
                if everything:
                    lv.append(B.csr_to_arrays(Pl.contents.diagT))
                    cf = C.cast(lib.hypre_amd_BoomerAMGGetCFMarker(s, l), C.POINTER(B.IntArray)).contents
                    lv.append((B.fetch(cf.data, cf.size, np.int32, cf.memory_location),))
            l1p = lib.hypre_amd_BoomerAMGGetL1Norms(s, l)
            if everything and l1p:
                lv.append((B.vec_to_numpy(C.cast(l1p, C.POINTER(B.Vector))),))
    finally:
        lib.HYPRE_BoomerAMGDestroy(s)
        lib.hypre_ParCSRMatrixDestroy(A)
    return lv, built, coarsened, path


def _same(h0, h1):
    assert len(h0) == len(h1)
    for m0, m1 in zip(h0, h1):
        assert len(m0) == len(m1)
        for a, b in zip(m0, m1):
            assert np.array_equal(a, b)


_host = {}


def _host_hierarchy(lib, interp_type, kw, everything=False):
    """the host-built hierarchy of one case: computed once, shared, never changed"""
    from hypre_amd import ij
    key = (interp_type, json.dumps(kw, sort_keys=True), everything)
    if key not in _host:
        lib.hypre_amd_SetSetupDeviceRAP(0, 50)
        lib.hypre_amd_SetSetupDeviceInterp(0)
        lib.hypre_amd_SetSetupDeviceCoarsen(0 if everything else 1)
        opt = ij.IJOptions(**dict(dict(coarsen_type=8, relax_type=18, interp_type=interp_type), **kw))
        lv, built, coarsened, _ = _hierarchy(lib, opt, everything)
        assert built == 0 and (coarsened == 0 or not everything)
        _host[key] = lv
    return _host[key]


@pytest.mark.parametrize("kw", [dict(n=(40, 39, 38)), P27,
                                dict(n=(32, 32, 32), problem="difconv", a=(3.0, 2.0, 1.0), P_max_elmts=0),
                                dict(n=(34, 33, 32), coarsen_type=10, P_max_elmts=0),
                                dict(n=(40, 40, 20), P_max_elmts=2)])
@pytest.mark.parametrize("rung", [0, 2])
@pytest.mark.parametrize("interp_type", TYPES)
def test_device_interpolation_is_the_host_interpolation(gpu_lib, interp_type, rung, kw):
    from hypre_amd import ij
    lib = gpu_lib
    try:
        host = _host_hierarchy(lib, interp_type, kw)
        lib.hypre_amd_SetSetupDeviceRAP(0, 50)
        lib.hypre_amd_SetSetupDeviceInterp(1 + rung)
        opt = ij.IJOptions(**dict(dict(coarsen_type=8, relax_type=18, interp_type=interp_type), **kw))
        dev, built, _, _ = _hierarchy(lib, opt)
    finally:
        _restore(lib)
    assert built >= 2, built
    _same(host, dev)


@pytest.mark.parametrize("interp_type", TYPES)
def test_a_wave_that_owns_many_rows(gpu_lib, interp_type):
    """three waves for all rows: the tags of the map are reused row after row, and type 7's count of direct C points starts
    from zero in every row"""
    from hypre_amd import ij
    lib = gpu_lib
    try:
        host = _host_hierarchy(lib, interp_type, P27)
        lib.hypre_amd_SetSetupDeviceRAP(0, 50)
        lib.hypre_amd_SetSetupDeviceInterp(1)
        lib.hypre_amd_SetDeviceInterpWaves(3)
        dev, built, _, _ = _hierarchy(lib, ij.IJOptions(coarsen_type=8, relax_type=18, interp_type=interp_type, **P27))
    finally:
        _restore(lib)
    assert built >= 2
    _same(host, dev)


def _two_level(lib, A, on, interp_type):
    """two-level setup of a scipy matrix, wholly on the host or wholly on the device from the smallest tables on: the
    marker, P, its stored transpose, the coarse operator and the smoother diagonals; the counters and the path"""
    from hypre_amd import binding as B, ij
    from util import parcsr
    lib.hypre_amd_SetSetupDeviceRAP(on, 1)
    lib.hypre_amd_SetSetupDeviceInterp(on)
    lib.hypre_amd_SetSetupDeviceCoarsen(on)
    opt = ij.IJOptions(coarsen_type=8, interp_type=interp_type, max_levels=2, P_max_elmts=0, relax_type=18)
    Ap = parcsr(lib, B, A, B.HYPRE_MEMORY_HOST)
    s = ij.create_amg(opt, memory_location=B.HYPRE_MEMORY_DEVICE)
    try:
        lib.HYPRE_BoomerAMGSetup(s, Ap, None, None)
        B.check()                       # the error flag is clear, whoever built the level
        assert lib.hypre_amd_BoomerAMGGetNumLevels(s) == 2
        built, coarsened = lib.hypre_amd_SetSetupDeviceInterp(-1), lib.hypre_amd_SetSetupDeviceCoarsen(-1)
        rep = (C.c_int * 5)(-9, -9, -9, -9, -9)
        lib.hypre_amd_GetDeviceInterpPath(rep)
        path = dict(zip(("first", "rung", "attempts", "count_then_write", "declined"), list(rep)))
        cf = C.cast(lib.hypre_amd_BoomerAMGGetCFMarker(s, 0), C.POINTER(B.IntArray)).contents
        Pl = C.cast(lib.hypre_amd_BoomerAMGGetP(s, 0), C.POINTER(B.ParCSRMatrix))
        A1 = C.cast(lib.hypre_amd_BoomerAMGGetA(s, 1), C.POINTER(B.ParCSRMatrix))
        lv = [(B.fetch(cf.data, cf.size, np.int32, cf.memory_location),), B.csr_to_arrays(Pl.contents.diag),
              B.csr_to_arrays(Pl.contents.diagT), B.csr_to_arrays(A1.contents.diag)]
        for l in range(2):
            l1p = lib.hypre_amd_BoomerAMGGetL1Norms(s, l)
            if l1p:
                lv.append((B.vec_to_numpy(C.cast(l1p, C.POINTER(B.Vector))),))
    finally:
        lib.HYPRE_BoomerAMGDestroy(s)
        lib.hypre_ParCSRMatrixDestroy(Ap)
    return lv, built, coarsened, path


ROOM = (64, 128, 256, 1024)             # set members a row may have on the four rungs of the kernel's table ladder
TABLES_EXHAUSTED = 2


def _overflowing_operand(name):
    """Operands of test_device_coarsening_paths_gpu.py: point 0 is an F point with `direct` strong C neighbours and strong
    F neighbours that bring 10 C points each."""
    from test_device_coarsening_paths_gpu import long_row_operand, set_operand
    if name == "through-an-F-neighbour":          # 60 direct, 129 in all: 64 is passed in the middle of a neighbour's ballot
        return set_operand(129)
    if name == "direct-alone":                    # 70 direct: type 7's first pass overflows the smallest tables by itself
        return set_operand(129, direct=70)
    if name == "common-C":                        # 70 direct; six F neighbours with 9 new C points and one of the direct ones:
        return long_row_operand(4070, real=True, direct=70, groups=[10] * 6, shared=1)      # type 7 leaves those 54 out
    if name == "beyond-the-last-rung":
        return set_operand(1025)
    raise KeyError(name)


@pytest.mark.parametrize("name", ["through-an-F-neighbour", "direct-alone", "common-C", "beyond-the-last-rung"])
@pytest.mark.parametrize("interp_type", TYPES)
def test_a_row_that_does_not_fit_the_smallest_tables(gpu_lib, interp_type, name):
    """A row whose interpolatory set exceeds the 64 members of the first rung — through the ballot of an F neighbour (both
    types), through type 7's first pass over the direct C points alone, with F neighbours that type 7 does not extend
    through — and one beyond the last rung.  The kernel leaves the attempt, everyone climbs to the rung that holds the row
    (one attempt per rung), or the device declines ("tables exhausted") and the host loop builds the level with the error
    flag clear.  The rung is worked out from the host's row of P; the level is the host's, array for array."""
    lib = gpu_lib
    A = _overflowing_operand(name)
    try:
        host, built0, coarsened0, _ = _two_level(lib, A, 0, interp_type)
        dev, built, coarsened, path = _two_level(lib, A, 1, interp_type)
    finally:
        _restore(lib)
    assert built0 == 0 and coarsened0 == 0 and coarsened == 1
    size = int(np.max(np.diff(host[1][0])))
    assert size == int(host[1][0][1] - host[1][0][0]) > 64        # point 0's is the longest row
    want = {("common-C", 7): 70, ("common-C", 14): 124, ("beyond-the-last-rung", 7): 1025, ("beyond-the-last-rung", 14): 1025}
    assert size == want.get((name, interp_type), 129)
    fits = [r for r in range(4) if ROOM[r] >= size]
    print("%s, type %d: set of %d points, path %r" % (name, interp_type, size, path))
    if fits:
        assert fits[0] > 0 and built == 1
        assert path == dict(first=0, rung=fits[0], attempts=fits[0] + 1, count_then_write=1, declined=0), path
    else:
        assert built == 0
        assert path == dict(first=0, rung=-1, attempts=4, count_then_write=1, declined=TABLES_EXHAUSTED), path
    _same(host, dev)


@pytest.mark.parametrize("interp_type,kw,on_device", [(7, dict(n=(40, 39, 38)), False), (14, dict(n=(40, 39, 38)), True),
                                                      (7, P27, False), (14, P27, False), (7, P27, True)])
def test_whole_setup_on_the_device_is_the_host_setup(gpu_lib, interp_type, kw, on_device):
    """strength, PMIS, interpolation, Galerkin product and smoother diagonals on the device (with on_device the caller's
    matrix is there already): markers, operators, stored transposes and l1 norms are the host setup's"""
    from hypre_amd import ij
    lib = gpu_lib
    try:
        host = _host_hierarchy(lib, interp_type, kw, everything=True)
        if on_device:
            host = host[1:]           # the caller's matrix is not read back
        lib.hypre_amd_SetSetupDeviceRAP(1, 50)
        lib.hypre_amd_SetSetupDeviceInterp(1)
        lib.hypre_amd_SetSetupDeviceCoarsen(1)
        opt = ij.IJOptions(**dict(dict(coarsen_type=8, relax_type=18, interp_type=interp_type), **kw))
        dev, built, coarsened, _ = _hierarchy(lib, opt, everything=True, matrix_on_device=on_device)
    finally:
        _restore(lib)
    assert built >= 2 and coarsened >= 2, (built, coarsened)
    _same(host, dev)


@pytest.mark.parametrize("interp_type", [14, 7])
def test_pcg_on_a_device_built_hierarchy_matches_the_oracle(gpu_lib, oracle, interp_type):
    """AMG-PCG on the device, hierarchy set up there with the new type: the oracle's iteration count on the same hierarchy and
    its final residual to 1e-6 relative (the tolerance of the complete solves in test_amg_gpu.py)"""
    from hypre_amd import binding as B, ij
    lib = gpu_lib
    opt = ij.IJOptions(n=(30, 30, 30), problem="27pt", solver=1, coarsen_type=8, relax_type=18, interp_type=interp_type)
    A = ij.build_matrix(opt)
    s = ij.create_amg(opt, memory_location=B.HYPRE_MEMORY_DEVICE)
    lib.hypre_amd_SetSetupDeviceRAP(1, 50)
    try:
        lib.HYPRE_BoomerAMGSetup(s, A, None, None)
        B.check()
        assert lib.hypre_amd_SetSetupDeviceInterp(-1) >= 2
    finally:
        _restore(lib)
    lib.hypre_ParCSRMatrixMigrate(A, B.HYPRE_MEMORY_DEVICE)
    lib.HYPRE_BoomerAMGSetTol(s, 0.0)
    lib.HYPRE_BoomerAMGSetMaxIter(s, 1)
    b, x0 = ij.build_rhs_host(opt, A)
    dx, db = B.parvec_from_numpy(x0), B.parvec_from_numpy(b)
    pcg = C.c_void_p()
    lib.HYPRE_ParCSRPCGCreate(0, C.byref(pcg))
    lib.HYPRE_PCGSetTol(pcg, opt.tol)
    lib.HYPRE_PCGSetMaxIter(pcg, opt.max_iter)
    lib.HYPRE_PCGSetTwoNorm(pcg, 1)
    lib.HYPRE_PCGSetPrecond(pcg, C.cast(lib.HYPRE_BoomerAMGSolve, C.c_void_p), None, s)
    lib.HYPRE_ParCSRPCGSetup(pcg, A, db, dx)
    lib.HYPRE_ParCSRPCGSolve(pcg, A, db, dx)
    its, rel = C.c_int(), C.c_double()
    lib.HYPRE_PCGGetNumIterations(pcg, C.byref(its))
    lib.HYPRE_PCGGetFinalRelativeResidualNorm(pcg, C.byref(rel))
    B.check()
    amg = oracle.amg_from_solvers([s])
    xo = x0.copy()
    oits, orel, _ = amg.pcg(b, xo, tol=opt.tol, max_iter=opt.max_iter, two_norm=1)
    lib.HYPRE_ParCSRPCGDestroy(pcg)
    lib.HYPRE_BoomerAMGDestroy(s)
    lib.hypre_ParCSRMatrixDestroy(A)
    assert its.value == oits and 3 < oits < 30
    assert abs(rel.value - orel) <= 1e-6 * orel


def test_two_ranks_build_the_host_hierarchy_or_decline():
    """Two processes, 24 x 24 x 24 points each (split in z), both types behind one launch: the distributed levels set up by
    the device kernels equal the host-built ones on every rank.  Whether the interpolation of a level was built on the
    device or declined to the host builder shows in the counters: levels coarsened there against interpolations built."""
    from conftest import free_port
    from test_dist_golden import _tail
    cases = [{"name": "type%d" % t, "device": 1, "compare_setup": 1,
              "options": dict(n=[24, 24, 48], P=[1, 1, 2], relax_type=18, coarsen_type=8, interp_type=t)} for t in TYPES]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()), os.path.join(HERE, "dist_worker.py"),
           json.dumps({"batch": cases, "transport": "staged"})]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=dict(os.environ, OMP_NUM_THREADS="1", HYPRE_AMD_TEST_WATCHDOG="300"))
    res = {}
    for line in r.stdout.splitlines():
        if line.startswith("RESULT "):
            d = json.loads(line[len("RESULT "):])
            res[d["name"]] = d
    assert r.returncode == 0 and len(res) == len(cases), _tail(r)
    for name, out in sorted(res.items()):
        assert out["setup_equal"], (name, out["mismatch"])
        assert all(c[0] == 0 and c[1] == 0 for c in out["host_counts"]), out["host_counts"]
        for coarsened, built, _ in out["device_counts"]:
            # the levels went to the device, and every one of them had its interpolation built there: nothing in these
            # rows exceeds the tables, so a decline (built < coarsened) would have no cause
            assert coarsened >= 1 and built == coarsened, (name, out["device_counts"])
