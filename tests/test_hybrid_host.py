"""The hybrid solver, the convergence-factor setters and the fused-step switch as far as no GPU is needed: defaults against
parcsr_ls/amg_hybrid.c:99-160 through what can be read back, ranges and refusals of the setters, the golden file, and the
driver's three options (set in code; the command line keeps refusing `-solver 20`)."""
import ctypes as C
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = json.load(open(os.path.join(HERE, "golden", "ij_saved_hybrid.json")))


def test_the_golden_file_holds_the_four_reference_lines():
    """test/TEST_ij/solvers.jobs:41-44 with solvers.saved:25-47, number for number"""
    jobs = GOLD["jobs"]
    assert sorted(jobs) == ["solvers.out.10", "solvers.out.11", "solvers.out.8", "solvers.out.9"]
    want = {"solvers.out.8": (41, 0, 41, 6.698760e-09, {"hybrid": 1, "rhs": "rand"}),
            "solvers.out.9": (11, 7, 4, 6.805037e-10, {"hybrid": 1, "rhs": "rand", "cf_tol": 0.5}),
            "solvers.out.10": (9, 7, 2, 4.842561e-09, {"hybrid": 1, "rhs": "rand", "cf_tol": 0.5, "hybrid_solver_type": 2}),
            "solvers.out.11": (7, 4, 3, 1.289995e-10, {"hybrid": 1, "rhs": "rand", "cf_tol": 0.5, "hybrid_solver_type": 3})}
    for name, (its, pcg, dscg, rel, options) in want.items():
        assert jobs[name]["np"] == 2 and jobs[name]["options"] == options
        assert jobs[name]["expect"] == {"iterations": its, "pcg_iterations": pcg, "dscg_iterations": dscg, "rel_resid": rel}
        assert its == pcg + dscg
    assert sorted(GOLD["parent"]) == ["amg-gmres", "amg-pcg", "ds-gmres", "ds-pcg", "ds-pcg-two-norm"]


def test_the_driver_takes_the_three_options_in_code_only():
    from hypre_amd import ij
    opt = ij.check_options(ij.IJOptions(hybrid=1, hybrid_solver_type=3, cf_tol=0.5, rhs="rand"))
    assert (opt.hybrid, opt.hybrid_solver_type, opt.cf_tol, opt.solver) == (1, 3, 0.5, 0)
    d = ij.IJOptions()
    assert (d.hybrid, d.hybrid_solver_type, d.cf_tol) == (0, 1, 0.9)                  # test/ij.c:140, 157
    for name in GOLD["jobs"]:
        ij.check_options(ij.IJOptions(**GOLD["jobs"][name]["options"]))
    for bad in (dict(hybrid=1, solver=1), dict(hybrid=1, solver=2), dict(hybrid=1, solver=20), dict(hybrid=2), dict(cf_tol=0.5),
                dict(hybrid_solver_type=2), dict(hybrid=1, hybrid_solver_type=4), dict(hybrid=1, cf_tol=1.5),
                dict(hybrid=1, num_components=2), dict(solver=20)):
        with pytest.raises(SystemExit):
            ij.check_options(ij.IJOptions(**bad))
    with pytest.raises(SystemExit) as e:
        ij.parse_cli(["-solver", "20"])
    assert "-solver 20 is outside the scope of this driver" in str(e.value)
    for flag in ("-cf", "-solver_type"):
        with pytest.raises(SystemExit):
            ij.parse_cli([flag, "1"])


def test_hybrid_setters_getters_defaults_and_refusals(lib):
    lib.HYPRE_ClearAllErrors()
    h = C.c_void_p()
    assert lib.HYPRE_ParCSRHybridCreate(C.byref(h)) == 0 and h.value
    # what can be read back of a new object (amg_hybrid.c:99-160): no iterations, no norm, no times, no hierarchy
    its, pcg, dscg, rel, rec = C.c_int(-1), C.c_int(-1), C.c_int(-1), C.c_double(-1.0), C.c_int(-1)
    assert lib.HYPRE_ParCSRHybridGetNumIterations(h, C.byref(its)) == 0 and its.value == 0
    assert lib.HYPRE_ParCSRHybridGetPCGNumIterations(h, C.byref(pcg)) == 0 and pcg.value == 0
    assert lib.HYPRE_ParCSRHybridGetDSCGNumIterations(h, C.byref(dscg)) == 0 and dscg.value == 0
    assert lib.HYPRE_ParCSRHybridGetFinalRelativeResidualNorm(h, C.byref(rel)) == 0 and rel.value == 0.0
    assert lib.HYPRE_ParCSRHybridGetRecomputeResidual(h, C.byref(rec)) == 0 and rec.value == 0
    times = (C.c_double * 4)(9.0, 9.0, 9.0, 9.0)
    assert lib.HYPRE_ParCSRHybridGetSetupSolveTime(h, times) == 0 and list(times) == [0.0, 0.0, 0.0, 0.0]
    amg, kry = C.c_void_p(1), C.c_void_p(1)
    assert lib.hypre_amd_ParCSRHybridGetPrecond(h, C.byref(amg)) == 0 and amg.value is None
    assert lib.hypre_amd_ParCSRHybridGetKrylovSolver(h, C.byref(kry)) == 0 and kry.value is None
    # every setter takes its default (amg_hybrid.c:104-156)
    for name, v in (("Tol", 1.0e-6), ("AbsoluteTol", 0.0), ("ConvergenceTol", 0.9), ("StrongThreshold", 0.25), ("MaxRowSum", 0.9),
                    ("TruncFactor", 0.0), ("RelaxWt", 1.0), ("OuterWt", 1.0)):
        assert getattr(lib, "HYPRE_ParCSRHybridSet" + name)(h, v) == 0, name
    for name, v in (("DSCGMaxIter", 1000), ("PCGMaxIter", 200), ("TwoNorm", 0), ("StopCrit", 0), ("RelChange", 0), ("RecomputeResidual", 0),
                    ("SolverType", 1), ("KDim", 5), ("SetupType", 1), ("Logging", 0), ("PrintLevel", 0), ("PMaxElmts", 4), ("MaxLevels", 25),
                    ("MeasureType", 0), ("CoarsenType", 10), ("InterpType", 6), ("CycleType", 1), ("RelaxOrder", 0), ("KeepTranspose", 0),
                    ("MaxCoarseSize", 9), ("MinCoarseSize", 1), ("SeqThreshold", 0), ("AggNumLevels", 0), ("AggInterpType", 4), ("NumPaths", 1),
                    ("NumFunctions", 1), ("Nodal", 0), ("NumSweeps", 1), ("RelaxType", 6), ("TwoNorm", 1), ("SolverType", 2), ("SolverType", 3)):
        assert getattr(lib, "HYPRE_ParCSRHybridSet" + name)(h, v) == 0, name
    for k, t in ((1, 13), (2, 14), (3, 9)):
        assert lib.HYPRE_ParCSRHybridSetCycleRelaxType(h, t, k) == 0 and lib.HYPRE_ParCSRHybridSetCycleNumSweeps(h, 2, k) == 0
    assert lib.HYPRE_ParCSRHybridSetLevelRelaxWt(h, 0.8, 1) == 0 and lib.HYPRE_ParCSRHybridSetLevelOuterWt(h, 0.9, 0) == 0
    assert lib.HYPRE_ParCSRHybridSetNonGalerkinTol(h, 0, None) == 0
    assert lib.HYPRE_GetError() == 0
    # ranges, as the reference checks them: HYPRE_ERROR_ARG on the value
    for name, v in (("Tol", -1.0), ("Tol", 2.0), ("AbsoluteTol", -1.0), ("ConvergenceTol", 1.5), ("StrongThreshold", 2.0), ("MaxRowSum", -0.1),
                    ("TruncFactor", 1.5)):
        getattr(lib, "HYPRE_ParCSRHybridSet" + name)(h, v)
        assert lib.HYPRE_GetError() & 4 and lib.HYPRE_GetErrorArg() == 2, name
        lib.HYPRE_ClearAllErrors()
    for name, v in (("DSCGMaxIter", -1), ("PCGMaxIter", -1), ("KDim", 0), ("PMaxElmts", -1), ("MaxLevels", 0), ("InterpType", -1), ("CycleType", 3),
                    ("NumSweeps", 0), ("MaxCoarseSize", 0), ("MinCoarseSize", -1), ("SeqThreshold", -1), ("NumPaths", 0), ("AggNumLevels", -1),
                    ("NumFunctions", 0)):
        getattr(lib, "HYPRE_ParCSRHybridSet" + name)(h, v)
        assert lib.HYPRE_GetError() & 4 and lib.HYPRE_GetErrorArg() == 2, name
        lib.HYPRE_ClearAllErrors()
    for call in (lambda: lib.HYPRE_ParCSRHybridSetCycleRelaxType(h, 13, 4), lambda: lib.HYPRE_ParCSRHybridSetCycleNumSweeps(h, 1, 0),
                 lambda: lib.HYPRE_ParCSRHybridSetLevelRelaxWt(h, 1.0, 25), lambda: lib.HYPRE_ParCSRHybridSetLevelOuterWt(h, 1.0, -1)):
        call()
        assert lib.HYPRE_GetError() & 4 and lib.HYPRE_GetErrorArg() == 3
        lib.HYPRE_ClearAllErrors()
    # what the Krylov solvers do not carry is refused with a message, at once
    for name, v, word in (("RelChange", 1, b"relative-change"), ("RecomputeResidual", 1, b"RecomputeResidual"), ("StopCrit", 1, b"StopCrit"),
                          ("SolverType", 4, b"1 PCG, 2 GMRES, 3 BiCGSTAB"), ("SolverType", 0, b"1 PCG")):
        assert getattr(lib, "HYPRE_ParCSRHybridSet" + name)(h, v) != 0
        assert word in lib.hypre_amd_LastErrorMessage(), name
        lib.HYPRE_ClearAllErrors()
    assert lib.HYPRE_ParCSRHybridSetPrecond(h, C.cast(lib.HYPRE_ParCSRDiagScale, C.c_void_p), None, None) != 0
    assert b"HYPRE_ParCSRHybridSetPrecond" in lib.hypre_amd_LastErrorMessage()
    lib.HYPRE_ClearAllErrors()
    # null arguments
    assert lib.HYPRE_ParCSRHybridSolve(h, None, None, None) != 0
    lib.HYPRE_ClearAllErrors()
    assert lib.HYPRE_ParCSRHybridSetTol(None, 0.1) != 0 and lib.HYPRE_GetErrorArg() == 1
    lib.HYPRE_ClearAllErrors()
    assert lib.HYPRE_ParCSRHybridDestroy(h) == 0 and lib.HYPRE_ParCSRHybridDestroy(None) == 0
    assert lib.HYPRE_GetError() == 0


def test_convergence_factor_setters_and_the_fused_switch(lib):
    lib.HYPRE_ClearAllErrors()
    v, conv, used = C.c_double(-1.0), C.c_int(-1), C.c_int(-1)
    g = C.c_void_p()
    lib.HYPRE_ParCSRPCGCreate(0, C.byref(g))
    assert lib.HYPRE_PCGGetConvergenceFactorTol(g, C.byref(v)) == 0 and v.value == 0.0          # pcg.c:100
    assert lib.HYPRE_PCGSetConvergenceFactorTol(g, 0.7) == 0 and lib.HYPRE_PCGGetConvergenceFactorTol(g, C.byref(v)) == 0 and v.value == 0.7
    assert lib.HYPRE_PCGGetConverged(g, C.byref(conv)) == 0 and conv.value == 0
    assert lib.hypre_amd_PCGGetFusedDiagScaleUsed(g, C.byref(used)) == 0 and used.value == 0     # before Setup
    assert lib.hypre_amd_PCGSetFusedDiagScale(g, 0) == 0 and lib.hypre_amd_PCGSetFusedDiagScale(g, 1) == 0
    lib.hypre_amd_PCGSetFusedDiagScale(g, 2)
    assert lib.HYPRE_GetError() & 4 and lib.HYPRE_GetErrorArg() == 2
    lib.HYPRE_ClearAllErrors()
    lib.HYPRE_ParCSRPCGDestroy(g)
    lib.HYPRE_ParCSRGMRESCreate(0, C.byref(g))
    assert lib.HYPRE_GMRESGetConvergenceFactorTol(g, C.byref(v)) == 0 and v.value == 0.0        # gmres.c:85
    assert lib.HYPRE_GMRESSetConvergenceFactorTol(g, 0.6) == 0 and lib.HYPRE_GMRESGetConvergenceFactorTol(g, C.byref(v)) == 0 and v.value == 0.6
    assert lib.HYPRE_GMRESGetConverged(g, C.byref(conv)) == 0 and conv.value == 0
    lib.HYPRE_ParCSRGMRESDestroy(g)
    lib.HYPRE_ParCSRBiCGSTABCreate(0, C.byref(g))
    assert lib.HYPRE_BiCGSTABGetConvergenceFactorTol(g, C.byref(v)) == 0 and v.value == 0.0
    assert lib.HYPRE_BiCGSTABSetConvergenceFactorTol(g, 0.5) == 0 and lib.HYPRE_BiCGSTABGetConvergenceFactorTol(g, C.byref(v)) == 0 and v.value == 0.5
    assert lib.HYPRE_BiCGSTABGetConverged(g, C.byref(conv)) == 0 and conv.value == 0
    lib.HYPRE_ParCSRBiCGSTABDestroy(g)
    # FlexGMRES keeps "0.0 only"
    lib.HYPRE_ParCSRFlexGMRESCreate(0, C.byref(g))
    assert lib.HYPRE_FlexGMRESSetConvergenceFactorTol(g, 0.0) == 0
    assert lib.HYPRE_FlexGMRESSetConvergenceFactorTol(g, 0.5) != 0
    lib.HYPRE_ClearAllErrors()
    lib.HYPRE_ParCSRFlexGMRESDestroy(g)
    assert lib.hypre_amd_DotGridPassElements() == 1024 * 256 * 2
    assert lib.HYPRE_GetError() == 0
