"""BiCGSTAB in the driver and in the C ABI, as far as no GPU is needed: the reference's two BiCGSTAB job lines
(test/TEST_ij/vector.jobs:31 and :44, kept in tests/golden/ij_saved_bicgstab.json) parse verbatim through the command line
(`-solver 10`; `-solver 9` is AMG-BiCGSTAB), `-solver 11` (Pilut) stays outside; the setters, getters and the switch of
HYPRE_ParCSRBiCGSTAB* / HYPRE_BiCGSTAB* before any solve; a Solve without Setup is refused."""
import ctypes as C
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = json.load(open(os.path.join(HERE, "golden", "ij_saved_bicgstab.json")))


def test_the_golden_file_holds_the_two_reference_lines():
    """vector.saved:46-48 and :90-92, number for number."""
    assert set(GOLD) == {"vector.out.B3", "vector.out.B103"}
    assert {k: GOLD[k]["np"] for k in GOLD} == {"vector.out.B3": 1, "vector.out.B103": 4}
    assert GOLD["vector.out.B3"]["cmd"] == "-n 8 8 8 -solver 10 -rhsisone -nc 4"
    assert GOLD["vector.out.B103"]["cmd"] == "-n 8 8 8 -solver 10 -rhsisone -nc 6"
    for case in GOLD.values():
        assert case["expect"] == {"iterations": 12, "rel_resid": 6.282586e-09}


@pytest.mark.parametrize("name", sorted(GOLD))
def test_a_bicgstab_job_line_parses_verbatim(name):
    from hypre_amd import ij
    case = GOLD[name]
    opt = ij.parse_cli(case["cmd"].split())
    ref = ij.IJOptions(**{k: (tuple(v) if isinstance(v, list) else v) for k, v in case["options"].items()})
    assert vars(opt) == vars(ref), (name, vars(opt), vars(ref))
    assert opt.solver == 10 and opt.num_components == {"vector.out.B3": 4, "vector.out.B103": 6}[name]


def test_solver_9_and_10_are_served_and_their_neighbours_are_not():
    from hypre_amd import ij
    assert ij.parse_cli(["-solver", "9"]).solver == 9
    assert ij.parse_cli(["-solver", "10", "-difconv", "-a", "10", "10", "10"]).solver == 10
    assert ij.check_options(ij.IJOptions(solver=9)).solver == 9
    for solver in ("8", "11", "12", "45", "73", "20"):
        with pytest.raises(SystemExit) as e:
            ij.parse_cli(["-solver", solver])
        assert "-solver %s is outside the scope of this driver" % solver in str(e.value)
        with pytest.raises(SystemExit):
            ij.check_options(ij.IJOptions(solver=int(solver)))
    # BiCGSTAB is no GMRES: neither LGMRES nor its option rides on it
    for solver in (9, 10):
        with pytest.raises(SystemExit):
            ij.check_options(ij.IJOptions(solver=solver, lgmres=1))
        with pytest.raises(SystemExit):
            ij.check_options(ij.IJOptions(solver=solver, aug_dim=3))


def test_amg_bicgstab_on_several_components_follows_the_rules_of_amg():
    from hypre_amd import ij
    assert ij.parse_cli(["-solver", "9", "-rlx", "18", "-nc", "3"]).num_components == 3
    with pytest.raises(SystemExit) as e:
        ij.parse_cli(["-solver", "9", "-nc", "3"])
    assert "multicomponent" in str(e.value)
    with pytest.raises(SystemExit):
        ij.parse_cli(["-solver", "10", "-nc", "3", "-rhsrand"])


def test_setters_getters_and_the_switch(lib):
    g = C.c_void_p()
    assert lib.HYPRE_ParCSRBiCGSTABCreate(0, C.byref(g)) == 0 and g.value
    for par in ("HYPRE_BiCGSTAB", "HYPRE_ParCSRBiCGSTAB"):
        fn = lambda stem: getattr(lib, par + stem)
        assert fn("SetTol")(g, 1e-9) == 0 and fn("SetAbsoluteTol")(g, 1e-12) == 0
        assert fn("SetStopCrit")(g, 1) == 0 and fn("SetMinIter")(g, 2) == 0 and fn("SetMaxIter")(g, 30) == 0
        assert fn("SetLogging")(g, 1) == 0 and fn("SetPrintLevel")(g, 0) == 0
        marker = C.c_void_p(0x1234)
        assert fn("SetPrecond")(g, C.cast(lib.HYPRE_ParCSRDiagScale, C.c_void_p), C.cast(lib.HYPRE_ParCSRDiagScaleSetup, C.c_void_p), marker) == 0
        got = C.c_void_p()
        assert fn("GetPrecond")(g, C.byref(got)) == 0 and got.value == 0x1234
        its, rel = C.c_int(-1), C.c_double(-1.0)
        assert fn("GetNumIterations")(g, C.byref(its)) == 0 and its.value == 0
        assert fn("GetFinalRelativeResidualNorm")(g, C.byref(rel)) == 0 and rel.value == 0.0
    assert lib.HYPRE_BiCGSTABSetConvergenceFactorTol(g, 0.5) == 0
    conv, count, norms = C.c_int(-1), C.c_int(-1), C.POINTER(C.c_double)()
    assert lib.hypre_amd_BiCGSTABGetConverged(g, C.byref(conv)) == 0 and conv.value == 0
    assert lib.hypre_amd_BiCGSTABGetLoggedNorms(g, C.byref(count), C.byref(norms)) == 0 and count.value == 0
    # the switch takes 0 and 1
    assert lib.hypre_amd_BiCGSTABSetFusedUpdates(g, 0) == 0 and lib.hypre_amd_BiCGSTABSetFusedUpdates(g, 1) == 0
    lib.hypre_amd_BiCGSTABSetFusedUpdates(g, 2)
    assert lib.HYPRE_GetError() & 4 and lib.HYPRE_GetErrorArg() == 2
    lib.HYPRE_ClearAllErrors()
    # Solve before Setup has no work vectors
    assert lib.HYPRE_ParCSRBiCGSTABSolve(g, None, None, None) != 0
    assert b"HYPRE_ParCSRBiCGSTABSetup first" in lib.hypre_amd_LastErrorMessage()
    lib.HYPRE_ClearAllErrors()
    assert lib.HYPRE_BiCGSTABDestroy(g) == 0
    assert lib.HYPRE_ParCSRBiCGSTABDestroy(None) == 0
    assert lib.HYPRE_GetError() == 0
