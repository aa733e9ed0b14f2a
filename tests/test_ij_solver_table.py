"""The solver table of the driver (hypre_amd/ij.py, SOLVERS): the closing lines it gives every solver, the ids the
command line and check_options serve, and that every served id names something the module has.  The expected lines are
written out as the driver printed them before the table existed, not built from the table."""
import pytest

SERVED = {0, 1, 2, 3, 4, 9, 10, 16, 17, 60, 61, 80, 81, 82}
ON_THE_COMMAND_LINE = {0, 1, 2, 3, 4, 9, 10, 16, 17, 80, 81, 82}

CLOSING = [
    (dict(solver=1), ["", "Iterations = 7", "Final Relative Residual Norm = 1.250000e-09", ""]),
    (dict(solver=2), ["", "Iterations = 7", "Final Relative Residual Norm = 1.250000e-09", ""]),
    (dict(solver=3), ["", "GMRES Iterations = 7", "Final GMRES Relative Residual Norm = 1.250000e-09", ""]),
    (dict(solver=4), ["", "GMRES Iterations = 7", "Final GMRES Relative Residual Norm = 1.250000e-09", ""]),
    (dict(solver=4, lgmres=1), ["", "LGMRES Iterations = 7", "Final LGMRES Relative Residual Norm = 1.250000e-09", ""]),
    (dict(solver=3, lgmres=1), ["", "LGMRES Iterations = 7", "Final LGMRES Relative Residual Norm = 1.250000e-09", ""]),
    (dict(solver=9), ["", "BiCGSTAB Iterations = 7", "Final BiCGSTAB Relative Residual Norm = 1.250000e-09", ""]),
    (dict(solver=10), ["", "BiCGSTAB Iterations = 7", "Final BiCGSTAB Relative Residual Norm = 1.250000e-09", ""]),
    (dict(solver=16), ["", "COGMRES Iterations = 7", "Final COGMRES Relative Residual Norm = 1.250000e-09", ""]),
    (dict(solver=17), ["", "COGMRES Iterations = 7", "Final COGMRES Relative Residual Norm = 1.250000e-09", ""]),
    (dict(solver=60), ["", "FlexGMRES Iterations = 7", "Final FlexGMRES Relative Residual Norm = 1.250000e-09", ""]),
    (dict(solver=61), ["", "FlexGMRES Iterations = 7", "Final FlexGMRES Relative Residual Norm = 1.250000e-09", ""]),
    (dict(solver=80), ["", "hypre_ILU Iterations = 7", "Final Relative Residual Norm = 1.250000e-09", ""]),
    (dict(solver=81), ["", "GMRES Iterations = 7", "Final GMRES Relative Residual Norm = 1.250000e-09", ""]),
    (dict(solver=82), ["", "FlexGMRES Iterations = 7", "Final FlexGMRES Relative Residual Norm = 1.250000e-09", ""]),
]


@pytest.mark.parametrize("options, lines", CLOSING, ids=["-".join("%s%d" % kv for kv in o.items()) for o, _ in CLOSING])
def test_closing_lines(options, lines):
    from hypre_amd import ij
    assert ij.closing_lines(ij.IJOptions(**options), 7, 1.25e-9) == lines


def test_the_ids_check_options_and_the_command_line_serve():
    from hypre_amd import ij
    for solver in range(100):
        for serve, served, args in ((ij.check_options, SERVED, ij.IJOptions(solver=solver)),
                                    (ij.parse_cli, ON_THE_COMMAND_LINE, ["-solver", str(solver)])):
            if solver in served:
                assert serve(args).solver == solver
            else:
                with pytest.raises(SystemExit):         # a KeyError would say that the table was read before the id was checked
                    serve(args)


def test_every_served_id_names_a_solver_and_a_preconditioner_the_module_has():
    from hypre_amd import ij
    assert set(ij.SOLVERS) == SERVED
    assert {s for s, spec in ij.SOLVERS.items() if spec.cli} == ON_THE_COMMAND_LINE
    for solver, spec in ij.SOLVERS.items():
        assert spec.precond in ("amg", "ds", "ilu"), solver
        if spec.precond != "ds":
            assert callable(getattr(ij, "create_" + spec.precond)), solver
        if spec.method is None:
            assert spec.precond == "amg" and callable(ij.solve_amg), solver
        elif spec.method == "ILU":
            assert spec.precond == "ilu" and callable(ij.run_ilu), solver
        else:
            assert callable(getattr(ij, "solve_" + spec.method.lower())), solver
            assert ij.krylov_solver(ij.IJOptions(solver=solver)) is getattr(ij, "solve_" + spec.method.lower())
    for solver in (3, 4):
        assert ij.krylov_solver(ij.IJOptions(solver=solver, lgmres=1)) is ij.solve_lgmres
