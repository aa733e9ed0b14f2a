"""FlexGMRES in the driver (hypre_amd/ij.py): solver 60 (DS-FlexGMRES) and 61 (AMG-FlexGMRES) as driver options.  The
reference's four FlexGMRES job lines (test/TEST_ij/solvers.jobs:77-78, vector.jobs:33 and :46) are kept in
tests/golden/ij_saved_flexgmres.json with the options they stand for; the driver takes those options (check_options),
while the command line itself (parse_cli) keeps the two ids outside its scope, as tests/test_cogmres_cli.py pins it.
No GPU is needed."""
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = json.load(open(os.path.join(HERE, "golden", "ij_saved_flexgmres.json")))


def _options(case):
    from hypre_amd import ij
    return ij.IJOptions(**{k: (tuple(v) if isinstance(v, list) else v) for k, v in case["options"].items()})


@pytest.mark.parametrize("name", sorted(GOLD))
def test_the_options_of_a_flexgmres_job_line_are_served(name):
    """The golden options are what the job line says, flag by flag (parsed with a solver the command line takes in place
    of 60 / 61), and the driver accepts them."""
    from hypre_amd import ij
    case = GOLD[name]
    opt = ij.check_options(_options(case))
    assert opt.solver in (60, 61) and opt.k_dim == 5                      # test/ij.c:1731: the driver's 5, not the solver's 20
    stand_in = {60: "4", 61: "3"}[opt.solver]                             # DS-GMRES / AMG-GMRES: the same flags
    argv = case["cmd"].split()
    assert argv[argv.index("-solver") + 1] == str(opt.solver)
    argv[argv.index("-solver") + 1] = stand_in
    parsed = vars(ij.parse_cli(argv))
    parsed["solver"] = opt.solver
    assert parsed == vars(opt), (name, parsed, vars(opt))


def test_the_golden_file_holds_the_four_reference_lines():
    assert set(GOLD) == {"solvers.out.103", "solvers.out.104", "vector.out.B5", "vector.out.B105"}
    assert [GOLD[k]["np"] for k in sorted(GOLD)] == [2, 2, 4, 1]
    assert GOLD["solvers.out.103"]["expect"] == {"iterations": 93, "rel_resid": 8.225661e-09}
    assert GOLD["solvers.out.104"]["expect"] == {"iterations": 7, "rel_resid": 4.842561e-09}
    assert GOLD["vector.out.B5"]["expect"] == {"iterations": 54, "rel_resid": 7.982372e-09}
    assert GOLD["vector.out.B105"]["expect"]["iterations"] == 54


def test_amg_flexgmres_on_several_components_follows_the_rules_of_amg():
    """Solver 61 with N components runs BoomerAMG on a multivector: the smoothers it serves there pass, the default hybrid
    Gauss-Seidel is refused as for solver 3; DS-FlexGMRES takes several components as DS-GMRES does."""
    from hypre_amd import ij
    assert ij.check_options(ij.IJOptions(solver=61, num_components=3, relax_type=18)).num_components == 3
    with pytest.raises(SystemExit) as e:
        ij.check_options(ij.IJOptions(solver=61, num_components=3))
    assert "multicomponent" in str(e.value)
    assert ij.check_options(ij.IJOptions(solver=60, num_components=4)).num_components == 4
    with pytest.raises(SystemExit):
        ij.check_options(ij.IJOptions(solver=60, num_components=4, rhs="rand"))


def test_a_neighbour_outside_the_scope_is_still_refused():
    from hypre_amd import ij
    for solver in ("50", "51", "62", "72"):
        with pytest.raises(SystemExit) as e:
            ij.parse_cli(["-solver", solver])
        assert "-solver %s is outside the scope of this driver" % solver in str(e.value)
        with pytest.raises(SystemExit):
            ij.check_options(ij.IJOptions(solver=int(solver)))
