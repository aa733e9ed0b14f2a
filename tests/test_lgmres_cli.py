"""LGMRES in the driver (hypre_amd/ij.py): the option lgmres = 1 turns solver 4 into DS-LGMRES (the reference's
`ij -solver 50`) and solver 3 into AMG-LGMRES (51).  The reference's four LGMRES job lines (test/TEST_ij/solvers.jobs:75-76,
vector.jobs:32 and :45) are kept in tests/golden/ij_saved_lgmres.json with the options they stand for; the command line
(parse_cli) and check_options keep the ids 50 and 51 themselves outside their scope, as tests/test_flexgmres_cli.py pins
it.  The clamp of HYPRE_LGMRESSetAugDim is read back through the library.  No GPU is needed."""
import ctypes as C
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = json.load(open(os.path.join(HERE, "golden", "ij_saved_lgmres.json")))


def _options(case):
    from hypre_amd import ij
    return ij.IJOptions(**{k: (tuple(v) if isinstance(v, list) else v) for k, v in case["options"].items()})


def test_the_golden_file_holds_the_four_reference_lines():
    """solvers.saved:176-182 and vector.saved:50-52, :94-96, number for number."""
    assert set(GOLD) == {"solvers.out.101", "solvers.out.102", "vector.out.B4", "vector.out.B104"}
    assert {k: GOLD[k]["np"] for k in GOLD} == {"solvers.out.101": 2, "solvers.out.102": 2, "vector.out.B4": 1, "vector.out.B104": 4}
    assert GOLD["solvers.out.101"]["expect"] == {"iterations": 83, "rel_resid": 8.591967e-09}
    assert GOLD["solvers.out.102"]["expect"] == {"iterations": 7, "rel_resid": 4.842561e-09}
    assert GOLD["vector.out.B4"]["expect"] == {"iterations": 53, "rel_resid": 8.975949e-09}
    assert GOLD["vector.out.B104"]["expect"] == {"iterations": 53, "rel_resid": 8.975947e-09}
    assert GOLD["solvers.out.101"]["cmd"] == "-solver 50 -rhsrand" and GOLD["solvers.out.102"]["cmd"] == "-solver 51 -rhsrand"
    assert GOLD["vector.out.B4"]["cmd"] == "-n 8 8 8 -solver 50 -rhsisone -nc 4"
    assert GOLD["vector.out.B104"]["cmd"] == "-n 8 8 8 -solver 50 -rhsisone -nc 6"


@pytest.mark.parametrize("name", sorted(GOLD))
def test_the_options_of_an_lgmres_job_line_are_served(name):
    """The golden options are what the job line says, flag by flag (parsed with the solver that lgmres = 1 rides on in
    place of 50 / 51), and the driver accepts them."""
    from hypre_amd import ij
    case = GOLD[name]
    opt = ij.check_options(_options(case))
    assert opt.lgmres == 1 and opt.k_dim == 5 and opt.aug_dim == 2            # test/ij.c:1731, :1736: the driver's 5, not the solver's 20
    argv = case["cmd"].split()
    reference_id = argv[argv.index("-solver") + 1]
    assert {"50": 4, "51": 3}[reference_id] == opt.solver                     # DS-LGMRES on DS-GMRES's id, AMG-LGMRES on AMG-GMRES's
    argv[argv.index("-solver") + 1] = str(opt.solver)
    parsed = vars(ij.parse_cli(argv))
    assert parsed["lgmres"] == 0
    parsed["lgmres"] = 1
    assert parsed == vars(opt), (name, parsed, vars(opt))


def test_lgmres_rides_on_solvers_3_and_4_only():
    from hypre_amd import ij
    for solver in (3, 4):
        assert ij.check_options(ij.IJOptions(solver=solver, lgmres=1)).lgmres == 1
        assert ij.check_options(ij.IJOptions(solver=solver, lgmres=1, aug_dim=1)).aug_dim == 1
    for solver in (0, 1, 2, 16, 17, 60, 61):
        with pytest.raises(SystemExit) as e:
            ij.check_options(ij.IJOptions(solver=solver, lgmres=1))
        assert "LGMRES" in str(e.value)
    with pytest.raises(SystemExit):
        ij.check_options(ij.IJOptions(solver=4, lgmres=2))
    # the ids of the reference stay outside, with or without the option
    for solver in (50, 51):
        with pytest.raises(SystemExit):
            ij.check_options(ij.IJOptions(solver=solver, lgmres=1))
    # aug_dim is read by LGMRES alone: set for another solver it is refused, never dropped
    for solver in (0, 3, 4, 60):
        with pytest.raises(SystemExit) as e:
            ij.check_options(ij.IJOptions(solver=solver, aug_dim=3))
        assert "aug_dim" in str(e.value)
    # there is no -aug flag: the command line does not reach LGMRES
    with pytest.raises(SystemExit) as e:
        ij.parse_cli(["-solver", "4", "-aug", "3"])
    assert "-aug is outside the scope of this driver" in str(e.value)


def test_amg_lgmres_on_several_components_follows_the_rules_of_amg():
    from hypre_amd import ij
    assert ij.check_options(ij.IJOptions(solver=3, lgmres=1, num_components=3, relax_type=18)).num_components == 3
    with pytest.raises(SystemExit) as e:
        ij.check_options(ij.IJOptions(solver=3, lgmres=1, num_components=3))
    assert "multicomponent" in str(e.value)
    assert ij.check_options(ij.IJOptions(solver=4, lgmres=1, num_components=4)).num_components == 4


def test_set_aug_dim_clamps_against_the_k_dim_in_force(lib):
    """lgmres.c:970-986: below 0 becomes 0, above k_dim - 1 becomes k_dim - 1, with the k_dim set so far (20 after Create);
    a later SetKDim does not clamp again."""
    g = C.c_void_p()
    lib.HYPRE_ParCSRLGMRESCreate(0, C.byref(g))
    got = C.c_int(-7)

    def aug():
        lib.HYPRE_LGMRESGetAugDim(g, C.byref(got))
        return got.value

    assert aug() == 2                                   # hypre_LGMRESCreate
    for asked, k_dim, want in ((25, None, 19), (20, None, 19), (19, None, 19), (-3, None, 0), (0, None, 0),
                               (5, 5, 4), (4, 5, 4), (7, 1, 0), (1, 2, 1), (2, 2, 1)):
        if k_dim is not None:
            assert lib.HYPRE_LGMRESSetKDim(g, k_dim) == 0
        assert lib.HYPRE_ParCSRLGMRESSetAugDim(g, asked) == 0
        assert aug() == want, (asked, k_dim, want, aug())
    lib.HYPRE_LGMRESSetKDim(g, 30)
    lib.HYPRE_LGMRESSetAugDim(g, 12)
    lib.HYPRE_LGMRESSetKDim(g, 5)
    assert aug() == 12                                  # the reference does not look back either
    # ... but a cycle of 5 steps cannot end in 12 augmentation steps: Solve says so before it touches anything
    assert lib.HYPRE_ParCSRLGMRESSolve(g, None, None, None) != 0
    assert b"HYPRE_LGMRESSetAugDim after HYPRE_LGMRESSetKDim" in lib.hypre_amd_LastErrorMessage()
    lib.HYPRE_ClearAllErrors()
    p = C.c_void_p(1)
    lib.HYPRE_LGMRESGetPrecond(g, C.byref(p))
    assert p.value is None
    lib.HYPRE_ParCSRLGMRESDestroy(g)
    assert lib.HYPRE_GetError() == 0
