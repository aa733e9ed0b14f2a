"""COGMRES on the `ij`-compatible command line (hypre_amd/ij.py): `-solver 16 | 17`, `-cgs`, `-unroll`.  The reference's
five COGMRES job lines (test/TEST_ij/solvers.jobs:45-49) and the single-rank lines recorded from its driver, kept in
tests/golden/ij_saved_cogmres.json, parse into the options the golden file states."""
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = json.load(open(os.path.join(HERE, "golden", "ij_saved_cogmres.json")))


@pytest.mark.parametrize("name", sorted(GOLD))
def test_cogmres_job_line_parses_to_the_golden_options(name):
    from hypre_amd import ij
    case = GOLD[name]
    opt = ij.parse_cli(case["cmd"].split())
    ref = ij.IJOptions(**{k: (tuple(v) if isinstance(v, list) else v) for k, v in case["options"].items()})
    assert vars(opt) == vars(ref), (name, vars(opt), vars(ref))
    assert opt.solver in (16, 17)


def test_the_golden_file_holds_the_reference_lines_and_reaches_past_them():
    assert {"solvers.out.%d" % i for i in range(12, 17)} <= set(GOLD)
    assert all(GOLD["solvers.out.%d" % i]["np"] == 2 for i in range(12, 17))
    single = [c["options"] for c in GOLD.values() if c["np"] == 1]
    assert any(o.get("k_dim", 5) > 8 and o.get("cgs", 1) == 1 for o in single)        # chunked MassInnerProd / MassAxpy
    assert any(o.get("k_dim", 5) > 8 and o.get("cgs", 1) == 2 for o in single)        # chunked MassDotpTwo
    assert any(o["solver"] == 16 and o.get("cgs", 1) == 2 for o in single)            # cgs 2 behind AMG
    assert any(o.get("problem") == "27pt" for o in single)


def test_defaults_are_the_reference_drivers():
    from hypre_amd import ij
    opt = ij.parse_cli(["-solver", "17"])
    assert (opt.k_dim, opt.cgs, opt.unroll) == (5, 1, 0)                              # test/ij.c:1731-1733


def test_cogmres_refuses_several_components():
    from hypre_amd import ij
    for solver in ("16", "17"):
        with pytest.raises(SystemExit) as e:
            ij.parse_cli(["-solver", solver, "-nc", "3", "-rhsisone"])
        assert "COGMRES" in str(e.value)


def test_solvers_outside_the_scope_are_still_refused():
    from hypre_amd import ij
    for solver in ("5", "6", "15", "18", "50", "51", "60", "61"):
        with pytest.raises(SystemExit):
            ij.parse_cli(["-solver", solver])
    for bad in (["-solver", "17", "-cgs"], ["-solver", "17", "-unroll"]):
        with pytest.raises(SystemExit):
            ij.parse_cli(bad)
