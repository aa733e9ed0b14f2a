"""The host logic of GMRES, COGMRES and FlexGMRES (hypre_amd/csrc/gmres_core.hpp: Hessenberg matrix, Givens rotations,
restarts, the coefficient lists of the batched operations) as a stand-alone program under the address and
undefined-behaviour sanitizers: tests/host/gmres_host_check.cpp runs it on a dense system of 50 unknowns with plain
arrays behind the vector callbacks.  A CPU build of host code only; nothing is loaded into python and no GPU is touched."""
from util import assert_recorded_traces, run_host_program


def test_the_iteration_runs_clean_under_the_sanitizers(tmp_path):
    out = run_host_program("host/gmres_host_check.cpp", tmp_path)
    assert "flexgmres host check ok" in out
    assert "gmres host check ok: 5 configurations" in out
    # the sequence of vector operations and every scalar of it, as recorded before the steps shared with LGMRES were cut out
    assert_recorded_traces(out, "gmres")
