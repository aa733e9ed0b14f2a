"""The host logic of LGMRES (hypre_amd/csrc/lgmres_core.hpp: Hessenberg matrix of k_dim + aug_dim columns, Givens
rotations, the Arnoldi-or-augmentation decision, the order of the augmentation vectors, the term lists of the batched
correction) as a stand-alone program under the address and undefined-behaviour sanitizers:
tests/host/lgmres_host_check.cpp runs it on two dense systems of 60 unknowns with plain arrays behind the vector
callbacks.  A CPU build of host code only; nothing is loaded into python and no GPU is touched."""
from util import assert_recorded_traces, run_host_program


def test_the_lgmres_iteration_runs_clean_under_the_sanitizers(tmp_path):
    out = run_host_program("host/lgmres_host_check.cpp", tmp_path)
    assert "lgmres host check ok: 2 systems" in out
    # the sequence of vector operations and every scalar of it, as recorded before the steps shared with GMRES were cut out
    assert_recorded_traces(out, "lgmres")
