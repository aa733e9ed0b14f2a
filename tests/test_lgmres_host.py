"""The host logic of LGMRES (hypre_amd/csrc/lgmres_core.hpp: Hessenberg matrix of k_dim + aug_dim columns, Givens
rotations, the Arnoldi-or-augmentation decision, the order of the augmentation vectors, the term lists of the batched
correction) as a stand-alone program under the address and undefined-behaviour sanitizers:
tests/host/lgmres_host_check.cpp runs it on two dense systems of 60 unknowns with plain arrays behind the vector
callbacks.  A CPU build of host code only; nothing is loaded into python and no GPU is touched."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_lgmres_iteration_runs_clean_under_the_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "lgmres_host_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "hypre_amd", "csrc"),
                            os.path.join(ROOT, "tests", "host", "lgmres_host_check.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-3000:]
    assert "lgmres host check ok: 2 systems" in run.stdout
