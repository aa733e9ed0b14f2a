"""The map of the extended+i interpolation kernel, replayed on the host (tests/extpi_map_replay.cpp): the header the kernel
includes, compiled into a stand-alone program with the address and undefined-behaviour sanitizers.  It shows that the
kernel's guard on a row's strong-neighbour count is the bound under which every probe of the map ends, on every rung."""
import shutil

from util import run_host_program


def test_map_probes_end_under_the_guard(tmp_path):
    cxx = next((c for c in ("g++", "clang++", "/opt/rocm/llvm/bin/clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    # the sanitizer's runtime linked into the program itself: it then does not care what else the loader brings along
    static = ["-static-libasan", "-static-libubsan"] if cxx == "g++" else ["-static-libsan"]
    flags = ["-std=c++17"] + static + ["-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    lines = run_host_program("extpi_map_replay.cpp", tmp_path, flags=flags, cxx=cxx, timeout=300).splitlines()
    assert lines[-1] == "extpi map replay ok"
    # 3 * capR - 1 strong neighbours on every rung: 191 on the first (the benchmark hierarchies' rows stay below 134)
    assert [int(l.split()[-1]) for l in lines[:4]] == [191, 383, 767, 3071]
