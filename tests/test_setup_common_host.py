"""CPU: the host-only half of hypre_amd/csrc/setup_common.hpp (row blocks and their stitch, sorted-unique lists and index
maps, compaction of an off-rank column map, the P_ext split and the numbering of received product rows) as a stand-alone
program (tests/host/setup_common_check.cpp) under the address and undefined-behaviour sanitizers.  The program links no
library and touches no device."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_shared_setup_steps_under_sanitizers(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "setup_common_check")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    cmd = [hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-fopenmp", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "hypre_amd", "csrc"), "-Wall", "-Wno-unused-function", "-Wno-option-ignored", "-x", "hip"]
    for f in san:
        cmd += ["-Xarch_host", f]                      # host code only
    cmd += [os.path.join(HERE, "host", "setup_common_check.cpp"), "-o", exe, san[0]]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, OMP_NUM_THREADS="4",
               LSAN_OPTIONS="suppressions=%s:print_suppressions=0" % os.path.join(HERE, "host", "lsan.supp"))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "host checks passed" in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]
