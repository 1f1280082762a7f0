"""The arithmetic of the sum of odds per record (lightmotif_amd/csrc/seqset_sum_plan.hpp: lane runs, who writes a cell,
the reducer and the merge of the partial sums) and its test program tests/cpp/test_seqset_sum.cpp: compiled here for the
host alone, with the address and undefined-behaviour sanitizers linked into the program, and run directly.  No device is
needed."""
import shutil
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CPP = ROOT / "tests" / "cpp"


def test_cpp_seqset_sum_matches_brute_force(tmp_path):
    exe = tmp_path / "test_seqset_sum"
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    subprocess.run([hipcc, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
                    "-Wno-unused-function", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    f"-I{ROOT / 'include'}", f"-I{ROOT / 'lightmotif_amd' / 'csrc'}", str(CPP / "test_seqset_sum.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, text=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-4000:] + r.stdout
    assert "test_seqset_sum: all checks passed" in r.stdout
