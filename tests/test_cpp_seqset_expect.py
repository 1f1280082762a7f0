"""The arithmetic of the expected site counts of a set (lightmotif_amd/csrc/seqset_expect_plan.hpp: the fixed point, the
weight of a window, the run of a lane over the Walker) and its test program tests/cpp/test_seqset_expect.cpp: compiled
here for the host alone, with the address and undefined-behaviour sanitizers linked into the program, and run directly.
No device is needed."""
import shutil
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CPP = ROOT / "tests" / "cpp"


def test_cpp_seqset_expect_matches_brute_force(tmp_path):
    exe = tmp_path / "test_seqset_expect"
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    subprocess.run([hipcc, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
                    "-Wno-unused-function", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    f"-I{ROOT / 'include'}", f"-I{ROOT / 'lightmotif_amd' / 'csrc'}", str(CPP / "test_seqset_expect.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, text=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-4000:] + r.stdout
    assert "test_seqset_expect: all checks passed" in r.stdout
