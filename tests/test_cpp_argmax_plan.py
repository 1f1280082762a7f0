"""The host arithmetic of the fused argmax (lightmotif_amd/csrc/argmax_plan.hpp: who takes the candidate and the suffix
route, the sample geometry, the layouts of the scratch blocks and of the job table in the pinned block, the delivery form of
the exact route, the f32 -> 16-bit threshold map) and its test program tests/cpp/test_argmax_plan.cpp: compiled here for
the host alone, with the address and undefined-behaviour sanitizers linked into the program, and run directly.  No device
is needed."""
import shutil
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CPP = ROOT / "tests" / "cpp"


def test_cpp_argmax_plan_arithmetic_holds(tmp_path):
    exe = tmp_path / "test_argmax_plan"
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    subprocess.run([hipcc, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
                    "-Wno-unused-function", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    f"-I{ROOT / 'include'}", f"-I{ROOT / 'lightmotif_amd' / 'csrc'}", str(CPP / "test_argmax_plan.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, text=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-4000:] + r.stdout
    assert "test_argmax_plan: all checks passed" in r.stdout
