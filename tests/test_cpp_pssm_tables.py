"""The host builder of a scoring matrix's device image (lightmotif_amd/csrc/pssm_tables.hpp) and its test program
tests/cpp/test_pssm_tables.cpp: compiled here for the host alone, with the address and undefined-behaviour sanitizers
linked into the program, and run against tests/golden/pssm_tables_digest.json.  No device is needed."""
import shutil
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CPP = ROOT / "tests" / "cpp"


def test_cpp_pssm_tables_match_the_recorded_digests(tmp_path):
    exe = tmp_path / "test_pssm_tables"
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    subprocess.run([hipcc, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
                    "-Wno-unused-function", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    f"-I{ROOT / 'include'}", f"-I{ROOT / 'lightmotif_amd' / 'csrc'}", str(CPP / "test_pssm_tables.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, text=True)
    r = subprocess.run([str(exe), str(ROOT / "tests" / "golden" / "pssm_tables_digest.json")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-4000:] + r.stdout
    assert "test_pssm_tables: all checks passed (419 matrices)" in r.stdout
