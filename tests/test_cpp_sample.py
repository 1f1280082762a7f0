"""The C++ host mirror's SequenceSet::sample / count_pairs and its test program tests/cpp/test_sample.cpp, compiled here with a
command of its own; and tests/cpp/test_sample_plan.cpp, the host half of csrc/sample.hip (the generator, thresholds, row
validity, the offsets prefix, every refusal, the packed maps) as a program that needs neither the library nor a device --
built plainly and with the address and undefined-behaviour sanitizers."""
import os
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CPP = ROOT / "tests" / "cpp"


def build(tmp_path):
    exe = tmp_path / "test_sample"
    libdir = ROOT / "lightmotif_amd" / "csrc"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", f"-I{ROOT / 'include'}",
                    f"-I{ROOT / 'lightmotif_amd' / 'host'}", f"-I{libdir}", str(CPP / "test_sample.cpp"), "-o", str(exe), f"-L{libdir}",
                    "-llightmotif_hip", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"], check=True, capture_output=True, text=True)
    return exe


def test_cpp_sample_compiles_and_links(tmp_path):
    exe = build(tmp_path)
    out = subprocess.run(["ldd", str(exe)], capture_output=True, text=True).stdout
    assert "liblightmotif_hip.so" in out and "not found" not in out.split("liblightmotif_hip.so")[1].split("\n")[0]


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present")
def test_cpp_sample_without_device_raises_unsupported_backend(tmp_path):
    r = subprocess.run([str(build(tmp_path))], capture_output=True, text=True)
    assert r.returncode == 2 and "UnsupportedBackend" in r.stderr


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_the_host_half_of_the_unit_alone(tmp_path, sanitize):
    """Plain C++: no HIP header, no library, no device.  The sanitized build is a stand-alone program as well."""
    exe = tmp_path / "test_sample_plan"
    if sanitize:    # as tests/test_cpp_regions.py: the host compiler of hipcc, the sanitizers linked into the program
        compiler = [shutil.which("hipcc") or "/opt/rocm/bin/hipcc", "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-Wall",
                    "-Werror", "-Wno-unused-function", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                    "-fno-sanitize-recover=undefined"]
    else:
        compiler = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror"]
    subprocess.run([*compiler, f"-I{ROOT / 'include'}", f"-I{ROOT / 'lightmotif_amd' / 'csrc'}", str(CPP / "test_sample_plan.cpp"),
                    "-o", str(exe)], check=True, capture_output=True, text=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:] + r.stdout
    assert "test_sample_plan: all checks passed" in r.stdout


@pytest.mark.gpu
def test_cpp_sample_matches_the_rule(tmp_path):
    r = subprocess.run([str(build(tmp_path))], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    assert "test_sample: all checks passed" in r.stdout
