"""The C++ host mirror's variant_effects / variant_hits (SequenceSet) and its test program tests/cpp/test_variants.cpp,
compiled here with a command of its own; and tests/cpp/test_variants_plan.cpp, the host half of csrc/variants.hip (argument
checks, validity and clipping rules, chunk / batch / group plans) as a program that needs neither the library nor a device."""
import os
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CPP = ROOT / "tests" / "cpp"


def build(tmp_path):
    exe = tmp_path / "test_variants"
    libdir = ROOT / "lightmotif_amd" / "csrc"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", f"-I{ROOT / 'include'}",
                    f"-I{ROOT / 'lightmotif_amd' / 'host'}", str(CPP / "test_variants.cpp"), "-o", str(exe), f"-L{libdir}",
                    "-llightmotif_hip", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"], check=True, capture_output=True, text=True)
    return exe


def test_cpp_variants_compiles_and_links(tmp_path):
    exe = build(tmp_path)
    out = subprocess.run(["ldd", str(exe)], capture_output=True, text=True).stdout
    assert "liblightmotif_hip.so" in out and "not found" not in out.split("liblightmotif_hip.so")[1].split("\n")[0]


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present")
def test_cpp_variants_without_device_raises_unsupported_backend(tmp_path):
    r = subprocess.run([str(build(tmp_path))], capture_output=True, text=True)
    assert r.returncode == 2 and "UnsupportedBackend" in r.stderr


def test_the_host_half_of_the_unit_alone(tmp_path):
    """Plain C++: no HIP header, no library, no device."""
    exe = tmp_path / "test_variants_plan"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", f"-I{ROOT / 'include'}",
                    f"-I{ROOT / 'lightmotif_amd' / 'csrc'}", str(CPP / "test_variants_plan.cpp"), "-o", str(exe)], check=True,
                   capture_output=True, text=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    assert "test_variants_plan: all checks passed" in r.stdout


@pytest.mark.gpu
def test_cpp_variants_match_windows_scored_on_the_host(tmp_path):
    r = subprocess.run([str(build(tmp_path))], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    assert "test_variants: all checks passed" in r.stdout
