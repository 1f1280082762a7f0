"""The C++ host mirror's symbol counts (StripedSequence::count_symbols, SequenceSet::count_symbols,
background_from_counts) and their test program tests/cpp/test_composition.cpp, compiled here with a command of its own."""
import os
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CPP = ROOT / "tests" / "cpp"


def build(tmp_path):
    exe = tmp_path / "test_composition"
    libdir = ROOT / "lightmotif_amd" / "csrc"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", f"-I{ROOT / 'include'}",
                    f"-I{ROOT / 'lightmotif_amd' / 'host'}", str(CPP / "test_composition.cpp"), "-o", str(exe), f"-L{libdir}",
                    "-llightmotif_hip", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"], check=True, capture_output=True, text=True)
    return exe


def test_cpp_composition_compiles_and_links(tmp_path):
    exe = build(tmp_path)
    out = subprocess.run(["ldd", str(exe)], capture_output=True, text=True).stdout
    assert "liblightmotif_hip.so" in out and "not found" not in out.split("liblightmotif_hip.so")[1].split("\n")[0]


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present")
def test_cpp_composition_without_device_raises_unsupported_backend(tmp_path):
    r = subprocess.run([str(build(tmp_path))], capture_output=True, text=True)
    assert r.returncode == 2 and "UnsupportedBackend" in r.stderr


@pytest.mark.gpu
def test_cpp_composition_matches_a_plain_loop(tmp_path):
    r = subprocess.run([str(build(tmp_path))], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    assert "test_composition: all checks passed" in r.stdout
