"""The C++ host mirror's hit counts per record (Pipeline::scan_count over a SequenceSet) and its test program
tests/cpp/test_seqset_count.cpp, compiled here with a command of its own: the planted edge records of
tests/seqset_best_cases.py, checked against the values Python's scan_count_set gives for them."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from seqset_best_cases import consensus_matrix, edge_records

ROOT = Path(__file__).resolve().parent.parent
CPP = ROOT / "tests" / "cpp"


def build(tmp_path):
    exe = tmp_path / "test_seqset_count"
    libdir = ROOT / "lightmotif_amd" / "csrc"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", f"-I{ROOT / 'include'}",
                    f"-I{ROOT / 'lightmotif_amd' / 'host'}", str(CPP / "test_seqset_count.cpp"), "-o", str(exe), f"-L{libdir}",
                    "-llightmotif_hip", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"], check=True, capture_output=True, text=True)
    return exe


def test_cpp_seqset_count_compiles_and_links(tmp_path):
    exe = build(tmp_path)
    out = subprocess.run(["ldd", str(exe)], capture_output=True, text=True).stdout
    assert "liblightmotif_hip.so" in out and "not found" not in out.split("liblightmotif_hip.so")[1].split("\n")[0]


@pytest.mark.gpu
def test_cpp_seqset_count_matches_python(tmp_path, pli):
    import lightmotif_amd as lm
    m = 12
    consensus, records, notes = edge_records(m=m)
    seqset = pli.stripe_ascii_set(records)
    seqset.configure_wrap(m)
    cuts = np.asarray([[2.0 * m, 0.0, -np.inf]], dtype=np.float32)
    res = pli.scan_count_set([lm.ScoringMatrix(consensus_matrix(consensus, 2.0, lm.lib.stride(5, 4)))], cuts, seqset)
    assert res.counts.shape == (1, 3, len(records))
    assert res.counts[0, 0].sum() == len(notes["planted"]) + 1            # one record holds the consensus twice
    assert np.array_equal(res.counts[0, 2], res.windows[0])
    case = tmp_path / "case.txt"
    with open(case, "w") as fh:
        fh.write(f"{consensus}\n{len(records)} 3 " + " ".join(str(int(b)) for b in cuts[0].view(np.uint32)) + "\n")
        for r, text in enumerate(records):
            fh.write(f"{text or '-'} " + " ".join(str(int(c)) for c in res.counts[0, :, r]) + "\n")
    r = subprocess.run([str(build(tmp_path)), str(case)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    assert "test_seqset_count: all checks passed" in r.stdout
