"""CPU checks of the hit counts per record (lm_hip_scan_count_seqset): the header, the binding and the built library agree
on the entry point and its limit, misuse is a status before any device work, and the counting rule the GPU tests rely on
(tests/seqset_count_cases.py) equals a brute-force loop."""
import ctypes as C
import math
import re
import subprocess
from pathlib import Path

import numpy as np

from lightmotif_amd import _ffi
from seqset_count_cases import count_of

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "lightmotif_hip.h").read_text()
NAME = "lm_hip_scan_count_seqset"


def test_header_binding_and_library_agree():
    body = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    decl = re.search(r"int\s+" + NAME + r"\s*\(([^)]*)\)\s*;", body)
    assert decl, "the header does not declare " + NAME
    params = [re.sub(r"\s+", " ", p.strip()) for p in decl.group(1).split(",")]
    assert params == ["lm_hip_ctx *ctx", "const lm_hip_pssm *const *pssms", "const float *thresholds", "size_t levels", "size_t n",
                      "const lm_hip_seqset *set", "uint32_t *counts"]
    res, args = _ffi.SIGNATURES[NAME]
    assert res is C.c_int and len(args) == len(params)
    assert args[3] is C.c_size_t and args[4] is C.c_size_t and args[6] is C.POINTER(C.c_uint32)
    assert hasattr(_ffi.lib(), NAME)
    out = subprocess.run(["nm", "-D", "--defined-only", str(_ffi.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    assert re.search(r" T " + NAME + r"\b", out)


def test_the_limit_is_four_levels_in_both_places():
    assert re.search(r"^#define\s+LM_HIP_MAX_COUNT_LEVELS\s+4\s*$", HEADER, flags=re.M)
    assert _ffi.MAX_COUNT_LEVELS == 4


def test_the_block_cites_the_reference():
    block = HEADER[:HEADER.index("int " + NAME)]
    block = block[block.rindex("/*"):]
    for cite in ("scan.rs:185-190", "pli/mod.rs:96-105", "main.rs:502-561"):
        assert cite in block, cite


def test_null_arguments_are_a_status_with_a_message():
    L = _ffi.lib()
    assert L.lm_hip_scan_count_seqset(None, None, None, 0, 0, None, None) == _ffi.ERR_BAD_ARGS
    assert "scan_count_seqset" in _ffi.last_error()
    ts = (C.c_float * 1)(0.0)
    out = (C.c_uint32 * 1)()
    assert L.lm_hip_scan_count_seqset(None, None, ts, 1, 1, None, out) == _ffi.ERR_BAD_ARGS and _ffi.last_error()


def test_cli_counts_needs_a_threshold_and_excludes_the_list_modes(tmp_path):
    """Refused by the argument parser, before a device is asked for."""
    import pytest
    from lightmotif_amd import scan_cli
    (tmp_path / "m.pwm").write_text(">MA0002.1\tSECOND\nA  [ 20  0  0  5  9 ]\nC  [  0 20  0  5  1 ]\nG  [  0  0 20  5  1 ]\nT  [  0  0  0  5  9 ]\n")
    base = ["-m", str(tmp_path / "m.pwm"), "-s", str(tmp_path / "s.fa"), "-o", str(tmp_path / "o.tsv"), "--counts"]
    for extra in ([], ["-P", "1e-3", "--best"], ["-P", "1e-3", "--matched"], ["--abs-threshold", "3", "--site-matrices", str(tmp_path / "x")]):
        with pytest.raises(SystemExit) as err:
            scan_cli.main(base + extra)
        assert err.value.code == 2, extra


def brute(scores, t):
    n = 0
    for v in scores:
        v, c = float(v), float(np.float32(t))
        if math.isnan(v) or math.isnan(c):
            continue
        if v >= c:
            n += 1
    return n


def test_count_of_equals_a_brute_force_loop():
    scores = np.asarray([1.5, -2.0, np.nan, -np.inf, 0.0, 1.5, 3.25, np.inf, -0.0], dtype=np.float32)
    cuts = [-np.inf, np.nan, np.inf, 1.5, 0.0, -2.0, 3.25, 1.5000001, -3.0e38]
    for t in cuts:
        assert count_of(scores, t) == brute(scores, t), t
    assert count_of(scores, -np.inf) == len(scores) - 1           # everything but the NaN window
    assert count_of(scores, np.nan) == 0
    assert count_of(scores, np.inf) == 1                          # the +inf window alone
    assert count_of(scores[:7], np.inf) == 0
    assert count_of(scores, 1.5) == 4                             # t equal to a score: that score counts
    assert count_of(np.asarray([-np.inf, -np.inf, np.nan], np.float32), -np.inf) == 2
    assert count_of(np.asarray([-np.inf, -np.inf], np.float32), -3.4e38) == 0
    assert count_of(np.zeros(0, np.float32), -np.inf) == 0
    rng = np.random.default_rng(4)
    many = rng.normal(0, 3, 500).astype(np.float32)
    many[rng.random(500) < 0.05] = np.nan
    many[rng.random(500) < 0.05] = -np.inf
    for t in list(many[:40]) + [-np.inf, np.nan, np.inf]:
        assert count_of(many, t) == brute(many, t)
