"""CPU checks of the total odds per record (lm_hip_scan_sum_seqset): the header, the binding and the built library agree on
the entry point, misuse is a status before any device work, the summing rule the GPU tests rely on
(tests/seqset_sum_cases.py) gives the hand-worked values, ``SetSums`` derives what it promises and the CLI refuses the
modes ``--sum-odds`` excludes."""
import ctypes as C
import math
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import lightmotif_amd as lm
from lightmotif_amd import _ffi, scan_cli
from seqset_sum_cases import TOLERANCE, close, consensus_matrix, sum_of, sums_of, window_scores

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "lightmotif_hip.h").read_text()
NAME = "lm_hip_scan_sum_seqset"


def test_header_binding_and_library_agree():
    body = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    decl = re.search(r"int\s+" + NAME + r"\s*\(([^)]*)\)\s*;", body)
    assert decl, "the header does not declare " + NAME
    params = [re.sub(r"\s+", " ", p.strip()) for p in decl.group(1).split(",")]
    assert params == ["lm_hip_ctx *ctx", "const lm_hip_pssm *const *pssms", "const float *scales", "size_t n", "const lm_hip_seqset *set",
                      "double *sums"]
    res, args = _ffi.SIGNATURES[NAME]
    assert res is C.c_int and len(args) == len(params)
    assert args[2] is C.POINTER(C.c_float) and args[3] is C.c_size_t and args[5] is C.POINTER(C.c_double)
    assert hasattr(_ffi.lib(), NAME)
    out = subprocess.run(["nm", "-D", "--defined-only", str(_ffi.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    assert re.search(r" T " + NAME + r"\b", out)
    assert _ffi.lib().lm_hip_abi_version() == 1                    # an additive export


def test_the_block_states_the_rule_and_cites_the_reference():
    block = HEADER[:HEADER.index("int " + NAME)]
    block = block[block.rindex("/*"):]
    for cite in ("scan.rs:185-190", "pli/mod.rs:96-105", "rows_per_stream", "NaN", "+inf"):
        assert cite in block, cite


def test_null_arguments_are_a_status_with_a_message():
    L = _ffi.lib()
    assert L.lm_hip_scan_sum_seqset(None, None, None, 0, None, None) == _ffi.ERR_BAD_ARGS
    assert "scan_sum_seqset" in _ffi.last_error()
    out = (C.c_double * 1)()
    assert L.lm_hip_scan_sum_seqset(None, None, None, 1, None, out) == _ffi.ERR_BAD_ARGS and _ffi.last_error()


def test_the_rule_on_hand_worked_records():
    f = np.float32
    assert sum_of(np.asarray([0.0, 1.0, -1.0, 3.0], f)) == 1.0 + 2.0 + 0.5 + 8.0
    assert sum_of(np.asarray([2.0, np.nan, 2.0], f)) == 8.0                      # a NaN window adds nothing
    assert sum_of(np.asarray([-np.inf, 1.0], f)) == 2.0                          # an -inf window adds 0
    assert sum_of(np.asarray([-np.inf, -np.inf], f)) == 0.0
    assert sum_of(np.asarray([np.nan, np.nan], f)) == 0.0
    assert sum_of(np.asarray([1.0, np.inf], f)) == math.inf
    assert sum_of(np.zeros(0, f)) == 0.0                                         # no window
    assert sum_of(np.asarray([4.0, -6.0], f), 0.5) == 4.0 + 0.125                # the scale multiplies the score
    assert sum_of(np.asarray([1.0], f), math.log2(10.0)) == 2.0 ** float(f(math.log2(10.0)))   # ... in f32: one multiply
    assert sum_of(np.asarray([10.0], f), 100.0) == 2.0 ** 1000 and sum_of(np.asarray([-10.0], f), 100.0) == 2.0 ** -1000
    # a consensus of 3 over ACGTA: windows ACG (+6), CGT (-2 + -2 + -2), GTA
    p = consensus_matrix("ACG", 2.0)
    sym = np.asarray([0, 1, 3, 2, 0])                                            # A C G T A in the order ACTGN
    v = window_scores(p, sym)
    assert v.tolist() == [6.0, -6.0, -6.0]
    assert sum_of(v) == 64.0 + 2 * 2.0 ** -6
    table = sums_of([p, consensus_matrix("ACGTAC", 2.0)], [sym, sym[:2], sym[:0]], [1.0, 1.0])
    assert table.tolist() == [[64.0 + 2 * 2.0 ** -6, 0.0, 0.0], [0.0, 0.0, 0.0]]  # records shorter than the motif: 0.0
    assert sums_of([p], [sym], [0.5])[0, 0] == 8.0 + 2 * 2.0 ** -3
    assert close([1.0 + TOLERANCE / 2, 0.0, math.inf], [1.0, 0.0, math.inf])
    assert not close([1.0 + 3 * TOLERANCE], [1.0]) and not close([1e-300], [0.0]) and not close([1e300], [math.inf])


def test_set_sums_helpers():
    sums = np.asarray([[8.0, 0.0, 0.0], [3.0, math.inf, 1.0]])
    windows = np.asarray([[4, 2, 0], [3, 1, 1]], dtype=np.int64)
    res = lm.SetSums(sums, windows, "seqset_sum_fused<4>")
    assert res.shape == (2, 3) and len(res) == 2 and res.last_kernel == "seqset_sum_fused<4>"
    mean = res.mean()
    assert mean.dtype == np.float64 and mean[0, 0] == 2.0 and mean[0, 1] == 0.0 and math.isnan(mean[0, 2])
    assert mean[1, 0] == 1.0 and mean[1, 1] == math.inf and mean[1, 2] == 1.0
    log2 = res.log2()
    assert log2[0, 0] == 3.0 and log2[0, 1] == -math.inf and log2[1, 1] == math.inf and log2[1, 2] == 0.0
    assert scan_cli.log2_mean_odds(8.0, 4) == 1.0 and scan_cli.log2_mean_odds(0.0, 3) == -math.inf
    assert scan_cli.log2_mean_odds(math.inf, 3) == math.inf


def test_cli_sum_odds_excludes_the_other_modes(tmp_path):
    """Refused by the argument parser, before a device is asked for."""
    (tmp_path / "m.pwm").write_text(">MA0002.1\tSECOND\nA  [ 20  0  0  5  9 ]\nC  [  0 20  0  5  1 ]\nG  [  0  0 20  5  1 ]\nT  [  0  0  0  5  9 ]\n")
    (tmp_path / "v.tsv").write_text("rec0\t1\tA\tC\n")
    base = ["-m", str(tmp_path / "m.pwm"), "-s", str(tmp_path / "s.fa"), "-o", str(tmp_path / "o.tsv"), "--sum-odds"]
    for extra in (["--best"], ["-P", "1e-3", "--counts"], ["--variants", str(tmp_path / "v.tsv")], ["--matched"],
                  ["--site-matrices", str(tmp_path / "x")]):
        with pytest.raises(SystemExit) as err:
            scan_cli.main(base + extra)
        assert err.value.code == 2, extra
    args = scan_cli.build_parser().parse_args(base)                # no threshold is asked for
    assert args.sum_odds and args.pvalue is None and args.abs_threshold is None and args.rel_threshold is None
