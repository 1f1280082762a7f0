"""CPU checks of the expected site counts of a set (lm_hip_seqset_expected_counts) and of the EM around them: the header,
the binding and the built library agree on the entry point, the rule of tests/expect_rule.py keeps its own invariants
(equal row totals, gain 0, the clamp at 1, F from N), ``posterior_gains`` gives hand-worked OOPS and ZOOPS values, the
float-count M-step equals ``CountMatrix.to_scoring`` bit for bit on integer-valued counts, and the planted set of the GPU
test is strong enough for the rule itself to pass that test's two conditions."""
import ctypes as C
import math
from pathlib import Path

import numpy as np
import pytest

import lightmotif_amd as lm
from lightmotif_amd import _ffi, scan_cli
from seqset_best_cases import DNA_SYMBOLS, encode
from expect_rule import (consensus_matrix, expected_counts, expected_quanta, flattened_start, frac_bits_of, planted_case, quanta_of,
                         rule_em, window_scores)

ROOT = Path(__file__).resolve().parent.parent
NAME = "lm_hip_seqset_expected_counts"


def test_the_entry_point_is_declared_bound_and_exported():
    header = (ROOT / "include" / "lightmotif_hip.h").read_text()
    assert f"int {NAME}(lm_hip_ctx *ctx, const lm_hip_pssm *const *pssms, const float *scales," in header
    for cite in ("sampler.rs:528-538", "pwm/mod.rs:209-237", "scan.rs:185-190"):
        assert cite in header[header.index("The expected site counts"):header.index(f"int {NAME}")]
    restype, argtypes = _ffi.SIGNATURES[NAME]
    assert restype is C.c_int and len(argtypes) == 8
    L = _ffi.lib()
    assert L.lm_hip_seqset_expected_counts(None, None, None, None, 0, None, None, None) == _ffi.ERR_BAD_ARGS
    assert "seqset_expected_counts" in _ffi.last_error()


def test_frac_bits_follow_the_positions_of_the_set():
    assert frac_bits_of(0) == 40 and frac_bits_of(1) == 40 and frac_bits_of(2 ** 22 - 1) == 40
    assert frac_bits_of(2 ** 22) == 39 and frac_bits_of(2 ** 32) == 29 and frac_bits_of(2 ** 40) == 21
    for n in (1, 5, 2 ** 22 - 1, 2 ** 22, 2 ** 31 + 7, 2 ** 45):
        assert n * 2 ** frac_bits_of(n) < 2 ** 62                          # N windows of weight 1 fit a cell


def test_the_weight_of_a_window():
    f = 40
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    assert quanta_of([nan], 1.0, 1.0, f) == [0]                            # a NaN score contributes nothing
    assert quanta_of([inf], 1.0, 0.0, f) == [0]                            # +inf * 0 is NaN: nothing
    assert quanta_of([inf], 1.0, 2.0 ** -9, f) == [2 ** 40]                 # +inf clamps to 1
    assert quanta_of([-inf], 1.0, 1e300, f) == [0]
    assert quanta_of([3.0], 1.0, 1.0, f) == [2 ** 40]                      # the clamp at 1
    assert quanta_of([-3.0], 1.0, 0.5, f) == [2 ** 36]
    assert quanta_of([-41.0, -40.0], 1.0, 1.0, f) == [0, 1]                # half a quantum goes to even
    assert quanta_of([-40.0, -40.0], 1.0, 1.5, f) == [2, 2] and quanta_of([-40.0], 1.0, 2.5, f) == [2]
    assert quanta_of([-2.0], 2.0, 8.0, f) == [2 ** 39]                     # the scale multiplies the score
    assert quanta_of([5.0], 1.0, 0.0, f) == [0]                            # gain 0 switches the record off


def test_rule_invariants():
    rng = np.random.default_rng(5)
    records = [rng.integers(0, 5, n) for n in (0, 40, 3, 7, 120, 0, 64)]
    w = np.zeros((7, 8), np.float32)
    w[:, :5] = rng.normal(0, 2, (7, 5))
    gains = [0.3, 0.01, 5.0, 0.0, 2.0 ** -6, 1.0, 1e6]
    (res,), f = expected_counts([w], records, [gains])
    e, q, windows = res
    assert f == 40 and windows == 34 + 1 + 114 + 58
    totals = [sum(int(c) for c in row) for row in q]
    assert len(set(totals)) == 1 and totals[0] > 0                          # every row has the same total
    assert np.array_equal(e, np.asarray([[int(c) / 2.0 ** f for c in row] for row in q]))
    off = list(gains)
    off[4] = 0.0                                                            # switching a record off removes exactly its windows
    q_off, _ = expected_quanta(w, records, off)
    only, _ = expected_quanta(w, [records[4]], [gains[4]], frac_bits=f)
    assert all(int(a) - int(b) == int(c) for a, b, c in zip(q.ravel(), q_off.ravel(), only.ravel()))
    clamp, _ = expected_quanta(w, [records[6]], [1e30], frac_bits=f)        # every window at the clamp: the hard counts
    hard = np.zeros((7, 5), dtype=np.int64)
    for p in range(58):
        hard[np.arange(7), records[6][p:p + 7]] += 1
    assert all(int(a) == int(b) * 2 ** f for a, b in zip(clamp.ravel(), hard.ravel()))


def sums_stub(z, windows):
    return lm.SetSums(np.asarray(z, dtype=np.float64), np.asarray(windows, dtype=np.int64), "")


def test_posterior_gains_oops_and_zoops():
    s = sums_stub([[4.0, 0.0, 0.5, np.inf, 8.0, np.nan]], [[10, 5, 1, 3, 0, 2]])
    g = lm.posterior_gains(s)
    assert g.dtype == np.float64 and g.shape == (1, 6)
    assert g.tolist() == [[0.25, 0.0, 2.0, 0.0, 0.0, 0.0]]                 # Z of 0, +inf, NaN and no window: gain 0
    # ZOOPS, gamma 1/2: lambda = 1 / (2 W), g = lambda / (1/2 + lambda Z)
    z = lm.posterior_gains(s, "zoops", 0.5)
    assert z[0, 0] == (0.5 / 10) / (0.5 + (0.5 / 10) * 4.0) and z[0, 2] == 0.5 / (0.5 + 0.5 * 0.5)
    assert z[0, 1] == 0.0 and z[0, 3] == 0.0 and z[0, 4] == 0.0 and z[0, 5] == 0.0
    assert lm.posterior_gains(s, "zoops", 1.0)[0, 0] == (1.0 / 10) / ((1.0 / 10) * 4.0)   # gamma 1 is OOPS
    assert math.isclose(lm.posterior_gains(s, "zoops", 1.0)[0, 0], 0.25)
    two = sums_stub([[4.0, 2.0], [1.0, 8.0]], [[2, 2], [4, 4]])
    per = lm.posterior_gains(two, "zoops", [0.5, 0.25])                    # one gamma per motif
    assert per[0, 1] == 0.25 / (0.5 + 0.25 * 2.0) and per[1, 1] == (0.25 / 4) / (0.75 + (0.25 / 4) * 8.0)
    for bad in (dict(model="zoops"), dict(model="zoops", gamma=0.0), dict(model="zoops", gamma=1.5), dict(model="tcm")):
        with pytest.raises(ValueError):
            lm.posterior_gains(s, **bad)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("protein", [False, True], ids=["dna", "protein"])
def test_float_count_m_step_is_count_matrix_to_scoring(protein):
    rng = np.random.default_rng(9 + protein)
    k = 21 if protein else 5
    counts = rng.integers(0, 500, (12, k)).astype(np.uint32)
    counts[3] = 0
    counts[:, k - 1] = rng.integers(0, 3, 12)
    cm = lm.CountMatrix(counts, protein=protein)
    bg = rng.random(k).astype(np.float32)
    bg[k - 1] = 0
    bg /= bg.sum()
    for pseudo, background in ((None, None), (0.1, None), (0.5, bg), (1.0, bg)):
        want = cm.to_scoring(pseudo, background)
        got = lm.expected_to_scoring(counts.astype(np.float64), pseudo, background, protein=protein)
        assert np.array_equal(bits(got.data), bits(want.data)) and np.array_equal(bits(got.background), bits(want.background))
    assert np.array_equal(bits(cm.normalize(0.1).log_odds().data), bits(lm.expected_to_scoring(counts.astype(np.float64), 0.1, protein=protein).data))
    with pytest.raises(ValueError):
        lm.expected_to_scoring(np.zeros((4, k + 1)), protein=protein)


def test_the_planted_signal_carries_the_rule_through_em():
    """What tests/test_gpu_seqset_expect.py asks of the device, asked of the rule alone on the same set, start and seed: the
    OOPS log-likelihood does not decrease over 5 iterations and the refined matrix spells the planted word."""
    word, texts = planted_case()
    syms = [encode(t) for t in texts]
    counts = np.zeros((len(texts), 5), dtype=np.int64)
    for i, s in enumerate(syms):
        counts[i] = np.bincount(s, minlength=5)
    bg = lm.background_from_counts(counts)
    start = lm.expected_to_scoring(flattened_start(word), None, bg).data
    final, lls = rule_em(start, syms, 5, lambda e: lm.expected_to_scoring(e, 0.1, bg).data)
    assert len(lls) == 6
    for a, b in zip(lls, lls[1:]):
        assert b >= a - 1e-9 * abs(a), lls
    assert lls[-1] > lls[0] + 50
    assert "".join(DNA_SYMBOLS[int(s)] for s in np.argmax(final[:, :4], axis=1)) == word


def test_cli_refine_options_go_together(tmp_path):
    mats = tmp_path / "motifs.pwm"
    mats.write_text(">MA0002.1\tSECOND\nA  [ 20  0  0 ]\nC  [  0 20  0 ]\nG  [  0  0 20 ]\nT  [  0  0  0 ]\n")
    for argv in (["--refine", "2"], ["--refined", "x.pwm"], ["--refine", "0", "--refined", "x.pwm"]):
        with pytest.raises(SystemExit):
            scan_cli.main(["-m", str(mats), "-s", "none.fa", "-o", "none.tsv"] + argv)
