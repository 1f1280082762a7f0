"""The expected site counts of every motif over a sequence set, in one call (lm_hip_seqset_expected_counts,
csrc/seqset_expect.hip): the E-step of motif EM.  Expectations come from the rule of tests/expect_rule.py: bit for bit
where every weight of a window is exact (integer weights, scale 1, gains that are powers of two), within the derived bound
elsewhere; and the EM built on it (``Pipeline.em_step`` / ``refine``) on a planted set.

The C++ mirror (``Pipeline::expected_counts`` of host/lightmotif_hip.hpp) has no GPU program of its own: tests/cpp holds
no pattern for one, the mirror is compiled by tests/test_cpp_host.py and forwards to the entry point tested here."""
import ctypes as C
import math

import numpy as np
import pytest

import lightmotif_amd as lm
from lightmotif_amd.lib import stride as lm_stride
from lightmotif_amd import _ffi
from lightmotif_amd import io as lmio
from pathlib import Path
from seqset_best_cases import DNA_SYMBOLS, encode
from seqset_sum_cases import TOLERANCE, sums_of
from expect_rule import (consensus_matrix, edge_records, expected_counts, flattened_start, frac_bits_of, planted_case, window_scores)

pytestmark = pytest.mark.gpu

DNA, PROTEIN = np.frombuffer(b"ACTGN", dtype=np.uint8), np.frombuffer(b"ACDEFGHIKLMNPQRSTVWYX", dtype=np.uint8)
FIXTURE = Path(__file__).parent / "golden" / "JASPAR2024.pwm.gz"
ROWS_PER_STREAM = (0, 1, 7)
KERNEL = "seqset_expect_generic"


def integer_matrix(rng, m, k):
    """Integer weights in [-6, 6] on at most 8 rows, zeros elsewhere: the window scores are integers of a few tens, so that
    with gains 2^-k the weights of the windows spread over the whole fixed point: some clamp at 1, some round to 0."""
    p = np.zeros((m, lm_stride(k, 4)), np.float32)
    rows = rng.permutation(m)[:8]
    p[rows, :k] = rng.integers(-6, 7, (len(rows), k))
    return p


def random_matrix(rng, m, k, n_weight=-np.inf):
    p = np.zeros((m, lm_stride(k, 4)), np.float32)
    p[:, :k] = rng.normal(0, 1.5, (m, k))
    p[:, k - 1] = n_weight
    return p


def text_of(rng, length, k, unknown=0.02):
    sym = rng.integers(0, k - 1, int(length))
    sym[rng.random(int(length)) < unknown] = k - 1
    return (DNA if k == 5 else PROTEIN)[sym].copy()


def symbols_of(text, k):
    lut = np.full(256, k - 1, dtype=np.int64)
    lut[DNA if k == 5 else PROTEIN] = np.arange(k)
    raw = np.frombuffer(text.encode() if isinstance(text, str) else text, dtype=np.uint8) if isinstance(text, (str, bytes)) else np.asarray(text, dtype=np.uint8)
    return lut[raw]


def power_gains(rng, n, records):
    """2^-k, with records switched off (0) and records whose every window clamps (2^30)."""
    g = np.ldexp(1.0, -rng.integers(0, 13, (n, records)))
    pick = rng.random((n, records))
    g[pick < 0.1] = 0.0
    g[pick > 0.9] = 2.0 ** 30
    return g


def at_every_run_length(pli, call, rows_per_stream=ROWS_PER_STREAM):
    out = {}
    for rps in rows_per_stream:
        pli.set_rows_per_stream(rps)
        try:
            out[rps] = call()
        finally:
            pli.set_rows_per_stream(0)
    return out


def check_exact(pli, records, mats, gains, k=5, rows_per_stream=ROWS_PER_STREAM, scales=None):
    """The device equals the rule bit for bit, at every run length; returns the rule's answer."""
    protein = k == 21
    syms = [symbols_of(r, k) for r in records]
    want, f = expected_counts(mats, syms, gains, scales, k)
    seqset = pli.stripe_ascii_set(records, protein=protein, lossy=True)
    seqset.configure_wrap(max(p.shape[0] for p in mats))
    pssms = [lm.ScoringMatrix(p, protein=protein) for p in mats]
    for rps, res in at_every_run_length(pli, lambda: pli.expected_counts_set(pssms, seqset, gains, scale=scales), rows_per_stream).items():
        assert res.frac_bits == f == frac_bits_of(sum(len(r) for r in records)) and len(res) == len(mats)
        for i, (e, q, _) in enumerate(want):
            got = res.counts[i]
            assert got.dtype == np.float64 and got.shape == (mats[i].shape[0], k)
            assert got.tobytes() == e.tobytes(), (rps, i, mats[i].shape[0], np.argwhere(got != e)[:5], got[got != e][:5], e[got != e][:5])
            assert [int(x) for x in res.quanta()[i].ravel()] == [int(c) for c in q.ravel()]
    return want, seqset


@pytest.mark.parametrize("protein", [False, True], ids=["dna", "protein"])
def test_exact_counts_over_motif_lengths(pli, protein):
    """Mixed records -- empty ones at the start, in the middle and at the end, shorter than M, exactly M, over many lane
    runs, N / X symbols, the last record ending inside the last column (padding behind it) -- against every motif length of
    the sweep in one call, at lane runs of the default length, 1 and 7 rows (records cross runs and streams)."""
    k = 21 if protein else 5
    ms = (1, 12, 40) if protein else (1, 2, 7, 20, 36, 37, 70)
    rng = np.random.default_rng(100 + k)
    lengths = [0, 0, 300] + [m + d for m in ms for d in (-1, 0)] + [0, 1, 33, 450, 64, 0, 150, 75, 0]
    records = [text_of(rng, n, k) for n in lengths]
    assert sum(lengths) % 32 != 0                                     # the last column holds padding
    mats = [integer_matrix(rng, m, k) for m in ms]
    gains = power_gains(rng, len(ms), len(records))
    want, _ = check_exact(pli, records, mats, gains, k)
    for (e, q, windows), m in zip(want, ms):
        assert windows > 0 and e.any() and len({sum(int(c) for c in row) for row in q}) == 1
    assert any(e[:, k - 1].any() for e, _, _ in want)                 # the N / X column counts too


def test_exact_counts_on_the_planted_edges(pli):
    """The edge records of the best-hit tests (a consensus across every junction, at the first and the last base, an empty
    record, a record that is the motif, the tail window in the padding) with N weighing like a match: a missing cut would
    count the neighbour's bases or the padding."""
    m = 12
    consensus, records, notes = edge_records(m=m)
    p = consensus_matrix(consensus, 2.0, lm_stride(5, 4))
    rng = np.random.default_rng(2)
    gains = np.ldexp(1.0, -rng.integers(8, 30, (1, len(records)))).astype(np.float64)
    gains[0, notes["repeat"]] = 0.0
    want, _ = check_exact(pli, records, [p], gains)
    assert want[0][0].any()


def test_exact_counts_one_record_and_tiny_records(pli):
    rng = np.random.default_rng(4)
    q = integer_matrix(rng, 7, 5)
    full = text_of(rng, 32 * 40, 5)                                    # one record that fills the set, no padding at all
    _, seqset = check_exact(pli, [full], [q], np.asarray([[2.0 ** -6]]))
    assert seqset.rows == 40
    check_exact(pli, [full[:7]], [q], np.asarray([[0.5]]))             # a record of exactly M
    want, _ = check_exact(pli, [full[:6]], [q], np.asarray([[0.5]]))   # a record shorter than M: zeros
    assert not want[0][0].any()
    check_exact(pli, [b"N" * 50, full[:40]], [q], np.asarray([[0.25, 0.25]]))   # N symbols alone


def test_exact_counts_with_offsets_in_global_memory(pli):
    """5 000 records of 3 ... 9 symbols: the offsets table is read from global memory, most lanes cross several records."""
    rng = np.random.default_rng(6)
    records = [text_of(rng, n, 5) for n in rng.integers(3, 10, 5_000)]
    mats = [integer_matrix(rng, m, 5) for m in (1, 4, 7)]
    check_exact(pli, records, mats, power_gains(rng, 3, 5_000), rows_per_stream=(0, 7))


def test_exact_counts_of_four_motifs_one_degenerate(pli):
    rng = np.random.default_rng(8)
    records = [text_of(rng, n, 5) for n in (90, 0, 41, 200, 12)]
    ms = (5, sum(len(r) for r in records) + 1, 38, 16)                 # the second is longer than the whole set
    mats = [integer_matrix(rng, m, 5) for m in ms]
    want, seqset = check_exact(pli, records, mats, power_gains(rng, 4, 5), rows_per_stream=(0, 7))
    assert not want[1][0].any() and want[1][2] == 0
    res = pli.expected_counts_set([lm.ScoringMatrix(p) for p in mats], seqset, np.ones((4, 5)))
    assert res.kernel == KERNEL and not res.counts[1].any() and res.counts[1].shape == (ms[1], 5)


def test_clamp_and_gain_zero(pli):
    """Gains so large that every window clamps at 1 give the hard counts of all windows; gain 0 removes a record."""
    rng = np.random.default_rng(10)
    records = [text_of(rng, n, 5, unknown=0.0) for n in (60, 45, 80)]
    p = integer_matrix(rng, 9, 5)
    seqset = pli.stripe_ascii_set(records)
    seqset.configure_wrap(9)
    res = pli.expected_counts_set([lm.ScoringMatrix(p)], seqset, np.asarray([[2.0 ** 200, 0.0, 2.0 ** 200]]))
    hard = np.zeros((9, 5))
    for r in (0, 2):
        s = symbols_of(records[r], 5)
        for at in range(len(s) - 8):
            hard[np.arange(9), s[at:at + 9]] += 1
    assert np.array_equal(res.counts[0], hard)


def test_order_free(pli):
    """Random f32 weights and random gains: the same call at three lane-run lengths, alone and inside a batch of 9 motifs,
    and twice over, gives identical bytes."""
    rng = np.random.default_rng(12)
    records = [text_of(rng, n, 5) for n in rng.integers(100, 600, 12)]
    ms = (4, 9, 17, 36, 40, 12, 25, 8, 50)
    pssms = [lm.ScoringMatrix(random_matrix(rng, m, 5, n_weight=-1.0)) for m in ms]
    seqset = pli.stripe_ascii_set(records, lossy=True)
    seqset.configure_wrap(max(ms))
    sums = pli.scan_sum_set(pssms, seqset)
    gains = lm.posterior_gains(sums) * rng.uniform(0.2, 3.0, sums.shape)
    scales = rng.uniform(0.5, 1.5, len(ms)).astype(np.float32)
    sums_scaled = pli.scan_sum_set(pssms, seqset, scale=scales)
    gains_scaled = lm.posterior_gains(sums_scaled) * rng.uniform(0.2, 3.0, sums.shape)
    for g, sc in ((gains, None), (gains_scaled, scales)):
        tables = at_every_run_length(pli, lambda: [pli.expected_counts_set(pssms, seqset, g, scale=sc) for _ in range(2)], (0, 3, 64))
        first = tables[0][0]
        assert all(c.any() for c in first.counts)
        for rps, (a, b) in tables.items():
            for i in range(len(ms)):
                assert a.counts[i].tobytes() == b.counts[i].tobytes() == first.counts[i].tobytes(), (rps, i)
        for i in (0, 3, 4, 8):                                         # alone: another default run length, another grouping
            alone = pli.expected_counts_set([pssms[i]], seqset, g[i:i + 1], scale=None if sc is None else sc[i:i + 1])
            assert alone.counts[0].tobytes() == first.counts[i].tobytes() and alone.frac_bits == first.frac_bits, i


@pytest.mark.parametrize("scale", [1.0, 0.5])
def test_against_the_rule_with_real_weights(pli, scale):
    """Eight JASPAR matrices, OOPS gains 1 / Z_r from the rule's own sums.  Every cell within ``TOLERANCE * E_rule + W *
    2^-F``: TOLERANCE is the 2^-21 of tests/seqset_sum_cases.py (the bound of one term; all terms positive), and the
    device's e may differ from the rule's by an ulp of f32 and flip the rounding of q by one quantum, so each of the W
    windows gets one quantum.  Row totals are equal as integers, and under OOPS gains each lies within the same bound of
    the number of records that have a window."""
    rng = np.random.default_rng(14)
    motifs = [r.matrix for r in lmio.read(FIXTURE)][:8]
    pssms = [cm.to_scoring(0.1) for cm in motifs]
    mats = [p.data for p in pssms]
    records = [text_of(rng, n, 5, unknown=0.0) for n in rng.integers(8, 160, 40)]
    records[5] = records[5][:4]                                        # shorter than every motif
    syms = [symbols_of(r, 5) for r in records]
    scales = [scale] * len(mats)
    z = sums_of(mats, syms, scales)
    with np.errstate(divide="ignore"):
        gains = np.where(z > 0, 1.0 / z, 0.0)
    want, f = expected_counts(mats, syms, gains, scales)
    seqset = pli.stripe_ascii_set(records)
    seqset.configure_wrap(max(len(p) for p in pssms))
    res = pli.expected_counts_set(pssms, seqset, gains, scale=None if scale == 1.0 else scale)
    assert res.frac_bits == f and res.kernel == KERNEL
    unit = 2.0 ** -f
    for i, (e, q, windows) in enumerate(want):
        got = res.counts[i]
        bound = TOLERANCE * e + windows * unit
        err = np.abs(got - e)
        print(f"motif {i} (M = {len(pssms[i])}, {windows} windows) scale {scale}: worst error {err.max():.3e}, worst error / bound "
              f"{(err / bound).max():.3e}")
        assert np.all(err <= bound), (i, np.argwhere(err > bound)[:5])
        totals = [int(t) for t in res.quanta()[i].sum(axis=1)]
        assert len(set(totals)) == 1, (i, totals)
        with_window = sum(len(r) >= len(pssms[i]) for r in records)
        assert with_window > 30 and abs(totals[0] * unit - with_window) <= TOLERANCE * with_window + windows * unit, (i, totals[0] * unit, with_window)


def test_special_values(pli):
    """Windows that score NaN, -inf and +inf under a gain > 0: NaN contributes nothing, -inf contributes 0, +inf clamps to
    1; the other weights are integers, so the device equals the rule bit for bit."""
    rng = np.random.default_rng(16)
    p_nan, p_pinf, p_ninf, p_all = (integer_matrix(rng, 8, 5) for _ in range(4))
    p_nan[3, 0] = np.nan                                               # an A at offset 3
    p_pinf[2, 1] = np.inf                                              # a C at offset 2
    p_ninf[:, 4] = -np.inf                                             # any N
    p_all[:, :5] = np.nan
    records = ["N" * 30, "ACGT" * 10, "A" * 25, "GGTGGTAGGTTTGGAGGATGAGT", "CCCAGGGTTT", "ANNNNNNNNNNNNNNNNNNNNN", "TTGTTGTGGTTG"]
    gains = np.ldexp(1.0, -(np.arange(4 * 7).reshape(4, 7) % 11) - 1)
    want, seqset = check_exact(pli, records, [p_nan, p_pinf, p_ninf, p_all], gains, rows_per_stream=(0, 3))
    res = pli.expected_counts_set([lm.ScoringMatrix(p) for p in (p_nan, p_pinf, p_ninf, p_all)], seqset, gains)
    assert not res.counts[3].any()                                     # every window NaN
    nan_windows = sum(int(np.isnan(window_scores(p_nan, encode(r))).sum()) for r in records)
    assert nan_windows > 20 and res.counts[0].any()
    inf_windows = sum(int(np.isposinf(window_scores(p_pinf, encode(r))).sum()) for r in records)
    assert inf_windows > 5 and res.counts[1][2, 1] >= inf_windows     # each of them weighs exactly 1 at its C
    only_inf = p_pinf.copy()
    only_inf[:, :5] = np.where(np.isposinf(p_pinf[:, :5]), np.inf, -40.0)   # the finite windows score -320: they round to 0
    alone = pli.expected_counts_set([lm.ScoringMatrix(only_inf)], seqset, gains[1:2])
    assert alone.counts[0][2].tolist() == [0.0, float(inf_windows), 0.0, 0.0, 0.0]
    assert not res.counts[2][:, 4].any() and res.counts[2].any()       # no window with an N counts


def test_misuse_is_a_status(pli):
    rng = np.random.default_rng(18)
    records = [text_of(rng, n, 5) for n in (100, 200, 150, 100, 200)]
    seqset = pli.stripe_ascii_set(records, lossy=True)
    mat = integer_matrix(rng, 20, 5)
    p20 = lm.ScoringMatrix(mat)
    ones = np.ones((1, 5))
    with pytest.raises(lm.LightmotifHipError) as err:                      # no wrap rows yet
        pli.expected_counts_set([p20], seqset, ones)
    assert err.value.status == _ffi.ERR_WRAP
    seqset.configure_wrap(19)
    good = pli.expected_counts_set([p20], seqset, ones)
    assert good.counts[0].shape == (20, 5) and good.kernel == KERNEL
    prot = lm.ScoringMatrix(random_matrix(rng, 8, 21), protein=True)
    with pytest.raises(ValueError):                                        # the Python layer refuses first
        pli.expected_counts_set([prot], seqset, ones)
    L = _ffi.lib()
    call = L.lm_hip_seqset_expected_counts
    sentinel = -7.25
    out = (C.c_double * 200)(*[sentinel] * 200)
    untouched = lambda: list(out) == [sentinel] * 200
    g5 = (C.c_double * 5)(*[1.0] * 5)
    frac = C.c_int(-1)
    handles = (C.c_void_p * 1)(prot._device(pli))
    assert call(pli._h, handles, None, g5, 1, seqset._h, out, C.byref(frac)) == _ffi.ERR_BAD_ARGS and "alphabet" in _ffi.last_error()
    dna = (C.c_void_p * 1)(p20._device(pli))
    for bad in (0.0, -1.0, math.inf, -math.inf, math.nan):                 # a scale is finite and > 0
        assert call(pli._h, dna, (C.c_float * 1)(bad), g5, 1, seqset._h, out, None) == _ffi.ERR_BAD_ARGS, bad
        assert "scale" in _ffi.last_error() and untouched()
        with pytest.raises(lm.LightmotifHipError):
            pli.expected_counts_set([p20], seqset, ones, scale=bad)
    for bad in (math.nan, -1.0, math.inf, -math.inf, -1e-300):            # a gain is finite and >= 0
        gb = (C.c_double * 5)(1.0, 1.0, bad, 1.0, 1.0)
        assert call(pli._h, dna, None, gb, 1, seqset._h, out, None) == _ffi.ERR_BAD_ARGS, bad
        assert "gain" in _ffi.last_error() and "record 2" in _ffi.last_error() and untouched()
        with pytest.raises(lm.LightmotifHipError):
            pli.expected_counts_set([p20], seqset, np.asarray([[1.0, 1.0, bad, 1.0, 1.0]]))
    assert call(None, dna, None, g5, 1, seqset._h, out, None) == _ffi.ERR_BAD_ARGS and _ffi.last_error()
    assert call(pli._h, None, None, g5, 1, seqset._h, out, None) == _ffi.ERR_BAD_ARGS and _ffi.last_error()
    assert call(pli._h, dna, None, g5, 1, None, out, None) == _ffi.ERR_BAD_ARGS and _ffi.last_error()
    assert call(pli._h, dna, None, None, 1, seqset._h, out, None) == _ffi.ERR_BAD_ARGS and "gains" in _ffi.last_error()
    assert call(pli._h, dna, None, g5, 1, seqset._h, None, None) == _ffi.ERR_BAD_ARGS and _ffi.last_error()     # null counts, n > 0
    assert untouched()
    assert call(pli._h, None, None, None, 0, seqset._h, out, None) == _ffi.OK and untouched()                    # n == 0: nothing written
    empty = pli.stripe_ascii_set([])
    empty.configure_wrap(19)
    assert call(pli._h, dna, None, None, 1, empty._h, out, C.byref(frac)) == _ffi.OK and untouched() and frac.value == 40   # no records
    # the raw ABI with a scale array: the answer of the Python layer, bit for bit
    assert call(pli._h, dna, (C.c_float * 1)(0.5), g5, 1, seqset._h, out, C.byref(frac)) == _ffi.OK
    via = pli.expected_counts_set([p20], seqset, ones, scale=[0.5])
    assert np.asarray(list(out)[:100]).tobytes() == via.counts[0].tobytes() and frac.value == via.frac_bits and list(out)[100:] == [sentinel] * 100
    for bad in (np.ones((2, 5)), np.ones(5), np.ones((1, 4))):
        with pytest.raises(ValueError):
            pli.expected_counts_set([p20], seqset, bad)
    assert len(pli.expected_counts_set([], seqset, np.zeros((0, 5)))) == 0
    res = pli.expected_counts_set([p20], empty, np.zeros((1, 0)))
    assert res.kernel == "" and not res.counts[0].any() and res.counts[0].shape == (20, 5)


def test_em_step_and_refine_on_a_planted_set(pli):
    """200 records x 60 bp, a 10-mer planted in each with 10 % of its letters mutated, the start flattened towards the
    background (tests/test_expect_host.py checks with the rule alone that this set carries the rule through both
    conditions).  The OOPS log-likelihood does not decrease over 5 iterations -- with 1e-9 relative slack: the posteriors
    are quantised to 2^-40 and the device's exponential is right to an ulp of f32, so the M-step is the exact maximiser
    only to that precision -- and the refined matrix spells the planted word."""
    word, texts = planted_case()
    seqset = pli.stripe_ascii_set(texts)
    seqset.configure_wrap(len(word))
    bg = seqset.background()
    start = lm.expected_to_scoring(flattened_start(word), None, bg)
    mats, lls = pli.refine([start], seqset, 5)
    assert lls.shape == (6, 1) and np.isfinite(lls).all()
    print("log2-likelihood per iteration:", lls[:, 0].tolist())
    for a, b in zip(lls[:, 0], lls[1:, 0]):
        assert b >= a - 1e-9 * abs(a), lls[:, 0].tolist()
    assert lls[-1, 0] > lls[0, 0] + 50
    assert "".join(DNA_SYMBOLS[int(s)] for s in np.argmax(mats[0].data[:, :4], axis=1)) == word
    # one step is sums, gains, expected counts, matrices
    new, expected, gamma, ll = pli.em_step([start], seqset)
    sums = pli.scan_sum_set([start], seqset)
    direct = pli.expected_counts_set([start], seqset, lm.posterior_gains(sums))
    assert gamma is None and ll[0] == lls[0, 0] and expected.counts[0].tobytes() == direct.counts[0].tobytes()
    assert np.array_equal(new[0].data, lm.expected_to_scoring(direct.counts[0], 0.1, bg).data)
    rows = expected.quanta()[0].sum(axis=1)
    assert len(set(rows.tolist())) == 1 and abs(rows[0] * 2.0 ** -expected.frac_bits - 200) < 1e-4   # one site per record
    # ZOOPS: a site in every record, so the share of records with a site goes up from 1/2
    zm, zll, zexp = pli.refine([start], seqset, 3, model="zoops", gamma=0.5, return_counts=True)
    _, _, g1, _ = pli.em_step([start], seqset, model="zoops", gamma=0.5)
    assert 0.5 < g1[0] <= 1.0 and zll.shape == (4, 1) and zll[-1, 0] > zll[0, 0]
    assert "".join(DNA_SYMBOLS[int(s)] for s in np.argmax(zm[0].data[:, :4], axis=1)) == word
    assert zexp.counts[0].sum(axis=1).max() <= 200.0
