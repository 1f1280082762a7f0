"""The total odds of every motif in every record of a sequence set, in one call and without a hit list
(lm_hip_scan_sum_seqset, csrc/seqset_sum.hip): per (motif, record) the f64 sum of ``2 ** fl32(scale * score)`` over the
windows ``pos + M <= L`` (the reference's scan.rs:185-190, per record).  Expectations come from sums made on the host in the
reference's add order and the rule of tests/seqset_sum_cases.py: bit for bit where every term is an exact power of two
(that isolates the walk and the merge of the lanes' partial sums from the exponential), within the derived 2^-21
elsewhere."""
import ctypes as C
import math

import numpy as np
import pytest

import lightmotif_amd as lm
from lightmotif_amd.lib import stride as lm_stride
from lightmotif_amd import _ffi, scan_cli
from lightmotif_amd import io as lmio
from seqset_best_cases import encode
from seqset_sum_cases import TOLERANCE, close, consensus_matrix, edge_records, sum_of, sums_of, window_scores

pytestmark = pytest.mark.gpu

DNA, PROTEIN = np.frombuffer(b"ACTGN", dtype=np.uint8), np.frombuffer(b"ACDEFGHIKLMNPQRSTVWYX", dtype=np.uint8)
MOTIF_LENGTHS = (1, 4, 17, 36, 37, 64)          # fused kernels up to 36, the length-generic kernel beyond
POOL = sorted({0, 1, 31, 32, 33, 100} | {m + d for m in MOTIF_LENGTHS for d in (-1, 0, 1)})
ROWS_PER_STREAM = (0, 1, 7, 64)
LENGTHS = {1: [150], 2: [64, 100]}


def integer_matrix(rng, m, k):
    """Weights in {-1, 0, 1} on at most 20 rows: every window score is an integer in [-20, 20], every term an exact power
    of two and the terms of a record within 40 binades, so that any order of f64 additions gives the same sum."""
    p = np.zeros((m, lm_stride(k, 4)), np.float32)
    rows = rng.permutation(m)[:20]
    p[rows, :k] = rng.integers(-1, 2, (len(rows), k))
    return p


def random_matrix(rng, m, k, n_weight=-np.inf):
    p = np.zeros((m, lm_stride(k, 4)), np.float32)
    p[:, :k] = rng.normal(0, 2, (m, k))
    p[:, k - 1] = n_weight
    return p


def make_records(rng, n, k, lengths):
    """Record texts (uint8 arrays) with 2 % N / X."""
    alphabet = DNA if k == 5 else PROTEIN
    out = []
    for length in lengths:
        sym = rng.integers(0, k - 1, int(length))
        sym[rng.random(int(length)) < 0.02] = k - 1
        out.append(alphabet[sym].copy())
    assert len(out) == n
    return out


def lengths_for(rng, n_records):
    if n_records in LENGTHS:
        return LENGTHS[n_records]
    if n_records == 37:                                            # mixed: the pool and records of many lane runs
        return [int(rng.choice(POOL)) for _ in range(30)] + [int(x) for x in rng.integers(200, 900, 7)]
    return [int(rng.choice(POOL)) for _ in range(n_records)]


def symbols_of(text, k):
    lut = np.full(256, k - 1, dtype=np.int64)
    lut[DNA if k == 5 else PROTEIN] = np.arange(k)
    return lut[np.asarray(text, dtype=np.uint8)]


def at_every_run_length(pli, call, rows_per_stream=ROWS_PER_STREAM):
    out = {}
    for rps in rows_per_stream:
        pli.set_rows_per_stream(rps)
        try:
            out[rps] = call()
        finally:
            pli.set_rows_per_stream(0)
    return out


def worst(got, want):
    plain = np.isfinite(want) & (want != 0)
    return float(np.max(np.abs(got[plain] - want[plain]) / want[plain], initial=0.0))


@pytest.mark.parametrize("protein", [False, True], ids=["dna", "protein"])
@pytest.mark.parametrize("n_records", [1, 2, 37, 5_000])
def test_exact_sums(pli, protein, n_records):
    """All-zero weights: a cell is the number of windows, as an exact double.  Small-integer weights at scale 1: a cell is
    ``sum_of`` bit for bit.  Both kernels, offsets in LDS and (5 000 records) in global memory, mixed record lengths, lane
    runs of the default length, 1, 7 and 64 rows; with one and two records also a motif longer than the whole set."""
    k = 21 if protein else 5
    rng = np.random.default_rng(3_000 * n_records + k)
    records = make_records(rng, n_records, k, lengths_for(rng, n_records))
    ms = list(MOTIF_LENGTHS) + ([sum(len(r) for r in records) + 1] if n_records <= 2 else [])
    ints = [integer_matrix(rng, m, k) for m in ms]
    zeros = [np.zeros_like(p) for p in ints]
    syms = [symbols_of(r, k) for r in records]
    want = sums_of(ints, syms)
    windows = np.maximum(0, np.asarray([len(r) for r in records], dtype=np.int64)[None, :] - np.asarray(ms)[:, None] + 1)
    assert (want > 0).any(axis=1)[:len(MOTIF_LENGTHS)].all() and (windows == 0).any()
    seqset = pli.stripe_ascii_set(records, protein=protein, lossy=True)
    seqset.configure_wrap(max(ms))
    for name, mats, expect in (("zeros", zeros, windows.astype(np.float64)), ("integers", ints, want)):
        pssms = [lm.ScoringMatrix(p, protein=protein) for p in mats]
        tables = at_every_run_length(pli, lambda: pli.scan_sum_set(pssms, seqset))
        for rps, res in tables.items():
            assert res.sums.dtype == np.float64 and res.shape == (len(ms), n_records)
            assert res.last_kernel == "seqset_sum_generic"          # the last group launched: M = 64
            assert np.array_equal(res.windows, windows)
            assert res.sums.tobytes() == expect.tobytes(), (name, rps, np.argwhere(res.sums != expect)[:5])
        if n_records <= 2:
            assert not tables[0].sums[-1].any() and not windows[-1].any()   # longer than the whole set: a row of zeros
    short = pli.scan_sum_set(pli.prepare_batch([lm.ScoringMatrix(p, protein=protein) for p in ints[:4]]), seqset)   # a MotifBatch
    assert short.last_kernel.startswith("seqset_sum_fused<") and short.sums.tobytes() == want[:4].tobytes()


@pytest.mark.parametrize("protein", [False, True], ids=["dna", "protein"])
@pytest.mark.parametrize("n_records", [2, 37, 5_000])
def test_random_weights_within_the_derived_tolerance(pli, protein, n_records):
    """Random f32 weights, -inf in the N / X column: every cell within 2^-21 relative of ``sum_of`` (seqset_sum_cases.py
    derives the bound), cells of 0 exactly 0; scales of 1 (no array), and one per motif."""
    k = 21 if protein else 5
    rng = np.random.default_rng(5_000 * n_records + k)
    records = make_records(rng, n_records, k, lengths_for(rng, n_records))
    mats = [random_matrix(rng, m, k) for m in MOTIF_LENGTHS]
    syms = [symbols_of(r, k) for r in records]
    pssms = [lm.ScoringMatrix(p, protein=protein) for p in mats]
    seqset = pli.stripe_ascii_set(records, protein=protein, lossy=True)
    seqset.configure_wrap(max(MOTIF_LENGTHS))
    scales = np.asarray([1.0, 0.5, math.log2(10.0), 3.0, 0.25, 1.5], dtype=np.float32)
    for sc in (None, scales):
        want = sums_of(mats, syms, sc)
        assert np.isfinite(want).all() and (want > 0).any()
        if n_records > 2:                                          # every motif has a cell of 0 (an N in every window) and one above
            assert (want == 0).any(axis=1).all() and (want > 0).any(axis=1).all()
        for rps, res in at_every_run_length(pli, lambda: pli.scan_sum_set(pssms, seqset, scale=sc), (0, 7)).items():
            print(f"records {n_records} k {k} scales {sc is not None} rows_per_stream {rps}: worst relative error {worst(res.sums, want):.3e} "
                  f"(bound {TOLERANCE:.3e})")
            assert close(res.sums, want), (rps, worst(res.sums, want))
    if n_records == 2:
        one = pli.scan_sum_set(pssms, seqset, scale=0.5)           # one number: every motif
        assert close(one.sums, sums_of(mats, syms, [0.5] * len(mats)))


def check_exact(pli, records, mats, scales=None, rows_per_stream=ROWS_PER_STREAM):
    want = sums_of(mats, [encode(r) for r in records], scales)
    seqset = pli.stripe_ascii_set(records)
    seqset.configure_wrap(max(p.shape[0] for p in mats))
    pssms = [lm.ScoringMatrix(p) for p in mats]
    for rps, res in at_every_run_length(pli, lambda: pli.scan_sum_set(pssms, seqset, scale=scales), rows_per_stream).items():
        assert res.sums.tobytes() == want.tobytes(), (rps, np.argwhere(res.sums != want)[:5], [len(r) for r in records])
    return want, seqset


def test_planted_edges(pli):
    """N scores like a match, so padding and the neighbour's bases would add 2^(m) wherever the cut were missing.  The
    weights are +-2 and the scale 1/2: every term is an exact power of two within 24 binades, the cells are exact."""
    m = 12
    consensus, records, notes = edge_records(m=m)
    p = consensus_matrix(consensus, 2.0, lm_stride(5, 4))
    want, _ = check_exact(pli, records, [p], [0.5])
    full = 2.0 ** m
    for a, b in notes["split"]:                                    # a consensus across a junction adds to neither record
        assert want[0, a] < full and want[0, b] < full, (a, b)
    for r in notes["planted"]:
        assert want[0, r] >= full
    assert want[0, notes["empty"]] == 0.0 and want[0, notes["last"]] < full
    # records shorter than M and runs of empty records around a long one; a set of one record
    rng = np.random.default_rng(8)
    q = integer_matrix(rng, m, 5)
    text = "".join(rng.choice(list("ACGT"), 32 * 40))
    check_exact(pli, ["ACGT", "", "", text[:100], "", "ACGTACGTACG", text[100:400], ""], [q])
    check_exact(pli, [text[:500]], [q])
    check_exact(pli, [text[:m]], [q])
    check_exact(pli, [text[:m - 1]], [q])


def test_junctions_on_run_and_column_boundaries(pli):
    """A set of exactly 32 * R symbols has R rows: a junction at a multiple of R lies at the bottom of a column, where a
    lane's run ends and its last windows read the next column's top.  With lane runs of 7 rows a junction at 7 or 14 lies
    on a run boundary; several empty records share that offset.  The long records span three runs and more, so middle
    lanes have a head alone."""
    rows, m = 40, 12
    rng = np.random.default_rng(78)
    q = integer_matrix(rng, m, 5)
    text = "".join(rng.choice(list("ACGT"), 32 * rows))
    cases = 0
    for cut in (7, 14, rows - m, rows - 1, rows, rows + 1, 2 * rows, 2 * rows + 7):
        for empties in (0, 3):
            parts = [text[:cut]] + [""] * empties + [text[cut:]]
            _, seqset = check_exact(pli, parts, [q], rows_per_stream=(0, 7))
            assert seqset.rows == rows
            cases += 1
    assert cases == 16
    check_exact(pli, [text[:rows], text[rows:2 * rows], "", text[2 * rows:]], [q], rows_per_stream=(7, 64))   # a record that IS a column


def test_repeated_calls_are_bit_identical(pli):
    """37 records of many lane runs each, random weights, lane runs of 1 and 7 rows: three calls give the same bytes; the
    tables of different run lengths add the same terms in another order and agree within 2^-20."""
    rng = np.random.default_rng(12)
    records = make_records(rng, 37, 5, rng.integers(300, 900, 37))
    pssms = [lm.ScoringMatrix(random_matrix(rng, m, 5, n_weight=-1.0)) for m in (4, 17, 36, 40)]
    seqset = pli.stripe_ascii_set(records, lossy=True)
    seqset.configure_wrap(40)
    tables = {}
    for rps in (1, 7):
        calls = [at_every_run_length(pli, lambda: pli.scan_sum_set(pssms, seqset), (rps,))[rps].sums for _ in range(3)]
        assert calls[0].tobytes() == calls[1].tobytes() == calls[2].tobytes(), rps
        assert (calls[0] > 0).all()
        tables[rps] = calls[0]
    assert close(tables[1], tables[7], 2.0 ** -20)


def test_non_finite_values_and_range(pli):
    rng = np.random.default_rng(13)
    p_nan = random_matrix(rng, 8, 5, n_weight=-1.0)                # (a) a NaN cell: windows with an A at offset 3 add nothing
    p_nan[3, 0] = np.nan
    p_pinf = random_matrix(rng, 8, 5, n_weight=-1.0)               # (b) a +inf cell: a record with a C at offset 2 of a window is +inf
    p_pinf[2, 1] = np.inf
    p_ninf = random_matrix(rng, 8, 5)                              # (c) -inf for N
    p_long = random_matrix(rng, 45, 5)                             # (d) longer than every record
    records = ["N" * 30, "ACGT" * 10, "A" * 25, "GGTGGTAGGTTTGGAGGATGAGT", "CCCAGGGTTT", "ANNNNNNNNNNNNNNNNNNNNN"]
    syms = [encode(r) for r in records]
    mats = [p_nan, p_pinf, p_ninf, p_long]
    want = sums_of(mats, syms)
    seqset = pli.stripe_ascii_set(records)
    seqset.configure_wrap(45)
    got = pli.scan_sum_set([lm.ScoringMatrix(p) for p in mats], seqset)
    assert close(got.sums, want), (got.sums.tolist(), want.tolist())
    assert got.sums[0, 2] == 0.0 and got.windows[0, 2] == 18       # every window NaN
    nan_windows = np.isnan(window_scores(p_nan, syms[1]))
    assert nan_windows.any() and not nan_windows.all() and 0 < got.sums[0, 1] < math.inf
    assert got.sums[1, 1] == math.inf and got.sums[1, 4] == math.inf and math.isfinite(got.sums[1, 3]) and got.sums[1, 3] > 0
    assert got.sums[2, 0] == 0.0 and got.sums[2, 5] == 0.0 and got.windows[2, 0] == 23   # only -inf windows
    assert not got.sums[3].any() and not got.windows[3].any()
    # |scale * score| up to about 1 000: far outside f32 exp2, inside a double
    up = np.zeros((8, lm_stride(5, 4)), np.float32)
    up[:, :5] = rng.uniform(1.0, 1.5, (8, 5))
    scale = np.float32(990.0 / max(window_scores(up, s).max() for s in syms if len(s) >= 8))
    for sign in (1.0, -1.0):
        mat = (sign * up).astype(np.float32)
        x = scale * np.concatenate([window_scores(mat, s) for s in syms if len(s) >= 8])
        assert 600 < np.abs(x).min() and 950 < np.abs(x).max() < 1_000
        want = sums_of([mat], syms, [scale])
        res = pli.scan_sum_set([lm.ScoringMatrix(mat)], seqset, scale=scale)
        cells = res.windows[0] > 0
        assert np.isfinite(res.sums).all() and (res.sums[0, cells] != 0).all() and close(res.sums, want), (sign, res.sums.tolist(), want.tolist())
        assert (res.log2()[0, cells] > 600).all() if sign > 0 else (res.log2()[0, cells] < -600).all()


@pytest.mark.parametrize("protein", [False, True], ids=["dna", "protein"])
def test_agrees_with_the_counts_and_best_hits_of_the_same_walk(pli, protein):
    """``sums > 0`` exactly where a window scores above -inf (``scan_count_set`` at the lowest finite f32), and
    ``max <= sum <= windows * max``: log2 of the sum lies between the best score and the best score plus log2 of the
    windows, the tolerance of the sum (2^-21 relative, 2^-20 in log2) on either side."""
    k = 21 if protein else 5
    rng = np.random.default_rng(4_200 + k)
    records = make_records(rng, 37, k, lengths_for(rng, 37))
    ms = (1, 4, 17, 36, 40)
    mats = [random_matrix(rng, m, k) for m in ms]
    for p in mats:
        p[:, :k - 1][rng.random((p.shape[0], k - 1)) < 0.03] = -np.inf
    pssms = [lm.ScoringMatrix(p, protein=protein) for p in mats]
    seqset = pli.stripe_ascii_set(records, protein=protein, lossy=True)
    seqset.configure_wrap(max(ms))
    lowest = np.finfo(np.float32).min
    for rps in (0, 7):
        pli.set_rows_per_stream(rps)
        try:
            s = pli.scan_sum_set(pssms, seqset)
            c = pli.scan_count_set(pssms, [[-np.inf, lowest]] * len(ms), seqset)
            b = pli.scan_best_set(pssms, seqset)
        finally:
            pli.set_rows_per_stream(0)
        above = c.counts[:, 1] > 0
        assert above.any() and not above.all() and (c.counts[:, 0] > c.counts[:, 1]).any()
        assert np.array_equal(s.sums > 0, above), rps
        assert np.array_equal(s.windows, c.windows)
        log2 = s.log2()
        top = b.score.astype(np.float64)
        assert np.all(log2[b.found] >= top[b.found] - 2.0 ** -20), rps
        assert np.all(log2[above] <= top[above] + np.log2(s.windows[above]) + 2.0 ** -20), rps
        assert not s.sums[~b.found].any()


def test_misuse_is_a_status(pli):
    rng = np.random.default_rng(1)
    records = make_records(rng, 5, 5, [100, 200, 150, 100, 200])
    seqset = pli.stripe_ascii_set(records, lossy=True)
    mat = random_matrix(rng, 20, 5, n_weight=-1.0)
    p20 = lm.ScoringMatrix(mat)
    with pytest.raises(lm.LightmotifHipError) as err:                      # no wrap rows yet
        pli.scan_sum_set([p20], seqset)
    assert err.value.status == _ffi.ERR_WRAP
    seqset.configure_wrap(19)
    good = pli.scan_sum_set([p20], seqset)
    assert good.shape == (1, 5) and close(good.sums, sums_of([mat], [symbols_of(r, 5) for r in records]))
    prot = lm.ScoringMatrix(random_matrix(rng, 8, 21), protein=True)
    with pytest.raises(ValueError):                                        # the Python layer refuses first
        pli.scan_sum_set([prot], seqset)
    L = _ffi.lib()
    sentinel = -7.25
    out = (C.c_double * 5)(*[sentinel] * 5)
    untouched = lambda: list(out) == [sentinel] * 5
    handles = (C.c_void_p * 1)(prot._device(pli))
    assert L.lm_hip_scan_sum_seqset(pli._h, handles, None, 1, seqset._h, out) == _ffi.ERR_BAD_ARGS and "alphabet" in _ffi.last_error()
    dna = (C.c_void_p * 1)(p20._device(pli))
    for bad in (0.0, -1.0, math.inf, -math.inf, math.nan):                 # a scale is finite and > 0
        assert L.lm_hip_scan_sum_seqset(pli._h, dna, (C.c_float * 1)(bad), 1, seqset._h, out) == _ffi.ERR_BAD_ARGS, bad
        assert "scale" in _ffi.last_error() and untouched()
        with pytest.raises(lm.LightmotifHipError):
            pli.scan_sum_set([p20], seqset, scale=bad)
    assert L.lm_hip_scan_sum_seqset(None, dna, None, 1, seqset._h, out) == _ffi.ERR_BAD_ARGS and _ffi.last_error()
    assert L.lm_hip_scan_sum_seqset(pli._h, None, None, 1, seqset._h, out) == _ffi.ERR_BAD_ARGS and _ffi.last_error()
    assert L.lm_hip_scan_sum_seqset(pli._h, dna, None, 1, None, out) == _ffi.ERR_BAD_ARGS and _ffi.last_error()
    assert L.lm_hip_scan_sum_seqset(pli._h, dna, None, 1, seqset._h, None) == _ffi.ERR_BAD_ARGS and _ffi.last_error()
    assert L.lm_hip_scan_sum_seqset(pli._h, None, None, 0, seqset._h, out) == _ffi.OK and untouched()       # n == 0: nothing written
    empty = pli.stripe_ascii_set([])
    empty.configure_wrap(19)
    assert L.lm_hip_scan_sum_seqset(pli._h, dna, None, 1, empty._h, out) == _ffi.OK and untouched()          # no records
    # the raw ABI with a scale array: the answer of the Python layer, bit for bit
    assert L.lm_hip_scan_sum_seqset(pli._h, dna, (C.c_float * 1)(0.5), 1, seqset._h, out) == _ffi.OK
    assert np.asarray(list(out)).tobytes() == pli.scan_sum_set([p20], seqset, scale=[0.5]).sums.tobytes()
    for bad in ([1.0, 1.0], np.ones((1, 1))):
        with pytest.raises(ValueError):
            pli.scan_sum_set([p20], seqset, scale=bad)
    assert pli.scan_sum_set([], seqset).shape == (0, 5)
    res = pli.scan_sum_set([p20], empty)
    assert res.shape == (1, 0) and res.windows.shape == (1, 0) and res.last_kernel == ""


MATRICES = (">MA0001.1\tFIRST\n"
            "A  [ 10 12  4  1  2  2  0  0 ]\n"
            "C  [  2  2  7  1  0  8  0  0 ]\n"
            "G  [  3  1  1  0 23  0 26 26 ]\n"
            "T  [ 11 11 14 24  1 16  0  0 ]\n"
            ">MA0002.1\tSECOND\n"
            "A  [ 20  0  0  5  9 ]\n"
            "C  [  0 20  0  5  1 ]\n"
            "G  [  0  0 20  5  1 ]\n"
            "T  [  0  0  0  5  9 ]\n")


@pytest.mark.parametrize("reverse", [False, True])
def test_cli_sum_odds(tmp_path, reverse):
    rng = np.random.default_rng(44)
    lengths = rng.integers(0, 300, 60)
    lengths[[3, 30, 31, 59]] = 0
    lengths[[7, 40]] = [4, 7]                                              # shorter than the shortest / the longest motif
    lengths[50] = 3_000                                                    # larger than the budget below
    seqs = [(f"rec{i}", "".join(rng.choice(list("ACGTN"), int(n), p=[0.24, 0.24, 0.24, 0.24, 0.04]))) for i, n in enumerate(lengths)]
    fasta = tmp_path / "records.fa"
    with open(fasta, "w") as fh:
        for name, s in seqs:
            fh.write(f">{name} test record\n")
            for i in range(0, len(s), 70):
                fh.write(s[i:i + 70] + "\n")
    mats = tmp_path / "motifs.pwm"
    mats.write_text(MATRICES)
    outs = []
    for budget in (2_000, None):
        out = tmp_path / f"sums_{budget}.tsv"
        argv = ["-m", str(mats), "-s", str(fasta), "-o", str(out), "--sum-odds"] + (["--reverse"] if reverse else [])
        assert scan_cli.main(argv + (["--batch-bases", str(budget)] if budget else [])) == 0
        outs.append(out.read_text())
    lines = outs[1].splitlines()
    assert lines[0].split("\t") == ["seq_index", "seq_name", "motif_index", "motif_name", "strand", "windows", "sum_odds", "log2_mean_odds"]
    with open(mats) as fh:
        motifs = list(lmio.read(fh))
    direct = [r.matrix.normalize(0.1).log_odds() for r in motifs]
    strands = [("+", direct)] + ([("-", [p.reverse_complement() for p in direct])] if reverse else [])
    got = iter(lines[1:])
    n_lines = 0
    for si, (name, s) in enumerate(seqs):
        for strand, pssms in strands:
            for mi, p in enumerate(pssms):
                if len(s) < len(p):
                    continue                                               # one line per (sequence, strand, motif) with a window
                f = next(got).split("\t")
                assert f[:6] == [str(si + 1), name, str(mi + 1), motifs[mi].id, strand, str(len(s) - len(p) + 1)]
                total, mean = float(f[6]), float(f[7])
                assert f[6] == repr(total) and f[7] == repr(mean)
                want = sum_of(window_scores(p.data, encode(s)))
                assert close([total], [want]), (f, want)
                assert mean == scan_cli.log2_mean_odds(total, len(s) - len(p) + 1)
                n_lines += 1
    assert next(got, None) is None and n_lines > 100
    # another cut of the file into sets: the same lines, the sums within the tolerance of a reordered addition
    other = outs[0].splitlines()
    assert len(other) == len(lines)
    for a, b in zip(other[1:], lines[1:]):
        fa, fb = a.split("\t"), b.split("\t")
        assert fa[:6] == fb[:6] and close([float(fa[6])], [float(fb[6])], 2.0 ** -20)
