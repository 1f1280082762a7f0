"""How many windows of every motif reach a cut-off in every record of a sequence set, in one call and without a hit list
(lm_hip_scan_count_seqset, csrc/seqset_count.hip): per (motif, level, record) the number of windows ``pos + M <= L`` (the
reference's scan.rs:185-190, per record) with ``score >= t`` in f32.  Expectations come from ``scan_threshold_set`` at the
same thresholds counted in numpy, from the CPU oracle, and from sums made on the host in the reference's add order."""
import ctypes as C
import gzip
import sys
from collections import Counter
from pathlib import Path

import numpy as np
import pytest

import lightmotif_amd as lm
from lightmotif_amd.lib import stride as lm_stride
from lightmotif_amd import _ffi, scan_cli
from seqset_best_cases import best_of, consensus_matrix, edge_records, encode, window_scores
from seqset_count_cases import count_of, counts_of

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
DNA, PROTEIN = np.frombuffer(b"ACTGN", dtype=np.uint8), np.frombuffer(b"ACDEFGHIKLMNPQRSTVWYX", dtype=np.uint8)
MOTIF_LENGTHS = (4, 12, 20, 33, 40, 70)
POOL = sorted({0, 1, 31, 32, 33} | {m + d for m in MOTIF_LENGTHS for d in (-1, 0, 1)})


def make_matrix(rng, m, k, neg_inf_cells=False, n_weight=-1.0):
    p = np.zeros((m, lm_stride(k, 4)), np.float32)
    p[:, :k] = rng.normal(0, 2, (m, k))
    p[:, k - 1] = -np.inf if neg_inf_cells else n_weight
    if neg_inf_cells:
        p[:, :k][rng.random((m, k)) < 0.05] = -np.inf
    return p


def make_records(rng, n, k, lengths_pool, long_share):
    """Record texts (uint8 arrays): 2 % N / X, lossy junk, a share of the lengths from 1 000 ... 20 000."""
    alphabet = DNA if k == 5 else PROTEIN
    out = []
    for _ in range(n):
        length = int(rng.integers(1_000, 20_001)) if rng.random() < long_share else int(rng.choice(lengths_pool))
        sym = rng.integers(0, k - 1, length)
        sym[rng.random(length) < 0.02] = k - 1
        text = alphabet[sym].copy()
        if length:
            text[rng.random(length) < 0.005] = ord("?")           # lossy: becomes the default symbol
        out.append(text)
    return out


def symbols_of(text, k):
    """The symbol indices of a record text as the lossy encoder gives them (unknown bytes: the default symbol)."""
    lut = np.full(256, k - 1, dtype=np.int64)
    lut[DNA if k == 5 else PROTEIN] = np.arange(k)
    return lut[np.asarray(text, dtype=np.uint8)]


def list_counts(res, n_records):
    """Per (motif, record) the number of entries of a ``SetHits``."""
    return np.stack([np.bincount(res[mi][0], minlength=n_records) for mi in range(len(res))]).astype(np.uint32).reshape(len(res), n_records)


def quantile_value(values, q):
    """The q-quantile of `values` as one of the values themselves, so that ``v == t`` occurs."""
    v = np.sort(values)
    return v[int(q * (len(v) - 1))]


@pytest.mark.parametrize("protein", [False, True], ids=["dna", "protein"])
@pytest.mark.parametrize("n_records", [1, 2, 37, 5_000])
def test_equals_the_list_route(pli, protein, n_records):
    """Both roads (fused kernels up to M = 36, the length-generic kernel beyond), offsets in LDS and (5 000 records) in
    global memory, records that span several workgroups and columns; three levels per motif, each an actual score."""
    k = 21 if protein else 5
    rng = np.random.default_rng(2_000 * n_records + k)
    long_share = {1: 1.0, 2: 0.5, 37: 0.4, 5_000: 0.01}[n_records]
    records = make_records(rng, n_records, k, POOL, long_share)
    mats = [make_matrix(rng, m, k, neg_inf_cells=(m == 20)) for m in MOTIF_LENGTHS]
    pssms = [lm.ScoringMatrix(p, protein=protein) for p in mats]
    seqset = pli.stripe_ascii_set(records, protein=protein, lossy=True)
    seqset.configure_wrap(max(MOTIF_LENGTHS))
    every = pli.scan_threshold_set(pssms, [-np.inf] * len(pssms), seqset)
    cuts = np.zeros((len(pssms), 3), dtype=np.float32)
    for mi in range(len(pssms)):
        finite = every[mi][2][np.isfinite(every[mi][2])]
        assert len(finite) > 100, mi
        cuts[mi] = [quantile_value(finite, q) for q in (0.5, 0.9, 0.99)]
    want = np.stack([list_counts(pli.scan_threshold_set(pssms, cuts[:, li], seqset), n_records) for li in range(3)], axis=1)
    first = pli.scan_count_set(pssms, cuts, seqset)
    assert first.last_kernel == "seqset_count_generic"              # the last group launched: M = 70
    assert first.counts.dtype == np.uint32 and first.shape == (len(pssms), 3, n_records)
    lengths = np.asarray([len(r) for r in records], dtype=np.int64)
    assert first.windows.dtype == np.int64
    assert np.array_equal(first.windows, np.maximum(0, lengths[None, :] - np.asarray(MOTIF_LENGTHS)[:, None] + 1))
    assert np.array_equal(first.counts, want), np.argwhere(first.counts != want)[:5]
    sums = [int(first.counts[:, li].sum(dtype=np.int64)) for li in range(3)]
    assert 0 < sums[2] < sums[1] < sums[0] < int(first.windows.sum()), (sums, int(first.windows.sum()))
    second = pli.scan_count_set(pssms, cuts, seqset)
    assert first.counts.tobytes() == second.counts.tobytes()
    pli.set_prefilter(False)
    try:
        third = pli.scan_count_set(pssms, cuts, seqset)
    finally:
        pli.set_prefilter(True)
    assert first.counts.tobytes() == third.counts.tobytes()
    one = pli.scan_count_set(pssms, cuts[:, 0], seqset)             # one level: level 0 of the three
    assert one.shape == (len(pssms), 1, n_records) and np.array_equal(one.counts[:, 0], first.counts[:, 0])
    short = pli.scan_count_set(pli.prepare_batch(pssms[:3]), cuts[:3], seqset)   # fused kernels alone, a MotifBatch
    assert short.last_kernel.startswith("seqset_count_fused<")
    assert short.counts.tobytes() == first.counts[:3].tobytes()


def test_against_the_oracle(pli, oracle):
    """300 records of 0-900 bp, 8 motifs of 5-30 rows, from ASCII and from encoded symbols; levels -inf, 0.0 and the
    per-motif 0.99 quantile of the oracle's scores."""
    co = oracle
    rng = np.random.default_rng(2025)
    n_records = 300
    lengths = rng.integers(0, 900, n_records)
    encs = [rng.integers(0, 4, int(n)).astype(np.uint8) for n in lengths]
    for e in encs:
        e[rng.random(len(e)) < 0.01] = 4
    ms = [5, 8, 10, 12, 15, 19, 24, 30]
    mats = [make_matrix(rng, m, 5) for m in ms]
    scores = {}
    for mi, p in enumerate(mats):
        for ri, e in enumerate(encs):
            if len(e) < p.shape[0]:
                scores[mi, ri] = np.zeros(0, np.float32)
                continue
            st = co.stripe(e, 32, 5)
            co.configure_wrap(st, 30)
            sc, _ = co.score_rows(st, p)
            scores[mi, ri] = sc[:, :32].T.reshape(-1)[: len(e) - p.shape[0] + 1].astype(np.float32)
    cuts = np.zeros((len(ms), 3), dtype=np.float32)
    want = np.zeros((len(ms), 3, n_records), dtype=np.uint32)
    for mi in range(len(ms)):
        cuts[mi] = [-np.inf, 0.0, quantile_value(np.concatenate([scores[mi, ri] for ri in range(n_records)]), 0.99)]
        for ri in range(n_records):
            want[mi, :, ri] = [count_of(scores[mi, ri], t) for t in cuts[mi]]
    windows = np.maximum(0, lengths[None, :] - np.asarray(ms)[:, None] + 1)
    assert np.array_equal(want[:, 0], windows)                      # no weight is NaN: every window counts at -inf
    assert want[:, 2].sum() > 500 and np.all(want[:, 2].sum(axis=1) < want[:, 1].sum(axis=1))
    pssms = [lm.ScoringMatrix(p) for p in mats]
    seqset = pli.stripe_ascii_set([DNA[e] for e in encs], lossy=False)
    seqset.configure_wrap(30)
    got = pli.scan_count_set(pssms, cuts, seqset)
    assert np.array_equal(got.counts, want), ("ascii", np.argwhere(got.counts != want)[:5])
    assert np.array_equal(got.windows, windows) and np.array_equal(got.counts[:, 0], got.windows)
    seqset2 = pli.stripe_set([lm.EncodedSequence(e) for e in encs])
    seqset2.configure_wrap(30)
    got2 = pli.scan_count_set(pli.prepare_batch(pssms), cuts, seqset2)
    assert np.array_equal(got2.counts, want), ("encoded", np.argwhere(got2.counts != want)[:5])


def test_planted_edges(pli):
    """N scores like a match, so padding and the neighbour's bases reach the full score wherever the cut is missing."""
    m = 12
    consensus, records, notes = edge_records(m=m)
    p = consensus_matrix(consensus, 2.0, lm_stride(5, 4))
    full = np.float32(2.0 * m)
    want = counts_of([p], [encode(r) for r in records], [[full]], window_scores)
    seqset = pli.stripe_ascii_set(records)
    seqset.configure_wrap(m)
    got = pli.scan_count_set([lm.ScoringMatrix(p)], [full], seqset)
    assert np.array_equal(got.counts, want), np.argwhere(got.counts != want)[:5]
    hits = got.counts[0, 0]
    for a, b in notes["split"]:                                    # a consensus across a junction counts in neither record
        assert hits[a] == 0 and hits[b] == 0, (a, b)
    twice = [r for r in notes["planted"] if records[r].count(consensus) == 2]
    assert len(twice) == 1
    for r in notes["planted"]:                                     # last base, first base, the record that is the motif, twice
        assert hits[r] == (2 if r in twice else 1), r
    assert hits[notes["empty"]] == 0 and got.windows[0, notes["empty"]] == 0
    assert hits[notes["repeat"]] == 0
    last = notes["last"]                                           # the window at 50 would reach 2m over the padding
    assert last == len(records) - 1 and hits[last] == 0
    assert hits.sum() == len(notes["planted"]) + 1


def test_junction_against_the_column_boundary(pli):
    """Two records of 32 * R symbols together, so the matrix has exactly R rows: the junction sweeps across the bottom of
    the first and of the second column, where a lane's run ends and its last windows read the next column's top."""
    rows, m = 40, 12
    rng = np.random.default_rng(77)
    p = make_matrix(rng, m, 5)
    pssm = lm.ScoringMatrix(p)
    text = DNA[rng.integers(0, 4, 32 * rows)]
    med = np.float32(np.median(window_scores(p, symbols_of(text, 5))))
    cases = 0
    for around in (rows, 2 * rows):
        for first in range(around - m, around + 2):
            parts = [text[:first], text[first:]]
            seqset = pli.stripe_ascii_set(parts)
            assert seqset.rows == rows
            seqset.configure_wrap(m)
            cuts = [[-np.inf, med]]
            want = counts_of([p], [symbols_of(t, 5) for t in parts], cuts, window_scores)
            got = pli.scan_count_set([pssm], cuts, seqset)
            assert np.array_equal(got.counts, want), (first, got.counts.tolist(), want.tolist())
            assert np.array_equal(got.counts[0, 0], got.windows[0]) and 0 < got.counts[0, 1].sum() < got.windows.sum()
            cases += 1
    assert cases == 2 * (m + 2)


@pytest.mark.parametrize("rows_per_stream", [1, 7, 64])
def test_short_lane_runs(pli, rows_per_stream):
    """Runs shorter than M, several records inside one run, a record that spans many runs: the atomics of many lanes meet
    in one cell."""
    rng = np.random.default_rng(900 + rows_per_stream)
    records = make_records(rng, 37, 5, POOL, 0.0) + make_records(rng, 5, 5, [100, 250, 300, 640, 900], 0.0)
    ms = (4, 20, 33, 40)
    mats = [make_matrix(rng, m, 5, neg_inf_cells=(m == 20)) for m in ms]
    syms = [symbols_of(r, 5) for r in records]
    cuts = np.zeros((len(ms), 3), dtype=np.float32)
    for mi, p in enumerate(mats):
        allv = np.concatenate([window_scores(p, s) for s in syms])
        cuts[mi] = [-np.inf, quantile_value(allv[np.isfinite(allv)], 0.5), quantile_value(allv[np.isfinite(allv)], 0.95)]
    want = counts_of(mats, syms, cuts, window_scores)
    assert 0 < want[:, 2].sum() < want[:, 1].sum() < want[:, 0].sum()
    seqset = pli.stripe_ascii_set(records, lossy=True)
    seqset.configure_wrap(max(ms))
    pli.set_rows_per_stream(rows_per_stream)
    try:
        got = pli.scan_count_set([lm.ScoringMatrix(p) for p in mats], cuts, seqset)
    finally:
        pli.set_rows_per_stream(0)
    assert np.array_equal(got.counts, want), np.argwhere(got.counts != want)[:5]


@pytest.mark.parametrize("protein", [False, True], ids=["dna", "protein"])
def test_counts_and_best_hits_of_one_walk_agree(pli, protein):
    """The two reductions of the one record walk (csrc/seqset_walk.hpp) on the same set, at lane runs of the default
    length, 1 and 7 rows.  Every expectation comes from the host's window scores, neither call predicts the other: at
    -inf a cell holds the record's non-NaN windows; at the motif's lowest record best a cell is >= 1 exactly where the
    record has a best hit; just above the motif's highest record best every cell is 0; the best hits are ``best_of``."""
    k = 21 if protein else 5
    rng = np.random.default_rng(4_100 + k)
    records = make_records(rng, 37, k, POOL, 0.0)
    ms = (1, 4, 17, 36, 40)
    mats = [make_matrix(rng, m, k, neg_inf_cells=(m == 17)) for m in ms]
    syms = [symbols_of(r, k) for r in records]
    scores = [[window_scores(p, s) for s in syms] for p in mats]
    bests = [[best_of(v) for v in row] for row in scores]
    found = np.asarray([[b[0] for b in row] for row in bests])
    assert found.any(axis=1).all() and not found.all()               # every motif fits somewhere, some record is too short
    cuts = np.zeros((len(ms), 3), dtype=np.float32)
    for mi, row in enumerate(bests):
        top = np.asarray([b[2] for b in row if b[0]], dtype=np.float32)
        cuts[mi] = [-np.inf, top.min(), np.nextafter(top.max(), np.float32(np.inf))]
    want = counts_of(mats, syms, cuts, window_scores)
    for mi, row in enumerate(scores):
        assert want[mi, 0].tolist() == [int(np.count_nonzero(~np.isnan(v))) for v in row]
        assert np.array_equal(want[mi, 1] >= 1, found[mi]) and not want[mi, 2].any()
    pssms = [lm.ScoringMatrix(p, protein=protein) for p in mats]
    seqset = pli.stripe_ascii_set(records, protein=protein, lossy=True)
    seqset.configure_wrap(max(ms))
    for rows_per_stream in (0, 1, 7):
        pli.set_rows_per_stream(rows_per_stream)
        try:
            b = pli.scan_best_set(pssms, seqset)
            c = pli.scan_count_set(pssms, cuts, seqset)
        finally:
            pli.set_rows_per_stream(0)
        assert np.array_equal(c.counts, want), (rows_per_stream, np.argwhere(c.counts != want)[:5])
        assert np.array_equal(c.counts[:, 1] >= 1, b.found) and not c.counts[:, 2].any(), rows_per_stream
        assert np.array_equal(b.found, found), rows_per_stream
        for mi, row in enumerate(bests):
            for ri, (ok, pos, score) in enumerate(row):
                if ok:
                    assert (int(b.position[mi, ri]), np.float32(b.score[mi, ri]).tobytes()) == (pos, score.tobytes()), (rows_per_stream, mi, ri)


def test_non_finite_values(pli):
    rng = np.random.default_rng(11)
    p_inf = make_matrix(rng, 8, 5, n_weight=-np.inf)               # (a) an -inf N column: those windows count at -inf only
    p_nan = make_matrix(rng, 8, 5)                                 # (b) a NaN cell: windows with an A at offset 3 count nowhere
    p_nan[3, 0] = np.nan
    p_long = make_matrix(rng, 45, 5)                               # (c) a motif longer than every record
    records = ["N" * 30, "ACGT" * 10, "A" * 25, "CGTCGTACGTTTGCAGCATCAGT", "CCCAGGGTTT", "ANNNNNNNNNNNNNNNNNNNNN"]
    syms = [encode(r) for r in records]
    mats = [p_inf, p_nan, p_long]
    cuts = np.asarray([[-np.inf, -1.0e30, np.nan, np.inf]] * 3, dtype=np.float32)
    want = counts_of(mats, syms, cuts, window_scores)
    seqset = pli.stripe_ascii_set(records)
    seqset.configure_wrap(45)
    got = pli.scan_count_set([lm.ScoringMatrix(p) for p in mats], cuts, seqset)
    assert got.shape == (3, 4, len(records))
    assert np.array_equal(got.counts, want), np.argwhere(got.counts != want)[:5]
    assert got.counts[0, 0, 0] == 23 and got.counts[0, 1, 0] == 0  # only -inf windows: at -inf all, at a finite cut none
    assert got.counts[0, 0, 5] == 15 and got.counts[0, 1, 5] == 0
    nan_windows = np.isnan(window_scores(p_nan, syms[1]))
    assert nan_windows.any() and not nan_windows.all()
    assert got.counts[1, 0, 1] == np.count_nonzero(~nan_windows) < got.windows[1, 1]   # NaN windows: not even at -inf
    assert got.counts[1, 0, 2] == 0 and got.windows[1, 2] == 18    # every window NaN
    assert not got.counts[:, 2].any() and not got.counts[:, 3].any()   # a NaN threshold, a +inf threshold
    assert not got.counts[2].any() and not got.windows[2].any()


def test_misuse_is_a_status(pli):
    rng = np.random.default_rng(1)
    records = make_records(rng, 5, 5, [100, 200], 0.0)
    seqset = pli.stripe_ascii_set(records, lossy=True)
    p20 = lm.ScoringMatrix(make_matrix(rng, 20, 5))
    with pytest.raises(lm.LightmotifHipError) as err:                      # no wrap rows yet
        pli.scan_count_set([p20], [0.0], seqset)
    assert err.value.status == _ffi.ERR_WRAP
    seqset.configure_wrap(19)
    assert pli.scan_count_set([p20], [0.0], seqset).shape == (1, 1, 5)
    prot = lm.ScoringMatrix(make_matrix(rng, 8, 21), protein=True)
    with pytest.raises(ValueError):                                        # the Python layer refuses first
        pli.scan_count_set([prot], [0.0], seqset)
    L = _ffi.lib()
    handles = (C.c_void_p * 1)(prot._device(pli))
    ts = (C.c_float * 5)(0.0, 0.0, 0.0, 0.0, 0.0)
    out = (C.c_uint32 * 25)()
    before = pli.last_scan_counts
    st = L.lm_hip_scan_count_seqset(pli._h, handles, ts, 1, 1, seqset._h, out)
    assert st == _ffi.ERR_BAD_ARGS and "alphabet" in _ffi.last_error()
    assert pli.last_scan_counts == before                                  # nothing ran
    dna = (C.c_void_p * 1)(p20._device(pli))
    for levels in (0, 5):
        assert L.lm_hip_scan_count_seqset(pli._h, dna, ts, levels, 1, seqset._h, out) == _ffi.ERR_BAD_ARGS
        assert "levels" in _ffi.last_error()
    assert L.lm_hip_scan_count_seqset(pli._h, dna, ts, 1, 1, None, out) == _ffi.ERR_BAD_ARGS and _ffi.last_error()
    assert L.lm_hip_scan_count_seqset(pli._h, dna, None, 1, 1, seqset._h, out) == _ffi.ERR_BAD_ARGS and _ffi.last_error()
    assert L.lm_hip_scan_count_seqset(pli._h, dna, ts, 1, 1, seqset._h, None) == _ffi.ERR_BAD_ARGS and _ffi.last_error()
    assert L.lm_hip_scan_count_seqset(pli._h, None, None, 1, 0, seqset._h, None) == _ffi.OK       # n == 0
    for bad in ([0.0, 0.0], np.zeros((1, 5)), np.zeros((1, 0)), np.zeros((1, 2, 2))):
        with pytest.raises(ValueError):
            pli.scan_count_set([p20], bad, seqset)
    assert pli.scan_count_set([], [], seqset).shape == (0, 1, 5)
    assert pli.scan_count_set([], np.zeros((0, 3)), seqset).shape == (0, 3, 5)
    empty = pli.stripe_ascii_set([])
    empty.configure_wrap(19)
    res = pli.scan_count_set([p20], [[0.0, 1.0]], empty)
    assert res.shape == (1, 2, 0) and res.windows.shape == (1, 0)


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
MOTIF_ROWS = (8, 5)


@pytest.mark.parametrize("reverse", [False, True])
def test_cli_counts(tmp_path, reverse):
    rng = np.random.default_rng(43)
    lengths = rng.integers(0, 300, 120)
    lengths[[3, 50, 51, 119]] = 0
    lengths[[7, 60]] = [4, 7]                                              # shorter than the shortest / the longest motif
    lengths[100] = 5_000                                                   # larger than the budget below
    seqs = [(f"rec{i}", "".join(rng.choice(list("ACGTN"), int(n), p=[0.24, 0.24, 0.24, 0.24, 0.04]))) for i, n in enumerate(lengths)]
    fasta = tmp_path / "records.fa.gz"
    with gzip.open(fasta, "wt") as fh:
        for name, s in seqs:
            fh.write(f">{name} test record\n")
            for i in range(0, len(s), 70):
                fh.write(s[i:i + 70] + "\n")
    mats = tmp_path / "motifs.pwm"
    mats.write_text(MATRICES)
    outs = {}
    for mode in ("counts", "hits"):
        for budget in (2_000, None):
            out = tmp_path / f"{mode}_{budget}.tsv"
            argv = ["-m", str(mats), "-s", str(fasta), "-o", str(out), "-P", "1e-3"] + (["--reverse"] if reverse else [])
            argv += ["--counts"] if mode == "counts" else []
            if budget:
                argv += ["--batch-bases", str(budget)]
            assert scan_cli.main(argv) == 0
            outs[mode, budget] = out.read_bytes()
    assert outs["counts", 2_000] == outs["counts", None] and outs["hits", 2_000] == outs["hits", None]

    listed = Counter()                                                     # (seq_index, motif_index, strand) -> lines of the hit list
    for line in outs["hits", None].decode().splitlines()[1:]:
        f = line.split("\t")
        listed[int(f[0]), int(f[2]), f[5]] += 1
    assert sum(listed.values()) > 50
    lines = outs["counts", None].decode().splitlines()
    assert lines[0].split("\t") == ["seq_index", "seq_name", "motif_index", "motif_name", "strand", "windows", "hits"]
    names = ("MA0001.1", "MA0002.1")
    want = []
    for si, (name, s) in enumerate(seqs):
        for strand in ("+", "-") if reverse else ("+",):
            for mi, m in enumerate(MOTIF_ROWS):
                if len(s) >= m:                                            # one line per (sequence, strand, motif) with a window
                    want.append((si + 1, name, mi + 1, names[mi], strand, len(s) - m + 1, listed[si + 1, mi + 1, strand]))
    got = [tuple(int(x) if i in (0, 2, 5, 6) else x for i, x in enumerate(l.split("\t"))) for l in lines[1:]]
    assert got == want
    assert sum(g[6] for g in got) == sum(listed.values())                  # no hit of the list is outside a counted line
    assert any(g[6] == 0 for g in got) and any(g[6] > 1 for g in got)


def test_the_count_route_beats_the_dense_list(pli):
    """2 000 records x 500 bp x 8 JASPAR motifs at p = 1e-1, the dense regime the route exists for: ``scan_count_set`` (B)
    against ``scan_threshold_set`` plus one bincount per motif (A), the cheapest way before; medians of 5 alternating runs
    after a warm-up, equal answers first.  The margin is 1 x: a new route that is not faster than the road it replaces
    should not exist.  The other p values, B / C (the price of counting over ``scan_best_set``) and the three-level line
    are printed, not asserted (profiles/seqset_count_bench.json holds the measured medians and the crossover)."""
    sys.path.insert(0, str(ROOT / "tools"))
    import seqset_bench
    res = seqset_bench.measure_count(pli, 2_000, 500, 8, runs=5, warmup=1)
    for row in res["sweep"]:
        a, b, c = row["ms"]["A"], row["ms"]["B"], row["ms"]["C"]
        print(f"p {row['p']:g}  hits {row['hits']}  A (list + bincount) median {a['median']:.3f} ms [{a['min']:.3f}, {a['max']:.3f}]  "
              f"B (scan_count_set) median {b['median']:.3f} ms [{b['min']:.3f}, {b['max']:.3f}]  C (scan_best_set) median "
              f"{c['median']:.3f} ms  A/B {row['A_over_B']:.2f}  B/C {row['B_over_C']:.2f}")
    three = res["three_levels"]
    print(f"three levels: A3 median {three['ms']['A3']['median']:.3f} ms  B3 median {three['ms']['B3']['median']:.3f} ms  "
          f"A3/B3 {three['A3_over_B3']:.2f}  crossover p {res['crossover_p']}  kernels {res['kernel']}")
    assert res["answers_equal"] and all(row["answers_equal"] for row in res["sweep"]) and three["answers_equal"]
    dense = res["sweep"][0]
    assert dense["p"] == 1e-1 and dense["hits"] > 100_000
    assert len(dense["ms"]["A"]["all"]) >= 5 and len(dense["ms"]["B"]["all"]) >= 5
    assert dense["ms"]["B"]["median"] < dense["ms"]["A"]["median"]
