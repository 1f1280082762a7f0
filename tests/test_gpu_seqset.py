"""Many motifs x many resident sequences in one call (lm_hip_scan_threshold_seqset, csrc/seqset.hip): the result must
equal, bit for bit, the per-record loop -- every record striped and scanned alone, cut at ``pos + M <= L``
(the reference's scan.rs:185-190) -- and the oracle's scores, whatever route the scans take."""
import ctypes as C
import gzip
import io
import statistics
import sys
from pathlib import Path

import numpy as np
import pytest

import lightmotif_amd as lm
from lightmotif_amd.lib import stride as lm_stride
from lightmotif_amd import _ffi, scan_cli
from seqset_rule import offsets_of, segment_rule

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
DNA, PROTEIN = np.frombuffer(b"ACTGN", dtype=np.uint8), np.frombuffer(b"ACDEFGHIKLMNPQRSTVWYX", dtype=np.uint8)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def make_matrix(rng, m, k, neg_inf_cells=False):
    p = np.zeros((m, lm_stride(k, 4)), np.float32)
    p[:, :k] = rng.normal(0, 2, (m, k))
    p[:, k - 1] = -np.inf if neg_inf_cells else -1.0
    if neg_inf_cells:
        p[:, :k][rng.random((m, k)) < 0.05] = -np.inf
    return p


def make_records(rng, n, k, lengths_pool, long_share, lossy_junk=True):
    """Record texts (uint8 arrays) with lengths drawn from the pool, a share of them from 1 000 ... 20 000."""
    alphabet = DNA if k == 5 else PROTEIN
    out = []
    for _ in range(n):
        length = int(rng.integers(1_000, 20_001)) if rng.random() < long_share else int(rng.choice(lengths_pool))
        sym = rng.integers(0, k - 1, length)
        sym[rng.random(length) < 0.02] = k - 1                    # N / X
        text = alphabet[sym].copy()
        if lossy_junk and length:
            text[rng.random(length) < 0.005] = ord("?")           # lossy: becomes the default symbol
        out.append(text)
    return out


def per_record_loop(pli, records, pssms, ts, protein, wrap):
    """The expectation: each record alone through the existing one-sequence batch, cut and sorted on the host."""
    batch = pli.prepare_batch(pssms, ts)
    acc = [([], [], []) for _ in pssms]
    for r, text in enumerate(records):
        if len(text) == 0:                                         # (no window, no hit)
            continue
        seq = pli.stripe_ascii(text, protein=protein, lossy=True)
        seq.configure_wrap(wrap)
        rows, length = seq.rows, len(seq)
        for mi, ((coords, values), p) in enumerate(zip(pli.scan_threshold_batch(batch, None, seq), pssms)):
            pos = coords[:, 1] * rows + coords[:, 0]
            keep = pos + len(p) <= length
            pos, values = pos[keep], values[keep]
            order = np.argsort(pos, kind="stable")
            acc[mi][0].append(np.full(len(pos), r, dtype=np.int64))
            acc[mi][1].append(pos[order].astype(np.int64))
            acc[mi][2].append(values[order])
    return [(np.concatenate(a), np.concatenate(b), np.concatenate(c).astype(np.float32)) if a else
            (np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.float32)) for a, b, c in acc]


def assert_same_lists(got, want, tag):
    assert len(got) == len(want)
    for mi, ((gr, gp, gs), (wr, wp, ws)) in enumerate(zip(got, want)):
        assert len(gr) == len(wr), (tag, mi, len(gr), len(wr))
        assert np.array_equal(gr, wr), (tag, mi, "records")
        assert np.array_equal(gp, wp), (tag, mi, "positions")
        assert np.array_equal(bits(gs), bits(ws)), (tag, mi, "scores")


def assert_ordered(res, tag):
    """Strictly ascending in (record, position) per motif; counts add up."""
    assert int(np.sum(res.counts)) == len(res.hits) == res.total, tag
    for mi in range(len(res)):
        rec, pos, _ = res[mi]
        assert len(rec) == int(res.counts[mi])
        if len(rec) > 1:
            dr, dp = np.diff(rec), np.diff(pos)
            assert np.all((dr > 0) | ((dr == 0) & (dp > 0))), (tag, mi)


MOTIF_LENGTHS = (4, 12, 20, 33, 40, 70)


def motif_list(rng, k, records):
    """Motifs of every length class with thresholds that reach every route: mid-range (prefilter / exact), -inf (dense
    list), NaN (no hit), a matrix with -inf weights."""
    mats, ts = [], []
    for i, m in enumerate(MOTIF_LENGTHS):
        mats.append(make_matrix(rng, m, k, neg_inf_cells=(m == 20)))
        best = float(np.sum(np.max(mats[-1][:, :k - 1], axis=1)))
        ts.append(0.45 * best if k == 5 else 0.3 * best)
    mats.append(make_matrix(rng, 12, k))
    ts.append(-np.inf)                                            # every valid window is a hit
    mats.append(make_matrix(rng, 8, k))
    ts.append(np.nan)
    mats.append(make_matrix(rng, 33, k))
    ts.append(0.0)
    return mats, ts


@pytest.mark.parametrize("protein", [False, True], ids=["dna", "protein"])
@pytest.mark.parametrize("n_records", [1, 2, 37, 5_000])
def test_equals_the_per_record_loop(pli, protein, n_records):
    k = 21 if protein else 5
    rng = np.random.default_rng(1_000 * n_records + k)
    pool = sorted({0, 1, 31, 32, 33} | {m + d for m in MOTIF_LENGTHS for d in (-1, 0, 1)})
    long_share = {1: 1.0, 2: 0.5, 37: 0.4, 5_000: 0.01}[n_records]
    records = make_records(rng, n_records, k, pool, long_share)
    mats, ts = motif_list(rng, k, records)
    pssms = [lm.ScoringMatrix(p, protein=protein) for p in mats]
    wrap = max(MOTIF_LENGTHS)
    seqset = pli.stripe_ascii_set(records, protein=protein, lossy=True)
    assert len(seqset) == n_records and seqset.lengths.tolist() == [len(r) for r in records]
    assert seqset.total_length == sum(len(r) for r in records) and seqset.protein == protein
    seqset.configure_wrap(wrap)
    assert seqset.wrap == wrap
    want = per_record_loop(pli, records, pssms, ts, protein, wrap)
    assert sum(len(w[0]) for w in want) > 0
    for tag in ("first call", "second call (ordering sized from the first)"):
        res = pli.scan_threshold_set(pssms, ts, seqset)
        assert_ordered(res, tag)
        assert_same_lists([res[i] for i in range(len(res))], want, (tag, protein, n_records))
    pli.set_prefilter(False)
    try:
        res = pli.scan_threshold_set(pssms, ts, seqset)
    finally:
        pli.set_prefilter(True)
    assert_same_lists([res[i] for i in range(len(res))], want, ("prefilter off", protein, n_records))


def test_long_list_takes_the_radix_sort_road(pli):
    """More hits than hits.hip's kSortFrom (2^17): the list is radix-sorted, speculatively on the second call."""
    rng = np.random.default_rng(77)
    records = make_records(rng, 400, 5, [0, 3, 11, 12, 13, 500, 1_500], 0.02)
    mats = [make_matrix(rng, 12, 5), make_matrix(rng, 4, 5), make_matrix(rng, 20, 5)]
    ts = [-np.inf, -np.inf, 1.0]
    pssms = [lm.ScoringMatrix(p) for p in mats]
    seqset = pli.stripe_ascii_set(records, lossy=True)
    seqset.configure_wrap(20)
    want = per_record_loop(pli, records, pssms, ts, False, 20)
    assert sum(len(w[0]) for w in want) > (1 << 17)
    for tag in ("exact form", "speculative form"):
        res = pli.scan_threshold_set(pssms, ts, seqset)
        assert_ordered(res, tag)
        assert_same_lists([res[i] for i in range(len(res))], want, tag)
    pli.set_option("sort_hits", 0)                                # the same list through the bucket passes
    try:
        res = pli.scan_threshold_set(pssms, ts, seqset)
    finally:
        pli.set_option("sort_hits", 1)
    assert_same_lists([res[i] for i in range(len(res))], want, "bucket passes")


def test_against_the_oracle(pli, oracle):
    co = oracle
    rng = np.random.default_rng(2024)
    n_records, n_motifs = 300, 8
    lengths = rng.integers(0, 900, n_records)
    encs = [rng.integers(0, 4, int(n)).astype(np.uint8) for n in lengths]
    for e in encs:
        e[rng.random(len(e)) < 0.01] = 4
    ms = [5, 8, 10, 12, 15, 19, 24, 30]
    mats = [make_matrix(rng, m, 5) for m in ms]
    scores = []                                                   # per motif, per record: scores by position (valid windows)
    for p in mats:
        per = []
        for e in encs:
            if len(e) < p.shape[0]:
                per.append(np.zeros(0, np.float32))
                continue
            st = co.stripe(e, 32, 5)
            co.configure_wrap(st, 30)
            sc, _ = co.score_rows(st, p)
            per.append(sc[:, :32].T.reshape(-1)[: len(e) - p.shape[0] + 1].copy())
        scores.append(per)
    # thresholds picked on the CPU: the 250 best windows of every motif (ties included)
    ts = [float(np.sort(np.concatenate(per))[-250]) for per in scores]
    want = []
    for per, t in zip(scores, ts):
        rec = np.concatenate([np.full(int(np.sum(s >= t)), r, np.int64) for r, s in enumerate(per)])
        pos = np.concatenate([np.nonzero(s >= t)[0].astype(np.int64) for s in per])
        val = np.concatenate([s[s >= t] for s in per]).astype(np.float32)
        want.append((rec, pos, val))
    assert sum(len(w[0]) for w in want) >= 1_000
    texts = [DNA[e] for e in encs]
    seqset = pli.stripe_ascii_set(texts, lossy=False)
    seqset.configure_wrap(30)
    res = pli.scan_threshold_set([lm.ScoringMatrix(p) for p in mats], ts, seqset)
    assert_ordered(res, "oracle")
    assert_same_lists([res[i] for i in range(len(res))], want, "oracle")
    # the same records from encoded symbols
    seqset2 = pli.stripe_set([lm.EncodedSequence(e) for e in encs])
    seqset2.configure_wrap(30)
    res2 = pli.scan_threshold_set([lm.ScoringMatrix(p) for p in mats], ts, seqset2)
    assert_same_lists([res2[i] for i in range(len(res2))], want, "oracle, encoded")


def consensus_matrix(consensus, n_weight):
    m = len(consensus)
    p = np.full((m, lm_stride(5, 4)), 0, np.float32)
    p[:, :4] = -2.0
    p[:, 4] = n_weight
    for j, c in enumerate(consensus):
        p[j, "ACTG".index(c)] = 2.0
    return p


def test_straddlers_are_dropped_and_edge_windows_kept(pli):
    rng = np.random.default_rng(3)
    m = 12
    consensus = "".join(rng.choice(list("ACGT"), m))
    assert all(consensus[:i] != consensus[-i:] for i in range(1, m))      # no self-overlap: a plant is one hit
    bg = lambda n: "".join(rng.choice(list("ACGT"), n))
    records, planted, absent = [], [], []
    for split in range(1, m):                                             # (a) across a junction, every split
        records.append(bg(40) + consensus[:split])
        absent.append((len(records) - 1, 40))
        records.append(consensus[split:] + bg(25))
    records.append(bg(33) + consensus)                                    # (b) ends on the last base of a record
    planted.append((len(records) - 1, 33))
    records.append(consensus + bg(17))                                    # (c) starts on the first base of a record
    planted.append((len(records) - 1, 0))
    records.append("")                                                    # an empty record between
    records.append(consensus)                                             # a record that IS the motif
    planted.append((len(records) - 1, 0))
    records.append(bg(50) + consensus[: m - 3])                           # (d) the window runs into the rows behind the end
    absent.append((len(records) - 1, 50))
    # N scores like a match, so the window of (d) over the padding behind the last record reaches the threshold as well
    p = lm.ScoringMatrix(consensus_matrix(consensus, 2.0))
    t = float(2.0 * m)
    want = sorted((r, q) for r, text in enumerate(records) for q in range(len(text) - m + 1) if text[q:q + m] == consensus)
    assert set(planted) <= set(want) and not set(absent) & set(want)
    seqset = pli.stripe_ascii_set(records)
    seqset.configure_wrap(m)
    res = pli.scan_threshold_set([p], [t], seqset)
    rec, pos, score = res[0]
    got = list(zip(rec.tolist(), pos.tolist()))
    assert got == want
    assert np.all(score == np.float32(t))
    for hit in planted:
        assert hit in got
    for hit in absent:
        assert hit not in got
    # the plain concatenation through the existing API holds strictly more: the cut had something to remove
    joined = "".join(records)
    seq = pli.stripe_ascii(joined)
    seq.configure_wrap(m)
    (coords, _), = pli.scan_threshold_batch([p], [t], seq)
    plain = np.sort(coords[:, 1] * seq.rows + coords[:, 0])
    assert len(plain) >= len(got) + (m - 1) + 1
    offs = offsets_of([len(r) for r in records])
    prec, plocal, keep = segment_rule(offs, plain, m)
    assert list(zip(prec[keep].tolist(), plocal[keep].tolist())) == got
    assert int(offs[-1]) - (m - 3) in plain.tolist() and not keep[plain.tolist().index(int(offs[-1]) - (m - 3))]


def test_a_motif_longer_than_every_record_has_no_hits(pli):
    rng = np.random.default_rng(9)
    records = make_records(rng, 60, 5, [0, 5, 20, 39, 40, 41, 60], 0.0)
    mats = [make_matrix(rng, 12, 5), make_matrix(rng, 70, 5), make_matrix(rng, 4, 5), make_matrix(rng, 61, 5)]
    ts = [-np.inf, -np.inf, 0.5, -np.inf]
    pssms = [lm.ScoringMatrix(p) for p in mats]
    seqset = pli.stripe_ascii_set(records, lossy=True)
    seqset.configure_wrap(70)
    res = pli.scan_threshold_set(pssms, ts, seqset)
    assert_ordered(res, "long motif")
    assert res.counts[1] == 0 and res.counts[3] == 0
    assert res.counts[0] == sum(max(len(r) - 12 + 1, 0) for r in records)         # -inf: every valid window
    assert_same_lists([res[i] for i in range(4)], per_record_loop(pli, records, pssms, ts, False, 70), "long motif")


def test_offsets_beyond_32_bits(pli):
    """A set of ~4.5 Gbp from a repeated random block: coordinates of planted hits in the first and the last record, and
    every reported hit checked against the text and the rule."""
    m = 16
    rng = np.random.default_rng(5)
    consensus = "".join(rng.choice(list("ACGT"), m))
    cons = np.frombuffer(consensus.encode(), dtype=np.uint8)
    block = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 1 << 20)]
    n_blocks = 4_300
    try:
        text = np.tile(block, n_blocks)
    except MemoryError:
        pytest.skip("the host cannot hold a 4.5 GB text")
    total = text.size
    assert total > (1 << 32)
    n_records = 90
    cuts = np.sort(rng.integers(1, total, n_records - 1).astype(np.uint64))
    offs = np.concatenate(([0], cuts, [total])).astype(np.uint64)
    first_pos, last_local = 1_234, int(offs[-1] - offs[-2]) - m          # the last window of the last record
    text[first_pos:first_pos + m] = cons
    text[int(offs[-2]) + last_local:int(offs[-2]) + last_local + m] = cons
    mid = int(offs[45])                                                   # and one across a junction: must not be reported
    text[mid - 5:mid - 5 + m] = cons
    try:
        seqset = pli.stripe_ascii_set(text, offsets=offs)
    except lm.LightmotifHipError as exc:
        if exc.status == _ffi.ERR_OOM:
            pytest.skip(f"the device cannot hold the set: {exc.message}")
        raise
    seqset.configure_wrap(m)
    assert seqset.total_length == total and len(seqset) == n_records
    res = pli.scan_threshold_set([lm.ScoringMatrix(consensus_matrix(consensus, -2.0))], [float(2.0 * m)], seqset)
    rec, pos, score = res[0]
    assert_ordered(res, "4.5 Gbp")
    got = list(zip(rec.tolist(), pos.tolist()))
    assert (0, first_pos) in got and (n_records - 1, last_local) in got
    glob = offs[rec] + pos.astype(np.uint64)
    assert int(glob.max()) > (1 << 32)
    prec, plocal, keep = segment_rule(offs, glob, m)
    assert keep.all() and np.array_equal(prec, rec) and np.array_equal(plocal, pos)
    assert mid - 5 not in glob.tolist()
    for g in glob.tolist():
        assert text[g:g + m].tobytes() == cons.tobytes()
    assert np.all(score == np.float32(2.0 * m))


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
def test_cli_over_many_sets(tmp_path, oracle, reverse):
    co = oracle
    rng = np.random.default_rng(41)
    lengths = rng.integers(0, 400, 300)
    lengths[[3, 50, 51, 299]] = 0                                          # empty records
    lengths[[7, 120]] = [4, 7]                                             # shorter than the shortest / the longest motif
    lengths[200] = 9_000                                                   # larger than the budget below
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
    for budget in (2_000, None):
        out = tmp_path / f"hits_{budget}.tsv"
        argv = ["-m", str(mats), "-s", str(fasta), "-o", str(out), "-P", "1e-3"] + (["--reverse"] if reverse else [])
        if budget:
            argv += ["--batch-bases", str(budget)]
        assert scan_cli.main(argv) == 0
        outs[budget] = out.read_bytes()
    assert len(scan_cli.batch_records([len(s) for _, s in seqs], 2_000)) > 10
    assert outs[2_000] == outs[None]                                       # byte for byte, whatever the sets

    records = list(lm.io.read(io.StringIO(MATRICES)))
    direct = [r.matrix.normalize(0.1).log_odds() for r in records]
    want = []
    for si, (name, s) in enumerate(seqs):
        enc = lm.EncodedSequence(s, lossy=True).data
        for strand in ("+", "-") if reverse else ("+",):
            for mi, p in enumerate(direct):
                if len(s) < len(p):
                    continue
                q = p if strand == "+" else p.reverse_complement()
                t = np.float32(p.score_for_pvalue(1e-3))
                st = co.stripe(enc, 32, 5)
                co.configure_wrap(st, 8)
                scores, _ = co.score_rows(st, q.data)
                by_pos = scores[:, :32].T.reshape(-1)[: len(s) - len(p) + 1]
                for pos in np.nonzero(by_pos >= t)[0]:
                    want.append((si + 1, name, mi + 1, records[mi].id, int(pos), strand,
                                 scan_cli._fmt_score(by_pos[pos]),
                                 scan_cli._fmt_exp(p.score_distribution.pvalue(float(by_pos[pos])))))
    lines = outs[2_000].decode().splitlines()
    assert lines[0].split("\t") == ["seq_index", "seq_name", "motif_index", "motif_name", "pos", "strand", "score", "pvalue"]
    got = [tuple(int(x) if i in (0, 2, 4) else x for i, x in enumerate(l.split("\t"))) for l in lines[1:]]
    assert len(want) > 100
    assert got == want


def test_misuse_is_a_status(pli):
    rng = np.random.default_rng(1)
    records = make_records(rng, 5, 5, [100, 200], 0.0)
    seqset = pli.stripe_ascii_set(records, lossy=True)
    p20 = lm.ScoringMatrix(make_matrix(rng, 20, 5))
    with pytest.raises(lm.LightmotifHipError) as err:                      # no wrap rows yet
        pli.scan_threshold_set([p20], [0.0], seqset)
    assert err.value.status == _ffi.ERR_WRAP
    seqset.configure_wrap(19)
    assert pli.scan_threshold_set([p20], [0.0], seqset).total >= 0
    prot = lm.ScoringMatrix(make_matrix(rng, 8, 21), protein=True)
    with pytest.raises(ValueError):                                        # the Python layer refuses first
        pli.scan_threshold_set([prot], [0.0], seqset)
    L = _ffi.lib()
    handles = (C.c_void_p * 1)(prot._device(pli))
    t = (C.c_float * 1)(0.0)
    counts = (C.c_size_t * 1)()
    hits = C.POINTER(_ffi.SetHit)()
    before = pli.last_scan_counts
    st = L.lm_hip_scan_threshold_seqset(pli._h, handles, t, 1, seqset._h, counts, C.byref(hits))
    assert st == _ffi.ERR_BAD_ARGS and "alphabet" in _ffi.last_error()
    assert pli.last_scan_counts == before                                  # nothing ran
    st = L.lm_hip_scan_threshold_seqset(pli._h, handles, t, 1, None, counts, C.byref(hits))
    assert st == _ffi.ERR_BAD_ARGS and _ffi.last_error()
    with pytest.raises(lm.InvalidSymbol) as bad:                           # strict mode names the record
        pli.stripe_ascii_set(["ACGT", "", "ACGTAC?T", "AC"])
    assert "sequence 2 at position 6" in str(bad.value)


def test_a_set_without_records_keeps_its_alphabet(pli):
    """An empty list of encoded records says nothing about its alphabet: ``stripe_set(..., protein=True)`` names it, and
    the empty protein set then takes protein motifs like the empty sets of the other two builders (seeds 17 and 32 of
    tests/test_gpu_seqset_fuzz.py are such sets; without the argument the encoded builder made a DNA set of them)."""
    rng = np.random.default_rng(13)
    prot = lm.ScoringMatrix(make_matrix(rng, 8, 21), protein=True)
    sets = [pli.stripe_set([], protein=True), pli.stripe_ascii_set([], protein=True), pli.stripe_fasta_set(b"", protein=True)]
    for s in sets:
        s.configure_wrap(7)
        assert s.protein and len(s) == 0 and s.total_length == 0 and s.rows == 0 and s._info()[5] == 21
        res = pli.scan_threshold_set([prot], [-np.inf], s)
        assert res.total == 0 and res.counts.tolist() == [0]
        assert pli.scan_best_set([prot], s).found.shape == (1, 0)
    assert not pli.stripe_set([]).protein                                  # DNA when nothing is said
    with pytest.raises(ValueError):                                        # records of the other alphabet
        pli.stripe_set([lm.EncodedSequence(np.zeros(4, np.uint8))], protein=True)
    one = pli.stripe_set([lm.EncodedSequence(np.zeros(9, np.uint8), protein=True)], protein=True)
    assert one.protein and one.lengths.tolist() == [9]


def test_the_set_beats_the_per_record_loop(pli):
    """2 000 records x 500 bp x 64 JASPAR motifs at p = 1e-5: one resident set + one call (B) against the loop of 2 000
    synchronising calls it replaces (A), medians of 5 alternating runs after a warm-up.  The margin is 1 x: anything not
    faster means the set path has no reason to exist (the measured ratio is in profiles/seqset_bench.json)."""
    sys.path.insert(0, str(ROOT / "tools"))
    import seqset_bench
    res = seqset_bench.measure(pli, 2_000, 500, 64, runs=5, warmup=1)
    a, b = res["ms"]["A"], res["ms"]["B"]
    print(f"A (loop) median {a['median']:.2f} ms [{a['min']:.2f}, {a['max']:.2f}]  B (set) median {b['median']:.2f} ms "
          f"[{b['min']:.2f}, {b['max']:.2f}]  A/B {res['A_over_B']:.1f}  B/C {res['B_over_C']:.2f}  hits {res['hits']}")
    assert len(a["all"]) >= 5 and len(b["all"]) >= 5
    assert res["hits"]["A"] == res["hits"]["B"] > 0
    assert b["median"] < a["median"]
