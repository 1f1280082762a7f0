"""The best window of every motif in every record of a sequence set in one call (lm_hip_scan_best_seqset,
csrc/seqset_best.hip): per (motif, record) the greatest exact f32 score over the windows ``pos + M <= L`` (the
reference's scan.rs:185-190, per record) and the lowest position holding it.  Expectations come (E1) from
``scan_threshold_set`` at thresholds of -inf reduced in numpy, (E2) from the CPU oracle, and from sums made on the host
in the reference's add order; scores compare as bit patterns."""
import ctypes as C
import gzip
import io
import sys
from pathlib import Path

import numpy as np
import pytest

import lightmotif_amd as lm
from lightmotif_amd.lib import stride as lm_stride
from lightmotif_amd import _ffi, scan_cli
from seqset_best_cases import best_of, consensus_matrix, edge_records, encode, window_scores

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
DNA, PROTEIN = np.frombuffer(b"ACTGN", dtype=np.uint8), np.frombuffer(b"ACDEFGHIKLMNPQRSTVWYX", dtype=np.uint8)
MOTIF_LENGTHS = (4, 12, 20, 33, 40, 70)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


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


def reduce_e1(res, n_records):
    """E1: (found, position, score) of shape (motifs, records) from the list of every window: per record the greatest
    score and the first of those in list order (NaN windows, if the list holds any, do not compete)."""
    n = len(res)
    found = np.zeros((n, n_records), dtype=bool)
    position = np.full((n, n_records), -1, dtype=np.int64)
    score = np.full((n, n_records), np.nan, dtype=np.float32)
    for mi in range(n):
        rec, pos, val = res[mi]
        keep = ~np.isnan(val)
        rec, pos, val = rec[keep], pos[keep], val[keep]
        if not len(rec):
            continue
        order = np.lexsort((pos, -val.astype(np.float64), rec))   # by record, then score descending, then position
        rec, pos, val = rec[order], pos[order], val[order]
        first = np.flatnonzero(np.concatenate(([True], rec[1:] != rec[:-1])))
        found[mi, rec[first]] = True
        position[mi, rec[first]] = pos[first]
        score[mi, rec[first]] = val[first]
    return found, position, score


def assert_same(got, want, tag):
    found, position, score = want
    assert got.found.shape == found.shape, tag
    assert got.found.dtype == np.bool_ and got.position.dtype == np.int64 and got.score.dtype == np.float32
    assert np.array_equal(got.found, found), (tag, "found", np.argwhere(got.found != found)[:5])
    assert np.array_equal(got.position, position), (tag, "position", np.argwhere(got.position != position)[:5])
    assert np.array_equal(bits(got.score)[found], bits(score)[found]), (tag, "scores")
    assert np.all(np.isnan(got.score[~found])) and np.all(got.position[~found] == -1), tag


def brute_force(mats, records_sym):
    """(found, position, score) from sums made on the host in the reference's add order."""
    n, r = len(mats), len(records_sym)
    found = np.zeros((n, r), dtype=bool)
    position = np.full((n, r), -1, dtype=np.int64)
    score = np.full((n, r), np.nan, dtype=np.float32)
    for mi, p in enumerate(mats):
        for ri, sym in enumerate(records_sym):
            found[mi, ri], position[mi, ri], score[mi, ri] = best_of(window_scores(p, sym))
    return found, position, score


@pytest.mark.parametrize("protein", [False, True], ids=["dna", "protein"])
@pytest.mark.parametrize("n_records", [1, 2, 37, 5_000])
def test_equals_the_reduced_list_of_every_window(pli, protein, n_records):
    """E1, both roads (fused kernels up to M = 36, the length-generic kernel beyond), offsets in LDS and (5 000 records)
    in global memory, records that span several workgroups and columns."""
    k = 21 if protein else 5
    rng = np.random.default_rng(2_000 * n_records + k)
    pool = sorted({0, 1, 31, 32, 33} | {m + d for m in MOTIF_LENGTHS for d in (-1, 0, 1)})
    long_share = {1: 1.0, 2: 0.5, 37: 0.4, 5_000: 0.01}[n_records]
    records = make_records(rng, n_records, k, pool, long_share)
    mats = [make_matrix(rng, m, k, neg_inf_cells=(m == 20)) for m in MOTIF_LENGTHS]
    pssms = [lm.ScoringMatrix(p, protein=protein) for p in mats]
    seqset = pli.stripe_ascii_set(records, protein=protein, lossy=True)
    seqset.configure_wrap(max(MOTIF_LENGTHS))
    want = reduce_e1(pli.scan_threshold_set(pssms, [-np.inf] * len(pssms), seqset), n_records)
    lengths = np.asarray([len(r) for r in records])
    for mi, m in enumerate(MOTIF_LENGTHS):                          # a record has a window or it does not
        assert np.array_equal(want[0][mi], lengths >= m), m
    assert want[0].sum() > 0
    first = pli.scan_best_set(pssms, seqset)
    assert first.last_kernel == "seqset_best_generic"               # the last group launched: M = 70
    assert_same(first, want, ("first call", protein, n_records))
    second = pli.scan_best_set(pssms, seqset)
    assert first.raw.tobytes() == second.raw.tobytes()
    pli.set_prefilter(False)
    try:
        third = pli.scan_best_set(pssms, seqset)
    finally:
        pli.set_prefilter(True)
    assert first.raw.tobytes() == third.raw.tobytes()
    short = pli.scan_best_set(pssms[:3], seqset)                    # fused kernels alone
    assert short.last_kernel.startswith("seqset_best_fused<")
    assert short.raw.tobytes() == first.raw[:3].tobytes()


def test_against_the_oracle(pli, oracle):
    """E2: 300 records of 0-900 bp, 8 motifs of 5-30 rows, from ASCII and from encoded symbols."""
    co = oracle
    rng = np.random.default_rng(2025)
    n_records = 300
    lengths = rng.integers(0, 900, n_records)
    encs = [rng.integers(0, 4, int(n)).astype(np.uint8) for n in lengths]
    for e in encs:
        e[rng.random(len(e)) < 0.01] = 4
    ms = [5, 8, 10, 12, 15, 19, 24, 30]
    mats = [make_matrix(rng, m, 5) for m in ms]
    found = np.zeros((len(ms), n_records), dtype=bool)
    position = np.full((len(ms), n_records), -1, dtype=np.int64)
    score = np.full((len(ms), n_records), np.nan, dtype=np.float32)
    for mi, p in enumerate(mats):
        for ri, e in enumerate(encs):
            if len(e) < p.shape[0]:
                continue
            st = co.stripe(e, 32, 5)
            co.configure_wrap(st, 30)
            sc, _ = co.score_rows(st, p)
            by_pos = sc[:, :32].T.reshape(-1)[: len(e) - p.shape[0] + 1]
            found[mi, ri], position[mi, ri], score[mi, ri] = best_of(by_pos)
    assert found.sum() > 2_000
    pssms = [lm.ScoringMatrix(p) for p in mats]
    seqset = pli.stripe_ascii_set([DNA[e] for e in encs], lossy=False)
    seqset.configure_wrap(30)
    assert_same(pli.scan_best_set(pssms, seqset), (found, position, score), "oracle, ascii")
    seqset2 = pli.stripe_set([lm.EncodedSequence(e) for e in encs])
    seqset2.configure_wrap(30)
    assert_same(pli.scan_best_set(pli.prepare_batch(pssms), seqset2), (found, position, score), "oracle, encoded")


def test_planted_edges(pli):
    """N scores like a match, so padding and the neighbour's bases can win wherever the cut is missing."""
    m = 12
    consensus, records, notes = edge_records(m=m)
    p = consensus_matrix(consensus, 2.0, lm_stride(5, 4))
    full = np.float32(2.0 * m)
    want = brute_force([p], [encode(r) for r in records])
    seqset = pli.stripe_ascii_set(records)
    seqset.configure_wrap(m)
    got = pli.scan_best_set([lm.ScoringMatrix(p)], seqset)
    assert_same(got, want, "edges")
    for a, b in notes["split"]:                                    # a consensus across a junction wins neither record
        assert got.found[0, a] and got.found[0, b] and got.score[0, a] < full and got.score[0, b] < full
    for r, pos in notes["planted"].items():                        # last base, first base, the record that is the motif, twice
        assert got.found[0, r] and got.position[0, r] == pos and got.score[0, r] == full, (r, pos)
    e = notes["empty"]
    assert not got.found[0, e] and got.position[0, e] == -1 and np.isnan(got.score[0, e])
    assert got.found[0, e - 1] and got.found[0, e + 1]
    r = notes["repeat"]
    assert got.found[0, r] and got.position[0, r] == 0
    last = notes["last"]                                           # the window at 50 would reach 2m over the padding
    assert last == len(records) - 1 and got.found[0, last] and got.score[0, last] < full
    assert got.raw["position"][0, e] == 0 and got.raw["found"][0, e] == 0   # the C ABI's form of "none"


def test_non_finite_values(pli):
    rng = np.random.default_rng(11)
    # (a) a record of only N under an -inf N column: found, -inf, position 0
    p_inf = make_matrix(rng, 8, 5, n_weight=-np.inf)
    # (b) a NaN cell: windows with an A at offset 3 are NaN and do not compete
    p_nan = make_matrix(rng, 8, 5)
    p_nan[3, 0] = np.nan
    # (c) a motif longer than every record
    p_long = make_matrix(rng, 45, 5)
    records = ["N" * 30, "ACGT" * 10, "A" * 25, "CGTCGTACGTTTGCAGCATCAGT", "CCCAGGGTTT", "ANNNNNNNNNNNNNNNNNNNNN"]
    syms = [encode(r) for r in records]
    mats = [p_inf, p_nan, p_long]
    want = brute_force(mats, syms)
    seqset = pli.stripe_ascii_set(records)
    seqset.configure_wrap(45)
    got = pli.scan_best_set([lm.ScoringMatrix(p) for p in mats], seqset)
    assert_same(got, want, "non-finite")
    assert got.found[0, 0] and got.position[0, 0] == 0 and got.score[0, 0] == -np.inf
    assert got.found[1, 1] and not np.isnan(got.score[1, 1])      # some windows NaN, the others compete
    assert np.isnan(window_scores(p_nan, syms[1])).any()
    assert not got.found[1, 2] and np.isnan(got.score[1, 2]) and got.position[1, 2] == -1   # every window NaN
    assert not got.found[2].any() and np.all(got.position[2] == -1)


def test_agrees_with_argmax_where_it_must(pli):
    """Where the maximum over the valid windows is unique and the N column is -inf, Maximum::argmax of the record striped
    alone finds the same cell: position = col * rows + row, same score bits."""
    rng = np.random.default_rng(21)
    ms = [6, 11, 20, 31]
    mats = [make_matrix(rng, m, 5, n_weight=-np.inf) for m in ms]
    pssms = [lm.ScoringMatrix(p) for p in mats]
    records = make_records(rng, 70, 5, list(range(31, 400)), 0.0)
    seqset = pli.stripe_ascii_set(records, lossy=True)
    seqset.configure_wrap(31)
    e1 = pli.scan_threshold_set(pssms, [-np.inf] * len(ms), seqset)
    got = pli.scan_best_set(pssms, seqset)
    pairs = 0
    for ri, text in enumerate(records):
        seq = pli.stripe_ascii(text, lossy=True)
        seq.configure_wrap(31)
        alone = pli.scan_argmax_batch(pssms, seq)
        for mi in range(len(ms)):
            rec, _, val = e1[mi]
            v = val[rec == ri]
            if not len(v) or np.sum(v == v.max()) != 1 or v.max() == -np.inf:
                continue                                           # not unique: the two rules may differ
            (row, col), value = alone[mi]
            assert got.found[mi, ri] and got.position[mi, ri] == col * seq.rows + row, (mi, ri)
            assert bits(got.score[mi, ri]) == bits(np.float32(value)), (mi, ri)
            pairs += 1
    assert pairs >= 200


def test_misuse_is_a_status(pli):
    rng = np.random.default_rng(1)
    records = make_records(rng, 5, 5, [100, 200], 0.0)
    seqset = pli.stripe_ascii_set(records, lossy=True)
    p20 = lm.ScoringMatrix(make_matrix(rng, 20, 5))
    with pytest.raises(lm.LightmotifHipError) as err:                      # no wrap rows yet
        pli.scan_best_set([p20], seqset)
    assert err.value.status == _ffi.ERR_WRAP
    seqset.configure_wrap(19)
    assert pli.scan_best_set([p20], seqset).found.shape == (1, 5)
    prot = lm.ScoringMatrix(make_matrix(rng, 8, 21), protein=True)
    with pytest.raises(ValueError):                                        # the Python layer refuses first
        pli.scan_best_set([prot], seqset)
    L = _ffi.lib()
    handles = (C.c_void_p * 1)(prot._device(pli))
    out = (_ffi.SetBest * 5)()
    before = pli.last_scan_counts
    st = L.lm_hip_scan_best_seqset(pli._h, handles, 1, seqset._h, out)
    assert st == _ffi.ERR_BAD_ARGS and "alphabet" in _ffi.last_error()
    assert pli.last_scan_counts == before                                  # nothing ran
    assert L.lm_hip_scan_best_seqset(pli._h, handles, 1, None, out) == _ffi.ERR_BAD_ARGS and _ffi.last_error()
    assert L.lm_hip_scan_best_seqset(pli._h, None, 0, seqset._h, None) == _ffi.OK      # n == 0
    none = pli.scan_best_set([], seqset)
    assert none.found.shape == (0, 5)
    empty = pli.stripe_ascii_set([])
    empty.configure_wrap(19)
    assert pli.scan_best_set([p20], empty).found.shape == (1, 0)


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
def test_cli_best(tmp_path, oracle, reverse):
    co = oracle
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
    for mode in ("best", "hits"):
        for budget in (2_000, None):
            out = tmp_path / f"{mode}_{budget}.tsv"
            argv = ["-m", str(mats), "-s", str(fasta), "-o", str(out)] + (["--reverse"] if reverse else [])
            argv += ["--best"] if mode == "best" else ["-P", "1e-3"]
            if budget:
                argv += ["--batch-bases", str(budget)]
            assert scan_cli.main(argv) == 0
            outs[mode, budget] = out.read_bytes()
    assert outs["best", 2_000] == outs["best", None] and outs["hits", 2_000] == outs["hits", None]

    records = list(lm.io.read(io.StringIO(MATRICES)))
    direct = [r.matrix.normalize(0.1).log_odds() for r in records]
    want_best, want_hits = [], []
    for si, (name, s) in enumerate(seqs):
        enc = lm.EncodedSequence(s, lossy=True).data
        for strand in ("+", "-") if reverse else ("+",):
            for mi, p in enumerate(direct):
                if len(s) < len(p):
                    continue
                q = p if strand == "+" else p.reverse_complement()
                st = co.stripe(enc, 32, 5)
                co.configure_wrap(st, 8)
                scores, _ = co.score_rows(st, q.data)
                by_pos = scores[:, :32].T.reshape(-1)[: len(s) - len(p) + 1]

                def line(pos):
                    return (si + 1, name, mi + 1, records[mi].id, int(pos), strand, scan_cli._fmt_score(by_pos[pos]),
                            scan_cli._fmt_exp(p.score_distribution.pvalue(float(by_pos[pos]))))
                found, pos, _ = best_of(by_pos)
                if found:
                    want_best.append(line(pos))
                t = np.float32(p.score_for_pvalue(1e-3))
                want_hits.extend(line(pos) for pos in np.nonzero(by_pos >= t)[0])
    header = ["seq_index", "seq_name", "motif_index", "motif_name", "pos", "strand", "score", "pvalue"]
    for mode, want in (("best", want_best), ("hits", want_hits)):
        lines = outs[mode, 2_000].decode().splitlines()
        assert lines[0].split("\t") == header
        got = [tuple(int(x) if i in (0, 2, 4) else x for i, x in enumerate(l.split("\t"))) for l in lines[1:]]
        assert len(want) > 50
        assert got == want, mode
    n_windows = sum(1 for _, s in seqs for p in direct if len(s) >= len(p)) * (2 if reverse else 1)
    assert len(want_best) == n_windows                                     # one line per (sequence, strand, motif) with a window


def test_the_fused_route_beats_the_dense_list(pli):
    """2 000 records x 500 bp x 8 JASPAR motifs: ``scan_best_set`` (B') against ``scan_threshold_set`` at -inf plus the
    reduction in numpy (A'), the cheapest single call that gave the answer before; medians of 5 alternating runs after a
    warm-up, equal answers first.  The margin is 1 x: a new route that is not faster than the road it replaces should not
    exist (the measured medians and ratios are in profiles/seqset_best_bench.json)."""
    sys.path.insert(0, str(ROOT / "tools"))
    import seqset_bench
    res = seqset_bench.measure_best(pli, 2_000, 500, 8, runs=5, warmup=1)
    a, b, c = res["ms"]["A"], res["ms"]["B"], res["ms"]["C"]
    print(f"A' (list at -inf + numpy) median {a['median']:.2f} ms [{a['min']:.2f}, {a['max']:.2f}]  B' (scan_best_set) median "
          f"{b['median']:.3f} ms [{b['min']:.3f}, {b['max']:.3f}]  C' (argmax of the concatenation) median {c['median']:.3f} ms  "
          f"A'/B' {res['A_over_B']:.1f}  B'/C' {res['B_over_C']:.2f}  windows {res['windows']}")
    assert res["answers_equal"] and res["found"] == 2_000 * 8
    assert len(a["all"]) >= 5 and len(b["all"]) >= 5
    assert b["median"] < a["median"]
