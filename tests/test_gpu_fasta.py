"""A resident sequence set straight from FASTA bytes (lm_hip_seqset_from_fasta, csrc/fasta.hip): the container is parsed
on the device.  The expectation is always the set ``stripe_ascii_set`` builds from the records the grammar's plain-Python
form (fasta_cases.parse) finds in the same bytes; the two sets are compared by their geometry, their record lengths and by
scans that expose every symbol, as raw bytes."""
import ctypes as C
import gzip
import re
import sys
from pathlib import Path

import numpy as np
import pytest

import lightmotif_amd as lm
from lightmotif_amd import _ffi, scan_cli
from lightmotif_amd.lib import fasta_names, stride as lm_stride
from fasta_cases import PLAIN, fasta, land_at, lines, parse, residues

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
T = _ffi.lib().lm_hip_fasta_tile_bytes()


def make_matrices(k):
    """M = 1 with k distinct weights (the hit list at -inf IS the sequence), and M = 12 random with a positive weight for
    the default symbol (so that what became N / X shows in the scores)."""
    rng = np.random.default_rng(11)
    one = np.zeros((1, lm_stride(k, 4)), np.float32)
    one[0, :k] = np.arange(1, k + 1, dtype=np.float32)
    twelve = np.zeros((12, lm_stride(k, 4)), np.float32)
    twelve[:, :k] = rng.normal(0, 2, (12, k))
    twelve[:, k - 1] = 0.75
    return [lm.ScoringMatrix(one, protein=k == 21), lm.ScoringMatrix(twelve, protein=k == 21)]


@pytest.fixture(scope="module")
def dna():
    return make_matrices(5)


@pytest.fixture(scope="module")
def protein():
    return make_matrices(21)


def exposed(pli, seqset, pssms):
    """Everything a set shows, as bytes."""
    out = [np.array([len(seqset), seqset.total_length, seqset.rows, seqset.columns]).tobytes(), seqset.lengths.tobytes()]
    seqset.configure_wrap(11)
    best = pli.scan_best_set(pssms, seqset)
    out.append(best.raw.tobytes())
    hits = pli.scan_threshold_set(pssms, [-np.inf] * len(pssms), seqset)
    out += [np.asarray(hits.counts).tobytes()] + [np.ascontiguousarray(hits.hits[f]).tobytes() for f in ("record", "position", "score")]
    return out


def same_as_parsed(pli, data, pssms, lossy=True):
    spans, records = parse(bytes(data))
    protein = pssms[0].protein
    want = pli.stripe_ascii_set(records, protein=protein, lossy=lossy)
    got = pli.stripe_fasta_set(data, protein=protein, lossy=lossy)
    assert len(got) == len(want) == len(records)
    assert got.total_length == want.total_length == sum(map(len, records))
    assert got.rows == want.rows and got.columns == want.columns and got.wrap == want.wrap == 0
    assert np.array_equal(got.lengths, want.lengths)
    assert got.header_spans.dtype == np.uint64 and got.header_spans.shape == spans.shape
    assert np.array_equal(got.header_spans, spans)
    assert want.header_spans is None
    a, b = exposed(pli, got, pssms), exposed(pli, want, pssms)
    assert a == b
    return got, records


# ---- tile borders ------------------------------------------------------------------------------------------------

BORDER_TAILS = {                                     # (tail, index of the byte that lands on the offset)
    "newline": (b"ACGT\nTTGA\n>next\nAC\n", 4),
    "header_start": (b"AC\n>next one\nACGTT\n", 3),
    "gt_in_mid_line": (b"ACG>TA\nCC\n", 3),
    "cr_lf": (b"ACGT\r\nTTGA\r\n>next\r\nAC\r\n", 5),  # the '\n' of the pair: the '\r' stands one byte before it
}


@pytest.mark.parametrize("kind", sorted(BORDER_TAILS))
def test_tile_borders(pli, dna, kind):
    """Each byte of interest at every offset T - 2 ... T + 2, and again around 2 T."""
    rng = np.random.default_rng(3)
    tail, mark = BORDER_TAILS[kind]
    for centre in (T, 2 * T):
        for at in range(centre - 2, centre + 3):
            data = land_at(rng, tail, at, mark)
            assert data[at] == tail[mark]
            same_as_parsed(pli, data, dna)


def test_the_first_header_after_text_without_one_at_a_tile_border(pli, dna):
    rng = np.random.default_rng(4)
    for centre in (T, 2 * T):
        for at in range(centre - 2, centre + 3):
            junk = lines(residues(rng, at), 60)[:at - 1] + b"\n"   # `at` bytes that belong to no record
            data = junk + b">first\nACGTNACGT\nAC\n>second\nGG\n"
            assert data[at:at + 1] == b">" and len(junk) == at
            got, records = same_as_parsed(pli, data, dna)
            assert records == [b"ACGTNACGTAC", b"GG"]


def test_whole_inputs_around_the_tile(pli, dna):
    rng = np.random.default_rng(6)
    long_header = b">" + residues(rng, 5 * T // 2, b"abc de") + b"\nACGT\n>b\nTT\n"
    long_line = b">a\nAC\n>b\n" + residues(rng, 5 * T // 2)                    # no newline at all behind the header
    in_header = land_at(rng, b">cut in the head", T - 3)                       # the input ends inside a header line
    no_newline = land_at(rng, b"ACGTAC", T + 9)
    empty_last = land_at(rng, b">empty\n", T - 7) + b">after\nACGT\n"          # a header line that ends a tile, no sequence
    assert empty_last[T - 1:T + 1] == b"\n>"
    exact = [land_at(rng, b"ACGT\n", n - 5) for n in (T - 1, T, T + 1)]
    assert [len(x) for x in exact] == [T - 1, T, T + 1]
    for data in [long_header, long_line, in_header, no_newline, empty_last] + exact + [x[:-1] for x in exact]:
        same_as_parsed(pli, data, dna)
    got, records = same_as_parsed(pli, empty_last, dna)
    assert records[-2:] == [b"", b"ACGT"]
    assert fasta_names(in_header, pli.stripe_fasta_set(in_header, lossy=True).header_spans)[-1] == "cut"


# ---- the grammar at small sizes ------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(PLAIN))
def test_plain_inputs(pli, dna, name):
    got, records = same_as_parsed(pli, PLAIN[name], dna)
    if name in ("empty", "junk_only"):
        assert len(got) == 0 and got.header_spans.shape == (0, 2)
    if name == "only_headers":
        assert records == [b"", b"", b""]
    if name == "gt_only":
        assert records == [b""] and got.header_spans.tolist() == [[1, 1]]


def test_whitespace_lowercase_and_buffers(pli, dna):
    spaced = b">a\nAC GT\tAC\x0b\x0cGT \r\n  A C G T\n>b\n \n\t\nT T\n"
    got, records = same_as_parsed(pli, spaced, dna)
    assert records == [b"ACGTACGTACGT", b"TT"]
    same_as_parsed(pli, b">lower\nacgtnACGTN\nxyz?\n", dna)             # whatever stripe_ascii_set does with them
    for buf in (bytearray(spaced), memoryview(spaced), np.frombuffer(spaced, dtype=np.uint8)):
        same_as_parsed(pli, buf, dna)


def test_protein(pli, protein):
    data = b">p1 a protein\nACDEFGHIKLMNPQRSTVWYX\nXXAC*DE\n>p2\n\n>p3\nMKV*\n"
    got, records = same_as_parsed(pli, data, protein)
    assert records == [b"ACDEFGHIKLMNPQRSTVWYXXXAC*DE", b"", b"MKV*"]
    with pytest.raises(lm.InvalidSymbol) as err:
        pli.stripe_fasta_set(data, protein=True)
    assert (err.value.record, err.value.index) == (0, 25)


# ---- strict mode ---------------------------------------------------------------------------------------------------

def strict_pair(pli, data):
    """(record, index) of the InvalidSymbol both constructors raise."""
    _, records = parse(data)
    with pytest.raises(lm.InvalidSymbol) as want:
        pli.stripe_ascii_set(records, lossy=False)
    with pytest.raises(lm.InvalidSymbol) as got:
        pli.stripe_fasta_set(data, lossy=False)
    a = tuple(map(int, re.search(r"sequence (\d+) at position (\d+)", str(want.value)).groups()))
    b = tuple(map(int, re.search(r"sequence (\d+) at position (\d+)", str(got.value)).groups()))
    assert a == b == (got.value.record, got.value.index)
    return b


def test_strict_mode_reports_the_first_invalid_residue(pli, dna):
    rng = np.random.default_rng(8)
    recs = [(b"r%d" % i, bytearray(residues(rng, n))) for i, n in enumerate((300, 0, T, 2 * T, 77))]
    clean = fasta([(h, bytes(s)) for h, s in recs])
    same_as_parsed(pli, clean, dna, lossy=False)                          # nothing invalid: strict builds the same set
    recs[2][1][40] = ord("x")
    assert strict_pair(pli, fasta([(h, bytes(s)) for h, s in recs])) == (2, 40)
    recs[3][1][T + 5] = ord("?")                                           # a second one, tiles away: the smaller position wins
    assert strict_pair(pli, fasta([(h, bytes(s)) for h, s in recs])) == (2, 40)
    recs[2][1][40] = ord("A")
    assert strict_pair(pli, fasta([(h, bytes(s)) for h, s in recs])) == (3, T + 5)
    assert strict_pair(pli, b">a\nACGT\n>b\nAC>GT\n") == (1, 2)            # a '>' in mid-line is a residue, and no symbol
    assert strict_pair(pli, b">a\nAC\xc3\xa9GT\n") == (0, 2)               # non-ASCII bytes are residues too
    with pytest.raises(lm.InvalidSymbol):
        pli.stripe_fasta_set(b">a\nACGU\n")                                # strict is the default, as stripe_ascii_set


# ---- fuzz ----------------------------------------------------------------------------------------------------------

def test_fuzz(pli, dna):
    """200 random texts of 1 to 3 tiles over a small byte set, newline-heavy: lossy all of them, strict a subset."""
    rng = np.random.default_rng(2024)
    alphabet = np.frombuffer(b"ACGTNacgt>\n\r \tx", dtype=np.uint8)
    weights = np.ones(len(alphabet))
    weights[10] = 3.0                                 # '\n'
    for i in range(200):
        w = weights.copy()
        w[10] = (0.3, 1.0, 3.0, 12.0)[i % 4]         # from long lines to mostly line ends
        data = bytes(alphabet[rng.choice(len(alphabet), int(rng.integers(T, 3 * T + 1)), p=w / w.sum())])
        same_as_parsed(pli, data, dna)
        if i % 10 == 0:
            _, records = parse(data)
            if any(c not in b"ACGTN" for r in records for c in set(r)):
                strict_pair(pli, data)
            clean = data.translate(bytes(c if c in b"ACGTN>\n\r \t" else ord("A") for c in range(256)))
            _, records = parse(clean)
            if any(b">" in r for r in records):
                strict_pair(pli, clean)
            else:
                same_as_parsed(pli, clean, dna, lossy=False)


def test_many_records_and_repeatability(pli, dna):
    """5 000 records of 0 ... 400 bp in one call; a second call gives the same bytes."""
    rng = np.random.default_rng(12)
    recs = [(b"rec%d description %d" % (i, i), residues(rng, int(n), b"ACGTN")) for i, n in enumerate(rng.integers(0, 401, 5_000))]
    data = fasta(recs)
    got, records = same_as_parsed(pli, data, dna)
    assert len(got) == 5_000 and records == [s for _, s in recs]
    assert fasta_names(data, got.header_spans) == [h.split()[0].decode() for h, _ in recs]
    again = pli.stripe_fasta_set(data, lossy=True)
    assert np.array_equal(again.header_spans, got.header_spans)
    assert exposed(pli, again, dna) == exposed(pli, got, dna)


# ---- misuse --------------------------------------------------------------------------------------------------------

def test_misuse_is_a_status(pli):
    L = _ffi.lib()
    text = b">a\nACGT\n"
    buf = np.frombuffer(text, dtype=np.uint8)
    h, spans, n = C.c_void_p(), C.c_void_p(), C.c_size_t(0)

    def call(ctx=pli._h, alphabet=b"D", ptr=buf.ctypes.data, nbytes=buf.size, cols=32, out=C.byref(h), headers=C.byref(spans),
             count=C.byref(n)):
        return L.lm_hip_seqset_from_fasta(ctx, alphabet, ptr, nbytes, cols, 1, out, headers, count, None, None)

    before = pli.last_scan_counts
    for bad in (dict(ctx=None), dict(out=None), dict(count=None), dict(ptr=None), dict(cols=0), dict(alphabet=b"R")):
        h.value = 1
        assert call(**bad) == _ffi.ERR_BAD_ARGS and _ffi.last_error(), bad
        if "out" not in bad and "ctx" not in bad and "count" not in bad:
            assert h.value is None                   # *out is NULL on failure
    assert pli.last_scan_counts == before
    h.value = None
    assert call(ptr=None, nbytes=0) == _ffi.OK and n.value == 0 and h.value and spans.value is None
    L.lm_hip_seqset_destroy(h)
    assert call(nbytes=0) == _ffi.OK and n.value == 0
    L.lm_hip_seqset_destroy(h)
    assert call(headers=None) == _ffi.OK and n.value == 1              # the caller may not want the spans
    lengths = (C.c_size_t * 1)()
    assert L.lm_hip_seqset_lengths(h, lengths, 1) == _ffi.OK and lengths[0] == 4
    L.lm_hip_seqset_destroy(h)


# ---- the command line ----------------------------------------------------------------------------------------------

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


@pytest.fixture(scope="module")
def cli_text():
    rng = np.random.default_rng(43)
    lengths = rng.integers(0, 300, 120)
    lengths[[3, 50, 51, 119]] = 0
    lengths[[7, 60]] = [4, 7]                        # shorter than the shortest / the longest motif
    lengths[100] = 5_000                             # larger than the budget below
    seqs = ["".join(rng.choice(list("ACGTN"), int(n), p=[0.24, 0.24, 0.24, 0.24, 0.04])) for n in lengths]
    return fasta([(b"rec%d test record" % i, s.encode()) for i, s in enumerate(seqs)], width=70)


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("variant", ["gz", "crlf", "no_final_newline"])
def test_cli_device_and_host_ingest_write_the_same(tmp_path, cli_text, variant, reverse):
    path = tmp_path / ("records.fa.gz" if variant == "gz" else "records.fa")
    if variant == "gz":
        with gzip.open(path, "wb") as fh:
            fh.write(cli_text)
    else:
        path.write_bytes(cli_text.replace(b"\n", b"\r\n") if variant == "crlf" else cli_text.rstrip(b"\n"))
    mats = tmp_path / "motifs.pwm"
    mats.write_text(MATRICES)
    outs = {}
    for mode in ("best", "hits"):
        for budget in (2_000, None):
            for ingest in ("device", "host"):
                out = tmp_path / f"{mode}_{budget}_{ingest}.tsv"
                argv = ["-m", str(mats), "-s", str(path), "-o", str(out), "--ingest", ingest] + (["--reverse"] if reverse else [])
                argv += ["--best"] if mode == "best" else ["-P", "1e-3"]
                if budget:
                    argv += ["--batch-bases", str(budget)]
                assert scan_cli.main(argv) == 0
                outs[mode, budget, ingest] = out.read_bytes()
            assert outs[mode, budget, "device"] == outs[mode, budget, "host"], (mode, budget)
        assert outs[mode, 2_000, "device"] == outs[mode, None, "device"]
        assert len(outs[mode, None, "device"].splitlines()) > 50


# ---- timing ----------------------------------------------------------------------------------------------------------

def test_the_device_reader_beats_the_line_loop(pli):
    """2 000 records x 5 000 bp in 60-column lines: ``stripe_fasta_set`` (B) against ``read_fasta`` + ``stripe_ascii_set``
    (A), the only road from a FASTA file to a set before; C is ``stripe_ascii`` of the joined residues, the floor.  Medians
    of 5 alternating runs after a warm-up, equal sets first.  The margin is 1 x: a road that does not beat the one it
    replaces should not exist (the measured medians and ratios are in profiles/fasta_ingest_bench.json)."""
    sys.path.insert(0, str(ROOT / "tools"))
    import fasta_ingest_bench
    res = fasta_ingest_bench.measure(pli, 2_000, 5_000, runs=5, warmup=1)
    a, b, c = res["ms"]["A"], res["ms"]["B"], res["ms"]["C"]
    print(f"A (read_fasta + stripe_ascii_set) median {a['median']:.2f} ms [{a['min']:.2f}, {a['max']:.2f}]  B (stripe_fasta_set) "
          f"median {b['median']:.3f} ms [{b['min']:.3f}, {b['max']:.3f}]  C (stripe_ascii) median {c['median']:.3f} ms  "
          f"A/B {res['A_over_B']:.1f}  B/C {res['B_over_C']:.2f}  bytes {res['fasta_bytes']}")
    assert res["sets_equal"]
    assert len(a["all"]) >= 5 and len(b["all"]) >= 5
    assert b["median"] < a["median"]
