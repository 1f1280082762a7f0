"""``scan_cli --null``: the TSV equals, line by line, that of a plain run over a FASTA file written from the rule's records
(tests/sample_rule.py) -- ``order0`` with every record's own composition and the record's index in the file as its number,
whatever ``--batch-bases`` is; ``order1`` with the one chain fitted on the whole file at the default batch size."""
import numpy as np
import pytest

from lightmotif_amd import scan_cli

import sample_rule as sr
from fasta_cases import fasta

pytestmark = pytest.mark.gpu

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
SYMBOLS = "ACTGN"                                   # abc.rs:106-108: the order of the symbol indices
CONTIGS = [("chr1", 3_000), ("chr2", 0), ("chr3", 4_500), ("scaffold_4", 300), ("chr5", 2_700), ("chr6", 1)]


def encode(text):
    return np.array([SYMBOLS.index(c) for c in text], dtype=np.uint8)


def decode(symbols):
    return "".join(SYMBOLS[int(x)] for x in symbols)


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("null_cli")
    rng = np.random.default_rng(23)
    seqs = []
    for i, (name, n) in enumerate(CONTIGS):
        p = np.array([0.3, 0.2, 0.2, 0.3, 0.0]) if i % 2 else np.array([0.2, 0.27, 0.27, 0.2, 0.06])
        seqs.append((name, "".join(rng.choice(list("ACGTN"), n, p=p))))
    fa = tmp / "peaks.fa"
    fa.write_bytes(fasta([(f"{name} test".encode(), text.encode()) for name, text in seqs], width=70))
    mats = tmp / "motifs.pwm"
    mats.write_text(MATRICES)
    return tmp, fa, mats, seqs


def write_records(path, seqs, records):
    path.write_bytes(fasta([(f"{name} test".encode(), decode(rec).encode()) for (name, _), rec in zip(seqs, records)], width=70))


def order0_records(seqs, seed):
    model = np.zeros((len(seqs), 5), dtype=np.float32)
    for r, (_, text) in enumerate(seqs):
        counts = np.bincount(encode(text), minlength=5) if text else np.zeros(5, dtype=np.int64)
        if counts.sum():
            model[r] = counts.astype(np.float32) / np.float32(counts.sum())
    return sr.sample([len(t) for _, t in seqs], model, seed=seed)


MODES = {"default": ["-P", "1e-2"], "best": ["--best"], "counts": ["--counts", "-P", "1e-2"], "sum_odds": ["--sum-odds"]}


@pytest.mark.parametrize("mode", sorted(MODES))
def test_order0_equals_a_run_on_the_rules_records_at_every_batch_size(inputs, mode):
    tmp, fa, mats, seqs = inputs
    drawn = tmp / "drawn0.fa"
    write_records(drawn, seqs, order0_records(seqs, 5))
    flags = MODES[mode] + ["--reverse"]
    want, got, split = tmp / f"want0_{mode}.tsv", tmp / f"got0_{mode}.tsv", tmp / f"split0_{mode}.tsv"
    assert scan_cli.main(["-m", str(mats), "-s", str(drawn), "-o", str(want)] + flags) == 0
    assert scan_cli.main(["-m", str(mats), "-s", str(fa), "-o", str(got), "--null", "order0", "--null-seed", "5"] + flags) == 0
    assert got.read_text().splitlines() == want.read_text().splitlines()
    assert len(want.read_text().splitlines()) > 8
    # split into several resident sets: still the plain run over the rule's records, split the same way ...
    want_split = tmp / f"want0_split_{mode}.tsv"
    assert scan_cli.main(["-m", str(mats), "-s", str(drawn), "-o", str(want_split), "--batch-bases", "3500"] + flags) == 0
    assert scan_cli.main(["-m", str(mats), "-s", str(fa), "-o", str(split), "--null", "order0", "--null-seed", "5", "--batch-bases",
                          "3500"] + flags) == 0
    assert split.read_bytes() == want_split.read_bytes()
    # ... and the same file as in one set, where the scan itself does not depend on how the records are laid out (the f64 sums
    # of --sum-odds are added in the order of the set's rows: their last digit may differ between layouts, null or not)
    if mode != "sum_odds":
        assert split.read_bytes() == got.read_bytes()
    if mode == "default":                             # a control is not the input, and another seed is another control
        plain, other = tmp / "plain.tsv", tmp / "other.tsv"
        assert scan_cli.main(["-m", str(mats), "-s", str(fa), "-o", str(plain)] + flags) == 0
        assert scan_cli.main(["-m", str(mats), "-s", str(fa), "-o", str(other), "--null", "order0", "--null-seed", "6"] + flags) == 0
        assert plain.read_bytes() != got.read_bytes() != other.read_bytes()


def test_order1_equals_a_run_on_the_rules_records(inputs):
    tmp, fa, mats, seqs = inputs
    records = [encode(text) for _, text in seqs]
    sym = np.array([np.bincount(r, minlength=5) if len(r) else np.zeros(5, dtype=np.int64) for r in records])
    initial, transitions = sr.markov_from_counts(sym, sr.count_pairs(records, 5))
    drawn = tmp / "drawn1.fa"
    write_records(drawn, seqs, sr.sample([len(r) for r in records], initial, transitions, seed=0))
    want, got = tmp / "want1.tsv", tmp / "got1.tsv"
    flags = ["-P", "1e-2", "--reverse"]
    assert scan_cli.main(["-m", str(mats), "-s", str(drawn), "-o", str(want)] + flags) == 0
    assert scan_cli.main(["-m", str(mats), "-s", str(fa), "-o", str(got), "--null", "order1"] + flags) == 0    # --null-seed 0
    assert got.read_text().splitlines() == want.read_text().splitlines() and len(want.read_text().splitlines()) > 8
    assert "N" not in drawn.read_text().replace("test", "")      # a chain fitted without the default symbol draws none


@pytest.mark.parametrize("argv, message", [
    (["--null", "order0", "--variants", "v.tsv"], "--null excludes"),
    (["--null", "order1", "--matched"], "--null excludes"),
    (["--null", "order0", "--site-matrices", "sites.pwm"], "--null excludes"),
    (["--null", "order2"], "invalid choice"),
    (["--null", "order0", "--null-seed", "-1"], "--null-seed"),
])
def test_flags_that_do_not_go_together(inputs, capsys, argv, message):
    tmp, fa, mats, seqs = inputs
    with pytest.raises(SystemExit) as e:
        scan_cli.main(["-m", str(mats), "-s", str(fa), "-o", str(tmp / "never.tsv")] + argv)
    assert e.value.code == 2 and message in capsys.readouterr().err
