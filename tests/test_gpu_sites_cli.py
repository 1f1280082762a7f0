"""``scan_cli --matched`` and ``--site-matrices``: the text of every hit's window and the count matrix of every motif's hits,
read out of the resident sets, against slices of the records ``read_fasta`` parses from the same file."""
import io

import numpy as np
import pytest

import lightmotif_amd as lm
from lightmotif_amd import io as lmio
from lightmotif_amd import scan_cli

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
            "T  [  0  0  0  5  9 ]\n"
            ">never\n"                                # 40 rows: longer than most records, so few windows or none
            + "".join(f"{s}  [ " + " ".join(["9"] * 40) + " ]\n" for s in "ACGT"))
COMPLEMENT = str.maketrans("ACGTN", "TGCAN")


@pytest.fixture(scope="module")
def fasta_text():
    rng = np.random.default_rng(47)
    lengths = rng.integers(0, 120, 60)
    lengths[[3, 20, 59]] = 0
    lengths[[7, 30]] = [4, 7]
    lengths[40] = 3_000                              # larger than the budget below: a set of its own
    seqs = ["".join(rng.choice(list("ACGTN"), int(n), p=[0.24, 0.24, 0.24, 0.24, 0.04])) for n in lengths]
    return fasta([(b"rec%d test record" % i, s.encode()) for i, s in enumerate(seqs)], width=70)


@pytest.mark.parametrize("best", [False, True])
@pytest.mark.parametrize("ingest", ["device", "host"])
def test_matched_column_and_site_matrices(tmp_path, fasta_text, best, ingest):
    path, mats = tmp_path / "records.fa", tmp_path / "motifs.pwm"
    path.write_bytes(fasta_text)
    mats.write_text(MATRICES)
    with open(path) as fh:
        texts = [text for _, text in scan_cli.read_fasta(fh)]
    motifs = list(lmio.read(io.StringIO(MATRICES)))
    base = ["-m", str(mats), "-s", str(path), "--reverse", "--ingest", ingest, "--batch-bases", "1500"]
    base += ["--best"] if best else ["-P", "1e-2"]
    plain, full, sites = tmp_path / "plain.tsv", tmp_path / "full.tsv", tmp_path / "sites.pwm"
    assert scan_cli.main(base + ["-o", str(plain)]) == 0
    assert scan_cli.main(base + ["-o", str(full), "--matched", "--site-matrices", str(sites)]) == 0
    plain_lines, full_lines = plain.read_text().splitlines(), full.read_text().splitlines()
    assert len(plain_lines) == len(full_lines) > 40
    assert full_lines[0] == plain_lines[0] + "\tmatched"
    windows = {(mi, strand): [] for mi in range(len(motifs)) for strand in "+-"}
    for a, b in zip(plain_lines[1:], full_lines[1:]):
        cells = b.split("\t")
        assert len(cells) == 9 and "\t".join(cells[:8]) == a                   # the first eight columns are untouched
        seq, mi, pos, strand = int(cells[0]) - 1, int(cells[2]) - 1, int(cells[4]), cells[5]
        window = texts[seq][pos:pos + len(motifs[mi].matrix)]
        assert len(window) == len(motifs[mi].matrix)
        want = window.translate(COMPLEMENT)[::-1] if strand == "-" else window
        assert cells[8] == want, (a, cells[8], want)
        windows[mi, strand].append(want)
    assert all(windows[mi, s] for mi in (0, 1) for s in "+-")
    back = list(lmio.read(str(sites)))
    assert [(r.id, r.description) for r in back] == [(r.id, r.description) for r in motifs]
    for mi, rec in enumerate(back):
        strings = windows[mi, "+"] + windows[mi, "-"]
        if strings:
            want = lm.CountMatrix.from_sequences([lm.EncodedSequence(s) for s in strings])
        else:
            want = lm.CountMatrix(np.zeros((len(motifs[mi].matrix), 5)))
        assert rec.matrix == want, mi
        assert (rec.matrix.data.sum(axis=1) == len(strings)).all()
    # the flags alone: each works without the other
    only = tmp_path / "only.tsv"
    assert scan_cli.main(base + ["-o", str(only), "--matched"]) == 0 and only.read_text() == full.read_text()
    assert scan_cli.main(base + ["-o", str(only), "--site-matrices", str(tmp_path / "again.pwm")]) == 0
    assert only.read_text() == plain.read_text() and (tmp_path / "again.pwm").read_text() == sites.read_text()


def test_a_motif_without_hits_gets_zeros(tmp_path):
    path, mats, sites = tmp_path / "one.fa", tmp_path / "motifs.pwm", tmp_path / "sites.pwm"
    path.write_bytes(b">short\nACGTACGTAC\n")
    mats.write_text(MATRICES)
    assert scan_cli.main(["-m", str(mats), "-s", str(path), "-o", str(tmp_path / "o.tsv"), "--best", "--matched", "--site-matrices",
                          str(sites)]) == 0
    back = list(lmio.read(str(sites)))
    assert len(back) == 3 and not back[2].matrix.data.any() and back[2].matrix.data.shape == (40, 5)
    assert (back[0].matrix.data.sum(axis=1) == 1).all() and (back[1].matrix.data.sum(axis=1) == 1).all()
    lines = (tmp_path / "o.tsv").read_text().splitlines()
    assert len(lines) == 3 and {line.split("\t")[8] for line in lines[1:]} <= {"ACGTACGTAC"[p:p + m] for p in range(10) for m in (5, 8)}
