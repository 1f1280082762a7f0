"""``scan_cli --variants``: a three-record FASTA, a variants file and two motifs on both strands; the TSV against one built
from tests/variant_reference.py, line by line, and every error exit."""
import io

import numpy as np
import pytest

from lightmotif_amd import io as lmio
from lightmotif_amd import scan_cli

import seqset_reference as sr
import variant_reference as vr
from fasta_cases import fasta
from variant_reference import small_case, variants_of

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
THRESHOLD = -3.0
HEADER = "seq_index\tseq_name\tpos\tref\talt\tmotif_index\tmotif_name\tstrand\tref_pos\tref_score\talt_pos\talt_score"


@pytest.fixture(scope="module")
def records():
    rng = np.random.default_rng(53)
    return [(name, "".join(rng.choice(list("ACGTN"), n, p=[0.24, 0.24, 0.24, 0.24, 0.04])))
            for name, n in (("chrA", 90), ("short", 6), ("chrB", 41))]


def write_inputs(tmp_path, records, variant_text):
    path, mats, var = tmp_path / "records.fa", tmp_path / "motifs.pwm", tmp_path / "variants.tsv"
    path.write_bytes(fasta([(f"{name} a record".encode(), text.encode()) for name, text in records], width=30))
    mats.write_text(MATRICES)
    var.write_text(variant_text)
    return ["-m", str(mats), "-s", str(path), "--variants", str(var), "--abs-threshold", str(THRESHOLD), "-o", str(tmp_path / "out.tsv")]


def variant_file(records, rng, count):
    """(text, list of (record index, 1-based pos, ref letter, alt letter)) in file order, records interleaved."""
    lines, listed = ["# seq_name\tpos\tref\talt", ""], []
    for _ in range(count):
        r = int(rng.integers(0, len(records)))
        name, text = records[r]
        pos = int(rng.choice([1, 2, len(text) - 1, len(text), int(rng.integers(1, len(text) + 1))]))
        alt = str(rng.choice(list("ACGTN")))
        listed.append((r, pos, text[pos - 1], alt))
        lines.append(f"{name}\t{pos}\t{text[pos - 1]}\t{alt if rng.random() < 0.8 else alt.lower()}")
        if rng.random() < 0.1:
            lines.append("   ")
    return "\n".join(lines) + "\n", listed


@pytest.mark.parametrize("ingest", ["device", "host"])
def test_the_table_matches_the_reference(tmp_path, records, ingest):
    rng = np.random.default_rng(54)
    text, listed = variant_file(records, rng, 160)
    args = write_inputs(tmp_path, records, text) + ["--reverse", "--ingest", ingest]
    assert scan_cli.main(args) == 0
    got = (tmp_path / "out.tsv").read_text().splitlines()

    motifs = list(lmio.read(io.StringIO(MATRICES)))
    direct = [r.matrix.normalize(0.1).log_odds() for r in motifs]
    strands = [("+", [p.data for p in direct]), ("-", [p.reverse_complement().data for p in direct])]
    symbols = [sr.encode_text(t.encode(), False, lossy=False) for _, t in records]
    want = [HEADER]
    # by sequence, then variant in file order, then strand, then motif
    for r, (name, _) in enumerate(records):
        mine = [v for v in listed if v[0] == r]
        for strand, mats in strands:
            case = small_case(mats, symbols)
            variants = variants_of(case, [r] * len(mine), [v[1] - 1 for v in mine], ["ACTGN".index(v[3]) for v in mine])
            effects = vr.reference(case, variants)
            strand_lines = {}
            for mi in range(len(mats)):
                rp, ap = effects.position(variants, "ref")[mi], effects.position(variants, "alt")[mi]
                for j in vr.kept(effects, mi, THRESHOLD):
                    sides = "\t".join(f"{int(q)}\t{scan_cli._fmt_score(s)}" if q >= 0 else ".\t."
                                      for q, s in ((rp[j], effects.ref_score[mi, j]), (ap[j], effects.alt_score[mi, j])))
                    strand_lines[(int(j), mi)] = (f"{r + 1}\t{name}\t{mine[j][1]}\t{mine[j][2]}\t{mine[j][3]}\t{mi + 1}\t{motifs[mi].id}\t"
                                                  f"{strand}\t{sides}")
            want.append((strand, strand_lines))
    # interleave the two strands of a record variant by variant
    lines = [HEADER]
    blocks = want[1:]
    for r in range(len(records)):
        plus, minus = blocks[2 * r][1], blocks[2 * r + 1][1]
        for j in sorted({key[0] for key in plus} | {key[0] for key in minus}):
            for block in (plus, minus):
                lines += [block[key] for key in sorted(k for k in block if k[0] == j)]
    assert len(lines) > 40
    assert got == lines


def run_error(tmp_path, records, variant_text, capsys, extra=()):
    with pytest.raises(SystemExit) as exit_info:
        scan_cli.main(write_inputs(tmp_path, records, variant_text) + list(extra))
    assert exit_info.value.code == 2
    return capsys.readouterr().err


def test_error_exits_name_the_line(tmp_path, records, capsys):
    text = records[0][1]
    good = f"chrA\t5\t{text[4]}\tA\n"
    wrong_ref = "ACGT"[("ACGT".index(text[9]) + 1) % 4] if text[9] in "ACGT" else "A"
    cases = {
        "ref": (good + f"chrA\t10\t{wrong_ref}\tC\n", "variants.tsv:2", "disagrees"),
        "multi": (good + "\n" + "chrA\t7\tAC\tG\n", "variants.tsv:3", "single letter"),
        "multi alt": (good + "chrA\t7\tA\tGT\n", "variants.tsv:2", "single letter"),
        "text pos": (good + "chrA\tseven\tA\tG\n", "variants.tsv:2", "1-based"),
        "zero pos": ("chrA\t0\tA\tG\n", "variants.tsv:1", "1-based"),
        "end": (good + "# a comment\nshort\t7\tA\tG\n", "variants.tsv:3", "behind the end"),
        "name": (good + "chrZ\t1\tA\tG\n", "variants.tsv:2", "no record is called `chrZ`"),
        "letter": ("chrA\t1\tA\tZ\n", "variants.tsv:1", "not one of"),
    }
    for what, (variant_text, line, message) in cases.items():
        err = run_error(tmp_path, records, variant_text, capsys)
        assert line in err and message in err, (what, err)
    for flag in (["--best"], ["--counts"], ["--matched"], ["--site-matrices", str(tmp_path / "s.pwm")]):
        assert "--variants excludes" in run_error(tmp_path, records, good, capsys, flag)


def test_no_variants_is_an_empty_table(tmp_path, records):
    assert scan_cli.main(write_inputs(tmp_path, records, "# nothing\n\n")) == 0
    assert (tmp_path / "out.tsv").read_text().splitlines() == [HEADER]
