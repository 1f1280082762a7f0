"""``scan_cli --regions``: the TSV equals, byte for byte, that of the CLI run WITHOUT ``--regions`` on a FASTA file of the
regions extracted on the host (``rec[s:e]``, reverse-complemented for ``-`` rows, named by the BED name or
``chrom:start-end`` + ``(-)``)."""
import numpy as np
import pytest

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
            "T  [  0  0  0  5  9 ]\n")
COMPLEMENT = str.maketrans("ACGTN", "TGCAN")
CONTIGS = [("chr1", 6_000), ("chr2", 0), ("chr3", 9_000), ("scaffold_4", 300), ("chr5", 4_700)]


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """A 5-contig FASTA of about 20 kb, a 60-line BED (names on some rows, minus strands on some, rows that stick out of their
    contig or miss it), and the matrices."""
    tmp = tmp_path_factory.mktemp("regions_cli")
    rng = np.random.default_rng(19)
    seqs = {name: "".join(rng.choice(list("ACGTN"), n, p=[0.24, 0.24, 0.24, 0.24, 0.04])) for name, n in CONTIGS}
    fa = tmp / "genome.fa"
    fa.write_bytes(fasta([(f"{name} test contig".encode(), seqs[name].encode()) for name, _ in CONTIGS], width=70))
    rows = ["track name=peaks", "# chrom start end name score strand"]
    names = [name for name, _ in CONTIGS]
    for i in range(60):
        chrom = names[int(rng.integers(0, 5))]
        length = dict(CONTIGS)[chrom]
        start = int(rng.integers(-30, max(length, 1) + 10))
        end = start + int(rng.integers(0, 400))
        if i % 3 == 0:
            rows.append(f"{chrom}\t{start}\t{end}")
        elif i % 3 == 1:
            rows.append(f"{chrom}\t{start}\t{end}\tpeak_{i}")
        else:
            rows.append(f"{chrom}\t{start}\t{end}\t{'peak_%d' % i if i % 2 else '.'}\t0\t{'+-.'[i % 7 % 3]}")
    bed = tmp / "peaks.bed"
    bed.write_text("\n".join(rows) + "\n")
    mats = tmp / "motifs.pwm"
    mats.write_text(MATRICES)
    return tmp, fa, bed, mats, seqs, names


def extracted_fasta(path, bed_path, seqs, names, flank=None):
    """The regions cut on the host, in file order, as a FASTA file."""
    bed = lmio.read_bed(str(bed_path), names)
    starts, ends = (bed.starts, bed.ends) if flank is None else lmio.resize_regions(bed.starts, bed.ends, flank=flank)
    records = []
    for chrom, s, e, strand, name in zip(bed.chroms, starts.tolist(), ends.tolist(), bed.strands.tolist(), bed.names):
        text = seqs[chrom][max(s, 0):max(min(e, len(seqs[chrom])), 0)] if s < e else ""
        if strand:
            text = text.translate(COMPLEMENT)[::-1]
        label = name if name is not None else f"{chrom}:{s}-{e}" + ("(-)" if strand else "")
        records.append((label.encode(), text.encode()))
    path.write_bytes(fasta(records, width=70))
    return len(records), sum(1 for _, t in records if t), bed


MODES = {"default": ["-P", "1e-2"], "best": ["--best"], "counts": ["--counts", "-P", "1e-2"], "matched": ["-P", "1e-2", "--matched"]}


@pytest.mark.parametrize("reverse", [False, True], ids=["forward", "reverse"])
@pytest.mark.parametrize("mode", sorted(MODES))
def test_regions_equal_a_run_on_the_extracted_fasta(inputs, mode, reverse):
    tmp, fa, bed, mats, seqs, names = inputs
    cut = tmp / "cut.fa"
    n, live, table = extracted_fasta(cut, bed, seqs, names)
    assert n == 60 and 40 < live < 60 and table.strands.sum() > 5 and sum(x is not None for x in table.names) > 20
    flags = MODES[mode] + (["--reverse"] if reverse else [])
    got, want = tmp / f"got_{mode}_{reverse}.tsv", tmp / f"want_{mode}_{reverse}.tsv"
    assert scan_cli.main(["-m", str(mats), "-s", str(fa), "-o", str(got), "--regions", str(bed)] + flags) == 0
    assert scan_cli.main(["-m", str(mats), "-s", str(cut), "-o", str(want)] + flags) == 0
    assert got.read_bytes() == want.read_bytes()
    assert len(want.read_text().splitlines()) > 40
    if mode == "default" and not reverse:            # names of both kinds, and of a minus-strand region, are in the output
        text = got.read_text()
        assert "\tpeak_" in text and "(-)\t" in text and "\tchr" in text


@pytest.mark.parametrize("mode", ["default", "best"])
def test_flank_and_resize(inputs, mode):
    tmp, fa, bed, mats, seqs, names = inputs
    cut = tmp / "cut_flank.fa"
    extracted_fasta(cut, bed, seqs, names, flank=10)
    flags = MODES[mode] + ["--reverse"]
    got, want = tmp / f"got_flank_{mode}.tsv", tmp / f"want_flank_{mode}.tsv"
    assert scan_cli.main(["-m", str(mats), "-s", str(fa), "-o", str(got), "--regions", str(bed), "--flank", "10"] + flags) == 0
    assert scan_cli.main(["-m", str(mats), "-s", str(cut), "-o", str(want)] + flags) == 0
    assert got.read_bytes() == want.read_bytes() and len(want.read_text().splitlines()) > 40
    plain = tmp / f"got_default_{mode}.tsv"
    assert scan_cli.main(["-m", str(mats), "-s", str(fa), "-o", str(plain), "--regions", str(bed)] + flags) == 0
    assert plain.read_bytes() != got.read_bytes()
    resized = tmp / f"got_resize_{mode}.tsv"
    assert scan_cli.main(["-m", str(mats), "-s", str(fa), "-o", str(resized), "--regions", str(bed), "--resize", "50"] + flags) == 0
    for line in resized.read_text().splitlines()[1:]:
        assert int(line.split("\t")[4]) + 5 <= 50    # a window of at most 50 symbols holds every hit


def test_small_batches_and_the_sequence_background(inputs):
    """Batches are whole records, so the regions of a record are cut from one set wherever the FASTA is split; with
    ``--background sequences`` the composition is that of the regions, as it is on the extracted file."""
    tmp, fa, bed, mats, seqs, names = inputs
    flags = ["-P", "1e-2", "--reverse", "--background", "sequences"]
    one, many = tmp / "one.tsv", tmp / "many.tsv"
    assert scan_cli.main(["-m", str(mats), "-s", str(fa), "-o", str(one), "--regions", str(bed)] + flags) == 0
    cut = tmp / "cut_bg.fa"
    extracted_fasta(cut, bed, seqs, names)
    want = tmp / "want_bg.tsv"
    assert scan_cli.main(["-m", str(mats), "-s", str(cut), "-o", str(want)] + flags) == 0
    assert one.read_bytes() == want.read_bytes()
    # split sets: the same lines, grouped by the set their contig fell into
    assert scan_cli.main(["-m", str(mats), "-s", str(fa), "-o", str(many), "--regions", str(bed), "--batch-bases", "5000", "-P", "1e-2"]) == 0
    whole = tmp / "whole.tsv"
    assert scan_cli.main(["-m", str(mats), "-s", str(fa), "-o", str(whole), "--regions", str(bed), "-P", "1e-2"]) == 0
    strip = lambda p: sorted(line.split("\t", 1)[1] for line in p.read_text().splitlines()[1:])   # noqa: E731  (all but seq_index)
    assert strip(many) == strip(whole) and len(strip(many)) > 40


@pytest.mark.parametrize("argv, message", [
    (["--regions", "BED", "--variants", "v.tsv"], "--regions excludes --variants"),
    (["--flank", "5"], "need --regions"),
    (["--resize", "5"], "need --regions"),
    (["--regions", "BED", "--flank", "5", "--resize", "9"], "not allowed with"),
])
def test_flags_that_do_not_go_together(inputs, capsys, argv, message):
    tmp, fa, bed, mats, seqs, names = inputs
    argv = [str(bed) if a == "BED" else a for a in argv]
    with pytest.raises(SystemExit) as e:
        scan_cli.main(["-m", str(mats), "-s", str(fa), "-o", str(tmp / "never.tsv")] + argv)
    assert e.value.code == 2 and message in capsys.readouterr().err


def test_a_bed_row_on_an_unknown_contig_names_its_line(inputs, capsys):
    tmp, fa, bed, mats, seqs, names = inputs
    bad = tmp / "bad.bed"
    bad.write_text("chr1\t0\t50\nchrUn\t0\t50\n")
    with pytest.raises(SystemExit) as e:
        scan_cli.main(["-m", str(mats), "-s", str(fa), "-o", str(tmp / "never.tsv"), "--regions", str(bad)])
    assert e.value.code == 2 and f"{bad}:2: no record is called `chrUn`" in capsys.readouterr().err
