"""``scan_cli --background sequences`` and ``--composition`` end to end, built like
``test_cli_end_to_end_against_the_oracle``: the expectation is made on the host -- the background from a ``bincount`` of the
texts, ``to_scoring(0.1, background)``, the oracle's scores and ``score_distribution`` of those matrices."""
import gzip
import io

import numpy as np
import pytest

import lightmotif_amd as lm
from lightmotif_amd import scan_cli
from lightmotif_amd.lib import background_from_counts

from test_scan_cli import MATRICES

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def genome(tmp_path_factory):
    """Two records of skewed composition, N included, as gzipped FASTA; the matrices; the host's symbols and counts."""
    rng = np.random.default_rng(23)
    seqs = {"chrA": "".join(rng.choice(list("ACGT"), 20_011, p=[0.4, 0.1, 0.15, 0.35])),
            "chrB": "".join(rng.choice(list("ACGTN"), 7_777, p=[0.15, 0.3, 0.3, 0.15, 0.1]))}
    root = tmp_path_factory.mktemp("background")
    fasta = root / "genome.fa.gz"
    with gzip.open(fasta, "wt") as fh:
        for name, s in seqs.items():
            fh.write(f">{name} test record\n")
            for i in range(0, len(s), 70):
                fh.write(s[i:i + 70] + "\n")
    mats = root / "motifs.pwm"
    mats.write_text(MATRICES)
    encoded = {name: lm.EncodedSequence(s, lossy=True).data for name, s in seqs.items()}
    counts = np.stack([np.bincount(e, minlength=5) for e in encoded.values()]).astype(np.int64)
    return root, fasta, mats, seqs, encoded, counts


def expected_lines(oracle, seqs, encoded, counts, reverse):
    records = list(lm.io.read(io.StringIO(MATRICES)))
    background = background_from_counts(counts.sum(axis=0), unknown=False)
    assert background[4] == 0 and abs(float(background[:4].sum()) - 1) < 1e-6 and background.max() > 0.3
    direct = [r.matrix.to_scoring(0.1, background) for r in records]
    want = []
    for si, (name, s) in enumerate(seqs.items()):
        for strand in ("+", "-") if reverse else ("+",):
            for mi, p in enumerate(direct):
                q = p if strand == "+" else p.reverse_complement()
                t = np.float32(p.score_for_pvalue(1e-3))
                st = oracle.stripe(encoded[name], 32, 5)
                oracle.configure_wrap(st, 8)
                scores, _ = oracle.score_rows(st, q.data)
                by_pos = scores[:, :32].T.reshape(-1)[: len(s) - len(p) + 1]
                for pos in np.nonzero(by_pos >= t)[0]:
                    want.append("\t".join(map(str, (si + 1, name, mi + 1, records[mi].id, int(pos), strand,
                                                    scan_cli._fmt_score(by_pos[pos]),
                                                    scan_cli._fmt_exp(p.score_distribution.pvalue(float(by_pos[pos])))))))
    return want


@pytest.mark.parametrize("reverse", [False, True])
def test_background_from_the_sequences_against_the_oracle(genome, oracle, reverse):
    root, fasta, mats, seqs, encoded, counts = genome
    out, comp = root / f"hits{int(reverse)}.tsv", root / f"composition{int(reverse)}.tsv"
    base = ["-m", str(mats), "-s", str(fasta), "-P", "1e-3"] + (["--reverse"] if reverse else [])
    assert scan_cli.main(base + ["-o", str(out), "--background", "sequences"]) == 0
    lines = out.read_text().splitlines()
    assert lines[0].split("\t") == ["seq_index", "seq_name", "motif_index", "motif_name", "pos", "strand", "score", "pvalue"]
    want = expected_lines(oracle, seqs, encoded, counts, reverse)
    assert len(want) > 20
    assert lines[1:] == want
    # the uniform background gives another table (the flag did something), and "uniform" is the default
    uniform, named = root / f"uniform{int(reverse)}.tsv", root / f"named{int(reverse)}.tsv"
    assert scan_cli.main(base + ["-o", str(uniform), "--composition", str(comp)]) == 0
    assert scan_cli.main(base + ["-o", str(named), "--background", "uniform"]) == 0
    assert uniform.read_bytes() == named.read_bytes() and uniform.read_text().splitlines()[1:] != want
    # one line per record from the set's table, whatever the background
    got = [l.split("\t") for l in comp.read_text().splitlines()]
    assert got[0] == ["seq_index", "seq_name", "length", "A", "C", "T", "G", "N"]
    assert got[1:] == [[str(i + 1), name, str(len(s))] + [str(int(c)) for c in counts[i]] for i, (name, s) in enumerate(seqs.items())]


def test_ingest_and_pvalue_roads_write_the_same_bytes(genome):
    root, fasta, mats, _, _, _ = genome
    written = {}
    for ingest in ("device", "host"):
        for pvalues in ("device", "host"):
            out, comp = root / f"{ingest}_{pvalues}.tsv", root / f"{ingest}_{pvalues}.comp.tsv"
            # small sets: the first pass adds several tables up, the second scans several sets
            assert scan_cli.main(["-m", str(mats), "-s", str(fasta), "-o", str(out), "-P", "1e-3", "--reverse", "--background",
                                  "sequences", "--composition", str(comp), "--ingest", ingest, "--pvalues", pvalues,
                                  "--batch-bases", "21000"]) == 0
            written[ingest, pvalues] = (out.read_bytes(), comp.read_bytes())
    first = written["device", "device"]
    assert len(first[0].splitlines()) > 20 and len(first[1].splitlines()) == 3
    assert all(w == first for w in written.values())


def test_a_file_without_a_base_is_an_argparse_error(genome, capsys):
    root, _, mats, _, _, _ = genome
    for i, text in enumerate(("", ">only\nNNNNNNNN\n>empty\n")):
        fasta = root / f"nothing{i}.fa"
        fasta.write_text(text)
        with pytest.raises(SystemExit) as err:
            scan_cli.main(["-m", str(mats), "-s", str(fasta), "-o", str(root / "nothing.tsv"), "--background", "sequences"])
        assert err.value.code == 2 and "holds no base to count" in capsys.readouterr().err
