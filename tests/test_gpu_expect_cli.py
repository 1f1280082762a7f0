"""``scan_cli --refine N --refined PATH``: the refined matrices are those of ``Pipeline.refine`` on the same inputs, and the
hit TSV is byte for byte that of a run without the option."""
import numpy as np
import pytest

import lightmotif_amd as lm
from lightmotif_amd import io as lmio
from lightmotif_amd import scan_cli
from expect_rule import planted_case

pytestmark = pytest.mark.gpu


def jaspar_of(word, name):
    """A count matrix of 20 sites: 11 of the word's letter, 3 of every other one."""
    rows = {c: " ".join("11" if w == c else " 3" for w in word) for c in "ACGT"}
    return f">{name}\t{name.lower()}\n" + "".join(f"{c}  [ {rows[c]} ]\n" for c in "ACGT")


@pytest.mark.parametrize("model", ["oops", "zoops"])
def test_cli_refine_writes_what_refine_returns_and_leaves_the_hits_alone(pli, tmp_path, model):
    word, texts = planted_case(seed=11, records=60, length=50, m=8)
    fasta = tmp_path / "records.fa"
    fasta.write_text("".join(f">rec{i} planted\n{t}\n" for i, t in enumerate(texts)))
    mats = tmp_path / "motifs.pwm"
    mats.write_text(jaspar_of(word, "MA9001.1") + jaspar_of(word[2:] + "ACGTA", "MA9002.1"))
    plain, with_refine, refined = tmp_path / "plain.tsv", tmp_path / "refine.tsv", tmp_path / "refined.pwm"
    common = ["-m", str(mats), "-s", str(fasta), "-P", "1e-3"]
    assert scan_cli.main(common + ["-o", str(plain)]) == 0
    assert scan_cli.main(common + ["-o", str(with_refine), "--refine", "2", "--refined", str(refined), "--refine-model", model]) == 0
    assert with_refine.read_bytes() == plain.read_bytes() and len(plain.read_text().splitlines()) > 10

    records = list(lmio.read(str(mats)))
    direct = [r.matrix.normalize(0.1).log_odds() for r in records]
    seqset = pli.stripe_ascii_set(texts, lossy=True)
    seqset.configure_wrap(max(len(p) for p in direct))
    new, lls, expected = pli.refine(direct, seqset, 2, model=model, return_counts=True)
    assert lls.shape == (3, 2) and (model != "oops" or (lls[1:] >= lls[:-1] - 1e-9 * np.abs(lls[:-1])).all())
    got = list(lmio.read(str(refined)))
    assert [(r.id, r.description) for r in got] == [(r.id, r.description) for r in records]
    for r, e in zip(got, expected.counts):
        assert np.array_equal(r.matrix.data, np.rint(e).astype(np.uint32)) and r.matrix == scan_cli.refined_counts(e)
    assert got[0].matrix.data.sum(axis=1).min() >= (55 if model == "oops" else 1)      # OOPS: one site per record
    # an input larger than one resident set is refused, not refined in part
    with pytest.raises(SystemExit):
        scan_cli.main(common + ["-o", str(with_refine), "--refine", "2", "--refined", str(refined), "--batch-bases", "500"])
