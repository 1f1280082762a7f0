"""The host side of hit windows: ``CountMatrix.reverse_complement`` (pwm/mod.rs:313-321), the JASPAR-2016 writer ``io.write``,
``decode`` and the normalisation of the ``sites`` / ``widths`` / ``shifts`` arguments of ``StripedSequenceSet.windows`` and
``count_sites``.  No device is needed."""
import io

import numpy as np
import pytest

import lightmotif_amd as lm
from lightmotif_amd import io as lmio
from lightmotif_amd.lib import SET_HIT_DTYPE, SetHits, _site_args, decode


def test_reverse_complement_of_a_hand_written_matrix():
    # columns A C T G N
    m = lm.CountMatrix(np.array([[1, 2, 3, 4, 5], [6, 7, 8, 9, 10], [0, 0, 11, 0, 1]]))
    rc = m.reverse_complement()
    assert isinstance(rc, lm.CountMatrix) and rc.data.dtype == np.uint32 and not rc.protein
    assert rc.data.tolist() == [[11, 0, 0, 0, 1], [8, 9, 6, 7, 10], [3, 4, 1, 2, 5]]
    assert rc.reverse_complement() == m and rc != m
    assert m.data.tolist()[0] == [1, 2, 3, 4, 5]                      # the original is untouched
    # the counts of the reverse-complemented sequences: pwm/mod.rs:313-321 commutes with from_sequences
    seqs = ["ATGCA", "TTGCN", "CCGTA"]
    comp = str.maketrans("ACGTN", "TGCAN")
    direct = lm.CountMatrix.from_sequences([lm.EncodedSequence(s) for s in seqs])
    turned = lm.CountMatrix.from_sequences([lm.EncodedSequence(s.translate(comp)[::-1]) for s in seqs])
    assert direct.reverse_complement() == turned
    assert len(lm.CountMatrix(np.zeros((0, 5))).reverse_complement()) == 0


def test_a_protein_matrix_has_no_complement():
    with pytest.raises(ValueError):
        lm.CountMatrix(np.zeros((3, 21)), protein=True).reverse_complement()


def test_write_then_read_round_trips(tmp_path):
    rng = np.random.default_rng(5)
    records = [lmio.Record("MA0001.1", "FIRST one", lm.CountMatrix(rng.integers(0, 3000, (9, 5)))),
               lmio.Record("zero", None, lm.CountMatrix(np.zeros((4, 5)))),
               lmio.Record("no_n", "x", lm.CountMatrix(np.hstack([rng.integers(0, 9, (12, 4)), np.zeros((12, 1), dtype=np.int64)]))),
               lmio.Record("one_row", None, lm.CountMatrix(np.array([[4000000000, 0, 1, 2, 0]])))]
    text = io.StringIO()
    lmio.write(records, text)
    assert text.getvalue().startswith(">MA0001.1\tFIRST one\nA  [")
    assert "\nN  [" not in text.getvalue().split(">zero")[1].split(">no_n")[0]      # the default symbol's line only with counts
    text.seek(0)
    back = list(lmio.read(text))
    assert [(r.id, r.description) for r in back] == [(r.id, r.description) for r in records]
    assert all(a.matrix == b.matrix for a, b in zip(back, records))
    for name in ("m.pwm", "m.pwm.gz"):                               # paths, gzipped by their name as `read` opens them
        lmio.write(records, str(tmp_path / name))
        assert [r.matrix for r in lmio.read(str(tmp_path / name))] == [r.matrix for r in records]
    lmio.write([], str(tmp_path / "none.pwm"))
    assert list(lmio.read(str(tmp_path / "none.pwm"))) == []


def test_decode():
    assert decode([0, 1, 2, 3, 4]) == "ACTGN" and decode(np.zeros(0, np.uint8)) == ""
    assert decode(lm.EncodedSequence("TTGACA")) == "TTGACA"
    assert decode([0, 20], protein=True) == "AX"
    for bad in ([5], [255], [0, 21]):
        with pytest.raises(ValueError):
            decode(bad, protein=len(bad) == 2)
    assert "decode" in lm.lib.__all__


def test_sites_widths_and_shifts_are_normalised():
    counts, widths, shifts, buf, stride = _site_args([([0, 1], [2, 2 ** 64 - 1]), ([], []), (np.array([3]), np.array([-1]))],
                                                     [3, 4, lm.ScoringMatrix(np.zeros((7, 8), np.float32))])
    assert counts.tolist() == [2, 0, 1] and widths.tolist() == [3, 4, 7] and shifts.tolist() == [0, 0, 0] and stride == 16
    assert buf.dtype == np.uint64 and buf.tolist() == [[0, 2], [1, 2 ** 64 - 1], [3, 2 ** 64 - 1]]
    assert _site_args([([0], [0])], [2], shifts=-3)[2].tolist() == [-3]
    assert _site_args([([0], [0]), ([], [])], [2, 2], shifts=[1, -2 ** 62])[2].tolist() == [1, -2 ** 62]
    hits = np.zeros(3, dtype=SET_HIT_DTYPE)
    hits["record"], hits["position"] = [0, 0, 1], [4, 5, 6]
    counts, widths, _, buf, stride = _site_args(SetHits(hits, np.array([1, 2])), [5, 6])
    assert counts.tolist() == [1, 2] and stride == 24 and buf is hits           # the hit list passes as it is
    counts, *_ = _site_args([], [])
    assert len(counts) == 0


@pytest.mark.parametrize("sites, widths, shifts", [
    ([([0], [0])], [2, 2], 0),                       # more widths than motifs
    ([([0], [0]), ([1], [1])], [2], 0),              # fewer
    ([([0], [0])], [2], [0, 0]),                     # shifts
    ([([0, 1], [0])], [2], 0),                       # records against positions
    ([([0], [0], [0])], [2], 0),                     # not a pair
    ([([0], [0])], [0], 0),                          # an empty window
    ([([[0]], [[0]])], [2], 0),                      # not one-dimensional
])
def test_mismatched_arguments_are_rejected(sites, widths, shifts):
    with pytest.raises(ValueError):
        _site_args(sites, widths, shifts)


def test_widths_must_be_a_list():
    with pytest.raises(TypeError):
        _site_args([([0], [0])], 3)
    with pytest.raises(TypeError):
        _site_args([([0.5], [0])], [3])
