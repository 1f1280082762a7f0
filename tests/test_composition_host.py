"""The host side of symbol counts and backgrounds: ``background_from_counts`` (abc.rs:389-456),
``EncodedSequence.count_symbols`` (seq.rs:61-70), ``CountMatrix.to_scoring`` (pwm/mod.rs:240-258, 415-430) and the two new
flags of ``scan_cli``.  No device is needed."""
from pathlib import Path

import numpy as np
import pytest

import lightmotif_amd as lm
from lightmotif_amd import io as lmio
from lightmotif_amd import scan_cli
from lightmotif_amd.lib import background_from_counts

JASPAR = Path(__file__).parent / "golden" / "JASPAR2024.pwm.gz"
F32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_background_from_counts_is_the_reference_example():
    """abc.rs:382-387."""
    bg = background_from_counts([2, 2, 5, 1, 0])
    assert bg.dtype == np.float32 and bg.shape == (5,)
    assert np.array_equal(bits(bg), bits([F32(0.2), F32(0.2), F32(0.5), F32(0.1), F32(0)]))
    assert "background_from_counts" in lm.lib.__all__


def test_the_unknown_symbol_counts_only_when_asked_for():
    counts = [2, 2, 5, 1, 10]
    assert np.array_equal(bits(background_from_counts(counts)), bits(background_from_counts([2, 2, 5, 1, 0])))
    with_n = background_from_counts(counts, unknown=True)
    assert np.array_equal(bits(with_n), bits([F32(2) / F32(20), F32(2) / F32(20), F32(5) / F32(20), F32(1) / F32(20), F32(10) / F32(20)]))
    assert with_n[0] != background_from_counts(counts)[0]


@pytest.mark.parametrize("counts", [[0, 0, 0, 0, 0], [0, 0, 0, 0, 7], [[0, 0, 0, 0, 1], [0, 0, 0, 0, 0]]])
def test_a_table_without_counts_is_an_error(counts):
    with pytest.raises(ValueError):
        background_from_counts(counts)
    if np.sum(counts):
        assert background_from_counts(counts, unknown=True)[-1] == 1.0


def test_large_counts_take_one_conversion_and_one_divide():
    """Above 2^24 an integer is no longer an f32: each count and the integer total are converted once (`as f32`, round to
    nearest even) and divided once in f32."""
    counts = np.array([(1 << 24) + 1, (1 << 31) + 12345, (1 << 40) + 7, 3 * (1 << 33) + 1, 99], dtype=np.int64)
    total = int(counts[:4].sum())
    want = np.array([F32(int(c)) / F32(total) for c in counts[:4]] + [F32(0)], dtype=np.float32)
    assert F32((1 << 24) + 1) == F32(1 << 24)            # (the conversion does round)
    got = background_from_counts(counts)
    assert np.array_equal(bits(got), bits(want))
    assert np.array_equal(bits(background_from_counts(counts.astype(np.uint64))), bits(want))
    total_n = int(counts.sum())
    want_n = np.array([F32(int(c)) / F32(total_n) for c in counts], dtype=np.float32)
    assert np.array_equal(bits(background_from_counts(counts, unknown=True)), bits(want_n))


def test_a_table_of_records_equals_its_column_sums():
    rng = np.random.default_rng(5)
    for k in (5, 21):
        table = rng.integers(0, 1 << 30, (37, k))
        for unknown in (False, True):
            assert np.array_equal(bits(background_from_counts(table, unknown)), bits(background_from_counts(table.sum(axis=0), unknown)))
    assert np.array_equal(bits(background_from_counts([[1, 2, 3, 4, 5]], True)), bits(background_from_counts([1, 2, 3, 4, 5], True)))


def test_encoded_sequence_counts_its_symbols():
    """abc.rs:415-420: the sequence behind the counts of the reference example."""
    got = lm.EncodedSequence("TTATGTTACC").count_symbols()
    assert got.dtype == np.int64 and got.tolist() == [2, 2, 5, 1, 0]
    assert lm.EncodedSequence("", protein=True).count_symbols().tolist() == [0] * 21
    prot = lm.EncodedSequence("MKVXXA", protein=True).count_symbols()
    assert prot.sum() == 6 and prot[20] == 2 and prot[0] == 1


@pytest.fixture(scope="module")
def jaspar():
    return [r.matrix for r in lmio.read(JASPAR)]


def test_to_scoring_without_a_background_is_normalize_then_log_odds(jaspar):
    assert len(jaspar) == 2346
    for cm in jaspar:
        a, b = cm.to_scoring(0.1), cm.normalize(0.1).log_odds()
        assert np.array_equal(bits(a.data), bits(b.data)) and np.array_equal(bits(a.background), bits(b.background))
    assert np.array_equal(bits(jaspar[0].to_scoring().data), bits(jaspar[0].normalize().log_odds().data))


def test_to_scoring_with_a_background_follows_into_scoring(jaspar):
    """pwm/mod.rs:415-430: log2(freq / f) per cell in f32, -inf where f == 0 -- never NaN, unlike `log_odds(background=)`."""
    skew = np.array([0.3, 0.2, 0.3, 0.2, 0], dtype=np.float32)
    for cm in jaspar[:200]:
        p = cm.to_scoring(0.1, skew)
        body = p.data[:, :5]
        assert not np.isnan(body).any() and np.isneginf(body[:, 4]).all() and np.isfinite(body[:, :4]).all()
        assert np.array_equal(bits(p.background), bits(skew))
    cm = jaspar[0]
    pseudo = np.array([0.1, 0.1, 0.1, 0.1, 0], dtype=np.float32)
    for i in range(len(cm)):
        row = (cm.data[i].astype(np.float32) + pseudo).astype(np.float32)
        total = F32(0)
        for x in row:
            total = F32(total + x)
        want = np.log2(((row / total).astype(np.float32)[:4] / skew[:4]).astype(np.float32), dtype=np.float32)
        assert np.array_equal(bits(cm.to_scoring(0.1, skew).data[i, :4]), bits(want))
    as_dict = cm.to_scoring(0.1, {"A": 0.3, "C": 0.2, "T": 0.3, "G": 0.2})
    assert np.array_equal(bits(as_dict.data), bits(cm.to_scoring(0.1, skew).data))
    no_c = cm.to_scoring(0.1, np.array([0.4, 0, 0.3, 0.3, 0], dtype=np.float32)).data
    assert np.isneginf(no_c[:, 1]).all() and np.isneginf(no_c[:, 4]).all() and np.isfinite(no_c[:, [0, 2, 3]]).all()
    with pytest.raises(ValueError):
        cm.to_scoring(0.1, np.ones(4, dtype=np.float32))
    # the road scan_cli must not take: rescale makes the default column NaN
    with np.errstate(all="ignore"):
        assert np.isnan(cm.normalize(0.1).log_odds({"A": 0.3, "C": 0.2, "T": 0.3, "G": 0.2}).data[:, 4]).all()


def test_the_cli_knows_the_two_flags():
    ap = scan_cli.build_parser()
    base = ["-m", "m.pwm", "-s", "s.fa", "-o", "o.tsv"]
    args = ap.parse_args(base)
    assert args.background == "uniform" and args.composition is None
    args = ap.parse_args(base + ["--background", "sequences", "--composition", "c.tsv"])
    assert args.background == "sequences" and args.composition == "c.tsv"
    with pytest.raises(SystemExit):
        ap.parse_args(base + ["--background", "gc"])
