"""The sampling rule itself (tests/sample_rule.py), without a device: the generator's known answers, the small vectors of
the rule, prefix stability, and the statistical sanity of what the device reproduces bit for bit.  The chi-square bounds are
the 0.999 quantiles of their distributions (16.27 at 3 degrees of freedom, 43.82 at 19, 32.91 at 12); the seeds are fixed, so
these are conditions, not measurements."""
import numpy as np
import pytest

import sample_rule as sr

F = np.array([0.3, 0.2, 0.15, 0.35, 0], dtype=np.float32)
TRANSITIONS = np.array([[.1, .2, .3, .4, 0], [.4, .3, .2, .1, 0], [.25, .25, .25, .25, 0], [.7, .1, .1, .1, 0], [0, 0, 0, 0, 0]],
                       dtype=np.float32)


@pytest.mark.parametrize("counter, key, want", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff, 0xffffffff), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_known_answers(counter, key, want):
    got = sr.philox4x32_10(counter, key)
    assert tuple(int(g[0]) for g in got) == want


@pytest.mark.parametrize("seed, R, want", [(1, 0, [3, 3, 2, 3, 3, 3, 1, 3]), (1, 1, [2, 0, 0, 0, 3, 3, 0, 0]), (2, 0, [1, 1, 3, 1, 0, 0, 3, 1])])
def test_small_vectors(seed, R, want):
    assert sr.record_order0(F, seed, R, 8).tolist() == want
    assert sr.sample([0] * R + [8], F, seed=seed)[R].tolist() == want


def test_thresholds_and_their_edges():
    T = sr.thresholds(F)
    assert T.dtype == np.uint64 and T.tolist() == sorted(T.tolist()) and T[3] == 1 << 32      # N has no mass: never drawn
    assert sr.thresholds(np.array([0, 0, 1, 0, 0], dtype=np.float32)).tolist() == [0, 0, 1 << 32, 1 << 32]
    u = np.array([0, 1, 0xFFFFFFFF], dtype=np.uint64)
    assert sr.draw([0, 0, 1 << 32, 1 << 32], u).tolist() == [2, 2, 2]
    assert sr.draw([1, 1, 1, 1], u).tolist() == [0, 4, 4]
    assert sr.valid(F) and not sr.valid([0] * 5) and not sr.valid([1, -1, 1, 1, 1]) and not sr.valid([1, np.nan, 0, 0, 0])
    assert not sr.valid([np.inf, 0, 0, 0, 0])


def test_a_longer_record_extends_a_shorter_one_and_records_are_independent():
    long = sr.record_order0(F, 9, 5, 1_003)
    for n in (0, 1, 3, 4, 5, 17, 1_000):
        assert np.array_equal(sr.record_order0(F, 9, 5, n), long[:n])
    long1 = sr.record_order1(F, TRANSITIONS, 9, 5, 301)
    for n in (0, 1, 2, 5, 300):
        assert np.array_equal(sr.record_order1(F, TRANSITIONS, 9, 5, n), long1[:n])
    a = sr.sample([10, 20, 30], F, seed=4, record_base=7)
    b = sr.sample([5, 0, 11, 30], F, seed=4, record_base=6)
    assert np.array_equal(a[2], b[3]) and np.array_equal(a[0][:0], b[1])
    assert not np.array_equal(sr.record_order0(F, 4, 9, 30), sr.record_order0(F, 5, 9, 30))
    # hi32(R) takes part
    assert not np.array_equal(sr.record_order0(F, 4, 1, 64), sr.record_order0(F, 4, (1 << 32) + 1, 64))


def chi2(observed, expected):
    observed, expected = np.asarray(observed, dtype=np.float64), np.asarray(expected, dtype=np.float64)
    return float(((observed - expected) ** 2 / expected).sum())


def test_order0_dna_follows_its_model():
    text = np.concatenate(sr.sample([2_000] * 100, F, seed=12345))
    counts = np.bincount(text, minlength=5)
    assert counts[4] == 0
    x = chi2(counts[:4], F[:4].astype(np.float64) * text.size)
    print(f"chi2(3) = {x:.2f}")
    assert x < 16.3


def test_order0_protein_follows_its_model():
    f = np.array([0.05] * 20 + [0], dtype=np.float32)
    text = np.concatenate(sr.sample([2_000] * 100, f, seed=7))
    counts = np.bincount(text, minlength=21)
    assert counts[20] == 0
    x = chi2(counts[:20], np.full(20, text.size / 20))
    print(f"chi2(19) = {x:.2f}")
    assert x < 43.8


def test_order1_follows_its_transitions():
    records = sr.sample([1_000] * 60, F, TRANSITIONS, seed=99)
    pairs = sr.count_pairs(records, 5)
    assert pairs[4].sum() == 0 and pairs[:, 4].sum() == 0
    x = sum(chi2(pairs[a, :4], TRANSITIONS[a, :4].astype(np.float64) * pairs[a].sum()) for a in range(4))
    print(f"chi2(12) = {x:.2f}")
    assert x < 32.9


def test_markov_from_counts_restated():
    records = sr.sample([300] * 20, np.array([0.2, 0.3, 0.2, 0.2, 0.1], dtype=np.float32), seed=3)
    sym = np.array([np.bincount(r, minlength=5) for r in records])
    pairs = sr.count_pairs(records, 5)
    initial, transitions = sr.markov_from_counts(sym, pairs)
    assert initial.dtype == transitions.dtype == np.float32 and initial[4] == 0
    assert not transitions[4].any() and not transitions[:, 4].any()
    assert np.allclose(transitions[:4].sum(axis=1), 1, atol=1e-6)
    initial, transitions = sr.markov_from_counts(sym, pairs, pseudocount=1.0, unknown=True)
    assert (transitions > 0).all() and initial[4] > 0
