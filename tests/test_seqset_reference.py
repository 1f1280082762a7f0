"""Pins the reference of the set fuzz (tests/seqset_reference.py) on the host: the scores it reads off the concatenation
equal, as f32 bit patterns, ``window_scores`` of every record alone and the C oracle's ``score_rows`` of every record
striped alone at 32 columns; its best window per record is ``best_of``; its p-values are ``dist.py``'s; and the generator
keeps the shares of empty cases, column counts and large sets the fuzz counts on."""
import numpy as np
import pytest

import lightmotif_amd as lm
import seqset_reference as sr
from fasta_cases import parse
from seqset_best_cases import best_of, window_scores

SEEDS = range(40)
DEFAULT_FUZZ_SEEDS = range(120)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def per_record(case, windows, mi):
    """Motif ``mi``'s scores of the reference, one array per record."""
    w = windows[mi]
    cuts = np.searchsorted(w.record, np.arange(len(case.lengths) + 1))
    return [w.score[a:b] for a, b in zip(cuts[:-1], cuts[1:])], [w.position[a:b] for a, b in zip(cuts[:-1], cuts[1:])]


@pytest.fixture(scope="module")
def cases():
    out = {}
    for seed in SEEDS:
        case = sr.draw_case(seed)
        out[seed] = (case, sr.reference(case))
    return out


def test_the_sample_covers_what_it_must(cases):
    all_cases = [c for c, _ in cases.values()]
    assert any(c.protein for c in all_cases) and any(c.has_nan for c in all_cases)
    assert any((c.lengths == 0).any() for c in all_cases)                                   # empty records
    assert any((c.lengths[c.lengths > 0] < min(p.shape[0] for p in c.mats)).any() for c in all_cases)   # shorter than a motif
    assert any(np.isneginf(p[:, :c.k - 1]).any() for c in all_cases for p in c.mats)     # -inf weights off the N column
    assert any(np.isneginf(w.score).any() for _, ws in cases.values() for w in ws)
    assert sum(len(w.score) for _, ws in cases.values() for w in ws) > 1_000_000


@pytest.mark.parametrize("seed", SEEDS)
def test_equals_every_record_alone(cases, oracle, seed):
    co = oracle
    case, windows = cases[seed]
    n = len(case.lengths)
    for mi, p in enumerate(case.mats):
        m = p.shape[0]
        scores, positions = per_record(case, windows, mi)
        found, position, score = windows[mi].best(n)
        for r, sym in enumerate(case.symbols):
            length = len(sym)
            alone = window_scores(p, sym)
            assert len(scores[r]) == max(length - m + 1, 0), (mi, r)
            assert np.array_equal(positions[r], np.arange(len(alone))), (mi, r)
            assert np.array_equal(bits(scores[r]), bits(alone)), (mi, r)
            want = best_of(alone)
            assert (bool(found[r]), int(position[r])) == want[:2], (mi, r)
            assert bits(score[r]) == bits(want[2]) if want[0] else np.isnan(score[r]), (mi, r)
            if length >= m:
                st = co.stripe(sym, 32, case.k)
                co.configure_wrap(st, case.wrap)
                sc, _ = co.score_rows(st, p)
                by_pos = sc[:, :32].T.reshape(-1)[: length - m + 1]
                assert np.array_equal(bits(scores[r]), bits(by_pos)), (mi, r, "oracle")


@pytest.mark.parametrize("seed", SEEDS)
def test_hit_lists_and_thresholds(cases, seed):
    case, windows = cases[seed]
    assert len(case.thresholds) == len(case.mats)
    for w, kind, t in zip(windows, case.threshold_kinds, case.thresholds):
        rec, pos, val = w.hits(t)
        live = w.score[~np.isnan(w.score)]
        assert not np.isnan(val).any()
        if len(rec) > 1:
            dr, dp = np.diff(rec), np.diff(pos)
            assert np.all((dr > 0) | ((dr == 0) & (dp > 0)))
        if not len(live):
            assert len(rec) == 0 or kind == "-inf"
            continue
        want = {"min": len(live), "-inf": len(live), "max": int(np.sum(live == live.max())), "above": 0, "+inf": 0,
                "nan": 0}.get(kind)
        if kind == "above" and np.isneginf(live.max()):
            want = None                                   # nextafter(-inf) is the lowest finite number: no window reaches it
            assert len(rec) == 0
        if want is not None:
            assert len(rec) == want, kind
        if kind in ("median", "q99"):
            assert 0 < len(rec) <= len(live) and t in live


@pytest.mark.parametrize("seed", SEEDS)
def test_text_and_fasta_hold_the_same_records(cases, seed):
    case, _ = cases[seed]
    spans, records = parse(case.fasta)
    assert records == case.texts and len(spans) == len(case.texts)
    for text, sym in zip(case.texts, case.symbols):
        assert np.array_equal(sr.encode_text(text, case.protein), sym)
        assert np.array_equal(lm.EncodedSequence(text, protein=case.protein, lossy=True).data, sym)
    assert [len(s) for s in case.symbols] == case.lengths.tolist()


def test_pvalues_equal_dist_py(cases):
    checked = 0
    for case, windows in cases.values():
        if case.has_nan:
            continue
        for p, w in zip(case.mats, windows):
            finite = w.score[np.isfinite(w.score)][:300]
            if not len(finite):
                continue
            dist = lm.ScoringMatrix(p, protein=case.protein).score_distribution
            extra = np.asarray([-1e30, 1e30, finite.min() - 1, finite.max() + 1], np.float32)
            scores = np.concatenate((finite, extra))
            want = np.asarray([dist.pvalue(float(s)) for s in scores], dtype=np.float64)
            assert np.array_equal(sr.pvalues_of(dist, scores).view(np.uint64), want.view(np.uint64))
            checked += len(scores)
    assert checked > 10_000


def test_the_generator_keeps_its_shares():
    """What the fuzz asserts again over its own run: at most a quarter of the default seeds without a window, at least 15
    with a column count other than 32, at least 8 with more than 4 095 records."""
    drawn = [sr.draw_case(seed) for seed in DEFAULT_FUZZ_SEEDS]
    assert 4 * sum(not c.has_window for c in drawn) <= len(drawn)
    assert sum(c.cols != 32 for c in drawn) >= 15
    assert sum(len(c.lengths) > 4095 for c in drawn) >= 8
    assert {len(c.lengths) for c in drawn} == set(sr.RECORD_COUNTS)
    assert {k for c in drawn for k in c.threshold_kinds} == set(sr.THRESHOLD_KINDS)
    assert sum(c.total < c.cols and c.has_window for c in drawn) >= 1          # shorter than one row
    assert max(c.total for c in drawn) < 400_000
    with_hits = with_pvalues = 0
    for c in drawn:
        want = [w.hits(t) for w, t in zip(sr.reference(c), c.thresholds)]
        scores = np.concatenate([w[2] for w in want])
        with_hits += len(scores) > 0
        with_pvalues += len(scores) > 0 and not c.has_nan and bool(np.isfinite(scores).all())
    assert 2 * with_hits >= len(drawn) and with_pvalues >= 10
