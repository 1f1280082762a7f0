"""Pins tests/variant_reference.py, the reference of tests/test_gpu_variants.py, against a second, independent route, and
asserts what its seeded variants cover -- so that the GPU test cannot pass by comparing nones.

The second route builds the mutated RECORD, takes every window of the original and of the mutated record from
``seqset_reference.motif_windows`` (whole-record scores and the segment rule), keeps the windows that cover ``p`` and
picks the best with a sort instead of ``best_of``.  It is run for a seeded sample of each seed's variants (whole records are
scored once per variant and motif); the coverage figures are over ALL variants of seeds 0-39."""
import numpy as np
import pytest

import variant_reference as vr
from seqset_reference import motif_windows
from seqset_rule import offsets_of

SEEDS = range(40)
SAMPLE = 40             # variants per seed that go through the second route


def second_route(weights, record, p):
    """(score, back) of the best window covering ``p``: all windows of the record, filtered, sorted."""
    m = weights.shape[0]
    w = motif_windows(weights, np.asarray(record, dtype=np.uint8), offsets_of([len(record)]))
    cover = (w.position <= p) & (w.position + m > p) & ~np.isnan(w.score)
    pos, val = w.position[cover], w.score[cover]
    if not len(pos):
        return np.float32(np.nan), vr.NONE
    order = np.lexsort((pos, -val.astype(np.float64)))
    return val[order[0]], p - int(pos[order[0]])


def same(a, b):
    a, b = np.float32(a), np.float32(b)
    return (np.isnan(a) and np.isnan(b)) or a.view(np.uint32) == b.view(np.uint32)


@pytest.mark.parametrize("seed", SEEDS)
def test_reference_agrees_with_whole_record_scores(seed):
    case, variants, effects = vr.case_of(seed)
    rng = np.random.default_rng(77_000 + seed)
    picks = np.arange(len(variants)) if len(variants) <= SAMPLE else np.sort(rng.choice(len(variants), SAMPLE, replace=False))
    for j in picks:
        if not variants.valid[j]:
            assert effects.ref_symbol[j] == 0xFF
            assert np.isnan(effects.ref_score[:, j]).all() and np.isnan(effects.alt_score[:, j]).all()
            assert (effects.ref_back[:, j] == vr.NONE).all() and (effects.alt_back[:, j] == vr.NONE).all()
            continue
        r, p, a = int(variants.record[j]), int(variants.position[j]), int(variants.alt[j])
        record = case.symbols[r]
        mutated = np.array(record)
        mutated[p] = a
        assert effects.ref_symbol[j] == record[p]
        for i, weights in enumerate(case.mats):
            for side, text in (("ref", record), ("alt", mutated)):
                score, back = second_route(weights, text, p)
                assert same(getattr(effects, side + "_score")[i, j], score), (seed, i, j, side)
                assert getattr(effects, side + "_back")[i, j] == back, (seed, i, j, side)


def test_the_seeds_cover_what_the_kernels_can_get_wrong():
    pairs = with_window = left = right = plain = invalid = 0
    tie = all_nan = neg_inf = same_symbol = 0
    for seed in SEEDS:
        case, variants, effects = vr.case_of(seed)
        pairs += effects.has_window.size
        with_window += int(effects.has_window.sum())
        invalid += int((~variants.valid).sum()) * len(case.mats)
        for i, weights in enumerate(case.mats):
            m = weights.shape[0]
            for j in np.flatnonzero(effects.has_window[i]):
                r, p = int(variants.record[j]), int(variants.position[j])
                length = int(case.lengths[r])
                clipped_left, clipped_right = p - m + 1 < 0, p > length - m
                left += clipped_left
                right += clipped_right
                plain += not (clipped_left or clipped_right)
        same_symbol += int((variants.valid & (variants.alt == effects.ref_symbol)).sum())
        with np.errstate(invalid="ignore"):
            all_nan += int((effects.has_window & (np.isnan(effects.ref_score) | np.isnan(effects.alt_score))).sum())
            neg_inf += int((effects.ref_score == -np.inf).sum() + (effects.alt_score == -np.inf).sum())
        # a tie decided by the lowest start: the best score occurs again at a HIGHER start among the covering windows
        for i, weights in enumerate(case.mats):
            if tie or case.kinds[i] != "ties":
                continue
            m = weights.shape[0]
            for j in np.flatnonzero(effects.has_window[i])[:200]:
                r, p = int(variants.record[j]), int(variants.position[j])
                lo, hi = vr.windows_of(p, int(case.lengths[r]), m)
                scores = vr.window_scores(weights, case.symbols[r][lo:hi + m])
                best = effects.ref_score[i, j]
                if not np.isnan(best) and int((scores == best).sum()) > 1:
                    first = int(np.flatnonzero(scores == best)[0])
                    assert effects.ref_back[i, j] == p - (lo + first)
                    tie += 1
                    break
    print(f"{pairs} pairs: {with_window} with a window ({100.0 * with_window / pairs:.1f} %), {left} left-clipped, "
          f"{right} right-clipped, {plain} unclipped, {invalid} of an invalid variant; ties {tie}, all-NaN sides {all_nan}, "
          f"-inf bests {neg_inf}, alt == ref {same_symbol}")
    assert 3 * with_window >= pairs
    assert left >= 2000 and right >= 2000 and plain >= 2000
    assert tie >= 1 and all_nan >= 1 and neg_inf >= 1 and same_symbol >= 1


def test_windows_of_matches_the_definition():
    """All windows inside the record that cover p, by brute force."""
    for length in range(0, 9):
        for m in range(1, 7):
            for p in range(length):
                starts = [s for s in range(0, length - m + 1) if s <= p < s + m]
                lo, hi = vr.windows_of(p, length, m)
                assert list(range(lo, hi + 1)) == starts
