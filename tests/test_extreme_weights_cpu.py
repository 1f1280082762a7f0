"""The constructions of tests/extreme_weights.py do what their names claim (no GPU): both oracles agree on them bit for
bit, and each produces its edge -- so a GPU test on them cannot pass or fail because of a generator that missed it."""
import numpy as np
import pytest

import extreme_weights as xw
from oracle import c_oracle as co
from oracle import np_oracle as no

COLS = 32


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def both_oracles(enc, pssm, k, cols=COLS):
    m = pssm.shape[0]
    s = co.stripe(enc, cols, k)
    co.configure_wrap(s, max(m - 1, 0))
    want, mi = co.score_rows(s, pssm)
    d = no.stripe(enc, cols, k - 1)
    d, _ = no.configure_wrap(d, d.shape[0], cols, 0, max(m - 1, 0), k - 1)
    assert np.array_equal(d, s.data)
    got, mi2 = no.score_rows(d, cols, len(enc), pssm, 0, s.rows)
    assert mi2 == mi and np.array_equal(bits(got[:, :cols]), bits(want[:, :cols])), "the two oracles differ"
    assert co.argmax(want, cols) == no.argmax(want, cols)
    return s, want


def real_sums(s, pssm, k, cols=COLS):
    """Each window's sum in float64 (exact enough at these magnitudes; -inf terms give -inf)."""
    m = pssm.shape[0]
    w = pssm[:, :k].astype(np.float64)
    rows = s.rows
    acc = np.zeros((rows, cols))
    with np.errstate(invalid="ignore"):
        for j in range(m):
            acc = acc + w[j][s.data[j:j + rows, :cols]]
    return acc


CASES = [(r, v, k, m) for r, v in xw.REGIMES for k in (5, 21) for m in (3, 12, 37) if m >= xw.min_length(r)]


@pytest.mark.parametrize("regime,variant,k,m", CASES,
                         ids=[f"{xw.regime_id(r, v)}-K{k}-M{m}" for r, v, k, m in CASES])
def test_construction(regime, variant, k, m):
    pssm = xw.make_pssm(regime, variant, m, k)
    enc = xw.make_sequence(regime, variant, 5_000, k, m)
    s, want = both_oracles(enc, pssm, k)
    sc = want[:, :COLS]
    for t in xw.thresholds(want, COLS, pssm, k, xw.extra_thresholds(regime)):
        assert np.array_equal(co.threshold(want, COLS, t), no.threshold(want, COLS, t)), t
    assert not np.isnan(xw.thresholds(want, COLS, pssm, k)[8:]).any()
    if regime == "overflow_inf":
        real = real_sums(s, pssm, k)
        inf = np.isposinf(sc)
        assert inf.any()
        assert not xw.prefilter_sound(pssm, k) and xw.abs_sum(pssm, k) > xw.FLT_MAX
        if m >= 3:
            # A A A: +inf in f32 while the real sum stays below t = 3.2e38; A A C: +inf and above it
            assert (inf & (real < 3.2e38)).any() and (inf & (real >= 3.2e38)).any()
            assert np.isfinite(sc[real < 3.2e38][~inf[real < 3.2e38]]).any()
    elif regime == "overflow_nan":
        assert np.isnan(sc).any() and not np.isnan(pssm).any()
        assert np.isnan(sc[0, 0]) == (variant == "first")
        if variant == "first":
            assert co.argmax(want, COLS) == (0, 0)   # NaN at (0, 0): nothing compares >= it
        else:
            assert co.argmax(want, COLS) != (0, 0) and not np.isnan(sc[co.argmax(want, COLS)])
        assert not xw.prefilter_sound(pssm, k)
    elif regime == "near_overflow":
        lim = xw.no_overflow_limit(m)
        a = xw.abs_sum(pssm, k)
        assert (a < lim) == (variant == "below") and abs(a / lim - 1) < 2e-6
        assert xw.prefilter_sound(pssm, k) == (variant == "below")
        if variant == "below":                        # no window overflows (above the limit a few may)
            assert np.isfinite(sc[np.isfinite(real_sums(s, pssm, k))]).all()
        assert np.nanmax(np.where(np.isfinite(sc), sc, np.nan)) > 0.25 * xw.FLT_MAX / (1 if m < 37 else 4)
    elif regime == "wide_range":
        big = sc[np.isfinite(sc) & (sc > 1e29)]
        assert big.size and np.unique(big).size < big.size   # the small terms are absorbed: ties
        assert xw.prefilter_sound(pssm, k)
    elif regime == "subnormal":
        fin = sc[np.isfinite(sc)]
        sub = (fin != 0) & (np.abs(fin) < np.finfo(np.float32).tiny)
        assert sub.any() and (fin > 0).any() and (fin < 0).any()
        if variant == "mixed":
            assert (np.abs(fin) >= np.finfo(np.float32).tiny).any()
        else:
            assert (np.abs(fin) < np.finfo(np.float32).tiny).all()
        assert xw.prefilter_sound(pssm, k)
    elif regime == "signed_zero":
        assert (bits(pssm[0, :k]) == 0x80000000).all() and (bits(pssm[:, :k]) == 0x80000000).any()
        assert (bits(sc) == 0).all()                  # every score is +0.0: 0.0 + -0.0 = +0.0
        assert not xw.prefilter_sound(pssm, k)        # no spread
    elif regime == "tiny_range":
        assert xw.prefilter_sound(pssm, k)
        fin = sc[np.isfinite(sc)]
        assert xw.prefilter_td(pssm, k, float(fin.max())) < 1   # the error bound swamps the step: the exact route


def test_worked_example_of_the_overflow_hole():
    """DNA, M = 3, all weights 0 except w0[A] = w1[A] = 3e38, w2[A] = -3e38, N = -inf: AAA scores +inf in f32 while its
    real sum is 3e38, so it reaches t = 3.2e38; the discrete image of the old prefilter could not flag it."""
    k, m = 5, 3
    pssm = np.zeros((m, co.stride(k, 4)), np.float32)
    pssm[0, 0] = pssm[1, 0] = 3e38
    pssm[2, 0] = -3e38
    pssm[:, 4] = -np.inf
    enc = np.array([0, 0, 0, 1, 2, 3, 1, 2], np.uint8)   # AAA AAC ACT CTG TGC GCT
    s, want = both_oracles(enc, pssm, k, cols=1)
    assert np.isposinf(want[0, 0]) and np.isposinf(want[1, 0]) and want[2, 0] == np.float32(3e38)
    assert [tuple(map(int, rc)) for rc in co.threshold(want, 1, 3.2e38)] == [(0, 0), (1, 0)]
    assert not xw.prefilter_sound(pssm, k)
    # without the overflow check, AAA's discrete sum would sit below the discrete threshold
    step = 9e38 / 32000
    d_aaa = sum(int(np.ceil((float(np.float32(w)) - lo) / step)) for w, lo in ((3e38, 0.0), (3e38, 0.0), (-3e38, -3e38)))
    assert d_aaa < xw.prefilter_td(pssm, k, 3.2e38)


def test_kmer_bound_is_the_sequential_sum():
    pssm = xw.make_pssm("overflow_inf", "ninf_head", 7, 5)
    assert np.isposinf(xw.kmer_bound(pssm, 5))
    pssm = xw.make_pssm("wide_range", "", 7, 5)
    b = np.float32(0)
    for row in pssm[:, :5]:
        b = np.float32(b + row.max())
    assert bits(xw.kmer_bound(pssm, 5)) == bits(b)


def test_planted_argmax_construction():
    """The 101 Mbp candidate-route case: the only +inf windows are the planted ones, the reference's argmax is the last
    of them, the sample of the route reads none of them (nor a NaN), and the image of real sums would not flag the
    argmax at the sample's bound -- so without the no-overflow limit the route would return a finite maximum."""
    k, m, cols = 5, xw.PLANT_M, xw.PLANT_COLS
    enc, plants = xw.planted_argmax_sequence()
    s = co.stripe(enc, cols, k)
    co.configure_wrap(s, m - 1)
    pssm = xw.planted_argmax_pssm(True)
    want, _ = co.score_rows(s, pssm)
    sc = want[:, :cols]
    inf = np.argwhere(np.isposinf(sc))
    assert sorted(map(tuple, inf.tolist())) == sorted(plants)
    assert np.isnan(sc).sum() == len(plants)
    assert co.argmax(want, cols) == max(plants)
    sample, _ = xw.sampled_rows(s.rows)
    bound = sc[sample]
    assert not np.isnan(bound).any() and not np.isposinf(bound).any()   # (-inf: T + T) and bound.max() > 2e38
    assert xw.unflagged_near(enc, pssm, max(plants), float(np.max(bound[np.isfinite(bound)])))
    assert not xw.prefilter_sound(pssm, k) and xw.prefilter_sound(xw.planted_argmax_pssm(False), k)
