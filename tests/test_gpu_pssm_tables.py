"""Every table of a scoring matrix's device image (csrc/pssm_tables.hpp: one allocation per matrix, lm_hip_pssm's d_* fields
are views into it) reaches the route that reads it: one case per table, C = 32, on 12 800 symbols (400 rows: more than any
slice length, several streams per kernel) of DNA and of protein, bit for bit against the C oracle -- f32 bit patterns of the
stored scores, exact hit lists and values of the fused threshold at a threshold with 10 ... 200 hits.  ``last_kernel`` is
asserted wherever it names the route, so that a fallback cannot hide a wrong table.  Then matrices whose image has no
prefilter (a NaN weight, weights above the no-overflow limit), and handles created, destroyed and created again."""
import functools

import numpy as np
import pytest

import extreme_weights as xw
import lightmotif_amd as lm
from oracle import c_oracle as co

pytestmark = pytest.mark.gpu
COLS, LENGTH, HITS = 32, 12_800, 60


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def ceil4(m):
    return -(-m // 4) * 4


@functools.lru_cache(maxsize=None)
def encoded(k):
    rng = np.random.default_rng(1000 + k)
    enc = rng.integers(0, k - 1, LENGTH).astype(np.uint8)
    enc[rng.random(LENGTH) < 0.005] = k - 1   # N / X
    enc.setflags(write=False)
    return enc


def weights(m, k, seed=0):
    """(M, stride(K)) f32: normal weights, the default symbol's column -inf."""
    p = np.zeros((m, co.stride(k, 4)), np.float32)
    p[:, :k - 1] = np.random.default_rng([m, k, seed]).normal(0, 2, (m, k - 1))
    p[:, k - 1] = -np.inf
    return p


def expected(pssm_np, k, cols=COLS):
    """The oracle's scores and a threshold that HITS of its finite scores reach."""
    s = co.stripe(encoded(k), cols, k)
    co.configure_wrap(s, pssm_np.shape[0] - 1)
    want, _ = co.score_rows(s, pssm_np)
    fin = np.sort(want[:, :cols][np.isfinite(want[:, :cols])].ravel())
    return want, float(fin[-HITS])


@functools.lru_cache(maxsize=None)
def case(m, k, seed=0):
    pssm_np = weights(m, k, seed)
    want, t = expected(pssm_np, k)
    want.setflags(write=False)
    return lm.ScoringMatrix(pssm_np, protein=k == 21), want, t


_PIPES = {}


def pipeline(**options):
    key = tuple(sorted(options.items()))
    if key not in _PIPES:
        _PIPES[key] = lm.Pipeline.hip(0)
        for name, value in options.items():
            _PIPES[key].set_option(name, value)
    return _PIPES[key]


def striped(pli, k, m, cols=COLS):
    seq = pli.stripe(lm.EncodedSequence(encoded(k), protein=k == 21), cols)
    seq.configure_wrap(m - 1)
    return seq


def check_score(pli, pssm, want, k, kernel=None, cols=COLS):
    got = pli.score(pssm, striped(pli, k, len(pssm), cols)).matrix()
    assert got.shape == want.shape and np.array_equal(bits(got[:, :cols]), bits(want[:, :cols])), (len(pssm), k, pli.last_kernel)
    assert kernel is None or pli.last_kernel == kernel, (len(pssm), k, pli.last_kernel)


def check_hits(rc, vals, want, t, ctx):
    wrc = co.threshold(want, COLS, t)
    assert 10 <= len(wrc) <= 200, (ctx, len(wrc))
    assert [tuple(map(int, x)) for x in rc] == [tuple(x) for x in wrc.tolist()], ctx
    assert np.array_equal(bits(vals), bits(want[wrc[:, 0], wrc[:, 1]])), ctx


def check_threshold(pli, pssm, want, t, k, kernel, scanned=None):
    rc, vals = pli.score_threshold(pssm, striped(pli, k, len(pssm)), t)
    ctx = (len(pssm), k, pli.last_kernel, pli.last_scan_info)
    check_hits(rc, vals, want, t, ctx)   # (the exact re-scoring behind a prefilter scan reads d_dense)
    assert pli.last_kernel == kernel and (scanned is None or pli.last_scan_info[0] == scanned), ctx


def test_dense_table_scores_one_column():
    pssm_np = weights(12, 5)
    want, _ = expected(pssm_np, 5, cols=1)
    pli = pipeline()
    check_score(pli, lm.ScoringMatrix(pssm_np), want, 5, cols=1)
    assert pli.last_kernel in ("score_tiled", "score_generic<0>")


@pytest.mark.parametrize("m,k", [(8, 5), (36, 5), (8, 21), (36, 21)])
def test_transposed_table(m, k):
    pssm, want, _ = case(m, k)
    check_score(pipeline(), pssm, want, k, f"score_c32<{m},0>")


@pytest.mark.parametrize("m,k", [(5, 5), (19, 5), (30, 5), (19, 21), (33, 5)])
def test_padded_table(m, k):
    """M = 33 has no padded table (36 rows would cost more than they save): it still scores, as 33 rows."""
    pssm, want, _ = case(m, k)
    check_score(pipeline(), pssm, want, k, f"score_c32<{m if m > 32 else ceil4(m)},0>")


@pytest.mark.parametrize("m,k", [(40, 5), (64, 5), (37, 21)])
def test_one_slice_store_and_exact_threshold(m, k):
    pssm, want, t = case(m, k)
    check_score(pipeline(), pssm, want, k, f"score_c32<{ceil4(m)},0>")
    check_threshold(pipeline(prefilter=0), pssm, want, t, k, f"score_c32<{ceil4(m)},2>")


@pytest.mark.parametrize("m,k", [(72, 5), (88, 5), (67, 21)])
def test_one_slice_store_only(m, k):
    pssm, want, _ = case(m, k)
    check_score(pipeline(), pssm, want, k, f"score_c32<{-(-m // 8) * 8},0>")


@pytest.mark.parametrize("m,k,options", [(100, 5, {}), (100, 21, {}), (72, 5, {"xlong_store": 0})])
def test_slices(m, k, options):
    """(the option is set before the matrix gets its device handle on that pipeline: it decides how the motif is cut)"""
    pssm, want, _ = case(m, k)
    check_score(pipeline(**options), pssm, want, k, "score_c32_sliced")


@pytest.mark.parametrize("m", [8, 12])
def test_one_symbol_image_protein(m):
    pssm, want, t = case(m, 21)
    check_threshold(pipeline(), pssm, want, t, 21, "score_c32_prefilter_blk", scanned=m)
    check_threshold(pipeline(block_prefilter=0), pssm, want, t, 21, "score_c32_prefilter", scanned=m)


@pytest.mark.parametrize("m", [12, 40, 100])
def test_pair_image_dna(m):
    """M = 12 has no drop form; 40 and 100 are the long-motif branch (the pair table alone)."""
    pssm, want, t = case(m, 5)
    check_threshold(pipeline(), pssm, want, t, 5, "score_c32_prefilter2", scanned=m)


@pytest.mark.parametrize("m", [20, 36])
def test_drop_last_image_dna(m):
    pssm, want, t = case(m, 5)
    check_threshold(pipeline(), pssm, want, t, 5, "score_c32_prefilter2", scanned=m - 1)
    check_threshold(pipeline(drop_last=0), pssm, want, t, 5, "score_c32_prefilter2", scanned=m)


def test_multi_motif_images_in_one_batch():
    pli = pipeline()
    cases = [case(12, 5, seed) for seed in range(4)] + [case(20, 5, seed) for seed in range(3)]
    seq = striped(pli, 5, 20)
    hits = pli.scan_threshold_batch([c[0] for c in cases], [c[2] for c in cases], seq)
    assert pli.last_kernel == "score_c32_prefilter2_multi"
    for i, (pssm, want, t) in enumerate(cases):
        rc, vals = hits[i]
        check_hits(rc, vals, want, t, (i, len(pssm)))


@pytest.mark.parametrize("what", ["nan", "above_limit"])
def test_matrices_without_an_image_take_the_exact_route(what):
    m, k = 20, 5
    if what == "nan":
        pssm_np = weights(m, k, seed=9)
        pssm_np[7, 2] = np.nan
    else:
        pssm_np = xw.make_pssm("near_overflow", "above", m, k)
    assert not xw.prefilter_sound(pssm_np, k)
    want, t = expected(pssm_np, k)
    pli = pipeline()
    pssm = lm.ScoringMatrix(pssm_np)
    got = pli.score(pssm, striped(pli, k, m)).matrix()
    nan = np.isnan(want[:, :COLS])   # (the bits of a computed NaN are the adding unit's choice)
    assert np.array_equal(np.isnan(got[:, :COLS]), nan) and np.array_equal(bits(got[:, :COLS][~nan]), bits(want[:, :COLS][~nan]))
    check_threshold(pli, pssm, want, t, k, f"score_c32<{m},2>")


def test_handles_created_destroyed_and_created_again():
    pli = pipeline()
    shapes = [(m, k) for m in (3, 8, 19, 20, 33, 36, 40, 72, 100, 130) for k in (5, 21)]

    def make(i):
        m, k = shapes[i % len(shapes)]
        pssm_np = weights(m, k, seed=100 + i)
        pssm = lm.ScoringMatrix(pssm_np, protein=k == 21)
        pssm._device(pli)   # the device handle, now
        return pssm, pssm_np, k

    live = [make(i) for i in range(40)]
    live = live[::2]                                      # every second one goes (ScoringMatrix.__del__ destroys its handles)
    live += [make(i) for i in range(40, 60)]
    survivor, survivor_np, _ = next(x for x in live if x[2] == 5 and len(x[0]) == 20)
    rc = survivor.reverse_complement()                    # made by the library from the survivor's handle
    live.append((rc, np.ascontiguousarray(rc.data), 5))
    assert np.array_equal(bits(rc.data[:, :5]), bits(survivor_np[::-1, [2, 3, 0, 1, 4]]))
    for pssm, pssm_np, k in live:
        want, _ = expected(pssm_np, k)
        check_score(pli, pssm, want, k)
