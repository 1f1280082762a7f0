"""Many-motif batches (lm_hip_scan_threshold_batch / lm_hip_scan_argmax_batch) against the C oracle, job by job.

The batch entry points do not loop over the single-motif calls: they sort every job into a kind (skip, pair scan with
several motifs per pass or one, one-symbol prefilter, exact, chunked, generic), group the jobs, pad multi-motif groups,
upload one job table and re-score candidates with the weights in LDS or in global memory.  These tests build batches
that reach each of those parts on purpose -- protein batches, long motifs, other column counts, +-inf / NaN thresholds
and weights, groups past 32 768 jobs, state carried from call to call -- and compare every job with
``co.score_rows`` + ``co.argmax`` / ``co.threshold``: hit coordinates in row-major order, hit values, the argmax cell and
its value, bit for bit (any NaN equals any NaN, see ``test_gpu_extreme_weights.same``).

``test_dna_batch_routes`` scores every job of the all-kinds batch alone and asserts the kind it was built to take, so
that the construction, not luck, decides which paths the batches cover."""
import os
import re
import time
from functools import lru_cache

import numpy as np
import pytest

import extreme_weights as xw
import lightmotif_amd as lm
from oracle import c_oracle as co

pytestmark = pytest.mark.gpu

_PIPES = {}


def pipeline(options):
    key = tuple(sorted(options.items()))
    if key not in _PIPES:
        p = lm.Pipeline.hip(0)
        for name, value in options.items():
            p.set_option(name, value)
        _PIPES[key] = p
    return _PIPES[key]


def opt_id(options):
    return ",".join(f"{k}={v}" for k, v in options.items()) or "default"


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(a, b):
    """Bit for bit, except that any NaN equals any NaN (test_gpu_extreme_weights.same)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(bits(a[~na]), bits(b[~nb]))


def realised(want, cols, kind):
    """A threshold at a score the matrix realises on this sequence (quantile, minimum or maximum of the finite cells),
    just above the maximum, or one of the non-finite ones."""
    if kind in ("-inf", "+inf", "nan"):
        return {"-inf": -np.inf, "+inf": np.inf, "nan": np.nan}[kind]
    v = want[:, :cols]
    fin = np.sort(v[np.isfinite(v)])
    if fin.size == 0:
        return 0.0
    if kind == "min":
        return float(fin[0])
    if kind == "max":
        return float(fin[-1])
    if kind == "above":
        return float(np.nextafter(fin[-1], np.float32(np.inf)))
    q = float(kind[1:])
    return float(fin[min(int(q * (fin.size - 1)), fin.size - 1)])


def make_enc(rng, length, k, rare=0.02):
    enc = rng.integers(0, k - 1, length, dtype=np.uint8)
    enc[rng.random(length) < rare] = k - 1      # N / X
    return enc


def make_matrix(rng, m, k, kind="normal"):
    p = np.zeros((m, co.stride(k, 4)), np.float32)
    p[:, :k] = rng.integers(-3, 4, (m, k)) if kind == "ties" else rng.normal(0, 2, (m, k))
    if kind != "finite_default":
        p[:, k - 1] = -np.inf
    if kind == "neg_inf_cells":
        p[:, :k][rng.random((m, k)) < 0.05] = -np.inf
    if kind == "pos_inf":
        p[int(rng.integers(0, m)), int(rng.integers(0, k - 1))] = np.inf
    if kind == "nan":
        p[int(rng.integers(0, m)), int(rng.integers(0, k - 1))] = np.nan
    return p


class Case:
    """One sequence (host form for the oracle, device form per pipeline) and its motifs with their oracle scores."""

    def __init__(self, enc, k, cols, mats, extra_wrap=0, pssms=None):
        self.enc, self.k, self.cols, self.protein = enc, k, cols, k == 21
        self.mats = mats
        self.wrap = max(max(p.shape[0] for p in mats) - 1, 0) + extra_wrap
        self.ref = co.stripe(enc, cols, k)
        co.configure_wrap(self.ref, self.wrap)
        self.wants = [co.score_rows(self.ref, p)[0] for p in mats]
        self.pssms = [lm.ScoringMatrix(p, protein=self.protein) for p in mats] if pssms is None else pssms
        self._seqs = {}

    def seq(self, pli):
        if id(pli) not in self._seqs:
            s = pli.stripe(lm.EncodedSequence(self.enc, protein=self.protein), self.cols)
            s.configure_wrap(self.wrap)
            self._seqs[id(pli)] = s
        return self._seqs[id(pli)]


def check_threshold_batch(case, pli, ts, pssms=None, idx=None, seq=None, tag=""):
    idx = range(len(case.mats)) if idx is None else idx
    pssms = [case.pssms[i] for i in idx] if pssms is None else pssms
    hits = pli.scan_threshold_batch(pssms, [ts[i] for i in idx], case.seq(pli) if seq is None else seq)
    assert len(hits) == len(idx)
    for j, i in enumerate(idx):
        coords, values = hits[j]
        want = case.wants[i]
        if want.shape[0] == 0:
            assert len(coords) == 0, (tag, i)
            continue
        wrc = co.threshold(want, case.cols, ts[i]).astype(np.int64).reshape(-1, 2)
        assert np.array_equal(coords, wrc), (tag, i, case.mats[i].shape[0], ts[i], len(coords), len(wrc), pli.last_kernel)
        assert same(values, want[wrc[:, 0], wrc[:, 1]]), (tag, i, ts[i])
    return hits


def check_argmax_batch(case, pli, idx=None, tag=""):
    idx = range(len(case.mats)) if idx is None else idx
    am = pli.scan_argmax_batch([case.pssms[i] for i in idx], case.seq(pli))
    assert len(am) == len(idx)
    for j, i in enumerate(idx):
        want = case.wants[i]
        if want.shape[0] == 0:
            assert am[j] is None, (tag, i)
            continue
        wa = co.argmax(want, case.cols)
        if wa is None:
            assert am[j] is None, (tag, i)
            continue
        assert am[j] is not None and am[j][0] == wa, (tag, i, case.mats[i].shape[0], am[j], wa, pli.last_kernel)
        assert same(am[j][1], want[wa]), (tag, i)
    return am


# ---- a. protein batches -------------------------------------------------------------------------------------------

PROTEIN_OPTIONS = [{}, {"block_prefilter": 0}, {"pair_prefilter_protein": 1}, {"prefilter": 0}]
QUANTILES = ("q0.5", "q0.99", "q0.9999", "max", "above")


@lru_cache(maxsize=None)
def protein_case(which):
    rng = np.random.default_rng(4_100 if which == "short" else 4_200)
    if which == "short":   # every length of the short family, three motifs each
        lengths = [m for m in range(1, 37) for _ in range(3)]
        length = 30_011
    else:                  # long protein motifs: the wide exact kernels (M % 4 == 0 up to 64) and the chunked route
        lengths = [37, 40, 44, 48, 53, 60, 64, 64, 65, 72, 81, 88, 90]
        length = 20_003
    kinds = ["normal", "ties", "finite_default", "neg_inf_cells"]
    mats = [make_matrix(rng, m, 21, kinds[i % 4]) for i, m in enumerate(lengths)]
    return Case(make_enc(rng, length, 21), 21, 32, mats)


@pytest.mark.parametrize("options", PROTEIN_OPTIONS, ids=opt_id)
@pytest.mark.parametrize("which", ["short", "long"])
def test_protein_batch(which, options):
    case = protein_case(which)
    pli = pipeline(options)
    check_argmax_batch(case, pli, tag=which)
    for shift in range(len(QUANTILES)):     # every job meets every threshold kind once
        ts = [realised(w, 32, QUANTILES[(i + shift) % len(QUANTILES)]) for i, w in enumerate(case.wants)]
        check_threshold_batch(case, pli, ts, tag=f"{which} shift {shift}")


# ---- b. one DNA batch that reaches every kind ---------------------------------------------------------------------

SENTINEL_M = 3   # the store kernel run before each single job: no job of the batch has this length

MULTI_GROUPS = [(8, 6), (12, 4), (20, 3), (28, 2), (34, 2)]   # (M, jobs): 4 / 4 / 2 / 2 / 1 motifs per pass


def pair_multi(m):
    """Motifs per pass of score_c32_prefilter2_multi (score_prefilter2.hpp: prefilter2_multi)."""
    npair = ((m | 3) + 1) // 2
    return 4 if npair <= 8 else 2 if npair <= 16 else 1


@lru_cache(maxsize=None)
def dna_kinds_case():
    """The jobs, each with the kind it is built to take under the default options ("route") and its threshold."""
    rng = np.random.default_rng(4_300)
    jobs = []   # (route, pssm, threshold kind or value)
    for m, count in MULTI_GROUPS:
        for _ in range(count):
            jobs.append(("multi" if pair_multi(m) > 1 else "pair", make_matrix(rng, m, 5), "q0.99"))
    jobs.append(("pair", make_matrix(rng, 17, 5), "q0.999"))                # a lone motif: one pair pass
    jobs.append(("prefilter1", make_matrix(rng, 1, 5), "q0.9"))             # M = 1: the one-symbol scan
    p = make_matrix(rng, 10, 5)
    jobs.append(("skip", p, float(xw.kmer_bound(p, 5)) + 0.5))              # above the best k-mer
    jobs.append(("skip", make_matrix(rng, 14, 5), "+inf"))                   # +inf is above every best k-mer too
    jobs.append(("exact", make_matrix(rng, 6, 5), "-inf"))
    jobs.append(("exact", make_matrix(rng, 22, 5), "nan"))
    jobs.append(("exact", make_matrix(rng, 15, 5, "pos_inf"), "q0.99"))      # no sound prefilter
    jobs.append(("exact", make_matrix(rng, 26, 5, "pos_inf"), "+inf"))
    jobs.append(("exact", make_matrix(rng, 25, 5, "nan"), "q0.5"))
    jobs.append(("exact", make_matrix(rng, 18, 5), "min_kmer"))              # maps below 1 in the 16-bit range
    for m in (41, 64, 65, 97, 128):
        jobs.append(("pair", make_matrix(rng, m, 5), "q0.999"))
    for m in (129, 160, 200):
        jobs.append(("chunked", make_matrix(rng, m, 5), "q0.999"))
    case = Case(make_enc(rng, 120_007, 5, 0.01), 5, 32, [p for _, p, _ in jobs])
    case.routes = [r for r, _, _ in jobs]
    case.ts = []
    for (route, p, t), want in zip(jobs, case.wants):
        if t == "min_kmer":   # the sum of the finite row minima: the discrete map's zero
            t = float(np.nanmin(np.where(np.isneginf(p[:, :5]), np.nan, p[:, :5]), axis=1).astype(np.float32).sum())
        case.ts.append(realised(want, 32, t) if isinstance(t, str) else t)
    return case


DNA_OPTIONS = [{}, {"multi_motif": 0}, {"pair_prefilter": 0}, {"skip_unreachable": 0}, {"chunked_fused": 0},
               {"prefilter": 0}]


@pytest.mark.parametrize("options", DNA_OPTIONS, ids=opt_id)
def test_dna_batch_every_kind(options):
    case = dna_kinds_case()
    pli = pipeline(options)
    check_argmax_batch(case, pli, tag=opt_id(options))
    check_threshold_batch(case, pli, case.ts, tag=opt_id(options))


def test_dna_batch_routes():
    """Each job of the all-kinds batch alone (a batch of one) takes the kind it was built for, and gives what the
    batch and the oracle give; each multi-motif group alone runs the multi-motif passes."""
    case = dna_kinds_case()
    pli = pipeline({})
    seq = case.seq(pli)
    batch = check_threshold_batch(case, pli, case.ts, tag="batch")
    sentinel = lm.ScoringMatrix(make_matrix(np.random.default_rng(1), SENTINEL_M, 5))
    seen = set()
    for i, route in enumerate(case.routes):
        p, t = case.mats[i], case.ts[i]
        if route in ("multi", "pair", "prefilter1"):
            assert xw.prefilter_sound(p, 5) and xw.prefilter_td(p, 5, t) >= 1, (i, route)
        if route == "skip":
            assert xw.prefilter_sound(p, 5) and t > xw.kmer_bound(p, 5), i
        if route == "exact" and np.isfinite(t) and xw.prefilter_sound(p, 5):
            assert xw.prefilter_td(p, 5, t) < 1, i
        pli.score(sentinel, seq)
        before = pli.last_kernel   # a store kernel: no name a threshold scan leaves
        assert "prefilter" not in before and not before.endswith(",2>") and "reduce" not in before, before
        alone = check_threshold_batch(case, pli, case.ts, idx=[i], tag=f"alone {i}")
        got = pli.last_kernel
        if route == "skip":
            assert got == before and pli.last_scan_info == (0, 0), (i, got)
        elif route in ("multi", "pair"):
            assert got == "score_c32_prefilter2", (i, route, got)
        elif route == "prefilter1":
            assert got in ("score_c32_prefilter", "score_c32_prefilter_blk"), (i, got)
        elif route == "exact":
            assert re.fullmatch(r"score_c32<\d+,2>", got), (i, got)
        elif route == "chunked":
            assert got == "score_c32_sliced+reduce", (i, got)
        seen.add(route)
        assert np.array_equal(alone[0][0], batch[i][0]) and same(alone[0][1], batch[i][1]), i
    assert seen == {"multi", "pair", "prefilter1", "skip", "exact", "chunked"}
    for m, count in MULTI_GROUPS:
        idx = [i for i, p in enumerate(case.mats) if p.shape[0] == m]
        assert len(idx) == count
        check_threshold_batch(case, pli, case.ts, idx=idx, tag=f"group M={m}")
        assert pli.last_kernel == ("score_c32_prefilter2_multi" if pair_multi(m) > 1 else "score_c32_prefilter2"), m


# ---- c. where the re-scoring kernel keeps the weights ---------------------------------------------------------------

# (k, M, jobs): rescore_candidates stages the weights in LDS for n <= 8 jobs and sum(M * K) <= 2048 floats
RESCORE = {"dna-8-jobs": (5, 10, 8), "dna-9-jobs": (5, 10, 9), "dna-M128-x3": (5, 128, 3), "dna-M128-x4": (5, 128, 4),
           "protein-M36-x2": (21, 36, 2), "protein-M36-x3": (21, 36, 3)}


@pytest.mark.parametrize("which", sorted(RESCORE))
def test_rescore_table_placement(which):
    k, m, n = RESCORE[which]
    rng = np.random.default_rng([4_400, k, m, n])
    # no N / X: every window scores finitely, so the quantiles below make most cells candidates even at M = 128
    case = Case(make_enc(rng, 40_009, k, 0.0), k, 32, [make_matrix(rng, m, k) for _ in range(n)])
    pli = pipeline({})
    for q in ("q0.5", "q0.9"):   # dense: most cells are candidates and get re-scored
        ts = [realised(w, 32, q) for w in case.wants]
        hits = check_threshold_batch(case, pli, ts, tag=f"{which} {q}")
        assert hits.total > 1000 * n
    check_argmax_batch(case, pli, tag=which)


# ---- d. other column counts ---------------------------------------------------------------------------------------

@lru_cache(maxsize=None)
def cols_case(protein, cols, length):
    k = 21 if protein else 5
    rng = np.random.default_rng([4_500, k, cols, length])
    lengths = [1, 5, 12, 12, 12, 20, 36, 37, 64, 90] + ([] if protein else [128, 150])
    kinds = ["normal", "ties", "neg_inf_cells", "finite_default"]
    return Case(make_enc(rng, length, k), k, cols, [make_matrix(rng, m, k, kinds[i % 4]) for i, m in enumerate(lengths)])


# 3 001 positions: the generic / tiled kernels; 70 001: past the chunked route's 2^16 cells
COLS = [(p, c, n) for c in (16, 1, 33) for p in (False, True) for n in (3_001, 70_001)]


@pytest.mark.parametrize("protein,cols,length", COLS,
                         ids=[f"{'protein' if p else 'dna'}-C{c}-L{n}" for p, c, n in COLS])
def test_other_column_counts(protein, cols, length):
    case = cols_case(protein, cols, length)
    pli = pipeline({})
    check_argmax_batch(case, pli, tag=f"C={cols}")
    for kinds in (("q0.99", "q0.5", "max", "above"), ("-inf", "q0.9999", "min", "nan")):
        ts = [realised(w, cols, kinds[i % len(kinds)]) for i, w in enumerate(case.wants)]
        check_threshold_batch(case, pli, ts, tag=f"C={cols} {kinds}")


# ---- e. state carried from call to call -----------------------------------------------------------------------------

def test_state_across_calls():
    """Hit-list capacity is carried from call to call (the context's last counts) and a batch whose list overflows is
    re-run: a dense batch on a fresh pipeline, then a sparse one, then the dense one again, then the same prepared
    batches over sequences of other lengths and wraps -- all on one pipeline, every result against the oracle."""
    rng = np.random.default_rng(4_600)
    lengths = [8, 8, 8, 8, 8, 12, 20, 20, 33, 41, 70]
    mats = [make_matrix(rng, m, 5, "neg_inf_cells" if i % 3 == 0 else "normal") for i, m in enumerate(lengths)]
    first = Case(make_enc(rng, 150_001, 5), 5, 32, mats)
    pli = lm.Pipeline.hip(0)   # fresh: nothing carried from other tests
    dense_ts = [realised(w, 32, "min") for w in first.wants]
    sparse_ts = [realised(w, 32, "q0.9999") for w in first.wants]
    dense = pli.prepare_batch(first.pssms, dense_ts)
    sparse = pli.prepare_batch(first.pssms, sparse_ts)
    seq = first.seq(pli)
    n_dense = check_threshold_batch(first, pli, dense_ts, pssms=dense, seq=seq, tag="dense").total
    assert n_dense > (1 << 16) and n_dense > 150_001 * len(lengths) // 8192   # past the first call's capacity
    n_sparse = check_threshold_batch(first, pli, sparse_ts, pssms=sparse, seq=seq, tag="sparse").total
    assert 0 < n_sparse < n_dense // 100
    check_threshold_batch(first, pli, dense_ts, pssms=dense, seq=seq, tag="dense again")
    check_argmax_batch(first, pli, tag="argmax")
    for length, extra_wrap in ((40_003, 7), (333_331, 0)):
        other = Case(make_enc(rng, length, 5), 5, 32, mats, extra_wrap, first.pssms)
        s = other.seq(pli)
        assert s.wrap == other.wrap
        check_threshold_batch(other, pli, dense_ts, pssms=dense, seq=s, tag=f"dense L={length}")
        check_threshold_batch(other, pli, sparse_ts, pssms=sparse, seq=s, tag=f"sparse L={length}")
        check_argmax_batch(other, pli, tag=f"argmax L={length}")


# ---- f. very large batches ------------------------------------------------------------------------------------------

def test_forty_thousand_motifs():
    """40 000 jobs over 20 kbp: 36 000 of M = 8, all of them pair-scan jobs (asserted below), so that one group passes
    the 32 768-job limit and splits; the rest of every other length up to 36.  The job table is far past the single
    pinned copy (kPinnedBytes / 2).  Every job has a matrix handle of its own; the weights come from 2 571 distinct
    matrices (cycled, so that the motifs sharing a multi-motif pass differ; the oracle scores each once) and the
    thresholds cycle through several kinds, so a job that took another job's matrix, threshold or hits would show.  Creating the 40 000 handles is most of the test's time (the batch calls take
    a few tens of milliseconds); the test prints both."""
    rng = np.random.default_rng(4_700)
    enc = make_enc(rng, 20_011, 5)
    t0 = time.perf_counter()
    pool8 = [make_matrix(rng, 8, 5) for _ in range(331)]
    other = {m: [make_matrix(rng, m, 5) for _ in range(64)] for m in range(1, 37) if m != 8}
    lengths = [8] * 36_000 + [int(x) for x in rng.choice([m for m in range(1, 37) if m != 8], 4_000)]
    rng.shuffle(lengths)
    order = {}
    mats_np, keys = [], []
    for m in lengths:
        j = order.get(m, 0)
        order[m] = j + 1
        pool = pool8 if m == 8 else other[m]
        mats_np.append(pool[j % len(pool)])
        keys.append((m, j % len(pool)))
    pssms = [lm.ScoringMatrix(p) for p in mats_np]
    pli = pipeline({})
    for p in pssms:
        p._device(pli)
    t_create = time.perf_counter() - t0
    ref = co.stripe(enc, 32, 5)
    co.configure_wrap(ref, 35)
    want = {}
    for key, p in zip(keys, mats_np):
        if key not in want:
            want[key] = co.score_rows(ref, p)[0]
    kinds = ("q0.999", "q0.99", "q0.9999", "max", "above")   # M = 8: not "above" (it may pass the best k-mer: skipped)
    ts = [realised(want[key], 32, kinds[i % (4 if key[0] == 8 else 5)]) for i, key in enumerate(keys)]
    pair8 = {}   # (matrix, threshold) -> the classifier takes the pair scan: sound prefilter, no skip, td >= 1
    for i, key in enumerate(keys):
        if key[0] == 8 and (key, ts[i]) not in pair8:
            p = mats_np[i]
            pair8[key, ts[i]] = (xw.prefilter_sound(p, 5) and ts[i] <= xw.kmer_bound(p, 5)
                                 and xw.prefilter_td(p, 5, ts[i]) >= 1)
    assert sum(pair8[key, ts[i]] for i, key in enumerate(keys) if key[0] == 8) > 32_768
    seq = pli.stripe(lm.EncodedSequence(enc), 32)
    seq.configure_wrap(35)
    t1 = time.perf_counter()
    hits = pli.scan_threshold_batch(pssms, ts, seq)
    am = pli.scan_argmax_batch(pssms, seq)
    t_scan = time.perf_counter() - t1
    assert len(hits) == len(am) == 40_000
    for i, key in enumerate(keys):
        w = want[key]
        wrc = co.threshold(w, 32, ts[i]).astype(np.int64).reshape(-1, 2)
        coords, values = hits[i]
        assert np.array_equal(coords, wrc), (i, key, ts[i], len(coords), len(wrc))
        assert np.array_equal(bits(values), bits(w[wrc[:, 0], wrc[:, 1]])), i
        wa = co.argmax(w, 32)
        assert am[i][0] == wa and bits(np.float32(am[i][1])) == bits(w[wa]), (i, key)
    print(f"40 000 jobs: {len(pssms)} matrices ({len(want)} distinct) created in {t_create:.2f} s, both batch calls {t_scan:.2f} s, "
          f"{hits.total} hits")


def test_argmax_batch_both_sides_of_the_pinned_job_table():
    """scan_argmax_batch with 65 536 and with 65 537 jobs: the two sides of the edge at which the exact route's job table
    (16 bytes of result + 48 bytes of FinalizeJob per job, 64 n <= 4 194 304 = the pinned block; argmax_plan.hpp:
    exact_zero_copy, asserted at this figure by tests/cpp/test_argmax_plan.cpp) no longer fits the pinned block, so that
    table and results travel by staged copies through the device scratch instead of being read and written in place.
    The jobs cycle over 40 matrices of lengths 1 ... 36 on a 2 011 bp sequence (63 rows: far below the suffix and candidate
    routes); each matrix's best k-mer is planted at a place of its own, so that the answers differ, and one matrix has a
    NaN weight under the sequence's first window, so that the first-cell rule (pli/mod.rs:142-146) passes through both
    deliveries.  The oracle scores each matrix once."""
    rng = np.random.default_rng(65_537)
    lengths = list(range(1, 37)) + [4, 8, 20, 33]
    enc = make_enc(rng, 2_011, 5)
    mats = [make_matrix(rng, m, 5) for m in lengths]
    for i, p in enumerate(mats):   # the plant: 50 positions apart, the longest motif has 36 rows
        enc[3 + 50 * i:3 + 50 * i + p.shape[0]] = np.argmax(p[:, :4], axis=1)
    mats[11][0, enc[0]] = np.nan   # (M = 12) scores[0][0] is NaN: the answer is cell (0, 0), whatever else the matrix scores
    case = Case(enc, 5, 32, mats)
    assert np.isnan(case.wants[11][0, 0]) and co.argmax(case.wants[11], 32) == (0, 0)
    wants = [co.argmax(w, 32) for w in case.wants]
    assert len({wa for wa in wants}) >= 35   # the plants took: (nearly) every matrix has a cell of its own
    pli = pipeline({})
    seq = case.seq(pli)
    for n in (65_536, 65_537):
        pssms = [case.pssms[j % len(mats)] for j in range(n)]
        t0 = time.perf_counter()
        am = pli.scan_argmax_batch(pssms, seq)
        dt = time.perf_counter() - t0
        assert len(am) == n
        for j in range(n):
            i = j % len(mats)
            assert am[j] is not None and am[j][0] == wants[i], (n, j, lengths[i], am[j], wants[i])
            assert same(am[j][1], case.wants[i][wants[i]]), (n, j, lengths[i], am[j])
        print(f"scan_argmax_batch, {n} jobs over {len(mats)} matrices: {dt:.3f} s")


# ---- g. seeded mixed-batch fuzz -------------------------------------------------------------------------------------

MIX_SEEDS = range(int(os.environ.get("LM_FUZZ_BATCH_MIX_FIRST", "0")), int(os.environ.get("LM_FUZZ_BATCH_MIX_LAST", "60")))
MIX_OPTIONS = DNA_OPTIONS + [{"block_prefilter": 0}, {"pair_prefilter_protein": 1}]
MIX_THRESHOLDS = ("q0.5", "q0.99", "q0.9999", "max", "above", "min", "-inf", "+inf", "nan", "kmer")


@pytest.mark.parametrize("seed", MIX_SEEDS)
def test_random_mixed_batch(seed):
    """Alphabet, 1 ... 40 jobs of 1 ... 200 rows, the column count, weight kinds (+inf / NaN cells included),
    thresholds and option set drawn per seed; sequences short enough for some jobs to be degenerate (L < M)."""
    rng = np.random.default_rng(120_000 + seed)
    protein = rng.random() < 0.3
    k = 21 if protein else 5
    cols = int(rng.choice([32, 32, 16, 1, 33]))
    n = int(rng.integers(1, 41))
    pool = [int(x) for x in rng.integers(1, 201, 3)] + [int(x) for x in rng.integers(1, 37, 3)]
    lengths = [int(rng.choice(pool)) if rng.random() < 0.7 else int(rng.integers(1, 201)) for _ in range(n)]
    length = int(rng.choice([150, 2_000, 20_000, 70_000, 150_000]))
    wkinds = ["normal", "normal", "ties", "finite_default", "neg_inf_cells", "pos_inf", "nan"]
    mats = [make_matrix(rng, m, k, str(rng.choice(wkinds))) for m in lengths]
    case = Case(make_enc(rng, length, k, float(rng.choice([0.0, 0.01, 0.3]))), k, cols, mats)
    options = MIX_OPTIONS[int(rng.integers(0, len(MIX_OPTIONS)))]
    pli = pipeline(options)
    ts = []
    for p, w in zip(mats, case.wants):
        kind = str(rng.choice(MIX_THRESHOLDS))
        ts.append(float(xw.kmer_bound(p, k)) + 0.25 if kind == "kmer" else realised(w, cols, kind))
    tag = f"seed {seed} {'protein' if protein else 'dna'} C={cols} L={length} {opt_id(options)}"
    check_argmax_batch(case, pli, tag=tag)
    check_threshold_batch(case, pli, ts, tag=tag)
