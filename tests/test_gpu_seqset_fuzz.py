"""Seeded differential test of the sequence-set path: the three builders of a resident set (ASCII, encoded symbols, FASTA
bytes), ``scan_threshold_set``, ``scan_best_set`` and the p-values of the hits, over random record counts and lengths,
column counts, motif lengths, matrix kinds, thresholds, stream lengths and context options, against a reference that never
touches the GPU library (tests/seqset_reference.py, pinned on the host by tests/test_seqset_reference.py): records,
positions and score bits, f64 bits for p-values.

Every seed draws from one ``np.random.default_rng(310_000 + seed)``; ``LM_SETFUZZ_FIRST`` / ``LM_SETFUZZ_LAST`` pick the
seeds.  A seed without records, or in which no motif fits a record, checks the empty answers only; the module asserts
that at most a quarter of the default seeds are of that kind.  No call may refuse a shape the generator makes: the
header documents no restriction on column counts, totals or record counts, so every status is a failure here."""
import os

import numpy as np
import pytest

import lightmotif_amd as lm
import seqset_reference as sr

pytestmark = pytest.mark.gpu

DEFAULT_SEEDS = range(0, 120)
SEEDS = range(int(os.environ.get("LM_SETFUZZ_FIRST", str(DEFAULT_SEEDS.start))),
              int(os.environ.get("LM_SETFUZZ_LAST", str(DEFAULT_SEEDS.stop))))

_PIPES = {}
_SEEN = {}          # seed -> what the seed ran: kernel names, column count, records, whether it had a window


def pipeline(pli, options):
    """The session pipeline for the default options, one pipeline of its own per other option set."""
    if not options:
        return pli
    key = tuple(sorted(options.items()))
    if key not in _PIPES:
        p = lm.Pipeline.hip(0)
        for name, value in options.items():
            p.set_option(name, value)
        _PIPES[key] = p
    return _PIPES[key]


_MARKS = {}


def mark(pipe):
    """Leaves a known name ("dist_pvalues") in ``last_kernel``: a scan that launches nothing is then not credited with the
    kernel of the call before it."""
    if id(pipe) not in _MARKS:
        weights = np.zeros((1, 8), np.float32)
        weights[0, :4] = [1.0, -1.0, 0.5, -0.5]
        _MARKS[id(pipe)] = pipe.score_distributions([lm.ScoringMatrix(weights)])
    _MARKS[id(pipe)].pvalues([1], np.zeros(1, np.float32))
    assert pipe.last_kernel == MARK


MARK = "dist_pvalues"


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check_lists(res, want, tag):
    assert len(res) == len(want), tag
    assert int(np.sum(res.counts)) == len(res.hits) == res.total, tag
    for mi, (wr, wp, ws) in enumerate(want):
        gr, gp, gs = res[mi]
        assert len(gr) == int(res.counts[mi]) == len(wr), (tag, mi, int(res.counts[mi]), len(wr))
        assert np.array_equal(gr, wr), (tag, mi, "records")
        assert np.array_equal(gp, wp), (tag, mi, "positions")
        assert np.array_equal(bits(gs), bits(ws)), (tag, mi, "scores")
        if len(gr) > 1:
            dr, dp = np.diff(gr), np.diff(gp)
            assert np.all((dr > 0) | ((dr == 0) & (dp > 0))), (tag, mi, "order")


def check_best(got, want, tag):
    found, position, score = want
    assert got.found.shape == found.shape, tag
    assert got.found.dtype == np.bool_ and got.position.dtype == np.int64 and got.score.dtype == np.float32
    assert np.array_equal(got.found, found), (tag, "found", np.argwhere(got.found != found)[:5])
    assert np.array_equal(got.position, position), (tag, "position", np.argwhere(got.position != position)[:5])
    assert np.array_equal(bits(got.score)[found], bits(score)[found]), (tag, "scores")
    assert np.all(np.isnan(got.score[~found])) and np.all(got.position[~found] == -1), tag
    assert np.all(got.raw["position"][~found] == 0) and np.all(got.raw["found"][~found] == 0), tag   # the C ABI's "none"


def run_seed(pli, seed):
    case = sr.draw_case(seed)
    windows = sr.reference(case)
    n_records = len(case.lengths)
    pipe = pipeline(pli, case.options)
    tag = (seed, case.cols, n_records, [p.shape[0] for p in case.mats], case.threshold_kinds, case.options)
    kernels = set()
    pssms = [lm.ScoringMatrix(p, protein=case.protein) for p in case.mats]
    pipe.set_rows_per_stream(case.rows_per_stream)
    pipe.set_prefilter(case.prefilter)
    try:
        # 1. the three builders give the same set
        sets = {
            "ascii": pipe.stripe_ascii_set(case.texts, protein=case.protein, lossy=True, columns=case.cols),
            "encoded": pipe.stripe_set([lm.EncodedSequence(s, protein=case.protein) for s in case.symbols],
                                       columns=case.cols, protein=case.protein),
            "fasta": pipe.stripe_fasta_set(case.fasta, protein=case.protein, lossy=True, columns=case.cols),
        }
        for name, s in sets.items():
            s.configure_wrap(case.wrap)
            assert len(s) == n_records and s.lengths.tolist() == case.lengths.tolist(), (tag, name)
            assert s.total_length == case.total and s.columns == case.cols and s.protein == case.protein, (tag, name)
            assert s.rows == -(-case.total // case.cols) and s.wrap == case.wrap, (tag, name)
        assert len(sets["fasta"].header_spans) == n_records

        # 2. the hit lists
        want = [w.hits(t) for w, t in zip(windows, case.thresholds)]
        twice = ("ascii", "encoded", "fasta")[seed % 3]
        lists = {}
        for name, s in sets.items():
            for call in range(2 if name == twice else 1):          # the second call is sized from the first
                mark(pipe)
                lists[name] = pipe.scan_threshold_set(pssms, case.thresholds, s)
                kernels.add(pipe.last_kernel)
                check_lists(lists[name], want, (tag, name, call, pipe.last_kernel))

        # 3. the best window per record
        want_best = tuple(np.stack(x) for x in zip(*[w.best(n_records) for w in windows]))
        raws = []
        for name, s in sets.items():
            for call in range(2 if name == twice else 1):
                mark(pipe)
                got = pipe.scan_best_set(pssms, s)
                kernels.add(pipe.last_kernel)
                assert pipe.last_kernel.startswith("seqset_best_") or not case.has_window, tag  # some motif fits: a launch
                check_best(got, want_best, (tag, name, call, pipe.last_kernel))
                raws.append(got.raw.tobytes())
        assert all(r == raws[0] for r in raws), tag

        # 4. the p-values of the hits
        scores = np.concatenate([w[2] for w in want])
        if not case.has_nan and all(np.isfinite(p[:, :case.k]).any() for p in case.mats) and np.isfinite(scores).all():
            got_p = pipe.score_distributions(pssms).pvalues(lists["ascii"])
            hosts = [p.score_distribution for p in pssms]
            want_p = np.concatenate([sr.pvalues_of(d, w[2]) for d, w in zip(hosts, want)])
            assert np.array_equal(got_p.view(np.uint64), want_p.view(np.uint64)), (tag, "p-values")
            start = 0
            for d, w in zip(hosts, want):                          # dist.py itself on the ends of every list
                for i in sorted(set(range(len(w[2]))[:20]) | set(range(len(w[2]))[-20:])):
                    assert got_p[start + i] == d.pvalue(float(w[2][i])), (tag, "p-value", i)
                start += len(w[2])
            checked_p = len(scores)
        else:
            checked_p = 0

        # 5. every call left a name: its last kernel's, or the mark when it had nothing to launch
        assert kernels and all(kernels), tag
        kernels.discard(MARK)
        if not case.has_window:
            assert sum(len(w.score) for w in windows) == 0 and not want_best[0].any(), tag
    finally:
        pipe.set_rows_per_stream(0)
        pipe.set_prefilter(True)
    _SEEN[seed] = {"kernels": kernels, "cols": case.cols, "records": n_records,
                   "window": case.has_window, "hits": sum(len(w[0]) for w in want), "pvalues": checked_p}
    return _SEEN[seed]


@pytest.mark.parametrize("seed", SEEDS)
def test_random_set(pli, seed):
    run_seed(pli, seed)


def test_the_default_seeds_reach_what_they_must(pli):
    """Over seeds 0 to 119 (those this run has not been through yet are run here): the kernels of both best-hit roads, the
    pair prefilter, an exact C = 32 scan and the generic scan with position keys were seen; at least 15 seeds had a column
    count other than 32 and at least 8 more than 4 095 records; at most a quarter checked only empty answers."""
    seen = [_SEEN[seed] if seed in _SEEN else run_seed(pli, seed) for seed in DEFAULT_SEEDS]
    names = set().union(*[s["kernels"] for s in seen])
    print(sorted(names))
    assert any(k.startswith("seqset_best_fused<") for k in names), names
    assert "seqset_best_generic" in names, names
    assert any(k.startswith("score_c32_prefilter2") for k in names), names
    assert any(k.startswith("score_c32<") for k in names), names
    assert "score_generic<2>" in names, names
    assert sum(s["cols"] != 32 for s in seen) >= 15
    assert sum(s["records"] > 4095 for s in seen) >= 8
    assert 4 * sum(not s["window"] for s in seen) <= len(seen)
    assert sum(s["hits"] > 0 for s in seen) >= len(seen) // 2
    assert sum(s["pvalues"] > 0 for s in seen) >= 10
