"""The three forms of the hit-list ordering (csrc/hits.hip, planned by csrc/hits_plan.hpp) -- short, bucket passes, radix
sort -- each entered speculatively (enqueued behind the scans, sized from the previous call's count) and counted (after
reading the count), for the three outputs: coordinates + values, Scanner positions, the hits of a sequence set.

One DNA sequence of 1 000 003 symbols at C = 32 and one motif of M = 8: the smallest shape at which all three forms are
reachable (the sort needs >= 2^17 expected records, the short form <= 40 960).  On ONE context a walk of thresholds --
~3 k, 60 k, 60 k, 200 k, 200 k, 3 k, 3 k, 0, 1 hits -- makes the previous call's count steer the next call's form; the
``LM_HIP_TRACE`` line of every call names the form it took, and the walk must be SEEN to take the forms listed below: a
change of a constant that makes it miss one fails here, not silently.  Expected values come from the materialised route
(store kernel, then Threshold on the stored matrix), bit for bit; the set's from tests/seqset_reference.py."""
import re

import numpy as np
import pytest

import lightmotif_amd as lm
from lightmotif_amd.lib import stride as lm_stride
from seqset_reference import motif_windows
from seqset_rule import offsets_of

pytestmark = pytest.mark.gpu
COLS, LENGTH, M = 32, 1_000_003, 8
WALK = ("3k", "60k", "60k", "200k", "200k", "3k", "3k", "0", "1")
TARGET = {"0": 0, "1": 1, "3k": 3_000, "60k": 60_000, "200k": 200_000}
TRACE = re.compile(r"\[lm_hip\] fused threshold: (\d+) jobs, \d+ candidates, (\d+) hits; [^\[\n]*\[(\w+)/(\w+)\]")

# what each step of the walk must be seen to take: (form, speculative | counted)
SPEC, COUNTED = "speculative", "counted"
FORMS = {
    # 3k: nothing known, 4 096 expected -> short.  60k: 3 750 expected -> short, and its buckets hold.  60k: 75 k expected
    # -> bucket passes.  200k: outgrows the list's capacity -> grown, scanned again, counted: 2^17 <= 200 k -> sorted.
    # 200k: 250 k expected -> sorted.  3k: still 250 k expected, far too many.  3k: short again.  0: a threshold above the
    # best 8-mer's score is not scanned at all, and a call without a scan is not for the short form.  1: short.
    "default": [("short", SPEC), ("short", SPEC), ("buckets", SPEC), ("sorted", COUNTED), ("sorted", SPEC), ("sorted", SPEC),
                ("short", SPEC), ("buckets", SPEC), ("short", SPEC)],
    # never speculative: the count is read first, and an empty list is not ordered at all
    "speculate_order": [("buckets", COUNTED), ("buckets", COUNTED), ("buckets", COUNTED), ("sorted", COUNTED), ("sorted", COUNTED),
                        ("buckets", COUNTED), ("buckets", COUNTED), ("none", COUNTED), ("buckets", COUNTED)],
    "sort_hits": [("short", SPEC), ("short", SPEC), ("buckets", SPEC), ("buckets", COUNTED), ("buckets", SPEC), ("buckets", SPEC),
                  ("short", SPEC), ("buckets", SPEC), ("short", SPEC)],
    "short_order": [("buckets", SPEC), ("buckets", SPEC), ("buckets", SPEC), ("sorted", COUNTED), ("sorted", SPEC), ("sorted", SPEC),
                    ("buckets", SPEC), ("buckets", SPEC), ("buckets", SPEC)],
}
# a set is never ordered by the short form (the segment pass sits behind the long ordering)
SET_FORMS = {k: [("buckets", s) if f == "short" else (f, s) for f, s in v] for k, v in FORMS.items()}
OPTIONS = ["default", "speculate_order", "sort_hits", "short_order"]
BATCH_SECOND = ("buckets", SPEC)   # the second call of the 1 100-motif batch (the first guesses 4 096 records)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def kmer_codes(enc, m):
    code = np.zeros(len(enc) - m + 1, dtype=np.int64)
    for j in range(m):
        code = code * 4 + enc[j:len(enc) - m + 1 + j]
    return code


class Shape:
    """The sequence, the motif, the stored score matrix and, per step of the walk, the threshold with what the materialised
    route finds above it.  Computed once; nothing here changes afterwards."""

    def __init__(self):
        rng = np.random.default_rng(20_260)
        weights = np.zeros((M, lm_stride(5, 4)), np.float32)
        weights[:, :4] = rng.normal(0, 2, (M, 4))           # continuous weights: one best 8-mer, no tied scores between 8-mers by design
        weights[:, 4] = -1.0
        self.enc = rng.integers(0, 4, LENGTH, dtype=np.uint8)
        best = int(sum(int(np.argmax(weights[j, :4])) * 4 ** (M - 1 - j) for j in range(M)))
        for _ in range(100):                                 # leave the best 8-mer in the sequence exactly once: "one hit"
            at = np.nonzero(kmer_codes(self.enc, M) == best)[0]
            if len(at) <= 1:
                break
            self.enc[at[1:]] = (self.enc[at[1:]] + 1) % 4
        assert len(at) == 1
        self.pssm = lm.ScoringMatrix(weights)
        self.ref = lm.Pipeline.hip(0)
        seq = self.ref.stripe(lm.EncodedSequence(self.enc))
        seq.configure(self.pssm)
        self.rows = seq.rows
        scores = self.ref.score(self.pssm, seq)
        self.matrix = scores.matrix()[:, :COLS].copy()
        self.matrix.setflags(write=False)
        by_value = np.sort(self.matrix.ravel())
        self.t, self.coords, self.values = {}, {}, {}
        for name, n in TARGET.items():
            t = float(np.nextafter(by_value[-1], np.float32(np.inf))) if n == 0 else float(by_value[-n])
            rc = np.asarray(self.ref.threshold(scores, t), dtype=np.int64).reshape(-1, 2)   # Threshold on the stored matrix
            r, c = np.nonzero(self.matrix >= np.float32(t))                                 # ... which is the row-major order
            assert np.array_equal(rc, np.stack([r, c], axis=1)), name
            self.t[name], self.coords[name], self.values[name] = t, rc, self.matrix[rc[:, 0], rc[:, 1]]
        assert len(self.coords["0"]) == 0 and len(self.coords["1"]) == 1
        assert 2_500 <= len(self.coords["3k"]) <= 4_000 and 55_000 <= len(self.coords["60k"]) <= 65_000
        assert 190_000 <= len(self.coords["200k"]) <= 215_000
        # Scanner: ascending position col * rows + row, windows inside the sequence
        self.positions, self.position_scores = {}, {}
        for name, rc in self.coords.items():
            pos = rc[:, 1] * self.rows + rc[:, 0]
            order = np.argsort(pos, kind="stable")
            keep = pos[order] + M <= LENGTH
            self.positions[name], self.position_scores[name] = pos[order][keep], self.values[name][order][keep]
        # the same symbols cut into 200 records
        cuts = np.sort(rng.choice(np.arange(1, LENGTH), 199, replace=False))
        self.lengths = np.diff(np.concatenate([[0], cuts, [LENGTH]]))
        self.windows = motif_windows(weights, self.enc, offsets_of(self.lengths))


@pytest.fixture(scope="module")
def shape():
    return Shape()


def fresh_pipeline(option):
    pli = lm.Pipeline.hip(0)
    if option != "default":
        pli.set_option(option, 0)
    return pli


def taken(capfd, jobs=1):
    """(form, speculative | counted, hits) of the one fused call since the last look at stderr."""
    found = [m for m in TRACE.finditer(capfd.readouterr().err) if int(m.group(1)) == jobs]
    assert len(found) == 1, found
    return found[0].group(3), found[0].group(4), int(found[0].group(2))


@pytest.mark.parametrize("option", OPTIONS)
def test_coordinates_and_values_through_every_form(shape, option, monkeypatch, capfd):
    monkeypatch.setenv("LM_HIP_TRACE", "1")
    pli = fresh_pipeline(option)
    seq = pli.stripe(lm.EncodedSequence(shape.enc))
    seq.configure(shape.pssm)
    capfd.readouterr()
    seen = []
    for step in WALK:
        ptr_coords, values = pli.score_threshold(shape.pssm, seq, shape.t[step])
        form, how, hits = taken(capfd)
        seen.append((form, how))
        assert hits == len(shape.coords[step])
        assert np.array_equal(np.asarray(ptr_coords, dtype=np.int64).reshape(-1, 2), shape.coords[step]), (option, step)
        assert np.array_equal(bits(values), bits(shape.values[step])), (option, step)
    assert seen == FORMS[option]


@pytest.mark.parametrize("option", OPTIONS)
def test_scanner_positions_through_every_form(shape, option, monkeypatch, capfd):
    monkeypatch.setenv("LM_HIP_TRACE", "1")
    pli = fresh_pipeline(option)
    seq = pli.stripe(lm.EncodedSequence(shape.enc))
    seq.configure(shape.pssm)
    capfd.readouterr()
    seen = []
    for step in WALK:
        scanner = lm.Scanner(shape.pssm, seq, threshold=shape.t[step])
        got_pos, got_scores = scanner.positions, scanner.scores
        form, how, hits = taken(capfd)
        seen.append((form, how))
        assert np.array_equal(got_pos, shape.positions[step]), (option, step)
        assert np.array_equal(bits(got_scores), bits(shape.position_scores[step])), (option, step)
    assert seen == FORMS[option]


@pytest.mark.parametrize("option", OPTIONS)
def test_set_hits_through_every_form(shape, option, monkeypatch, capfd):
    monkeypatch.setenv("LM_HIP_TRACE", "1")
    pli = fresh_pipeline(option)
    offs = offsets_of(shape.lengths).astype(np.int64)
    seqset = pli.stripe_set([lm.EncodedSequence(shape.enc[a:b]) for a, b in zip(offs[:-1], offs[1:])])
    seqset.configure_wrap(M - 1)
    w = shape.windows
    capfd.readouterr()
    seen = []
    for step in WALK:
        res = pli.scan_threshold_set([shape.pssm], [shape.t[step]], seqset)
        form, how, hits = taken(capfd)
        seen.append((form, how))
        keep = w.score >= np.float32(shape.t[step])
        rec, pos, score = res[0]
        assert len(rec) == int(keep.sum()), (option, step)
        assert np.array_equal(rec, w.record[keep]) and np.array_equal(pos, w.position[keep]), (option, step)
        assert np.array_equal(bits(score), bits(w.score[keep])), (option, step)
    assert seen == SET_FORMS[option]


def test_more_than_1024_jobs_get_their_starts_from_a_launch_of_its_own(monkeypatch, capfd):
    """1 100 motifs of M = 6 ... 12 over 65 536 symbols in one batch call: beyond 1 024 jobs the bucket passes leave the job
    starts to hits_job_starts instead of the ranking kernel's first workgroup.  Every motif's share of the batch equals
    its single call."""
    monkeypatch.setenv("LM_HIP_TRACE", "1")
    rng = np.random.default_rng(1_100)
    enc = rng.integers(0, 4, 65_536, dtype=np.uint8)
    pssms, ts = [], []
    for i in range(1_100):
        m = 6 + i % 7
        weights = np.zeros((m, lm_stride(5, 4)), np.float32)
        weights[:, :4] = rng.normal(0, 2, (m, 4))
        weights[:, 4] = -1.0
        pssms.append(lm.ScoringMatrix(weights))
        ts.append(0.9 * float(np.sum(np.max(weights[:, :4], axis=1))))
    pli, single = lm.Pipeline.hip(0), lm.Pipeline.hip(0)
    seq = pli.stripe(lm.EncodedSequence(enc))
    seq.configure_wrap(11)
    seq1 = single.stripe(lm.EncodedSequence(enc))
    seq1.configure_wrap(11)
    batch = pli.prepare_batch(pssms, ts)
    capfd.readouterr()
    seen = []
    for call in range(2):
        res = pli.scan_threshold_batch(batch, None, seq)
        form, how, hits = taken(capfd, jobs=1_100)
        seen.append((form, how))
        assert 1_100 < hits < (1 << 17)                       # (the bucket passes, not the sort)
        for i in ([*range(1_100)] if call == 0 else [0, 511, 1_023, 1_024, 1_099]):
            coords, values = res[i]
            want_rc, want_v = single.score_threshold(pssms[i], seq1, ts[i])
            assert np.array_equal(coords, np.asarray(want_rc, dtype=np.int64).reshape(-1, 2)), (call, i)
            assert np.array_equal(bits(values), bits(want_v)), (call, i)
        capfd.readouterr()
    assert seen[1] == BATCH_SECOND and seen[0][0] == BATCH_SECOND[0]
