"""Every row of the kernel registry against the oracle, and proof from the library's own launch tally that it ran.

The scoring path is a registry of template instantiations (csrc/score_registry.hpp, the fused table of csrc/seqset_best.hip):
``Pipeline.registry_rows()`` lists the rows the build promises, ``Pipeline.launch_tally()`` the rows a context launched.
One test per family and alphabet drives every promised row of its family through a public entry point, compares what
comes back with the oracle -- never with another kernel -- and ends by asserting

    rows launched  ==  rows promised  -  UNREACHABLE        (rows that share one kernel count as one)

so that a row nobody can launch is either reached here or written down in ``UNREACHABLE`` with the planner line that
excludes it, and an entry of that table that does get launched fails the test as well.

Shapes (the smallest at which these kernels can still go wrong), the same for every row of length M:
  (a) ``32 * (4 * M + 70) - 11`` symbols: a ragged last row, M - 1 windows across the wrap; every row, default streams;
  (b) rows ``[3, rows - 2)`` of the same sequence with ``rows_per_stream`` = 33: a first stream that starts inside the
      matrix (the lead rows of the padded tables reach back before it), at least three streams and a partial last one.
Symbols are uniform with ~2 % N / X (for motifs beyond 100 rows 2 / M and none in the first M + 64 symbols, so that some
windows stay free of them: at 2 % a window of 1 000 symbols never is); weights are
normal(0, 2) with the N / X column at -inf, and small integers in [-3, 3] whose ties exercise the last-cell rule.
Thresholds are realised scores of the oracle's matrix: rank 20 from the top and the maximum."""
from collections import Counter
from contextlib import contextmanager

import numpy as np
import pytest

import lightmotif_amd as lm
import seqset_reference as sr
from oracle import c_oracle as co
from oracle import np_oracle as no

pytestmark = pytest.mark.gpu

KINDS = ("normal", "ties")
SHORT = list(range(1, 37))
LONG = list(range(40, 65, 4))
XLONG = [72, 80, 88]

# Rows no public call can launch: (family, wide, motif lengths, slot) -> the line that excludes them.
UNREACHABLE = {
    # The only launch of SLOT_CONTINUE is the slice loop of launch_score_store (score_store.hip:124, slices `i >= 1`), at the
    # length of a slice of a motif beyond kMaxLongM rows; pssm_tables.hpp:141-142 (build_pssm_tables: `part.m = real +
    # part.lead` with `lead = (unit - real % unit) % unit`, unit = 4) makes every slice a multiple of 4 rows.  27 lengths
    # x 2 alphabet widths = 54 compiled kernels.  (The multiples of 4 ARE reached: the last slice of a motif of 1024 + M rows.)
    ("c32", 0, tuple(m for m in SHORT if m % 4), "CONTINUE"): "pssm_tables.hpp:141-142: slices are multiples of 4 rows",
    ("c32", 1, tuple(m for m in SHORT if m % 4), "CONTINUE"): "pssm_tables.hpp:141-142: slices are multiples of 4 rows",
}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


class Case:
    """One sequence and one matrix with the oracle's scores of every row, computed once; ``view(g)`` cuts geometry g."""

    def __init__(self, m, k, kind, cols=32, shape_m=None):
        self.m, self.k, self.kind, self.cols, self.protein = m, k, kind, cols, k == 21
        rng = np.random.default_rng([m, k, KINDS.index(kind), cols])
        length = cols * (4 * (shape_m or m) + 70) - 11
        self.enc = rng.integers(0, k - 1, length).astype(np.uint8)
        unknown = rng.random(length) < min(0.02, 2.0 / m)
        if m > 100:
            unknown[:m + 64] = False                                # the first 65 windows hold no N / X: finite scores
        self.enc[unknown] = k - 1
        self.weights = np.zeros((m, co.stride(k, 4)), np.float32)
        if kind == "ties":
            self.weights[:, :k] = rng.integers(-3, 4, (m, k))
        else:
            self.weights[:, :k] = rng.normal(0, 2, (m, k))
            self.weights[:, k - 1] = -np.inf
        self.ref = co.stripe(self.enc, cols, k)
        co.configure_wrap(self.ref, m - 1)
        self.rows = self.ref.rows
        self.want, self.max_index = co.score_rows(self.ref, self.weights)
        assert self.want.shape[0] == self.rows and np.isfinite(self.want[:, :cols]).any(), "no finite score: change the seed"
        self.pssm = lm.ScoringMatrix(self.weights, protein=self.protein)

    def sequence(self, pipe):
        seq = pipe.stripe(lm.EncodedSequence(self.enc, protein=self.protein), self.cols)
        seq.configure_wrap(self.m - 1)
        assert np.array_equal(seq.matrix(), self.ref.data), "striped matrix differs"
        return seq

    def view(self, g):
        """(row range, rows_per_stream, the oracle's matrix of those rows)"""
        a, b = (0, self.rows) if g == "a" else (3, self.rows - 2)
        return range(a, b), (0 if g == "a" else 33), self.want[a:b]

    def thresholds(self, want):
        """Rank 20 from the top and the maximum of the finite scores: at least one hit, never all cells."""
        cells = want[:, :self.cols]
        v = np.sort(cells[np.isfinite(cells)])
        assert len(v) >= 20
        out = []
        for t in (float(v[-20]), float(v[-1])):
            hits = co.threshold(want, self.cols, t)
            assert 0 < len(hits) < cells.size, (self.m, self.kind, t)
            out.append((t, hits))
        return out


class Sweep:
    """A pipeline of the test's own with the launch tally on; ``ran`` asserts rows right after the call that should have
    launched them (the message then names the length), ``finish`` the completeness of the family."""

    def __init__(self, **options):
        self.pipe = lm.Pipeline.hip(0)
        self.pipe.set_option("tally_launches", 1)
        self.set(**options)
        self.seen = Counter()
        self.failures = []
        self.promised = lm.Pipeline.registry_rows()
        first = {}
        for key in sorted(self.promised):
            first.setdefault(self.promised[key], key)
        self.canon = {key: first[ident] for key, ident in self.promised.items()}   # rows that share a kernel count as one

    def set(self, **options):
        for name, value in options.items():
            if name == "rows_per_stream":
                self.pipe.set_rows_per_stream(value)
            else:
                self.pipe.set_option(name, value)

    def ran(self, *rows):
        t = self.pipe.launch_tally()
        self.seen.update(t)
        for row in rows:
            assert row in t, (row, sorted(t))

    @contextmanager
    def case(self, *label):
        """A comparison that fails is written down and the sweep goes on: the test then names EVERY case that differs (a
        wrong row fails its own cases and no others).  Errors of the library itself are not caught."""
        try:
            yield
        except AssertionError as e:
            self.failures.append((label, str(e).splitlines()[0][:300]))

    def finish(self, families, wide):
        self.ran()
        assert self.pipe.launch_tally() == {}                       # reading cleared it
        for f in self.failures:
            print("differs:", f)
        assert not self.failures, (len(self.failures), "cases differ, of the rows", sorted({f[0][:2] for f in self.failures}))
        mine = lambda key: key[0] in families and key[1] == wide
        assert set(self.seen) <= set(self.promised), sorted(set(self.seen) - set(self.promised))
        ledger = {(f, w, m, s) for (f, w, ms, s) in UNREACHABLE for m in ms}
        assert ledger <= set(self.promised), sorted(ledger - set(self.promised))
        launched = {self.canon[key] for key in self.seen if mine(key)}
        promised = {self.canon[key] for key in self.promised if mine(key)}
        barred = {self.canon[key] for key in ledger if mine(key)}
        assert launched & barred == set(), sorted(launched & barred)
        assert promised - barred - launched == set(), sorted(promised - barred - launched)
        assert launched == promised - barred
        self.pipe.close()


def check_matrix(pipe, case, seq, rows, want):
    """score_rows_into against the oracle bit for bit, max_index included; returns the scores handle."""
    scores = lm.StripedScores.empty(pipe, case.cols)
    pipe.score_rows_into(case.pssm, seq, rows, scores)
    got = scores.matrix()
    assert got.shape == want.shape and scores.max_index == case.max_index
    diff = np.argwhere(bits(got[:, :case.cols]) != bits(want[:, :case.cols]))
    assert len(diff) == 0, (case.m, case.kind, rows, pipe.last_kernel, "first differing cell", tuple(diff[0]))
    return scores


def check_argmax(case, got, want):
    """((row, col), value) against co.argmax and the bits of co.max_ on the oracle's matrix"""
    assert got is not None and got[0] == co.argmax(want, case.cols), (case.m, case.kind, got, co.argmax(want, case.cols))
    assert bits(np.float32(got[1])) == bits(co.max_(want, case.cols)), (case.m, case.kind)


def check_threshold(pipe, case, seq, rows, want):
    """The fused threshold at both thresholds against co.threshold of the oracle's matrix: the ordered list and the score bits."""
    for t, hits in case.thresholds(want):
        rc, values = pipe.score_threshold(case.pssm, seq, t, rows)
        wrc = [tuple(map(int, x)) for x in hits]
        assert rc == wrc, (case.m, case.kind, rows, t, pipe.last_kernel, len(rc), len(wrc))
        assert np.array_equal(bits(values), bits([want[r, c] for r, c in wrc])), (case.m, case.kind, rows, t)


def motif_of_row(mk, kind):
    """The motif length that runs the padded long / very long row `mk`: one leading zero row for the normal weights, none for the ties."""
    return mk - 1 if kind == "normal" and mk > 36 else mk


# ---- the exact f32 kernels ---------------------------------------------------------------------------------------


@pytest.mark.parametrize("k", [5, 21])
def test_c32_rows(k):
    wide = int(k == 21)
    sw = Sweep()
    row = lambda m, slot: ("c32", wide, m, slot)
    plain = dict(track_argmax=0, quad_loads=1, host_fold=1, track_fold_cells=8 << 20, prefilter=1)

    def stored(case, seq, g, slot, mk, tracked=False, **options):
        """One store route of one geometry: the matrix, the row that ran and, for the tracking forms, the cached argmax."""
        rows, rps, want = case.view(g)
        sw.set(**dict(plain, rows_per_stream=rps, **options))
        with sw.case(mk, slot, case.kind, g, options):
            scores = check_matrix(sw.pipe, case, seq, rows, want)
            sw.ran(row(mk, slot))
            if tracked:
                check_argmax(case, (sw.pipe.argmax(scores), sw.pipe.max(scores)), want)

    for mk in SHORT + LONG + XLONG:
        for kind in KINDS:
            case = Case(motif_of_row(mk, kind), k, kind)
            seq = case.sequence(sw.pipe)
            for g in "ab":
                if mk <= 36:                                        # byte symbol loads: every short length
                    stored(case, seq, g, "STORE", mk, quad_loads=0)
                if mk % 4 == 0:                                     # dword symbol loads
                    stored(case, seq, g, "STORE_QL", mk)
                if mk > 64:
                    continue                                        # the very long family: the plain store alone
                if mk % 4 == 0:                                     # store + tracked maximum in one launch, folded by the host / on the device
                    stored(case, seq, g, "STORE_TRACK", mk, tracked=True, track_argmax=1)
                    stored(case, seq, g, "STORE_TRACK", mk, tracked=True, track_argmax=1, host_fold=0)
                # store + block maxima, the route of large matrices; every short length through its unpadded table
                stored(case, seq, g, "STORE_ARGMAX", mk, tracked=True, track_argmax=1, track_fold_cells=0, quad_loads=int(mk > 36))
                # fused argmax and fused threshold through the exact kernels
                rows, rps, want = case.view(g)
                sw.set(**dict(plain, rows_per_stream=rps))
                with sw.case(mk, "ARGMAX", kind, g):
                    check_argmax(case, sw.pipe.score_argmax(case.pssm, seq, rows), want)
                    sw.ran(row(mk, "ARGMAX"))
                sw.set(prefilter=0)
                with sw.case(mk, "THRESHOLD", kind, g):
                    check_threshold(sw.pipe, case, seq, rows, want)
                    sw.ran(row(mk, "THRESHOLD"))
    # continue in place: the last slice of a motif of 16 slices of 64 rows and one of mk rows (pssm_tables.hpp)
    for mk in [m for m in SHORT + LONG if m % 4 == 0]:
        for kind in KINDS:
            case = Case(1024 + motif_of_row(mk, kind) - (1 if mk <= 36 and kind == "normal" else 0), k, kind, shape_m=mk)
            seq = case.sequence(sw.pipe)
            for g in "ab":
                stored(case, seq, g, "CONTINUE", mk)
                with sw.case(mk, "CONTINUE", kind, g, "first slice"):
                    assert sw.seen[row(64, "STORE_QL")] and sw.seen[row(64, "CONTINUE")]
    # four streams of 16 columns per wavefront: a matrix of 16 columns
    for mk in [m for m in SHORT if m % 4 == 0]:
        for kind in KINDS:
            case = Case(mk, k, kind, cols=16)
            seq = case.sequence(sw.pipe)
            for g in "ab":
                stored(case, seq, g, "STORE_C16", mk)
    sw.finish({"c32"}, wide)


# ---- the prefilter scans -------------------------------------------------------------------------------------------


def scan_family(family, k, lengths, **options):
    """Every length of one prefilter family through the fused threshold; the exact kernel is barred by the tally."""
    wide = int(k == 21)
    sw = Sweep(**options)
    for m in lengths:
        for kind in KINDS:
            case = Case(m, k, kind)
            seq = case.sequence(sw.pipe)
            for g in "ab":
                rows, rps, want = case.view(g)
                sw.set(rows_per_stream=rps)
                with sw.case(m, family, kind, g):
                    check_threshold(sw.pipe, case, seq, rows, want)
                    sw.ran((family, wide, m, ""))
    assert not any(key[0] == "c32" for key in sw.seen), sorted(key for key in sw.seen if key[0] == "c32")
    return sw


def test_pre_rows_dna():
    scan_family("pre", 5, SHORT, pair_prefilter=0).finish({"pre"}, 0)


def test_pre_rows_protein():
    scan_family("pre", 21, SHORT, block_prefilter=0).finish({"pre"}, 1)


def test_preblk_rows_protein():
    scan_family("preblk", 21, SHORT).finish({"preblk"}, 1)


def test_pre2_rows_dna():
    scan_family("pre2", 5, range(2, 129), drop_last=0).finish({"pre2"}, 0)


def test_pre2_protein_rows():
    scan_family("pre2_protein", 21, range(2, 37), pair_prefilter_protein=1).finish({"pre2_protein"}, 1)


def test_pre2_multi_rows_dna():
    """Three motifs of one length per call: each job's hits against its own oracle result."""
    sw = Sweep()
    lengths = sorted(m for (f, _, m, _) in sw.promised if f == "pre2_multi")
    assert lengths
    for m in lengths:
        for kind in KINDS:
            cases = [Case(m, 5, kind)]
            for j in (1, 2):                                        # two more matrices for the same sequence
                other = Case.__new__(Case)
                other.__dict__.update(cases[0].__dict__)
                rng = np.random.default_rng([m, j, KINDS.index(kind)])
                other.weights = cases[0].weights.copy()
                other.weights[:, :4] = rng.integers(-3, 4, (m, 4)) if kind == "ties" else rng.normal(0, 2, (m, 4))
                other.want, _ = co.score_rows(other.ref, other.weights)
                other.pssm = lm.ScoringMatrix(other.weights)
                cases.append(other)
            seq = cases[0].sequence(sw.pipe)
            for g, rps in (("a", 0), ("a", 33)):                    # (a batch scans every row of the sequence)
                sw.set(rows_per_stream=rps)
                for which in (0, 1):
                    wants = [c.thresholds(c.want)[which] for c in cases]
                    with sw.case(m, "pre2_multi", kind, rps, which):
                        res = sw.pipe.scan_threshold_batch([c.pssm for c in cases], [t for t, _ in wants], seq)
                        sw.ran(("pre2_multi", 0, m, ""))
                        for c, (t, hits), (rc, values) in zip(cases, wants, res):
                            assert np.array_equal(rc, hits.astype(np.int64)), (m, kind, t)
                            assert np.array_equal(bits(values), bits([c.want[r, col] for r, col in hits])), (m, kind, t)
    assert not any(key[0] == "c32" for key in sw.seen)
    sw.finish({"pre2_multi"}, 0)


# ---- u8 scores ---------------------------------------------------------------------------------------------------


def u8_family(family, k, lengths, **options):
    """Wrapping sums against co.score_rows_u8, saturating ones against np_oracle.score_rows_u8_saturating with weights
    that reach 255; two weight kinds: the whole byte range, and weights whose sums end near 255."""
    wide = int(k == 21 and family == "u8")
    sw = Sweep(**options)
    for m in lengths:
        for top in (255, min(255 // m + 2, 255)):
            rng = np.random.default_rng([m, k, top])
            length = 32 * (4 * m + 70) - 11
            enc = rng.integers(0, k - 1, length).astype(np.uint8)
            enc[rng.random(length) < 0.02] = k - 1
            weights = rng.integers(0, top + 1, (m, k), dtype=np.uint8)
            weights[0, 0] = 255                                     # so that a motif of one row saturates as well
            ref = co.stripe(enc, 32, k)
            co.configure_wrap(ref, m - 1)
            want_wrap, mi = co.score_rows_u8(ref, weights)
            want_sat = no.score_rows_u8_saturating(ref.data, 32, length, weights, 0, ref.rows)
            assert (want_sat == 255).any(), (m, top)
            dm = lm.DiscreteMatrix(weights, 1.0, np.zeros(m, np.float32), 0.0, protein=k == 21)
            seq = sw.pipe.stripe(lm.EncodedSequence(enc, protein=k == 21), 32)
            seq.configure_wrap(m - 1)
            for a, b, rps in ((0, ref.rows, 0), (3, ref.rows - 2, 33)):
                sw.set(rows_per_stream=rps)
                for saturate, want in ((False, want_wrap), (True, want_sat)):
                    with sw.case(m, family, top, (a, b), saturate):
                        got, gmi = sw.pipe.score_discrete(dm, seq, rows=range(a, b), saturate=saturate)
                        sw.ran((family, wide, m, ""))
                        assert gmi == mi and got.shape[0] == b - a
                        diff = np.argwhere(got[:, :32] != want[a:b, :32])
                        assert len(diff) == 0, (m, top, saturate, (a, b), "first differing cell", tuple(diff[0]))
    return sw


def test_u8_rows_dna():
    u8_family("u8", 5, SHORT, pair_prefilter=0).finish({"u8"}, 0)


def test_u8_rows_protein():
    u8_family("u8", 21, SHORT).finish({"u8"}, 1)


def test_u8_pairs_rows_dna():
    u8_family("u8_pairs", 5, range(2, 37)).finish({"u8_pairs"}, 0)


# ---- the best hit per record -------------------------------------------------------------------------------------


@pytest.mark.parametrize("k", [5, 21])
def test_best_fused_rows(k):
    """scan_best_set against tests/seqset_reference.py on five records whose cuts fall inside a row."""
    sw = Sweep()
    for m in SHORT:
        for kind in KINDS:
            rng = np.random.default_rng([m, k, KINDS.index(kind), 7])
            total = 32 * (4 * m + 70) - 11
            cuts = np.sort(rng.choice(np.arange(m + 3, total - 1, 2) | 1, 4, replace=False))   # odd: inside a row of 32
            lengths = np.diff(np.concatenate(([0], cuts, [total]))).astype(np.int64)
            assert (lengths > 0).all() and all(int(c) % 32 for c in cuts)
            sym = rng.integers(0, k - 1, total).astype(np.uint8)
            sym[rng.random(total) < 0.02] = k - 1
            weights = sr.make_matrix(rng, m, k, kind)
            offs = sr.offsets_of(lengths)
            found, position, score = sr.motif_windows(weights, sym, offs).best(len(lengths))
            assert found.any()
            records = [lm.EncodedSequence(sym[int(a):int(b)], protein=k == 21) for a, b in zip(offs[:-1], offs[1:])]
            seqset = sw.pipe.stripe_set(records, columns=32, protein=k == 21)
            seqset.configure_wrap(m - 1)
            for rps in (0, 33):
                sw.set(rows_per_stream=rps)
                with sw.case(m, "best_fused", kind, rps):
                    got = sw.pipe.scan_best_set([lm.ScoringMatrix(weights, protein=k == 21)], seqset)
                    sw.ran(("best_fused", 0, m, ""))
                    assert np.array_equal(got.found[0], found), (m, kind, rps)
                    assert np.array_equal(got.position[0], position), (m, kind, rps)
                    assert np.array_equal(bits(got.score[0])[found], bits(score)[found]), (m, kind, rps)
    sw.finish({"best_fused"}, 0)
