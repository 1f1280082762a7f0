"""The store kernels' stream geometry and paired row stores against the oracle, bit for bit.

The plain DNA store kernel with dword symbol loads of M = 16 and 20 (every DNA motif of 13 ... 20 rows) writes score rows
in pairs: the two half-waves of a wavefront keep their own streams, exchange completed rows and store 256 contiguous bytes
per instruction; its streams are T = q*M + 1 + R rows (csrc/score_kernels.hpp: store_pairs, store_extra_rows), always even.
Every other length and the tracking forms of the store keep single rows and T = q*M + 1.  The cases below do not care which
is which: every length, mode and row count must give the oracle's matrix, and the launch tally says that a store kernel
of the expected registry row carried it.

T0 is the stream length the planner picks for the matrices of this file (read back through ``last_stream_rows`` after a
plain store of the whole test sequence, never written down here).  Row counts, in rows of 32 columns:

    T0            one stream, its wave partner idle
    T0 + 1        a last stream shifted back by an odd number of rows: misaligned pairs, overlap with identical values
    2 T0          both halves of the wavefront live
    2 T0 + 7      a shifted, overlapping last stream
    9 T0 + 5      a second workgroup, an odd stream count
    M + 1 + R     the smallest input the T = q*M + 1 + R rule can take (R = 63 % M)
    M + R         one row less: whatever route it takes

All of them are row ranges of ONE sequence per length whose oracle scores are computed once; ranges with an odd first
row and an odd length are added for M = 20.  One case of 1.1 M rows runs the default stream of three groups and the
extra steps (two MAIN groups, the second in a frame of its own), which the small cases never reach: the planner shortens
streams on small inputs."""
import numpy as np
import pytest

import extreme_weights as xw
import lightmotif_amd as lm
from oracle import c_oracle as co

pytestmark = pytest.mark.gpu

DNA = [2, 3, 12, 19, 20, 21, 26, 27, 36]
PROTEIN = [12, 20]
MODES = {
    # name: the context options that send score_rows_into down that store route
    "plain": dict(track_argmax=0),
    "block_maxima": dict(track_argmax=1, track_fold_cells=0),
    "tracked": dict(track_argmax=1, track_fold_cells=8 << 20),
}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def extra_rows(m):
    return 63 % m


def paired(mk, k, mode, quad_loads=1):
    """The kernels that store rows in pairs (csrc/score_kernels.hpp: store_pairs), by the length the kernel runs at"""
    return mode == "plain" and quad_loads and k == 5 and mk in (16, 20)


class Case:
    """One sequence of `rows` rows and one matrix, with the oracle's scores of every row."""

    def __init__(self, m, k, rows, weights=None, enc=None, seed=0):
        self.m, self.k = m, k
        rng = np.random.default_rng([m, k, rows, seed])
        length = 32 * rows - 11
        if enc is None:
            enc = rng.integers(0, k - 1, length).astype(np.uint8)
            enc[rng.random(length) < 0.02] = k - 1
        self.enc = enc
        if weights is None:
            weights = np.zeros((m, co.stride(k, 4)), np.float32)
            weights[:, :k] = rng.normal(0, 2, (m, k))
            weights[:, k - 1] = -np.inf
        self.weights = weights
        self.ref = co.stripe(self.enc, 32, k)
        co.configure_wrap(self.ref, m - 1)
        self.rows = self.ref.rows
        assert self.rows == rows
        self.want, self.max_index = co.score_rows(self.ref, self.weights)
        self.pssm = lm.ScoringMatrix(self.weights, protein=k == 21)

    def sequence(self, pipe):
        seq = pipe.stripe(lm.EncodedSequence(self.enc, protein=self.k == 21), 32)
        seq.configure_wrap(self.m - 1)
        assert np.array_equal(seq.matrix(), self.ref.data)
        return seq


@pytest.fixture(scope="module")
def pipe():
    p = lm.Pipeline.hip(0)
    p.set_option("tally_launches", 1)
    yield p
    p.close()


def configure(pipe, mode, quad_loads=1, rows_per_stream=0):
    for name, value in dict(MODES[mode], quad_loads=quad_loads, host_fold=1).items():
        pipe.set_option(name, value)
    pipe.set_rows_per_stream(rows_per_stream)


def stored(pipe, case, seq, rows, mode):
    """score_rows_into of a row range against the oracle (and its argmax for the tracking forms); returns the tally."""
    want = case.want[rows.start:rows.stop]
    scores = lm.StripedScores.empty(pipe, 32)
    pipe.launch_tally()
    pipe.score_rows_into(case.pssm, seq, rows, scores)
    tally, kernel, t = pipe.launch_tally(), pipe.last_kernel, pipe.last_stream_rows
    got = scores.matrix()
    assert got.shape == want.shape, (case.m, mode, rows, kernel)
    diff = np.argwhere(bits(got[:, :32]) != bits(want[:, :32]))
    assert len(diff) == 0, (case.m, mode, rows, kernel, t, "first differing cell", tuple(diff[0]), len(diff))
    if mode != "plain":
        best = pipe.argmax(scores)
        assert best == co.argmax(want, 32), (case.m, mode, rows, kernel, best, co.argmax(want, 32))
        assert bits(np.float32(pipe.max(scores))) == bits(co.max_(want, 32)), (case.m, mode, rows, kernel)
    return tally, kernel, t


def kernel_rows(tally, wide):
    """The store rows of the C = 32 registry family that a call launched: {(M, slot)}"""
    return {(m, slot) for (family, w, m, slot) in tally if family == "c32" and w == wide and slot.startswith("STORE")}


def expected_slot(m, mode, quad_loads=1):
    """(kernel length, slot) a store of at least the smallest legal input runs (score_store.hip): under dword symbol loads
    a length that is no multiple of 4 runs the next multiple's kernel on a table padded with leading zero rows"""
    mk = (m + 3) // 4 * 4 if quad_loads else m
    if mode == "block_maxima":
        return mk, "STORE_ARGMAX"
    if mode == "tracked":
        return mk, "STORE_TRACK"
    return mk, "STORE_QL" if quad_loads else "STORE"


def stream_rows(pipe, case, seq):
    """T0: what the planner picks for a plain store of the whole sequence"""
    configure(pipe, "plain")
    _, _, t = stored(pipe, case, seq, range(0, case.rows), "plain")
    assert t >= case.m + 1
    return t


def sweep_lengths(pipe, k, lengths):
    wide = int(k == 21)
    for m in lengths:
        r = extra_rows(m)
        probe = Case(m, k, 4 * m + 70)
        t0 = stream_rows(pipe, probe, probe.sequence(pipe))
        case = Case(m, k, 9 * t0 + 5 + 3)
        seq = case.sequence(pipe)
        counts = [t0, t0 + 1, 2 * t0, 2 * t0 + 7, 9 * t0 + 5, m + 1 + r, m + r]
        for mode in MODES:
            configure(pipe, mode)
            for n in counts:
                tally, kernel, t = stored(pipe, case, seq, range(0, n), mode)
                mk, slot = expected_slot(m, mode)
                if n >= mk + 1 + extra_rows(mk):                    # legal for either stream rule: a C = 32 store kernel ran
                    assert (mk, slot) in kernel_rows(tally, wide), (m, mode, n, kernel, sorted(tally))
                    if paired(mk, k, mode):                         # even streams of q*M + 1 + R rows
                        assert t and t % 2 == 0 and (t - 1 - extra_rows(mk)) % mk == 0, (m, n, t)
                    elif mode == "plain":                           # the others: q*M + 1
                        assert t and (t - 1) % mk == 0, (m, n, t)


def test_motif_lengths_dna(pipe):
    sweep_lengths(pipe, 5, DNA)


def test_motif_lengths_protein(pipe):
    sweep_lengths(pipe, 21, PROTEIN)


@pytest.mark.parametrize("quad_loads", [1, 0], ids=["dword_loads", "byte_loads"])
def test_byte_and_dword_symbol_loads(pipe, quad_loads):
    """Both symbol-load forms of the even lengths at the small row counts (M = 18 pads to 20 under dword loads)."""
    for m in (6, 16, 18, 20, 22, 24, 26):
        case = Case(m, 5, 9 * 64 + 8, seed=quad_loads)
        seq = case.sequence(pipe)
        configure(pipe, "plain", quad_loads=quad_loads)
        for n in (m + 1 + extra_rows(m), 2 * (m + 1 + extra_rows(m)) + 7, case.rows):
            tally, kernel, t = stored(pipe, case, seq, range(0, n), "plain")
            assert expected_slot(m, "plain", quad_loads) in kernel_rows(tally, 0), (m, n, kernel, sorted(tally))


BIG_ROWS = 1_100_000 + 77     # / (64 streams per CU x 256 CUs of an MI355X) = 67 rows: the planner grants its default stream
_big = {}


def big_case(m):
    if m not in _big:
        _big[m] = Case(m, 5, BIG_ROWS)
    return _big[m]


@pytest.mark.parametrize("m", [20, 16])
def test_streams_of_several_groups(pipe, m):
    """Enough rows that the planner grants the default stream of 64 rows = three groups and the extra steps: two MAIN
    groups, the second in a frame of its own, and the shifted LAST one behind them; a range with an odd first row and
    a ragged count, so that the last stream is shifted back."""
    case = big_case(m)
    seq = case.sequence(pipe)
    configure(pipe, "plain")
    tally, kernel, t = stored(pipe, case, seq, range(5, case.rows - 2), "plain")
    assert expected_slot(m, "plain") in kernel_rows(tally, 0), (kernel, sorted(tally))
    assert t == 64, t


def test_row_ranges(pipe):
    """Odd first rows and odd lengths for M = 20: the score rows of a range start at its first row, so pairs of rows are
    256-byte aligned or not by the parity of the stream's first row within the RANGE."""
    m = 20
    case = Case(m, 5, 4 * m + 70)
    seq = case.sequence(pipe)
    t0 = stream_rows(pipe, case, seq)
    for mode in MODES:
        configure(pipe, mode)
        for a, b in ((1, case.rows), (3, 3 + 2 * t0 + 7), (7, 7 + t0), (0, case.rows - 1), (5, case.rows - 2), (2, 2 + 3 * t0 + 1)):
            assert b <= case.rows
            tally, kernel, _ = stored(pipe, case, seq, range(a, b), mode)
            assert expected_slot(m, mode) in kernel_rows(tally, 0), (mode, a, b, kernel, sorted(tally))


def test_constant_weights_ties(pipe):
    """Every score equal: the argmax of the tracking forms is the LAST cell (pli/mod.rs:144-151), whichever stream,
    half-wave or duplicate of a shifted stream wrote it."""
    for m in (12, 20):
        weights = np.zeros((m, co.stride(5, 4)), np.float32)
        weights[:, :5] = 0.25
        case = Case(m, 5, 4 * m + 70, weights=weights)
        seq = case.sequence(pipe)
        t0 = stream_rows(pipe, case, seq)
        for mode in ("block_maxima", "tracked"):
            configure(pipe, mode)
            for n in (t0, 2 * t0 + 7, case.rows):
                stored(pipe, case, seq, range(0, n), mode)


@pytest.mark.parametrize("regime,variant", xw.REGIMES, ids=[xw.regime_id(r, v) for r, v in xw.REGIMES])
def test_extreme_weights(pipe, regime, variant):
    """-0.0, +-inf, NaN, subnormals and sums that overflow through every store mode at M = 20, n = 2 T0 + 7."""
    m, k = 20, 5
    probe = Case(m, k, 4 * m + 70)
    t0 = stream_rows(pipe, probe, probe.sequence(pipe))
    rows = 2 * t0 + 7
    weights = xw.make_pssm(regime, variant, m, k)
    enc = xw.make_sequence(regime, variant, 32 * rows - 11, k, m)
    case = Case(m, k, rows, weights=weights, enc=enc)
    seq = case.sequence(pipe)
    for mode in MODES:
        configure(pipe, mode)
        scores = lm.StripedScores.empty(pipe, 32)
        pipe.score_rows_into(case.pssm, seq, range(0, rows), scores)
        got = scores.matrix()
        assert np.array_equal(bits(got[:, :32]), bits(case.want[:, :32])), (regime, variant, mode, pipe.last_kernel)


def test_stream_length_option(pipe):
    """rows_per_stream 44, 61 and 84 for M = 20: the oracle's matrix each time, and T the nearest legal length -- even
    whatever was asked -- below the planner's cap of rows / (64 streams per CU): 44, 64 and, for 84 capped at 67, 64 on
    the large matrix; the small matrix takes every request down to one group."""
    m = 20
    small = Case(m, 5, 4 * m + 70, seed=3)
    for case in (small, big_case(m)):
        seq = case.sequence(pipe)
        seen = []
        for want_t in (44, 61, 84):
            configure(pipe, "plain", rows_per_stream=want_t)
            _, _, t = stored(pipe, case, seq, range(0, case.rows), "plain")
            assert t and t % 2 == 0 and (t - 1 - extra_rows(m)) % m == 0 and t <= 84, (want_t, t)
            seen.append(t)
        if case is not small:
            assert seen == [44, 64, 64], seen
    pipe.set_rows_per_stream(0)
