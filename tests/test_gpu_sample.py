"""Null sequence sets drawn on the device: ``Pipeline.sample_set`` / ``StripedSequenceSet.null`` (``lm_hip_seqset_sample``,
csrc/sample.hip) and ``StripedSequenceSet.count_pairs`` (``lm_hip_seqset_count_pairs``, csrc/pairs.hip).  The expected values
come from the rule restated in numpy (tests/sample_rule.py) and every comparison is exact.  The shapes are the smallest at
which the kernels can go wrong: records around a lane's run of 16 bytes, around a Philox block of 4, around a workgroup's
tile, more records in one tile than its slab of offsets holds, record numbers whose high word changes inside the set.

A set shows its matrix only through the calls that read it: the records are read back position by position (``records()``),
and the set scans of the round trip read every cell of it; the geometry is compared field by field."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest
import torch  # noqa: F401  (loaded before the library, as tools/null_bench.py loads it: its leg C copies with torch)

import lightmotif_amd as lm
from lightmotif_amd import _ffi
from lightmotif_amd import io as lmio

import sample_rule as sr

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
JASPAR = Path(__file__).parent / "golden" / "JASPAR2024.pwm.gz"
T = _ffi.lib().lm_hip_sample_tile_bytes()
SLAB = 1024         # kLdsSlab of csrc/sample_plan.hpp: live-record offsets a workgroup stages in LDS

F = np.array([0.3, 0.2, 0.15, 0.35, 0], dtype=np.float32)
TRANSITIONS = np.array([[.1, .2, .3, .4, 0], [.4, .3, .2, .1, 0], [.25, .25, .25, .25, 0], [.7, .1, .1, .1, 0], [0, 0, 0, 0, 0]],
                       dtype=np.float32)
BORDER_LENGTHS = [0, 1, 3, 4, 5, 15, 16, 17, 0, 0, 63, 64, 65, T - 1, 1, T + 1, 2 * T + 5]
CARRY_LENGTHS = [1, 2, 16, 17, T - 1, T, T + 1, 3 * T + 7, 0, 1, 1, 1]


def check(pli, got, want, cols=32, protein=False, kernel="sample_iid"):
    total = sum(len(w) for w in want)
    assert pli.last_kernel == kernel or total == 0
    assert len(got) == len(want) and got.total_length == total and got.protein == protein
    assert got.rows == (total + cols - 1) // cols and got.columns == cols and got.wrap == 0
    assert np.array_equal(got.lengths, [len(w) for w in want])
    for i, (g, w) in enumerate(zip(got.records(), want)):
        if not np.array_equal(g.data, w):
            bad = np.flatnonzero(g.data != w)
            raise AssertionError(f"record {i} of {len(w)} symbols: {bad.size} differ, first at {bad[0]}")
    return got


def test_the_tile_is_what_the_test_thinks():
    assert T == 4096


@pytest.mark.parametrize("cols, protein", [(32, False), (16, False), (32, True)])
def test_borders_order0_shared_model(pli, cols, protein):
    f = np.array([0.05] * 20 + [0], dtype=np.float32) if protein else F
    for seed, base in ((1, 0), (12345, (1 << 32) - 3)):          # hi32(R) changes inside the second set
        got = pli.sample_set(BORDER_LENGTHS, f, seed=seed, record_base=base, protein=protein, columns=cols)
        check(pli, got, sr.sample(BORDER_LENGTHS, f, seed=seed, record_base=base), cols, protein)


@pytest.mark.parametrize("cols, protein", [(32, False), (16, False), (32, True)])
def test_borders_order0_per_record_models(pli, cols, protein):
    k = 21 if protein else 5
    rng = np.random.default_rng(11)
    f = rng.random((len(BORDER_LENGTHS), k)).astype(np.float32)
    f[rng.random(f.shape) < 0.3] = 0                             # T = 0 and T = 2^32 among the thresholds
    f[:, 1] += 0.1
    f[0] = np.nan                                                # the model of an EMPTY record is never looked at
    f[8] = 0
    got = pli.sample_set(BORDER_LENGTHS, f, seed=77, record_base=(1 << 32) - 3, protein=protein, columns=cols)
    check(pli, got, sr.sample(BORDER_LENGTHS, f, seed=77, record_base=(1 << 32) - 3), cols, protein)


def test_the_small_vectors_of_the_rule(pli):
    got = pli.sample_set([8, 8], F, seed=1).records()
    assert got[0].data.tolist() == [3, 3, 2, 3, 3, 3, 1, 3] and got[1].data.tolist() == [2, 0, 0, 0, 3, 3, 0, 0]
    assert pli.sample_set([8], F, seed=2).records()[0].data.tolist() == [1, 1, 3, 1, 0, 0, 3, 1]


def test_many_tiny_records_with_their_own_models(pli):
    """5 000 records of 0 ... 3 symbols: more live records in one tile than its slab of offsets holds."""
    rng = np.random.default_rng(5)
    lengths = rng.integers(0, 4, 5_000)
    assert (lengths > 0).sum() > 3 * SLAB and lengths.sum() < 2 * T
    f = rng.random((5_000, 5)).astype(np.float32) + np.float32(0.01)
    got = pli.sample_set(lengths, f, seed=9, record_base=40)
    check(pli, got, sr.sample(lengths, f, seed=9, record_base=40))


def test_records_are_independent_and_calls_repeat(pli):
    a_len, b_len = [5, 0, 900, 17, 4, 4, 4, 1_234, 60], [1, 77, 3, 0, 0, 5_000, 33, 1_234, 0, 12]
    a = pli.sample_set(a_len, F, seed=3)
    b = pli.sample_set(b_len, F, seed=3)
    ra, rb = a.records(), b.records()
    assert np.array_equal(ra[7].data, rb[7].data) and len(ra[7]) == 1_234
    again = pli.sample_set(a_len, F, seed=3)
    assert [r.data.tobytes() for r in again.records()] == [r.data.tobytes() for r in ra]
    other = pli.sample_set(a_len, F, seed=4)
    assert not np.array_equal(other.records()[7].data, ra[7].data)
    narrow = pli.sample_set(a_len, F, seed=3, columns=16)
    assert narrow.columns == 16 and narrow.rows != a.rows
    assert [r.data.tobytes() for r in narrow.records()] == [r.data.tobytes() for r in ra]
    # record_base shifts the numbering: record 2 of a set based at 5 is record 7
    shifted = pli.sample_set([3, 3, 1_234], F, seed=3, record_base=5)
    assert np.array_equal(shifted.records()[2].data, ra[7].data)
    # order 1 likewise
    c = pli.sample_set(a_len, F, TRANSITIONS, seed=3)
    d = pli.sample_set(b_len, F, TRANSITIONS, seed=3)
    assert np.array_equal(c.records()[7].data, d.records()[7].data)


def test_empty_sets_launch_nothing(pli):
    one = pli.sample_set([4], F)
    assert pli.last_kernel == "sample_iid" and len(one) == 1
    for order1 in (False, True):
        empty = pli.sample_set([0, 0, 0], F, TRANSITIONS if order1 else None)
        assert len(empty) == 3 and empty.total_length == 0 and empty.rows == 0 and [len(r) for r in empty.records()] == [0, 0, 0]
        none = pli.sample_set([], F, TRANSITIONS if order1 else None)
        assert len(none) == 0 and none.total_length == 0
    # models nobody uses are not judged
    assert len(pli.sample_set([0, 0], np.zeros(5, dtype=np.float32))) == 2


IDENTITY = np.eye(5, dtype=np.float32)
IDENTITY[4, 4] = 0
CYCLE = np.zeros((5, 5), dtype=np.float32)                          # A -> C -> T -> G -> A on symbol indices 0 1 2 3
for _a in range(4):
    CYCLE[_a, (_a + 1) % 4] = 1


def test_order1_carry_without_randomness(pli):
    """Transitions that leave nothing to chance: a lost or misapplied carry at a lane, wavefront, workgroup or tile border
    shows as a wrong symbol."""
    quarter = np.array([0.25, 0.25, 0.25, 0.25, 0], dtype=np.float32)
    for seed in (1, 2):
        got = pli.sample_set(CARRY_LENGTHS, quarter, IDENTITY, seed=seed)
        assert pli.last_kernel == "markov_emit"
        firsts = set()
        for n, rec in zip(CARRY_LENGTHS, got.records()):
            assert len(rec) == n
            if n:
                assert (rec.data == rec.data[0]).all()
                firsts.add(int(rec.data[0]))
        want = sr.sample(CARRY_LENGTHS, quarter, IDENTITY, seed=seed)
        assert [int(w[0]) for w in want if len(w)] == [int(r.data[0]) for r in got.records() if len(r)]
        assert len(firsts) > 1
        got = pli.sample_set(CARRY_LENGTHS, quarter, CYCLE, seed=seed)
        for rec, w in zip(got.records(), want):
            if len(w):
                assert np.array_equal(rec.data, (int(w[0]) + np.arange(len(w))) % 4)


@pytest.mark.parametrize("cols", [32, 16])
def test_order1_with_randomness(pli, cols):
    lengths = CARRY_LENGTHS + BORDER_LENGTHS
    for base in (0, (1 << 32) - 3):
        got = pli.sample_set(lengths, F, TRANSITIONS, seed=99, record_base=base, columns=cols)
        check(pli, got, sr.sample(lengths, F, TRANSITIONS, seed=99, record_base=base), cols, kernel="markov_emit")
    # N has mass and a row of its own
    rng = np.random.default_rng(2)
    initial = np.array([0.2, 0.2, 0.2, 0.2, 0.2], dtype=np.float32)
    with_n = rng.random((5, 5)).astype(np.float32)
    got = pli.sample_set(lengths, initial, with_n, seed=5, columns=cols)
    want = sr.sample(lengths, initial, with_n, seed=5)
    assert any((w == 4).any() for w in want)
    check(pli, got, want, cols, kernel="markov_emit")
    # a zero row in the middle stands for `initial`
    hole = with_n.copy()
    hole[2] = 0
    got = pli.sample_set(lengths, initial, hole, seed=6, columns=cols)
    check(pli, got, sr.sample(lengths, initial, hole, seed=6), cols, kernel="markov_emit")


def fuzzed_records(seed, k):
    rng = np.random.default_rng(seed)
    lengths = [0, 0, 1, 0, 1, 1, 0, 0, 0, 2, 700, 3, 0] + rng.integers(0, 40, 300).tolist() + [0, 0, 5_000, 0, 1, 0, 0]
    records = [rng.integers(0, k, n).astype(np.uint8) for n in lengths]
    records[10][100:400] = k - 1                                  # a run of the default symbol
    return records


@pytest.mark.parametrize("cols, protein", [(32, False), (16, False), (32, True), (16, True)])
def test_count_pairs(pli, cols, protein):
    k = 21 if protein else 5
    records = fuzzed_records(3 + cols + k, k)
    seqset = pli.stripe_set([lm.EncodedSequence(r, protein=protein) for r in records], columns=cols, protein=protein)
    assert max(len(r) for r in records) > seqset.rows            # a record longer than a column
    got = seqset.count_pairs()
    assert got.dtype == np.int64 and got.shape == (k, k)
    assert np.array_equal(got, sr.count_pairs(records, k))
    assert got.sum() == sum(max(len(r) - 1, 0) for r in records)
    assert np.array_equal(seqset.count_pairs(), got)
    seqset.configure_wrap(30)                                     # wrap rows are never read
    assert np.array_equal(seqset.count_pairs(), got)
    # sets without a pair
    for lengths in ([], [0, 0], [1], [0, 1, 0, 1, 1]):
        tiny = pli.stripe_set([lm.EncodedSequence(np.zeros(n, dtype=np.uint8), protein=protein) for n in lengths], columns=cols,
                              protein=protein)
        assert not tiny.count_pairs().any()
    two = pli.stripe_set([lm.EncodedSequence(np.array([1, 3], dtype=np.uint8), protein=protein)], columns=cols, protein=protein)
    assert two.count_pairs()[1, 3] == 1 and two.count_pairs().sum() == 1


def test_markov_from_counts_and_null(pli):
    rng = np.random.default_rng(8)
    records = [rng.choice(5, n, p=[0.3, 0.2, 0.2, 0.25, 0.05]).astype(np.uint8) for n in [300, 0, 5, 1, 2_000, 0, 0, 64]]
    seqset = pli.stripe_set([lm.EncodedSequence(r) for r in records])
    sym, pairs = seqset.count_symbols(), seqset.count_pairs()
    for kwargs in ({}, {"pseudocount": 0.5}, {"unknown": True}, {"pseudocount": 1.0, "unknown": True}):
        got, want = lm.markov_from_counts(sym, pairs, **kwargs), sr.markov_from_counts(sym, pairs, **kwargs)
        assert got[0].dtype == got[1].dtype == np.float32
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    # null(0): every record from its own composition, N included; null(1): one chain for the set
    lengths = [len(r) for r in records]
    model = np.zeros((len(records), 5), dtype=np.float32)
    for r, row in enumerate(sym):
        if row.sum():
            model[r] = row.astype(np.float32) / np.float32(row.sum())
    got = seqset.null(0, seed=21, record_base=3)
    check(pli, got, sr.sample(lengths, model, seed=21, record_base=3))
    assert any((r.data == 4).any() for r in got.records())
    initial, transitions = sr.markov_from_counts(sym, pairs)
    got = seqset.null(1, seed=22, record_base=3)
    check(pli, got, sr.sample(lengths, initial, transitions, seed=22, record_base=3), kernel="markov_emit")
    with pytest.raises(ValueError):
        seqset.null(2)


@pytest.fixture(scope="module")
def motifs():
    records = list(lmio.read(JASPAR))[:40:5]
    assert len(records) == 8
    return [r.matrix.normalize(0.1).log_odds() for r in records]


def test_a_null_set_is_interchangeable_with_a_built_one(pli, motifs):
    """2 000 x 200 bp: ``null(1)`` equals ``stripe_set`` of the rule's records under the set scans, table for table."""
    rng = np.random.default_rng(6)
    symbols = [rng.choice(5, 200, p=[0.24, 0.24, 0.24, 0.24, 0.04]).astype(np.uint8) for _ in range(2_000)]
    source = pli.stripe_set([lm.EncodedSequence(s) for s in symbols])
    initial, transitions = sr.markov_from_counts(source.count_symbols(), source.count_pairs())
    want = sr.sample([200] * 2_000, initial, transitions, seed=31)
    null = check(pli, source.null(1, seed=31), want, kernel="markov_emit")
    built = pli.stripe_set([lm.EncodedSequence(w) for w in want])
    max_m = max(len(m) for m in motifs)
    null.configure_wrap(max_m)
    built.configure_wrap(max_m)
    batch = pli.prepare_batch(motifs, [3.0] * len(motifs))
    a, b = pli.scan_count_set(batch, [3.0] * len(motifs), null), pli.scan_count_set(batch, [3.0] * len(motifs), built)
    assert a.counts.tobytes() == b.counts.tobytes() and a.windows.tobytes() == b.windows.tobytes() and a.counts.any()
    a, b = pli.scan_best_set(batch, null), pli.scan_best_set(batch, built)
    assert a.raw.tobytes() == b.raw.tobytes() and a.found.any()
    a, b = pli.scan_sum_set(batch, null), pli.scan_sum_set(batch, built)
    assert a.sums.tobytes() == b.sums.tobytes()
    assert np.array_equal(null.count_symbols(), built.count_symbols()) and np.array_equal(null.count_pairs(), built.count_pairs())


def abi(ctx, alphabet, lengths, n, freq, n_models, transitions, cols, out):
    return _ffi.lib().lm_hip_seqset_sample(ctx, alphabet, lengths, n, freq, n_models, transitions, 1, 0, cols, out)


def test_misuse_is_a_status(pli):
    lengths = np.array([3, 0, 40], dtype=np.uint64)
    f = np.ascontiguousarray(F)
    per = np.ascontiguousarray(np.tile(F, (3, 1)))
    t = np.ascontiguousarray(TRANSITIONS)
    SENTINEL = 0xDEAD0

    def refused(what, ctx=pli._h, alphabet=b"D", lens=lengths, n=3, freq=f, n_models=1, transitions=None, cols=32, with_out=True,
                status=_ffi.ERR_BAD_ARGS, names=None):
        out = C.c_void_p(SENTINEL)
        st = abi(ctx, alphabet, lens.ctypes.data if lens is not None else None, n, freq.ctypes.data if freq is not None else None,
                 n_models, transitions.ctypes.data if transitions is not None else None, cols, C.byref(out) if with_out else None)
        assert st == status, (what, st, _ffi.last_error())
        assert _ffi.last_error() and "seqset_sample" in _ffi.last_error(), what
        if names:
            assert names in _ffi.last_error(), (what, _ffi.last_error())
        if with_out:
            assert out.value is None, what            # *out == NULL after any failure

    refused("null ctx", ctx=None)
    refused("null out", with_out=False)
    refused("null frequencies", freq=None)
    refused("null lengths with records", lens=None)
    refused("zero columns", cols=0)
    refused("an unknown alphabet", alphabet=b"X")
    refused("two models for three records", freq=per, n_models=2)
    refused("no model", n_models=0)
    refused("a chain for protein", alphabet=b"P", freq=np.ones(21, dtype=np.float32), transitions=np.ones((21, 21), dtype=np.float32))
    refused("a chain per record", freq=per, n_models=3, transitions=t)
    bad = per.copy()
    bad[2, 1] = -1
    refused("an invalid row of a live record", freq=bad, n_models=3, names="record 2")
    refused("a shared row without mass", freq=np.zeros(5, dtype=np.float32), names="row 0")
    refused("a shared row with a NaN", freq=np.array([1, np.nan, 0, 0, 0], dtype=np.float32))
    refused("an infinite frequency", freq=np.array([np.inf, 1, 0, 0, 0], dtype=np.float32))
    broken = t.copy()
    broken[3, 0] = -0.25
    refused("a transition row that is neither a model nor zero", transitions=broken, names="row 3")
    refused("a chain that cannot start", freq=np.zeros(5, dtype=np.float32), transitions=t)
    huge = np.array([1 << 39, 1 << 39, 1], dtype=np.uint64)
    refused("past the cells of a hit list", lens=huge, status=_ffi.ERR_CAPACITY)
    wraps = np.array([(1 << 64) - 1, (1 << 64) - 1, 2], dtype=np.uint64)
    refused("lengths that would wrap", lens=wraps, status=_ffi.ERR_CAPACITY)
    # and what is no misuse: no records at all, an invalid row of an empty record, an invalid transition row nobody takes
    out = C.c_void_p(SENTINEL)
    assert abi(pli._h, b"D", None, 0, f.ctypes.data, 1, None, 32, C.byref(out)) == 0 and out.value not in (None, SENTINEL)
    _ffi.lib().lm_hip_seqset_destroy(out)
    ok = per.copy()
    ok[1] = -1
    out = C.c_void_p(SENTINEL)
    assert abi(pli._h, b"D", lengths.ctypes.data, 3, ok.ctypes.data, 3, None, 32, C.byref(out)) == 0 and out.value not in (None, SENTINEL)
    _ffi.lib().lm_hip_seqset_destroy(out)
    ones = np.array([1, 0, 1], dtype=np.uint64)
    out = C.c_void_p(SENTINEL)
    assert abi(pli._h, b"D", ones.ctypes.data, 3, f.ctypes.data, 1, broken.ctypes.data, 32, C.byref(out)) == 0
    _ffi.lib().lm_hip_seqset_destroy(out)
    # count_pairs
    seqset = pli.stripe_set([lm.EncodedSequence(np.zeros(9, dtype=np.uint8))])
    table = np.zeros(25, dtype=np.uint64)
    L = _ffi.lib()
    for args in ((None, seqset._h, table.ctypes.data, 25), (pli._h, None, table.ctypes.data, 25), (pli._h, seqset._h, None, 25)):
        assert L.lm_hip_seqset_count_pairs(*args) == _ffi.ERR_BAD_ARGS and "seqset_count_pairs" in _ffi.last_error()
    assert L.lm_hip_seqset_count_pairs(pli._h, seqset._h, table.ctypes.data, 24) == _ffi.ERR_CAPACITY
    # the Python layer refuses shapes before the library sees them
    with pytest.raises(ValueError):
        pli.sample_set([1, 2], np.ones((3, 5), dtype=np.float32))
    with pytest.raises(ValueError):
        pli.sample_set([1, 2], np.ones(4, dtype=np.float32))
    with pytest.raises(ValueError):
        pli.sample_set([1, 2], F, np.ones((4, 4), dtype=np.float32))
    with pytest.raises(_ffi.LightmotifHipError):
        pli.sample_set([1, 2], np.ones(21, dtype=np.float32), np.ones((21, 21), dtype=np.float32), protein=True)


def test_the_device_draw_beats_the_host_generator(pli):
    """2 000 records x 5 000 bp, every record from its own composition: ``StripedSequenceSet.null(0)`` (B) against numpy's
    ``Generator.choice`` per record + ``stripe_set`` (A), the only road before; C is a device-to-device copy of the result's
    bytes, the floor.  Medians of 5 alternating runs after a warm-up.  The margin is 1 x: A contains B's whole output as an
    upload plus a host generator (measured once: A 112 ms, B 0.43 ms, C 0.12 ms; DESIGN 4.6i, tools/null_bench.py)."""
    sys.path.insert(0, str(ROOT / "tools"))
    import null_bench
    res = null_bench.measure(pli, 2_000, 5_000, "order0_per_record", runs=5, warmup=1)
    a, b, c = res["ms"]["A"], res["ms"]["B"], res["ms"]["C"]
    print(f"A (numpy choice + stripe_set) median {a['median']:.2f} ms [{a['min']:.2f}, {a['max']:.2f}]  B (null) median "
          f"{b['median']:.3f} ms [{b['min']:.3f}, {b['max']:.3f}]  C (device copy) median {c['median']:.3f} ms [{c['min']:.3f}, "
          f"{c['max']:.3f}]  A/B {res['A_over_B']:.1f}  B/C {res['B_over_C']:.2f}  draw kernels {res.get('draw_kernels_ms')}")
    assert res["sets_alike"]
    assert len(a["all"]) >= 5 and len(b["all"]) >= 5
    assert b["median"] < a["median"]
