"""A sequence set cut out of a resident set on the device: ``StripedSequenceSet.regions`` (``lm_hip_seqset_from_regions``,
csrc/regions.hip).  The rule is a few lines of numpy on host copies of the records (tests/regions_rule.py): ``rec[s:e]``, or
the complement of ``rec[s:e]`` reversed; every comparison is exact.  The shapes are the smallest at which the gather can go
wrong: records that cross several source columns, more regions than one slab of offsets, region switches at every offset
of a lane's run.

Not covered: bytes >= k passing through unchanged.  No fixture builds a SET that holds such bytes (every set builder
validates its symbols, and only a single sequence can be adopted), so that point of the contract is checked on the host
map alone (tests/cpp/test_regions_plan.cpp: ``complement`` over all 256 bytes)."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest
import torch  # noqa: F401  (loaded before the library, as tools/regions_bench.py loads it: its leg C copies with torch)

import lightmotif_amd as lm
from lightmotif_amd import _ffi
from lightmotif_amd import io as lmio
from lightmotif_amd.lib import REGION_DTYPE

import regions_rule as rr

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
JASPAR = Path(__file__).parent / "golden" / "JASPAR2024.pwm.gz"
RUN = 16            # kRun of csrc/regions_plan.hpp: destination bytes per lane
TILE = 4096         # kTile: destination bytes per workgroup
SLAB = 1024         # kLdsSlab: destination offsets a workgroup stages in LDS


def make_set(pli, symbols, protein=False, cols=32):
    return pli.stripe_set([lm.EncodedSequence(np.asarray(s, dtype=np.uint8), protein=protein) for s in symbols], columns=cols,
                          protein=protein)


def random_records(seed, lengths, k=5):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, k, n).astype(np.uint8) for n in lengths]


def check(pli, source, symbols, records, starts, ends, strands, cols=32):
    """The derived set against the rule: the taken table, the records, and the geometry of an ordinary set."""
    want, want_taken = rr.extract(symbols, records, starts, ends, strands)
    derived, taken = source.regions(records, starts, ends, strands)
    assert pli.last_kernel == "region_gather" or sum(len(w) for w in want) == 0
    assert taken.shape == (len(want), 2) and taken.dtype == np.int64 and np.array_equal(taken, want_taken)
    total = sum(len(w) for w in want)
    assert len(derived) == len(want) and derived.total_length == total
    assert derived.rows == (total + cols - 1) // cols and derived.columns == cols and derived.wrap == 0
    assert np.array_equal(derived.lengths, [len(w) for w in want])
    got = derived.records()
    for i, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g.data, w), (i, int(records[i]), int(starts[i]), int(ends[i]), int(strands[i]))
    return derived, want


@pytest.fixture(scope="module")
def borders():
    """3 records of 0, 97 and 140 symbols, and every region [s, e) of the 97-symbol one with e - s <= 40 on both strands: about
    6 000 regions of 20 symbols on average, several slabs of offsets per call."""
    symbols = random_records(1, [0, 97, 140])
    se = [(s, e) for s in range(0, 98) for e in range(s, min(s + 40, 97) + 1)]
    starts = np.array([s for s, _ in se] * 2, dtype=np.int64)
    ends = np.array([e for _, e in se] * 2, dtype=np.int64)
    strands = np.repeat([0, 1], len(se)).astype(np.uint8)
    assert len(starts) > 6_000
    return symbols, np.ones(len(starts), dtype=np.int64), starts, ends, strands


@pytest.mark.parametrize("cols", [32, 16])
def test_column_and_tail_borders(pli, borders, cols):
    """At 32 columns the source has 8 rows (at 16, 15): every record crosses several source columns, in both directions."""
    symbols, records, starts, ends, strands = borders
    source = make_set(pli, symbols, cols=cols)
    assert source.rows == (237 + cols - 1) // cols
    check(pli, source, symbols, records, starts, ends, strands, cols)


@pytest.mark.parametrize("strand", [0, 1])
def test_run_and_region_borders(pli, strand):
    """Region lengths 0, 1, 2 ... 2 x run + 1 end to end, with empty and single-symbol regions between them and the whole
    ladder repeated from 16 different phases: every run of a lane sees a region switch at every offset.  Then 3 000
    single-symbol regions: more live regions inside one workgroup's tile than its slab of offsets holds."""
    symbols = random_records(2, [61, 0, 300])
    records, starts, ends = [], [], []
    for phase in range(RUN):
        records += [2] * phase                      # `phase` single symbols shift the ladder by that many bytes
        starts += list(range(phase))
        ends += [s + 1 for s in range(phase)]
        for n in range(2 * RUN + 2):
            records += [2, 1, 0, 2]                 # the region | an empty source record | a single symbol | start == end
            starts += [phase + n, 0, n, 5]
            ends += [phase + 2 * n, 10, n + 1, 5]
    a = len(records)
    records += [2] * 3_000
    starts += [i % 300 for i in range(3_000)]
    ends += [i % 300 + 1 for i in range(3_000)]
    strands = np.full(len(records), strand, dtype=np.uint8)
    assert 3_000 > SLAB and len(records) - a == 3_000
    source = make_set(pli, symbols)
    check(pli, source, symbols, np.array(records), np.array(starts), np.array(ends), strands)


def test_unsorted_duplicated_overlapping_and_whole_records(pli):
    symbols = random_records(3, [50, 5_000, 1, 0, 333])
    rng = np.random.default_rng(33)
    n = 400
    records = rng.integers(0, 5, n)
    starts = rng.integers(0, 400, n)
    ends = starts + rng.integers(0, 300, n)
    strands = rng.integers(0, 2, n).astype(np.uint8)
    lengths = np.array([len(s) for s in symbols])
    whole = np.array([1, 0, 4, 2, 3, 1, 1])         # whole records, one of them three times
    records = np.concatenate([records, whole, records[:50]])           # ... and 50 duplicates
    starts = np.concatenate([starts, np.zeros(len(whole), dtype=np.int64), starts[:50]])
    ends = np.concatenate([ends, lengths[whole], ends[:50]])
    strands = np.concatenate([strands, [0, 1, 0, 1, 0, 1, 0], strands[:50]]).astype(np.uint8)
    source = make_set(pli, symbols)
    check(pli, source, symbols, records, starts, ends, strands)
    # a result larger than its source: one 50-symbol record taken 300 times
    small = make_set(pli, symbols[:1])
    derived, _ = check(pli, small, symbols[:1], np.zeros(300, dtype=np.int64), np.zeros(300, dtype=np.int64), np.full(300, 50),
                       (np.arange(300) % 2).astype(np.uint8))
    assert derived.total_length == 300 * 50 > small.total_length * 4 and derived.total_length > 3 * TILE


def test_clipping_and_empty_regions_keep_their_indices(pli):
    symbols = random_records(4, [40, 0, 75])
    big = 2**63 - 1
    table = [  # record, start, end, strand -> taken
        (0, -7, 10, 0, (0, 10)), (0, 35, 100, 1, (35, 40)), (0, -big - 1, big, 0, (0, 40)), (0, -big - 1, big, 1, (0, 40)),
        (0, 40, 50, 0, (0, 0)), (0, -20, 0, 1, (0, 0)), (0, 41, 45, 0, (0, 0)), (0, 30, 20, 0, (0, 0)), (0, big, -big - 1, 1, (0, 0)),
        (3, 0, 10, 0, (0, 0)), (2**62, 0, 10, 1, (0, 0)), (1, 0, 10, 0, (0, 0)), (1, -big - 1, big, 1, (0, 0)),
        (2, 74, 75, 1, (74, 75)), (2, 74, big, 0, (74, 75)), (2, -1, 1, 1, (0, 1)), (2, 10, 10, 0, (0, 0)),
    ]
    records = np.array([t[0] for t in table], dtype=np.uint64)
    starts = np.array([t[1] for t in table], dtype=np.int64)
    ends = np.array([t[2] for t in table], dtype=np.int64)
    strands = np.array([t[3] for t in table], dtype=np.uint8)
    source = make_set(pli, symbols)
    want, want_taken = rr.extract(symbols, [int(r) for r in records], starts, ends, strands)
    assert [tuple(x) for x in want_taken.tolist()] == [t[4] for t in table]          # (the rule itself, against the table)
    derived, taken = source.regions(records, starts, ends, strands)
    assert np.array_equal(taken, want_taken)
    assert derived.lengths.tolist() == [b - a for _, _, _, _, (a, b) in table]
    for g, w in zip(derived.records(), want):
        assert np.array_equal(g.data, w)
    # nothing but empty regions: n empty records and no launch; no regions: a set of no records
    before = source.regions([0], [0], [1])[0]
    assert pli.last_kernel == "region_gather" and len(before) == 1
    pli.sync()
    empty, taken = source.regions([0, 1, 9], [50, 0, 0], [60, 5, 5], ["-", "+", "."])
    assert len(empty) == 3 and empty.total_length == 0 and empty.rows == 0 and empty.lengths.tolist() == [0, 0, 0]
    assert not taken.any() and [len(r) for r in empty.records()] == [0, 0, 0]
    none, taken = source.regions([], [], [])
    assert len(none) == 0 and none.total_length == 0 and taken.shape == (0, 2)
    # a source without symbols, and one without records
    for src in (make_set(pli, [[], []]), make_set(pli, [])):
        d, taken = src.regions([0, 1, 2], [0, 0, 0], [5, 5, 5], [0, 1, 0])
        assert len(d) == 3 and d.total_length == 0 and not taken.any()


def test_protein_sets_have_one_strand(pli):
    symbols = random_records(5, [0, 130, 45], k=21)
    source = make_set(pli, symbols, protein=True)
    rng = np.random.default_rng(55)
    n = 200
    records, starts = rng.integers(0, 4, n), rng.integers(-5, 130, n)
    ends = starts + rng.integers(0, 60, n)
    derived, want = check(pli, source, symbols, records, starts, ends, np.zeros(n, dtype=np.uint8))
    assert derived.protein and derived.count_symbols().shape == (n, 21)
    with pytest.raises(_ffi.LightmotifHipError, match="DNA only"):
        source.regions([1], [0], [5], ["-"])


@pytest.fixture(scope="module")
def motifs():
    records = list(lmio.read(JASPAR))[:40:5]
    assert len(records) == 8
    return [r.matrix.normalize(0.1).log_odds() for r in records]


def test_a_derived_set_is_interchangeable_with_a_built_one(pli, motifs):
    """2 000 x 200 bp, 500 mixed-strand regions, 8 JASPAR matrices: every set call on the derived set equals, bit for bit, the
    same call on ``stripe_set`` of the host-extracted records."""
    rng = np.random.default_rng(6)
    symbols = [rng.choice(5, 200, p=[0.24, 0.24, 0.24, 0.24, 0.04]).astype(np.uint8) for _ in range(2_000)]
    source = make_set(pli, symbols)
    n = 500
    records, starts = rng.integers(0, 2_000, n), rng.integers(-20, 190, n)
    ends = starts + rng.integers(0, 120, n)
    strands = rng.integers(0, 2, n).astype(np.uint8)
    derived, want = check(pli, source, symbols, records, starts, ends, strands)
    built = make_set(pli, want)
    max_m = max(len(m) for m in motifs)
    derived.configure_wrap(max_m)
    built.configure_wrap(max_m)
    batch = pli.prepare_batch(motifs, [3.0] * len(motifs))
    a, b = pli.scan_threshold_set(batch, None, derived), pli.scan_threshold_set(batch, None, built)
    assert np.array_equal(a.counts, b.counts) and a.hits.tobytes() == b.hits.tobytes() and a.total > 100
    a, b = pli.scan_best_set(batch, derived), pli.scan_best_set(batch, built)
    assert a.found.tobytes() == b.found.tobytes() and a.position.tobytes() == b.position.tobytes()
    assert a.score.tobytes() == b.score.tobytes() and a.found.any()
    a, b = pli.scan_count_set(batch, [3.0] * len(motifs), derived), pli.scan_count_set(batch, [3.0] * len(motifs), built)
    assert a.counts.tobytes() == b.counts.tobytes() and a.windows.tobytes() == b.windows.tobytes() and a.counts.any()
    assert np.array_equal(derived.count_symbols(), built.count_symbols())
    assert np.array_equal(derived.count_symbols(), [np.bincount(w, minlength=5) for w in want])


def test_wrap_rows_of_the_source_are_never_read_and_calls_repeat(pli, borders):
    symbols, records, starts, ends, strands = borders
    source = make_set(pli, symbols)

    def shown():
        derived, taken = source.regions(records, starts, ends, strands)
        return [taken.tobytes(), derived.lengths.tobytes()] + [r.data.tobytes() for r in derived.records()]

    first = shown()
    assert shown() == first
    source.configure_wrap(40)
    assert source.wrap == 40 and shown() == first


def abi(pli, src, regions, n, out, taken=None):
    return _ffi.lib().lm_hip_seqset_from_regions(pli, src, regions, n, out, taken)


def test_misuse_is_a_status(pli):
    dna = make_set(pli, random_records(7, [30, 20]))
    protein = make_set(pli, random_records(7, [30], k=21), protein=True)
    good = np.zeros(2, dtype=REGION_DTYPE)
    good["end"] = 10
    SENTINEL = 0xDEAD0

    def refused(ctx, src, reg, n, with_out=True, what=""):
        out = C.c_void_p(SENTINEL)
        st = abi(ctx, src, reg.ctypes.data if reg is not None else None, n, C.byref(out) if with_out else None)
        assert st == _ffi.ERR_BAD_ARGS, (what, st)
        assert _ffi.last_error() and "seqset_from_regions" in _ffi.last_error(), what
        if with_out:
            assert out.value is None, what            # *out == NULL after any failure
    refused(None, dna._h, good, 2, what="null ctx")
    refused(pli._h, None, good, 2, what="null src")
    refused(pli._h, dna._h, good, 2, with_out=False, what="null out")
    refused(pli._h, dna._h, None, 2, what="null regions with n > 0")
    for strand in (2, 3, ord("-"), ord("+"), 255):
        bad = good.copy()
        bad["strand"][1] = strand
        refused(pli._h, dna._h, bad, 2, what=f"strand {strand}")
    minus = good.copy()
    minus["strand"][1] = 1
    refused(pli._h, protein._h, minus, 2, what="strand 1 on a protein set")
    # and what is no misuse: null regions with n == 0, a null taken table, strand 0 on a protein set
    out = C.c_void_p(SENTINEL)
    assert abi(pli._h, dna._h, None, 0, C.byref(out)) == 0 and out.value not in (None, SENTINEL)
    _ffi.lib().lm_hip_seqset_destroy(out)
    out = C.c_void_p(SENTINEL)
    assert abi(pli._h, protein._h, good.ctypes.data, 2, C.byref(out), None) == 0 and out.value not in (None, SENTINEL)
    _ffi.lib().lm_hip_seqset_destroy(out)
    out = C.c_void_p(SENTINEL)
    assert abi(pli._h, dna._h, minus.ctypes.data, 2, C.byref(out), None) == 0 and out.value not in (None, SENTINEL)
    _ffi.lib().lm_hip_seqset_destroy(out)
    if lm.Pipeline.device_count() > 1:               # a set on another device than the context
        other = lm.Pipeline.hip(1)
        refused(other._h, dna._h, good, 2, what="another device")


def test_the_device_gather_beats_the_read_back(pli):
    """2 000 contigs x 5 000 bp, 20 000 regions x 200 bp, half of them on the minus strand: ``StripedSequenceSet.regions`` (B)
    against ``windows`` + a host reverse complement + ``stripe_set`` (A), the only road before; C is a device-to-device copy
    of the result's bytes, the floor.  Medians of 5 alternating runs after a warm-up, equal sets first.  The margin is 1 x: a
    road that does not beat the one it replaces should not exist (the measured medians and ratios of the workloads this is
    for are in profiles/regions_bench.json)."""
    sys.path.insert(0, str(ROOT / "tools"))
    import regions_bench
    res = regions_bench.measure(pli, 2_000, 5_000, 20_000, 200, runs=5, warmup=1)
    a, b, c = res["ms"]["A"], res["ms"]["B"], res["ms"]["C"]
    print(f"A (windows + host rc + stripe_set) median {a['median']:.2f} ms [{a['min']:.2f}, {a['max']:.2f}]  B (regions) median "
          f"{b['median']:.3f} ms [{b['min']:.3f}, {b['max']:.3f}]  C (device copy) median {c['median']:.3f} ms [{c['min']:.3f}, "
          f"{c['max']:.3f}]  A/B {res['A_over_B']:.1f}  B/C {res['B_over_C']:.2f}  bytes {res['result_bytes']}")
    assert res["sets_equal"]
    assert len(a["all"]) >= 5 and len(b["all"]) >= 5
    assert b["median"] < a["median"]
