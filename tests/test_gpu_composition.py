"""Symbol counts on the device: ``StripedSequence.count_symbols`` / ``StripedSequenceSet.count_symbols``
(``lm_hip_seq_count_symbols`` / ``lm_hip_seqset_count_symbols``, csrc/composition.hip) against ``np.bincount`` of the host's
symbols.  The option ``count_tile_rows`` makes small inputs span many blocks of the count table and of its scan."""
import contextlib

import numpy as np
import pytest
import torch

import lightmotif_amd as lm
from lightmotif_amd import _ffi
from lightmotif_amd.lib import background_from_counts

import seqset_reference as sr

pytestmark = pytest.mark.gpu

SEED_BASE = 7_300           # of this file's own: seeds of seqset_reference.draw_case
DEFAULT_TILE = 1024         # kCountTileRows of csrc/composition.hip


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@contextlib.contextmanager
def tile_rows(pli, rows):
    """``rows`` = None: the library's default."""
    pli.set_option("count_tile_rows", rows or 0)
    try:
        yield
    finally:
        pli.set_option("count_tile_rows", 0)


def draw_symbols(rng, n, k):
    """Skewed over the k - 1 proper symbols, 3 % of the default symbol: the padded tail holds the same byte as a real N."""
    weights = np.arange(1, k, dtype=np.float64) ** 1.5
    sym = rng.choice(k - 1, n, p=weights / weights.sum()).astype(np.uint8)
    sym[rng.random(n) < 0.03] = k - 1
    return sym


def host_counts(sym, k):
    return np.bincount(sym, minlength=k).astype(np.int64)


def host_table(symbols, k):
    """(records, k) from the per-record symbol arrays: a bincount of record * k + symbol."""
    lengths = np.array([len(s) for s in symbols], dtype=np.int64)
    if not len(symbols):
        return np.zeros((0, k), dtype=np.int64)
    cat = np.concatenate(symbols).astype(np.int64) if lengths.sum() else np.zeros(0, dtype=np.int64)
    rec = np.repeat(np.arange(len(symbols), dtype=np.int64), lengths)
    return np.bincount(rec * k + cat, minlength=len(symbols) * k).astype(np.int64).reshape(len(symbols), k)


def cut(sym, bounds):
    """The records [bounds[i], bounds[i + 1]) of one symbol array."""
    return [sym[a:b] for a, b in zip(bounds[:-1], bounds[1:])]


def check_set(pli, symbols, protein=False, cols=32, tiles=(None, 1, 3), wrap=0):
    k = 21 if protein else 5
    seqset = pli.stripe_set([lm.EncodedSequence(s, protein=protein) for s in symbols], columns=cols, protein=protein)
    if wrap:
        seqset.configure_wrap(wrap)
    want = host_table(symbols, k)
    for t in tiles:
        with tile_rows(pli, t):
            got = seqset.count_symbols()
        assert got.dtype == np.int64 and got.shape == want.shape, (t, got.shape)
        assert np.array_equal(got, want), (t, np.argwhere(got != want)[:5])
        assert np.array_equal(got.sum(axis=1), seqset.lengths) and int(got.sum()) == seqset.total_length
    return seqset


def test_reference_literal(pli):
    """seq.rs:573-598."""
    seq = pli.stripe(lm.EncodedSequence("ATGCAAGGAGATTCTAGAT"))
    assert seq.count_symbols().tolist() == [7, 2, 5, 5, 0]
    assert pli.last_kernel == "count_blocks"
    seq.configure_wrap(32)
    got = seq.count_symbols()
    assert got.dtype == np.int64 and got.tolist() == [7, 2, 5, 5, 0]
    assert [seq.count_symbol(s) for s in "ACTGN"] == [7, 2, 5, 5, 0]
    with pytest.raises(ValueError):
        seq.count_symbol("X")
    assert np.array_equal(bits(seq.background()), bits(background_from_counts([7, 2, 5, 5, 0])))


@pytest.mark.parametrize("cols", [1, 16, 32])
@pytest.mark.parametrize("protein", [False, True])
def test_geometry_of_a_single_sequence(pli, protein, cols):
    k = 21 if protein else 5
    rng = np.random.default_rng(100 * cols + protein)
    for length in (0, 1, 5, 31, 32, 33, 63, 64, 65, 1023, 1024, 1025, 4097, 100_003):
        sym = draw_symbols(rng, length, k)
        want = host_counts(sym, k)
        for wrap in (0, 7):
            seq = pli.stripe(lm.EncodedSequence(sym, protein=protein), cols)
            if wrap:
                seq.configure_wrap(wrap)
            assert seq.rows == -(-length // cols) and seq.wrap == wrap
            for t in (None, 1, 3, 64):
                with tile_rows(pli, t):
                    got = seq.count_symbols()
                assert np.array_equal(got, want), (length, wrap, t, got, want)
            assert int(got.sum()) == length


def test_sets_empty_records_and_single_records(pli):
    rng = np.random.default_rng(1)
    empty = np.zeros(0, dtype=np.uint8)
    assert check_set(pli, []).count_symbols().shape == (0, 5)                 # zero records
    assert check_set(pli, [], protein=True).count_symbols().shape == (0, 21)
    assert not check_set(pli, [empty]).count_symbols().any()                  # one empty record
    a, b, c = (draw_symbols(rng, n, 5) for n in (77, 1, 3000))
    check_set(pli, [empty, a, empty, empty, empty, b, c, empty])              # empty first, last and three in a row
    check_set(pli, [empty, empty, empty])
    check_set(pli, [b])                                                       # a record of length 1
    check_set(pli, [draw_symbols(rng, 70_001, 5)])                            # one record spanning the whole set
    check_set(pli, [draw_symbols(rng, 9_999, 21)], protein=True, wrap=5)


def test_sets_more_records_than_offsets_fit_in_lds(pli):
    rng = np.random.default_rng(2)
    for protein in (False, True):
        k = 21 if protein else 5
        lengths = rng.integers(0, 4, 4097)
        sym = draw_symbols(rng, int(lengths.sum()), k)
        check_set(pli, cut(sym, np.concatenate(([0], np.cumsum(lengths)))), protein=protein)


@pytest.mark.parametrize("rows", [96, 2100])
def test_sets_cut_on_and_beside_column_and_tile_boundaries(pli, rows):
    """A set of exactly 32 * R bases: column c starts at position c * R, block (c, t) at c * R + t * T.  R = 96 has tile
    boundaries for T = 1 and 3, R = 2 100 for the default T as well."""
    rng = np.random.default_rng(rows)
    total = 32 * rows
    sym = draw_symbols(rng, total, 5)
    columns = sorted({j * rows + d for j in (1, 2, 7, 16, 31) for d in (-1, 0, 1)})
    check_set(pli, cut(sym, [0] + columns + [total]))
    for t in (DEFAULT_TILE, 3, 1):
        if t >= rows:
            continue
        tiles = sorted({c * rows + i * t + d for c in (0, 5, 31) for i in (1, 2, rows // t) for d in (-1, 0, 1)} - {total + 1})
        tiles = [p for p in tiles if 0 <= p <= total]
        check_set(pli, cut(sym, [0] + tiles + [total]), tiles=(None, t))
    # both kinds together, with empty records on the boundaries themselves
    both = sorted(columns + columns + [c * rows + 3 * i for c in (3, 4) for i in range(1, 9)])
    check_set(pli, cut(sym, [0] + both + [total]), wrap=11)
    # records of 0 ... 3 bases throughout: a cut on and beside every boundary, through the prefix pass's lane-per-offset form
    # (the sets above, 64 bases per offset and more, take its wavefront-per-offset form)
    dense = np.minimum(np.cumsum(rng.integers(0, 4, total)), total)
    check_set(pli, cut(sym, [0] + dense[:int(np.searchsorted(dense, total))].tolist() + [total]), tiles=(None, 1, 3, 1000))


@pytest.mark.parametrize("block", range(4))
def test_the_three_builders_give_the_table_of_the_symbols(pli, block):
    for seed in range(SEED_BASE + 10 * block, SEED_BASE + 10 * block + 10):
        case = sr.draw_case(seed)
        want = host_table(case.symbols, case.k)
        sets = {
            "ascii": pli.stripe_ascii_set(case.texts, protein=case.protein, lossy=True, columns=case.cols),
            "encoded": pli.stripe_set([lm.EncodedSequence(s, protein=case.protein) for s in case.symbols], columns=case.cols,
                                      protein=case.protein),
            "fasta": pli.stripe_fasta_set(case.fasta, protein=case.protein, lossy=True, columns=case.cols),
        }
        for name, s in sets.items():
            if name != "ascii":
                s.configure_wrap(case.wrap)
            with tile_rows(pli, (None, 1, 3, 64)[seed % 4]):
                got = s.count_symbols()
            assert np.array_equal(got, want), (seed, name, case.cols, len(case.lengths))


def test_mid_size_set_with_one_long_record(pli):
    """About 20 Mbp: 30 000 records of skewed lengths and one of 5 Mbp in the middle; default tile, DNA, 32 columns."""
    rng = np.random.default_rng(3)
    lengths = np.minimum(rng.pareto(1.2, 30_000) * 150, 20_000).astype(np.int64)
    lengths[rng.random(30_000) < 0.01] = 0
    lengths = np.concatenate((lengths[:15_000], [5_000_000], lengths[15_000:]))
    total = int(lengths.sum())
    assert 12_000_000 < total < 30_000_000
    sym = draw_symbols(rng, total, 5)
    offsets = np.concatenate(([0], np.cumsum(lengths))).astype(np.uint64)
    text = np.frombuffer(b"ACTGN", dtype=np.uint8)[sym]
    seqset = pli.stripe_ascii_set(text, offsets=offsets)
    rec = np.repeat(np.arange(len(lengths), dtype=np.int64), lengths)
    want = np.bincount(rec * 5 + sym, minlength=len(lengths) * 5).astype(np.int64).reshape(-1, 5)
    got = seqset.count_symbols()
    assert np.array_equal(got, want)
    assert np.array_equal(got.sum(axis=0), np.bincount(sym, minlength=5)) and np.array_equal(got.sum(axis=1), lengths)
    seqset.configure_wrap(40)
    assert np.array_equal(seqset.count_symbols(), want)


def test_foreign_bytes_are_counted_nowhere(pli):
    """Cells holding a byte >= k.  ``Pipeline.upload`` refuses them among the live columns (LM_HIP_ERR_INVALID_SYMBOL), so
    they reach the kernel in the two ways they can: in the padding between ``cols`` and ``stride`` of an uploaded matrix,
    and anywhere in an adopted one."""
    rng = np.random.default_rng(4)
    # uploaded: 16 live columns of 32, the padding full of bytes that are no symbol
    rows, wrap, cols, length = 700, 3, 16, 700 * 16 - 5
    host = np.full((rows + wrap, 32), 0xEE, dtype=np.uint8)
    host[:, :cols] = draw_symbols(rng, (rows + wrap) * cols, 5).reshape(rows + wrap, cols)
    live = host[:rows, :cols].T.reshape(-1)[:length]
    seq = pli.upload(host, length, wrap, cols)
    for t in (None, 1, 64):
        with tile_rows(pli, t):
            assert np.array_equal(seq.count_symbols(), host_counts(live, 5)), t
    with pytest.raises(lm.InvalidSymbol):
        bad = host.copy()
        bad[5, 2] = 9
        pli.upload(bad, length, wrap, cols)
    # adopted: foreign bytes among the live cells, 5 ... 255
    for protein, k in ((False, 5), (True, 21)):
        rows, wrap, cols = 1500, 2, 32
        length = rows * cols - 17
        mat = draw_symbols(rng, (rows + wrap) * cols, k).reshape(rows + wrap, cols)
        foreign = rng.random(mat.shape) < 0.05
        mat[foreign] = rng.integers(k, 256, int(foreign.sum()))
        mat[3, 3], mat[rows - 1, 0] = 255, k
        dev = torch.from_numpy(mat.copy()).to(torch.device("cuda", 0))
        seq = pli.adopt_sequence(dev.data_ptr(), rows, wrap, cols, cols, length, protein=protein, keepalive=dev)
        live = mat[:rows].T.reshape(-1)[:length]
        want = host_counts(live[live < k], k)
        for t in (None, 1, 3):
            with tile_rows(pli, t):
                got = seq.count_symbols()
            assert np.array_equal(got, want), (protein, t)
        assert int(got.sum()) == int((live < k).sum()) < length


def test_calls_repeat_also_around_a_scan_that_shares_the_scratch(pli):
    rng = np.random.default_rng(6)
    lengths = rng.integers(0, 900, 500)
    sym = draw_symbols(rng, int(lengths.sum()), 5)
    symbols = cut(sym, np.concatenate(([0], np.cumsum(lengths))))
    seqset = check_set(pli, symbols, tiles=(None,))
    first = seqset.count_symbols()
    assert np.array_equal(first, seqset.count_symbols())
    weights = np.zeros((9, 5), dtype=np.float32)
    weights[:, :4] = rng.normal(0, 2, (9, 4))
    weights[:, 4] = -np.inf
    seqset.configure_wrap(8)
    hits = pli.scan_threshold_set([lm.ScoringMatrix(weights)], [2.0], seqset)
    assert hits.total > 0
    assert np.array_equal(first, seqset.count_symbols())
    single = pli.stripe(lm.EncodedSequence(sym))
    assert np.array_equal(single.count_symbols(), first.sum(axis=0))
    assert np.array_equal(first, seqset.count_symbols())


def test_misuse_is_a_status(pli):
    L = pli._L
    rng = np.random.default_rng(8)
    sym = draw_symbols(rng, 5000, 5)
    seq = pli.stripe(lm.EncodedSequence(sym))
    seqset = pli.stripe_set([lm.EncodedSequence(s) for s in cut(sym, [0, 10, 10, 4000, 5000])])
    mark = 0xABABABABABABABAB
    for call, handle, need in ((L.lm_hip_seq_count_symbols, seq._h, 5), (L.lm_hip_seqset_count_symbols, seqset._h, 20)):
        buf = np.full(need, mark, dtype=np.uint64)
        assert call(pli._h, handle, buf.ctypes.data, need - 1) == _ffi.ERR_CAPACITY and _ffi.last_error()
        assert (buf == mark).all()
        assert call(pli._h, handle, buf.ctypes.data, 0) == _ffi.ERR_CAPACITY and (buf == mark).all()
        assert call(pli._h, handle, None, need) == _ffi.ERR_BAD_ARGS and call(None, handle, buf.ctypes.data, need) == _ffi.ERR_BAD_ARGS
        assert call(pli._h, None, buf.ctypes.data, need) == _ffi.ERR_BAD_ARGS and (buf == mark).all()
        assert call(pli._h, handle, buf.ctypes.data, need) == _ffi.OK and int(buf.sum()) == 5000
    for bad in (-1, 65537, float("nan")):
        with pytest.raises(lm.LightmotifHipError):
            pli.set_option("count_tile_rows", bad)
    # a closed context
    other = lm.Pipeline.hip(0)
    theirs = other.stripe_set([lm.EncodedSequence(sym)])
    theirs_seq = other.stripe(lm.EncodedSequence(sym))
    assert theirs.count_symbols().tolist() == [host_counts(sym, 5).tolist()]
    other.close()
    for closed in (theirs, theirs_seq):
        with pytest.raises(lm.LightmotifHipError):
            closed.count_symbols()
    # a handle of another device's context
    ordinals = lm.Pipeline.device_ordinals()
    if len(ordinals) > 1:
        far = lm.Pipeline.hip(ordinals[1])
        far_set, far_seq = far.stripe_set([lm.EncodedSequence(sym)]), far.stripe(lm.EncodedSequence(sym))
        buf = np.full(5, mark, dtype=np.uint64)
        assert L.lm_hip_seqset_count_symbols(pli._h, far_set._h, buf.ctypes.data, 5) == _ffi.ERR_BAD_ARGS
        assert L.lm_hip_seq_count_symbols(pli._h, far_seq._h, buf.ctypes.data, 5) == _ffi.ERR_BAD_ARGS and (buf == mark).all()
        assert far_set.count_symbols().tolist() == [host_counts(sym, 5).tolist()]


def test_background_of_a_set_and_of_a_sequence(pli):
    rng = np.random.default_rng(9)
    for protein, k in ((False, 5), (True, 21)):
        lengths = rng.integers(0, 3000, 60)
        sym = draw_symbols(rng, int(lengths.sum()), k)
        symbols = cut(sym, np.concatenate(([0], np.cumsum(lengths))))
        seqset = pli.stripe_set([lm.EncodedSequence(s, protein=protein) for s in symbols], protein=protein)
        seq = pli.stripe(lm.EncodedSequence(sym, protein=protein))
        for unknown in (False, True):
            want = background_from_counts(host_table(symbols, k), unknown)
            assert np.array_equal(bits(seqset.background(unknown)), bits(want))
            assert np.array_equal(bits(seq.background(unknown)), bits(background_from_counts(host_counts(sym, k), unknown)))
            assert np.array_equal(bits(seq.background(unknown)), bits(want))
        assert seqset.background()[k - 1] == 0 and seqset.background(True)[k - 1] > 0
    with pytest.raises(ValueError):
        pli.stripe_set([lm.EncodedSequence("NNNN")]).background()
    with pytest.raises(ValueError):
        pli.stripe_set([]).background(True)
