"""Hit windows read back out of a resident set: ``StripedSequenceSet.windows`` / ``count_sites`` / ``record`` / ``records``
(``lm_hip_seqset_windows`` / ``lm_hip_seqset_count_sites``, csrc/sites.hip).  The oracle is numpy slicing of the host's
per-record symbol arrays; every comparison is exact.  The option ``site_chunk`` makes small site lists cross chunk
boundaries."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import lightmotif_amd as lm
from lightmotif_amd import _ffi
from lightmotif_amd.lib import decode

import seqset_reference as sr
from fasta_cases import PLAIN, parse

pytestmark = pytest.mark.gpu

SEEDS = range(0, 40)        # of seqset_reference.draw_case
SITE_SEED_BASE = 8_800      # of this file's own generator
CHUNKS = (0, 1, 7)
STRIDES = (16, 24, 40)
LDS_COUNTERS = 12288        # kLdsCounters of csrc/sites_plan.hpp


@contextlib.contextmanager
def site_chunk(pli, sites):
    pli.set_option("site_chunk", sites)
    try:
        yield
    finally:
        pli.set_option("site_chunk", 0)


def make_set(pli, symbols, protein=False, cols=32, wrap=0):
    seqset = pli.stripe_set([lm.EncodedSequence(np.asarray(s, dtype=np.uint8), protein=protein) for s in symbols], columns=cols,
                            protein=protein)
    if wrap:
        seqset.configure_wrap(wrap)
    return seqset


def dna(text):
    return sr.encode_text(text.encode(), False, lossy=False)


# ---- the oracle ------------------------------------------------------------------------------------------------------

def want_windows(symbols, rec, pos, width, shift):
    """(count, width) bytes and valid flags of one motif's sites, by slicing; Python ints, so nothing wraps."""
    out = np.full((len(rec), width), 0xFF, dtype=np.uint8)
    valid = np.zeros(len(rec), dtype=bool)
    for i, (r, p) in enumerate(zip(rec, pos)):
        r, start = int(r), int(p) + int(shift)
        if r < len(symbols) and start >= 0 and start + width <= len(symbols[r]):
            out[i] = symbols[r][start:start + width]
            valid[i] = True
    return out, valid


def want_table(win, valid, k):
    width = win.shape[1]
    table = np.zeros((width, k), dtype=np.int64)
    rows = win[valid].astype(np.int64)
    np.add.at(table, (np.tile(np.arange(width), len(rows)), rows.reshape(-1)), 1)
    return table


def want_all(symbols, k, sites, widths, shifts):
    wins = [want_windows(symbols, r, p, w, s) for (r, p), w, s in zip(sites, widths, shifts)]
    return wins, [want_table(w, v, k) for w, v in wins], np.array([int(v.sum()) for _, v in wins], dtype=np.int64)


# ---- the C ABI with any stride ---------------------------------------------------------------------------------------

def pack_sites(sites, stride):
    """The sites of all motifs ``stride`` bytes apart: record at +0, position at +8, 0xEE everywhere else."""
    total = sum(len(r) for r, _ in sites)
    raw = np.full((max(total, 1), stride), 0xEE, dtype=np.uint8)
    if total:
        raw[:total, 0:8] = np.concatenate([np.asarray(r, dtype=np.uint64) for r, _ in sites]).view(np.uint8).reshape(-1, 8)
        raw[:total, 8:16] = np.concatenate([np.asarray(p, dtype=np.uint64) for _, p in sites]).view(np.uint8).reshape(-1, 8)
    return raw


def abi_call(pli, seqset, name, sites, widths, shifts, stride, out, extra):
    counts = np.array([len(r) for r, _ in sites], dtype=np.uintp)
    w = np.asarray(widths, dtype=np.uintp)
    sh = np.asarray(shifts, dtype=np.int64)
    raw = pack_sites(sites, stride)
    return getattr(_ffi.lib(), name)(pli._h, seqset._h, counts.ctypes.data, w.ctypes.data, sh.ctypes.data, len(counts), raw.ctypes.data,
                                     stride, out.ctypes.data, out.size, extra.ctypes.data)


def abi_windows(pli, seqset, sites, widths, shifts, stride):
    counts = [len(r) for r, _ in sites]
    out = np.full(max(sum(c * w for c, w in zip(counts, widths)), 1), 0xAB, dtype=np.uint8)
    valid = np.full(max(sum(counts), 1), 0xAB, dtype=np.uint8)
    _ffi.check(abi_call(pli, seqset, "lm_hip_seqset_windows", sites, widths, shifts, stride, out, valid))
    res, a, b = [], 0, 0
    for c, w in zip(counts, widths):
        res.append((out[a:a + c * w].reshape(c, w), valid[b:b + c]))
        a, b = a + c * w, b + c
    return res


def abi_counts(pli, seqset, k, sites, widths, shifts, stride):
    tables = np.full(max(k * sum(widths), 1), 0xABABABAB, dtype=np.uint64)
    used = np.full(max(len(widths), 1), 0xABABABAB, dtype=np.uint64)
    _ffi.check(abi_call(pli, seqset, "lm_hip_seqset_count_sites", sites, widths, shifts, stride, tables, used))
    res, a = [], 0
    for w in widths:
        res.append(tables[a:a + w * k].reshape(w, k).astype(np.int64))
        a += w * k
    return res, used[:len(widths)].astype(np.int64)


def check_against(pli, seqset, symbols, k, sites, widths, shifts, stride, tag):
    wins, tables, used = want_all(symbols, k, sites, widths, shifts)
    got = abi_windows(pli, seqset, sites, widths, shifts, stride)
    for i, ((gw, gv), (ww, wv)) in enumerate(zip(got, wins)):
        assert gv.dtype == np.uint8 and set(np.unique(gv).tolist()) <= {0, 1}, (tag, i)
        assert np.array_equal(gv != 0, wv), (tag, i, "valid", np.flatnonzero((gv != 0) != wv)[:5])
        assert np.array_equal(gw, ww), (tag, i, "bytes", np.argwhere(gw != ww)[:5])
    got_tables, got_used = abi_counts(pli, seqset, k, sites, widths, shifts, stride)
    assert np.array_equal(got_used, used), (tag, "used", got_used, used)
    for i, (g, w) in enumerate(zip(got_tables, tables)):
        assert np.array_equal(g, w), (tag, i, "table", np.argwhere(g != w)[:5])
        assert (g.sum(axis=1) == got_used[i]).all(), (tag, i, "row sums")


def u64(values):
    return np.array([int(v) % (1 << 64) for v in values], dtype=np.uint64)


# ---- 1. literal ------------------------------------------------------------------------------------------------------

def test_literal(pli):
    records = ["ATGCAAGG", "", "TTACG"]
    seqset = make_set(pli, [dna(t) for t in records])
    # ACTGN = 0 1 2 3 4
    sites = [([0, 0, 0, 1, 3, 2], [0, 5, 6, 0, 0, 2])]
    (win, valid), = seqset.windows(sites, [3])
    assert pli.last_kernel == "site_windows"
    assert win.dtype == np.uint8 and win.shape == (6, 3) and valid.dtype == np.bool_
    assert valid.tolist() == [True, True, False, False, False, True]
    assert win.tolist() == [[0, 2, 3],            # ATG: the start of record 0
                            [0, 3, 3],            # AGG: its end
                            [255, 255, 255],      # one past the end
                            [255, 255, 255],      # the empty record
                            [255, 255, 255],      # record 3 does not exist
                            [0, 1, 3]]            # ACG: the end of record 2
    assert [decode(w) for w in win[valid]] == ["ATG", "AGG", "ACG"]
    with pytest.raises(ValueError):
        decode(win[2])
    (mat,), used = seqset.count_sites(sites, [3])
    assert pli.last_kernel == "site_counts_lds"
    assert used.tolist() == [3] and isinstance(mat, lm.CountMatrix)
    assert mat.data.tolist() == [[3, 0, 0, 0, 0], [0, 1, 1, 1, 0], [0, 0, 0, 3, 0]]
    seqs = [lm.EncodedSequence(t) for t in ("ATG", "AGG", "ACG")]
    assert mat == lm.CountMatrix.from_sequences(seqs)
    # a shift moves the window, not the site: TGC GG? CG?
    (win, valid), = seqset.windows(sites, [3], shifts=1)
    assert valid.tolist() == [True, False, False, False, False, False] and win[0].tolist() == [2, 3, 1]
    (win, valid), = seqset.windows(sites, [3], shifts=[-2])
    assert valid.tolist() == [False, True, True, False, False, True]
    assert [decode(w) for w in win[valid]] == ["CAA", "AAG", "TTA"]
    assert [str(r) for r in seqset.records()] == records and str(seqset.record(2)) == "TTACG" and str(seqset.record(-2)) == ""
    with pytest.raises(IndexError):
        seqset.record(3)


# ---- 2. differential -------------------------------------------------------------------------------------------------

_SEEN = {}


def draw_sites(rng, case, n_motifs):
    n_records = len(case.lengths)
    empty = int(rng.integers(1, n_motifs - 1))              # a motif between two others without a site
    sites, widths, shifts = [], [], []
    for i in range(n_motifs):
        count = 0 if i == empty else int(rng.integers(0, 301))
        width = int(rng.choice([1, 2, 3, 8, 12, 31, 33, 64, 200]))
        shift = int(rng.integers(-3, 4))
        rec = rng.integers(0, n_records + 2, count)            # records and records + 1 do not exist
        lengths = np.where(rec < n_records, case.lengths[np.minimum(rec, max(n_records - 1, 0))] if n_records else 0, 0)
        pos = rng.integers(-4, 5, count) + (rng.random(count) * (lengths - width + 1)).astype(np.int64) * (rng.random(count) < 0.9)
        sites.append((u64(rec), u64(pos)))
        widths.append(width)
        shifts.append(shift)
    return sites, widths, shifts, empty


def run_seed(pli, seed):
    case = sr.draw_case(seed)
    rng = np.random.default_rng(SITE_SEED_BASE + seed)
    seqset = make_set(pli, case.symbols, case.protein, case.cols, case.wrap)
    sites, widths, shifts, empty = draw_sites(rng, case, int(rng.integers(3, 7)))
    assert len(sites[empty][0]) == 0 and 0 < empty < len(sites) - 1
    stride = STRIDES[seed % 3]
    for chunk in CHUNKS:
        with site_chunk(pli, chunk):
            check_against(pli, seqset, case.symbols, case.k, sites, widths, shifts, stride, (seed, chunk, stride))
    if stride == 16:       # the same through the Python mirror, whose pairs are packed 16 bytes apart
        wins, tables, used = want_all(case.symbols, case.k, sites, widths, shifts)
        got = seqset.windows(sites, widths, shifts)
        assert all(np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1]) for g, w in zip(got, wins)), seed
        mats, got_used = seqset.count_sites(sites, widths, shifts)
        assert np.array_equal(got_used, used) and all(np.array_equal(m.data, t) for m, t in zip(mats, tables)), seed
    _SEEN[seed] = (case.protein, case.cols, case.wrap, len(case.lengths), int(sum(v.sum() for _, v in want_all(
        case.symbols, case.k, sites, widths, shifts)[0])))
    return _SEEN[seed]


@pytest.mark.parametrize("seed", SEEDS)
def test_differential(pli, seed):
    run_seed(pli, seed)


def test_the_seeds_reach_what_they_must(pli):
    """DNA and protein, three column counts and more, wrap values, no record at all and 4 097 of them (seeds this run has
    not been through yet are run here)."""
    seen = [_SEEN[s] if s in _SEEN else run_seed(pli, s) for s in SEEDS]
    assert any(p for p, *_ in seen) and any(not p for p, *_ in seen)
    assert {c for _, c, *_ in seen} >= {32} and len({c for _, c, *_ in seen}) >= 3
    assert len({w for _, _, w, *_ in seen}) >= 5
    assert any(r == 4097 for *_, r, _ in seen) and any(r == 0 for *_, r, _ in seen)
    assert sum(v > 0 for *_, v in seen) >= len(seen) // 2


# ---- 3. geometry -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cols", [32, 3])
def test_a_window_over_the_bottom_of_a_column(pli, cols):
    rng = np.random.default_rng(SITE_SEED_BASE + 100 + cols)
    symbols = [rng.integers(0, 4, n).astype(np.uint8) for n in (17, 1000, 5)]
    seqset = make_set(pli, symbols, cols=cols)
    rows = seqset.rows
    assert rows == -(-1022 // cols)
    # positions of the concatenation rows - 3 ... : the last rows of column 0 and the first of column 1; record 1 starts at 17
    starts = [c * rows - 3 - 17 for c in range(1, min(cols, 4)) if c * rows - 3 - 17 >= 0 and c * rows + 10 - 17 <= 1000]
    assert starts
    sites = [([1] * len(starts), starts), ([1], [0])]
    widths = [10, 1000]
    wins, tables, used = want_all(symbols, 5, sites, widths, [0, 0])
    assert all(v.all() for _, v in wins)
    before = seqset.windows(sites, widths), seqset.count_sites(sites, widths)
    assert seqset.wrap == 0
    seqset.configure_wrap(40)
    assert seqset.wrap == 40
    after = seqset.windows(sites, widths), seqset.count_sites(sites, widths)
    for (got_w, (got_m, got_u)) in (before, after):
        assert all(np.array_equal(g[0], w[0]) and g[1].all() for g, w in zip(got_w, wins))
        assert all(np.array_equal(m.data, t) for m, t in zip(got_m, tables)) and np.array_equal(got_u, used)


# ---- 4. widths -------------------------------------------------------------------------------------------------------

def test_widths(pli):
    rng = np.random.default_rng(SITE_SEED_BASE + 200)
    symbols = [rng.integers(0, 5, n).astype(np.uint8) for n in (90, 0, 71, 70, 36, 1)]
    seqset = make_set(pli, symbols)
    sites, widths = [], [1, 2, 36, 70, 91]
    for w in widths:
        rec = rng.integers(0, len(symbols), 150)
        pos = np.array([rng.integers(0, max(len(symbols[r]) - w, 0) + 2) for r in rec])
        sites.append((u64(rec), u64(pos)))
    for chunk in (0, 40):
        with site_chunk(pli, chunk):
            check_against(pli, seqset, symbols, 5, sites, widths, [0] * len(widths), 16, ("widths", chunk))
    assert pli.last_kernel == "site_counts_lds"
    (win, valid), = seqset.windows(sites[-1:], [91])             # longer than every record: nothing is valid
    assert not valid.any() and (win == 0xFF).all()
    (mat,), used = seqset.count_sites(sites[-1:], [91])
    assert used.tolist() == [0] and mat.data.shape == (91, 5) and not mat.data.any()
    (mat,), used = seqset.count_sites(sites[-1:], [5000])            # ... and longer than the whole set
    assert used.tolist() == [0] and mat.data.shape == (5000, 5) and not mat.data.any()


def test_a_table_beyond_lds_takes_the_direct_route(pli):
    rng = np.random.default_rng(SITE_SEED_BASE + 201)
    width, k = 3000, 21
    assert width * k + 1 > LDS_COUNTERS
    symbols = [rng.integers(0, k, n).astype(np.uint8) for n in (3000, 3300, 10, 3001)]
    seqset = make_set(pli, symbols, protein=True)
    rec = rng.integers(0, 4, 40)
    pos = rng.integers(0, 3, 40)
    sites = [(u64(rec), u64(pos)), (u64([1, 3, 2]), u64([7, 0, 0]))]
    wins, tables, used = want_all(symbols, k, sites, [width, 9], [0, 0])
    assert 0 < used[0] < 40
    mats, got_used = seqset.count_sites(sites[:1], [width])
    assert pli.last_kernel == "site_counts_direct"
    assert np.array_equal(got_used, used[:1]) and np.array_equal(mats[0].data, tables[0])
    # both routes in one call: the narrow motif behind the wide one runs last
    mats, got_used = seqset.count_sites(sites, [width, 9])
    assert pli.last_kernel == "site_counts_lds"
    assert np.array_equal(got_used, used) and all(np.array_equal(m.data, t) for m, t in zip(mats, tables))
    mats, got_used = seqset.count_sites(sites[::-1], [9, width])
    assert pli.last_kernel == "site_counts_direct"
    assert np.array_equal(got_used, used[::-1]) and all(np.array_equal(m.data, t) for m, t in zip(mats, tables[::-1]))


# ---- 5. contention ---------------------------------------------------------------------------------------------------

def test_many_copies_of_one_site(pli):
    symbols = [dna("ACGTTGCAACGT"), dna("TTGACA")]
    seqset = make_set(pli, symbols)
    n = 20_000
    sites = [(np.full(n, 1, np.uint64), np.full(n, 0, np.uint64)), (np.full(n, 0, np.uint64), np.full(n, 2, np.uint64))]
    mats, used = seqset.count_sites(sites, [6, 8])
    assert used.tolist() == [n, n]
    for mat, text in zip(mats, ("TTGACA", "GTTGCAAC")):
        want = np.zeros((len(text), 5), dtype=np.int64)
        want[np.arange(len(text)), dna(text)] = n
        assert np.array_equal(mat.data, want)


# ---- 6. overflow -----------------------------------------------------------------------------------------------------

def test_positions_and_shifts_that_would_wrap(pli):
    symbols = [dna("ACGTACGTAC"), dna("TTTT")]
    seqset = make_set(pli, symbols)
    big = [2 ** 63, 2 ** 64 - 1, 2 ** 63 - 1, 2 ** 64 - 3, 0, 5]
    sites = [([0] * len(big), big)]
    for shift, ok in ((0, [0, 0, 0, 0, 1, 1]), (3, [0, 0, 0, 0, 1, 0]), (-2 ** 62, [0] * 6), (2 ** 63 - 1, [0] * 6), (-2 ** 63, [1, 0, 0, 0, 0, 0]),
                      (-5, [0, 0, 0, 0, 0, 1]), (6, [0, 0, 0, 0, 1, 0])):
        (win, valid), = seqset.windows(sites, [4], shifts=[shift])
        assert valid.tolist() == [bool(x) for x in ok], shift
        want, want_valid = want_windows(symbols, [0] * len(big), big, 4, shift)
        assert np.array_equal(win, want) and np.array_equal(valid, want_valid), shift
        (mat,), used = seqset.count_sites(sites, [4], shifts=[shift])
        assert used.tolist() == [sum(ok)] and np.array_equal(mat.data, want_table(want, want_valid, 5)), shift
    # a position that wraps to a valid one with the shift: 2^64 - 2 + 3 = 1 (mod 2^64) is still no window
    (win, valid), = seqset.windows([([0], [2 ** 64 - 2])], [4], shifts=[3])
    assert not valid.any() and (win == 0xFF).all()
    # record numbers are 64-bit as well
    (win, valid), = seqset.windows([([2 ** 32, 2 ** 63, 2 ** 64 - 1, 1], [0, 0, 0, 0])], [4])
    assert valid.tolist() == [False, False, False, True]


# ---- 7. repeatability ------------------------------------------------------------------------------------------------

def test_two_calls_give_the_same_bytes(pli):
    case = sr.draw_case(9)
    rng = np.random.default_rng(SITE_SEED_BASE + 300)
    seqset = make_set(pli, case.symbols, case.protein, case.cols, case.wrap)
    sites, widths, shifts, _ = draw_sites(rng, case, 5)
    runs = []
    for _ in range(2):
        wins = abi_windows(pli, seqset, sites, widths, shifts, 16)
        tables, used = abi_counts(pli, seqset, case.k, sites, widths, shifts, 16)
        runs.append(b"".join(w.tobytes() + v.tobytes() for w, v in wins) + b"".join(t.tobytes() for t in tables) + used.tobytes())
    assert runs[0] == runs[1] and len(runs[0]) > 0


# ---- 8. arguments ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["lm_hip_seqset_windows", "lm_hip_seqset_count_sites"])
def test_misuse_is_a_status(pli, name):
    L = _ffi.lib()
    seqset = make_set(pli, [dna("ACGTACGT"), dna("TT")])
    windows = name.endswith("windows")
    counts = np.array([2, 1], dtype=np.uintp)
    widths = np.array([3, 2], dtype=np.uintp)
    zero_width = np.array([3, 0], dtype=np.uintp)
    shifts = np.zeros(2, dtype=np.int64)
    sites = np.array([[0, 0], [0, 4], [1, 0]], dtype=np.uint64)
    need = 8 if windows else 25
    out = np.full(64, 0xAB, dtype=np.uint8 if windows else np.uint64)
    extra = np.full(8, 0xAB, dtype=np.uint8 if windows else np.uint64)
    fn = getattr(L, name)

    def call(ctx=pli._h, handle=seqset._h, c=counts.ctypes.data, w=widths.ctypes.data, s=shifts.ctypes.data, n=2, p=sites.ctypes.data,
             stride=16, o=out.ctypes.data, capacity=need, e=extra.ctypes.data):
        return fn(ctx, handle, c, w, s, n, p, stride, o, capacity, e)

    mark = pli.last_kernel
    for bad in (dict(ctx=None), dict(handle=None), dict(c=None), dict(w=None), dict(p=None), dict(o=None), dict(w=zero_width.ctypes.data),
                dict(stride=8), dict(stride=15), dict(stride=0)):
        assert call(**bad) == _ffi.ERR_BAD_ARGS and _ffi.last_error(), bad
        assert (out == out[0]).all() and (extra == extra[0]).all() and int(out[0]) & 0xFF == 0xAB, bad
    for capacity in (0, need - 1):
        assert call(capacity=capacity) == _ffi.ERR_CAPACITY and _ffi.last_error()
        assert (out == out[0]).all() and (extra == extra[0]).all() and int(out[0]) & 0xFF == 0xAB
    assert pli.last_kernel == mark                       # nothing ran
    assert call(n=0) == _ffi.OK and call(n=0, c=None, w=None, s=None, p=None, o=None, e=None, capacity=0) == _ffi.OK
    assert (out == out[0]).all() and (extra == extra[0]).all()
    # no sites at all: OK, the tables zero-filled, nothing launched
    none = np.zeros(2, dtype=np.uintp)
    assert call(c=none.ctypes.data, capacity=0 if windows else need) == _ffi.OK and pli.last_kernel == mark
    if windows:
        assert (out == 0xAB).all()
    else:
        assert not out[:need].any() and (out[need:] == out[-1]).all() and not extra[:2].any() and (extra[2:] == extra[-1]).all()
    # NULL shifts are zeros, NULL valid / used is allowed; exact capacity suffices
    out[:] = out[-1]
    assert call(s=None, e=None) == _ffi.OK
    if windows:
        assert out[:need].tolist() == [0, 1, 3, 0, 1, 3, 2, 2] and (out[need:] == 0xAB).all()
    else:
        assert out[:need].reshape(5, 5).tolist() == [[2, 0, 0, 0, 0], [0, 2, 0, 0, 0], [0, 0, 0, 2, 0], [0, 0, 1, 0, 0], [0, 0, 1, 0, 0]]
    for bad in (-1.0, 2.0 ** 33, float("nan")):
        with pytest.raises(lm.LightmotifHipError):
            pli.set_option("site_chunk", bad)


def test_the_mirror_rejects_what_cannot_be_a_site_list(pli):
    seqset = make_set(pli, [dna("ACGT")])
    with pytest.raises(ValueError):
        seqset.windows([([0], [0])], [2, 2])
    with pytest.raises(ValueError):
        seqset.count_sites([([0], [0, 1])], [2])
    with pytest.raises(ValueError):
        seqset.windows([([0], [0])], [0])
    assert seqset.windows([], []) == [] and seqset.count_sites([], [])[0] == []


def test_counts_beyond_u32_overflow_a_count_matrix(pli, monkeypatch):
    """The table is u64; ``CountMatrix`` is u32 (pwm/mod.rs:178): the mirror refuses to truncate."""
    seqset = make_set(pli, [dna("ACGT")])
    real = seqset._pli._L.lm_hip_seqset_count_sites

    class Patched:
        def __getattr__(self, name):
            return getattr(_ffi.lib(), name)

        @staticmethod
        def lm_hip_seqset_count_sites(*args):
            status = real(*args)
            C.cast(C.c_void_p(args[8]), C.POINTER(C.c_uint64))[0] = 2 ** 32
            return status

    monkeypatch.setattr(seqset._pli, "_L", Patched())
    with pytest.raises(OverflowError):
        seqset.count_sites([([0], [0])], [2])


# ---- 9. tie to the scans ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", [0, 8, 10, 12])
def test_windows_of_hits_score_as_the_hits(pli, seed):
    case = sr.draw_case(seed)
    sr.reference(case)                                      # fills the thresholds
    if case.has_nan:
        pytest.fail("pick a seed without NaN weights")
    seqset = make_set(pli, case.symbols, case.protein, case.cols, case.wrap)
    pssms = [lm.ScoringMatrix(p, protein=case.protein) for p in case.mats]
    thresholds = [t if np.isfinite(t) else 0.0 for t in case.thresholds]
    hits = pli.scan_threshold_set(pssms, thresholds, seqset)
    assert hits.total > 0
    got = seqset.windows(hits, pssms)                       # the lm_hip_set_hit list as it is: a stride of 24
    mats, used = seqset.count_sites(hits, pssms)
    for i, (p, (win, valid)) in enumerate(zip(case.mats, got)):
        rec, pos, score = hits[i]
        assert valid.all() and win.shape == (len(rec), p.shape[0])
        mine = sr.window_scores(p, win.reshape(-1))[::p.shape[0]]      # the windows end to end: every M-th score is a row's
        assert np.array_equal(mine.view(np.uint32), np.ascontiguousarray(score).view(np.uint32)), (seed, i)
        assert all(np.array_equal(w, case.symbols[r][q:q + p.shape[0]]) for w, r, q in zip(win[:50], rec[:50], pos[:50]))
        assert used[i] == len(rec) and np.array_equal(mats[i].data, want_table(win, valid, case.k))


# ---- 10. records -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(PLAIN))
def test_records_of_a_fasta_set_equal_the_host_parse(pli, name):
    seqset = pli.stripe_fasta_set(PLAIN[name], lossy=True)
    _, texts = parse(PLAIN[name])
    want = [sr.encode_text(t, False) for t in texts]
    got = seqset.records()
    assert len(got) == len(want)
    for r, (g, w) in enumerate(zip(got, want)):
        assert isinstance(g, lm.EncodedSequence) and np.array_equal(g.data, w), (name, r)
        assert np.array_equal(seqset.record(r).data, w), (name, r)


def test_a_long_record_reads_back(pli):
    rng = np.random.default_rng(SITE_SEED_BASE + 400)
    symbols = [rng.integers(0, 5, n).astype(np.uint8) for n in (11, 3_000_003, 0, 77)]
    seqset = make_set(pli, symbols)
    assert np.array_equal(seqset.record(1).data, symbols[1])
    with site_chunk(pli, 2):
        got = seqset.records()
    assert all(np.array_equal(g.data, w) for g, w in zip(got, symbols))
