"""Host side of the sequence-set path (no device): the C ABI's argument checks, the CLI's record batching and the
position -> (record, local position, keep?) rule that the GPU tests use as their expectation."""
import ctypes as C

import numpy as np
import pytest

from lightmotif_amd import _ffi, scan_cli
from seqset_rule import offsets_of, segment_rule


def _from_ascii(text, offsets, total=None, cols=32):
    L = _ffi.lib()
    offs = np.asarray(offsets, dtype=np.uint64)
    buf = np.frombuffer(text, dtype=np.uint8) if text is not None else None
    h = C.c_void_p()
    st = L.lm_hip_seqset_from_ascii(None, b"D", buf.ctypes.data if buf is not None and buf.size else None,
                                    len(text) if total is None else total, offs.ctypes.data, len(offs) - 1, cols, 1, C.byref(h),
                                    None, None)
    return st, _ffi.last_error()


def test_offsets_are_validated_before_any_device_work():
    st, msg = _from_ascii(b"ACGTACGT", [0, 5, 3, 8])
    assert st == _ffi.ERR_BAD_ARGS and "decrease" in msg and "record 1" in msg
    st, msg = _from_ascii(b"ACGTACGT", [1, 4, 8])
    assert st == _ffi.ERR_BAD_ARGS and "offsets[0]" in msg
    st, msg = _from_ascii(None, [0, 4, 8], total=8)
    assert st == _ffi.ERR_BAD_ARGS and "null data" in msg
    st, msg = _from_ascii(b"ACGTACGT", [0, 4, 7])
    assert st == _ffi.ERR_BAD_ARGS and "end at 7" in msg
    st, msg = _from_ascii(b"ACGTACGT", [0, 4, 8], cols=0)
    assert st == _ffi.ERR_BAD_ARGS and msg
    # well-formed offsets get as far as the (missing) context
    st, msg = _from_ascii(b"ACGTACGT", [0, 0, 4, 4, 8])
    assert st == _ffi.ERR_BAD_ARGS and "null argument" in msg


def test_a_set_beyond_the_key_space_is_a_capacity_status():
    """hits.hip addresses 2^40 cells per job: a longer concatenation is refused when the set is made, not when it is scanned.
    (Nothing is read: the checks come before the first byte of the text is touched.)"""
    L = _ffi.lib()
    total = (1 << 40) + 1
    offs = np.asarray([0, total], dtype=np.uint64)
    dummy = np.zeros(1, dtype=np.uint8)
    h = C.c_void_p()
    st = L.lm_hip_seqset_from_encoded(None, dummy.ctypes.data, total, offs.ctypes.data, 1, 32, 5, C.byref(h))
    assert st == _ffi.ERR_CAPACITY and "2^40" in _ffi.last_error()
    st = L.lm_hip_seqset_from_encoded(None, dummy.ctypes.data, 1 << 40, np.asarray([0, 1 << 40], dtype=np.uint64).ctypes.data, 1, 32, 5,
                                      C.byref(h))
    assert st == _ffi.ERR_BAD_ARGS   # fits: the next thing missing is the context


def test_null_set_handles_are_statuses():
    L = _ffi.lib()
    n = C.c_size_t(0)
    assert L.lm_hip_seqset_info(None, C.byref(n), None, None, None, None, None) == _ffi.ERR_BAD_ARGS and _ffi.last_error()
    assert L.lm_hip_seqset_record_length(None, 0, C.byref(n)) == _ffi.ERR_BAD_ARGS
    assert L.lm_hip_seqset_configure_wrap(None, None, 4) == _ffi.ERR_BAD_ARGS
    assert L.lm_hip_seqset_destroy(None) == _ffi.OK
    hits = C.POINTER(_ffi.SetHit)()
    assert L.lm_hip_scan_threshold_seqset(None, None, None, 0, None, None, C.byref(hits)) == _ffi.ERR_BAD_ARGS


BATCH_CASES = [
    # lengths, budget, expected sets [first, end)
    ([], 10, []),
    ([3, 4, 3], 10, [(0, 3)]),                                   # exact fit
    ([3, 4, 3, 1], 10, [(0, 3), (3, 4)]),                        # one base too many
    ([5, 50, 5], 10, [(0, 1), (1, 2), (2, 3)]),                  # an oversized record stands alone
    ([50], 10, [(0, 1)]),
    ([0, 0, 50, 0, 2], 10, [(0, 3), (3, 5)]),                    # empty records in front of it ride along
    ([0, 0, 0], 10, [(0, 3)]),                                   # only empty records: one set
    ([4, 0, 0, 6, 0, 1], 10, [(0, 5), (5, 6)]),                  # empty records never close a set
    ([1, 1, 0, 1], 1, [(0, 1), (1, 3), (3, 4)]),                 # budget of 1
    ([2, 1], 1, [(0, 1), (1, 2)]),
    ([10, 10, 10], 10, [(0, 1), (1, 2), (2, 3)]),
]


@pytest.mark.parametrize("lengths,budget,want", BATCH_CASES)
def test_record_batching(lengths, budget, want):
    got = scan_cli.batch_records(lengths, budget)
    assert got == want
    # every record in exactly one set, in order; no set over the budget unless it holds one non-empty record
    assert [i for a, b in got for i in range(a, b)] == list(range(len(lengths)))
    for a, b in got:
        bases = sum(lengths[a:b])
        assert bases <= budget or sum(1 for n in lengths[a:b] if n) == 1


def test_record_batching_refuses_a_budget_of_zero():
    with pytest.raises(ValueError):
        scan_cli.batch_records([1, 2], 0)


def test_segment_rule_small():
    # records: [0,5) [5,5) [5,9) [9,10): lengths 5, 0, 4, 1
    offs = offsets_of([5, 0, 4, 1])
    assert offs.tolist() == [0, 5, 5, 9, 10]
    pos = np.arange(12)
    rec, local, keep = segment_rule(offs, pos, 3)
    assert rec.tolist() == [0, 0, 0, 0, 0, 2, 2, 2, 2, 3, 4, 4]
    assert local[:10].tolist() == [0, 1, 2, 3, 4, 0, 1, 2, 3, 0]
    #                   record 0: windows at 0..2 fit | record 2 (length 4): 0, 1 fit | record 3 (length 1): none
    assert keep.tolist() == [True, True, True, False, False, True, True, False, False, False, False, False]
    rec, local, keep = segment_rule(offs, pos, 1)
    assert keep.tolist() == [True] * 10 + [False, False]
    rec, local, keep = segment_rule(offs, pos, 6)          # longer than every record
    assert not keep.any()


def test_segment_rule_is_64_bit():
    big = (1 << 32) + 12_345
    offs = offsets_of([big, 7, 0, (1 << 33) + 1, 20])
    assert offs.dtype == np.uint64 and int(offs[-1]) == big + 7 + (1 << 33) + 1 + 20
    m = 8
    pos = np.asarray([0, big - m, big - m + 1, big, big + 6, big + 7, big + 7 + (1 << 33) + 1 - m, big + 7 + (1 << 33) + 1,
                      int(offs[-1]) - m, int(offs[-1]) - m + 1, int(offs[-1]), int(offs[-1]) + 31], dtype=np.uint64)
    rec, local, keep = segment_rule(offs, pos, m)
    assert rec.tolist() == [0, 0, 0, 1, 1, 3, 3, 4, 4, 4, 5, 5]
    assert local[:10].tolist() == [0, big - m, big - m + 1, 0, 6, 0, (1 << 33) + 1 - m, 0, 20 - m, 20 - m + 1]
    assert keep.tolist() == [True, True, False, False, False, True, True, True, True, False, False, False]
    # the same rule, one position at a time in Python integers
    for p, r, l, k in zip(pos.tolist(), rec.tolist(), local.tolist(), keep.tolist()):
        o = [int(x) for x in offs]
        want_r = max(i for i in range(len(o)) if o[i] <= p)
        assert r == want_r
        if want_r < len(o) - 1:
            assert l == p - o[want_r] and k == (p + m <= o[want_r + 1])
        else:
            assert not k
