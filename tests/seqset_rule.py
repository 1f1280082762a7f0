"""The rule of a scan over a sequence set, restated in numpy (no device): records laid end to end, a hit at position
``p`` of the concatenation with a motif of ``m`` rows belongs to the record that holds ``p`` and is kept only when its
whole window lies inside that record -- ``position + M <= L`` per RECORD (the reference's scan.rs:185-190).  64-bit
throughout: a concatenation may exceed 2^32 symbols."""
import numpy as np


def offsets_of(lengths):
    offs = np.zeros(len(lengths) + 1, dtype=np.uint64)
    np.cumsum(np.asarray(lengths, dtype=np.uint64), out=offs[1:])
    return offs


def segment_rule(offsets, positions, m):
    """-> (record, local position, keep) per position; the record of a position is the LAST one that starts at or
    before it (empty records own nothing); positions at or behind the end of the set belong to no record (record =
    number of records, keep False)."""
    offsets = np.asarray(offsets, dtype=np.uint64)
    positions = np.asarray(positions, dtype=np.uint64)
    n = len(offsets) - 1
    rec = np.searchsorted(offsets, positions, side="right").astype(np.int64) - 1
    inside = rec < n
    safe = np.minimum(rec, max(n - 1, 0))
    local = positions - offsets[safe]
    keep = inside & (positions + np.uint64(m) <= offsets[safe + 1]) if n else np.zeros(len(positions), dtype=bool)
    return rec, local.astype(np.int64), keep
