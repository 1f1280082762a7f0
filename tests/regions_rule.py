"""The rule of a derived set (``lm_hip_seqset_from_regions``), restated in numpy on host copies of the records (no
device): region ``[start, end)`` of a record is clipped to it, ``s = max(start, 0)``, ``e = min(end, L)``, and read as
``rec[s:e]`` or, on the minus strand, as the complement of ``rec[s:e]`` reversed (abc.rs:174-185 on symbol bytes:
0 <-> 2, 1 <-> 3, everything else itself).  Python ints throughout, so nothing wraps."""
import numpy as np

COMPLEMENT = np.arange(256, dtype=np.uint8)
COMPLEMENT[[0, 1, 2, 3]] = [2, 3, 0, 1]


def clip(start, end, length):
    """-> (s, e); (0, 0) when nothing is left"""
    s, e = max(int(start), 0), min(int(end), int(length))
    return (s, e) if s < e else (0, 0)


def extract(symbols, records, starts, ends, strands=None):
    """``symbols``: one uint8 array per source record.  -> (one uint8 array per region, the (n, 2) int64 ``taken`` table);
    a region whose record does not exist, or that clips to nothing, is empty and takes (0, 0)."""
    strands = [0] * len(records) if strands is None else strands
    out, taken = [], np.zeros((len(records), 2), dtype=np.int64)
    for i, (r, start, end, strand) in enumerate(zip(records, starts, ends, strands)):
        r = int(r)
        s, e = clip(start, end, len(symbols[r])) if 0 <= r < len(symbols) else (0, 0)
        piece = np.asarray(symbols[r][s:e], dtype=np.uint8) if e > s else np.zeros(0, dtype=np.uint8)
        out.append(COMPLEMENT[piece[::-1]] if strand else piece.copy())
        taken[i] = (s, e)
    return out, taken


def to_source(records, taken, strands, region, position, width):
    """Brute force of ``RegionMap.to_source`` for one window: the source positions the window's symbols came from, in the
    order the source holds them, are ``start .. start + width - 1``."""
    s, e = int(taken[region][0]), int(taken[region][1])
    where = [e - 1 - j for j in range(e - s)] if strands[region] else [s + j for j in range(e - s)]   # derived j -> source
    cells = sorted(where[position:position + width])
    assert len(cells) == width and cells == list(range(cells[0], cells[0] + width))
    return int(records[region]), cells[0]
