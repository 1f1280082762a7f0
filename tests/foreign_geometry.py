"""Placing a row-major matrix at a foreign stride and alignment inside a larger buffer of canaries.

The device-pointer entry points take a pointer and a stride that are independent of the column count: a torch view
with a storage offset, one row shard of a wider buffer, a matrix whose rows are longer than their live columns.
``embed`` builds such a placement -- guard rows of canaries before and behind the matrix, canaries in the padding
of every row, the first element at a chosen byte offset from a 64-byte boundary -- and ``extract`` reads the
matrix back and names every canary that changed.  The same pair serves inputs (the canaries are then poison: a
kernel that reads with the wrong stride computes a wrong answer) and outputs (a kernel that writes with the wrong
stride, or past its rows, changes a canary).

Works on CPU tensors as well (tests/test_foreign_geometry_helper.py needs no GPU)."""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

GUARD_ROWS = 64           # canary rows in front of and behind the matrix
MIN_GUARD = 256           # ... and never fewer elements than this (a one-row "matrix" of a few bytes)
BASE_ALIGN = 64           # the byte offset of an embedding counts from a multiple of this

CANARY_F32 = 0x7FC0DEAD   # a NaN payload no score can produce (as uint32 words)
CANARY_U8 = 0xA5
_SLACK = 0x5A             # the bytes of the allocation outside the guard rows


@dataclass
class Embedded:
    """A matrix of ``rows x cols`` elements whose row ``r`` starts ``r * stride`` elements behind ``first``."""
    buf: torch.Tensor      # 1-D uint8, owns the memory
    dtype: np.dtype
    rows: int
    cols: int
    stride: int
    byte_offset: int
    first: int             # byte index in ``buf`` of element (0, 0)
    guard: int             # canary elements in front of (0, 0) and behind the last row
    canary: np.ndarray     # the pattern, cycled over every canary element in buffer order

    @property
    def ptr(self) -> int:
        """Address of element (0, 0)."""
        return self.buf.data_ptr() + self.first

    @property
    def itemsize(self) -> int:
        return self.dtype.itemsize

    def row_ptr(self, row: int) -> int:
        return self.ptr + row * self.stride * self.itemsize


def _pattern(canary, dtype: np.dtype) -> np.ndarray:
    pat = np.atleast_1d(np.asarray(canary)).astype(dtype)
    assert pat.ndim == 1 and pat.size >= 1
    return pat


def _canary_run(pat: np.ndarray, start: int, n: int) -> np.ndarray:
    """Canary elements ``start .. start + n`` of the buffer (the pattern is anchored at the region's first element)."""
    return pat[(start + np.arange(n)) % pat.size]


def embed(matrix: np.ndarray, stride: int, byte_offset: int, canary: Union[int, float, Sequence], device="cpu") -> Embedded:
    """Places the 2-D ``matrix`` row-major at ``stride`` elements per row, its first element ``byte_offset`` bytes
    behind a 64-byte boundary, with ``GUARD_ROWS`` rows of ``canary`` in front and behind and ``canary`` in the
    ``stride - cols`` elements of padding of every row.  ``canary`` is one value or a pattern that is cycled (row
    padding that holds +inf AND NaN, say).  The offset must be a multiple of the element size: pointers handed to the
    library are element-aligned."""
    matrix = np.asarray(matrix)
    assert matrix.ndim == 2, "embed: a 2-D matrix"
    rows, cols = matrix.shape
    dtype = matrix.dtype
    size = dtype.itemsize
    if stride < cols:
        raise ValueError(f"embed: stride {stride} below the column count {cols}")
    if byte_offset < 0 or byte_offset % size:
        raise ValueError(f"embed: byte offset {byte_offset} is not a multiple of the element size {size}")
    pat = _pattern(canary, dtype)
    guard = max(GUARD_ROWS * stride, MIN_GUARD)
    n_elems = guard + rows * stride + guard
    host = np.empty(n_elems, dtype=dtype)
    host[:] = _canary_run(pat, 0, n_elems)
    if rows:
        host[guard: guard + rows * stride].reshape(rows, stride)[:, :cols] = matrix
    nbytes = n_elems * size
    buf = torch.empty(nbytes + byte_offset + 2 * BASE_ALIGN, dtype=torch.uint8, device=device)
    lead = (-buf.data_ptr()) % BASE_ALIGN + byte_offset
    first = lead + guard * size
    raw = np.full(buf.numel(), _SLACK, dtype=np.uint8)   # the slack around the region is checked as well
    raw[lead: lead + nbytes] = host.view(np.uint8)
    buf.copy_(torch.from_numpy(raw))
    emb = Embedded(buf, dtype, rows, cols, stride, byte_offset, first, guard, pat)
    assert emb.ptr % BASE_ALIGN == byte_offset % BASE_ALIGN
    return emb


def extract(emb: Embedded, padding: Optional[Union[int, float]] = None,
            padded_rows: Optional[Tuple[int, int]] = None) -> Tuple[np.ndarray, List[str]]:
    """Reads the buffer back: ``(payload, problems)``.  ``payload`` is the ``rows x cols`` matrix as it stands now;
    ``problems`` names every canary that no longer holds its value -- the guard rows in front, the guard rows behind,
    the padding of each row, the slack around them -- compared bit for bit (a NaN canary equals itself).  An empty
    list: nothing but the payload was written.

    ``padding`` / ``padded_rows``: rows ``[a, b)`` are expected to hold ``padding`` in place of the canary in their
    ``stride - cols`` padding elements (an entry point that promises to fill the padding of the rows it writes)."""
    size = emb.itemsize
    raw = emb.buf.cpu().numpy()
    lead = emb.first - emb.guard * size
    n_elems = 2 * emb.guard + emb.rows * emb.stride
    host = raw[lead: lead + n_elems * size].view(emb.dtype)
    bits = np.dtype(f"u{size}")
    want = _canary_run(emb.canary, 0, n_elems)
    problems: List[str] = []

    def differs(got: np.ndarray, exp: np.ndarray) -> np.ndarray:
        return np.flatnonzero(got.view(bits) != np.ascontiguousarray(exp).view(bits))

    if (raw[:lead] != _SLACK).any() or (raw[lead + n_elems * size:] != _SLACK).any():
        problems.append("bytes outside the guard rows changed")
    g = emb.guard
    bad = differs(host[:g], want[:g])
    if bad.size:
        problems.append(f"{bad.size} canaries in front of the matrix changed (nearest: {g - int(bad[-1])} elements before it)")
    tail0 = g + emb.rows * emb.stride
    bad = differs(host[tail0:], want[tail0:])
    if bad.size:
        problems.append(f"{bad.size} canaries behind the matrix changed (first: {int(bad[0])} elements past its end)")
    if emb.rows:
        body = host[g:tail0].reshape(emb.rows, emb.stride)
        payload = body[:, :emb.cols].copy()
        if emb.stride > emb.cols:
            exp = want[g:tail0].reshape(emb.rows, emb.stride)[:, emb.cols:].copy()
            if padding is not None:
                a, b = padded_rows if padded_rows is not None else (0, emb.rows)
                exp[a:b] = np.asarray(padding).astype(emb.dtype)
            pad = np.ascontiguousarray(body[:, emb.cols:])
            bad = differs(pad.reshape(-1), exp.reshape(-1))
            if bad.size:
                w = emb.stride - emb.cols
                r, c = divmod(int(bad[0]), w)
                problems.append(f"{bad.size} elements of row padding are wrong (first: row {r}, column {emb.cols + c})")
    else:
        payload = np.empty((0, emb.cols), dtype=emb.dtype)
    return payload, problems


def uncovered_pairs(table: Sequence[Sequence], axes: Sequence[Sequence]) -> List[Tuple[int, int, object, object]]:
    """The value pairs of two different axes that NO row of ``table`` holds together: ``(axis i, axis j, value of i,
    value of j)``.  ``table`` rows have one value per axis; an empty result means the table is a pairwise cover."""
    missing = []
    for i in range(len(axes)):
        for j in range(i + 1, len(axes)):
            seen = {(row[i], row[j]) for row in table}
            missing += [(i, j, a, b) for a in axes[i] for b in axes[j] if (a, b) not in seen]
    return missing
