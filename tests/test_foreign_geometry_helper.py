"""Host tier of tests/foreign_geometry.py: embed / extract round trips, detection of a writer or reader that uses the
wrong stride, and the pairwise cover of the case tables of tests/test_gpu_foreign_geometry.py.  Needs no GPU."""
import numpy as np
import pytest

from foreign_geometry import BASE_ALIGN, CANARY_F32, CANARY_U8, GUARD_ROWS, embed, extract, uncovered_pairs


class host_view:
    """The elements of an embedding on a CPU tensor, indexed from element (0, 0) of the matrix; negative indices reach
    into the guard rows in front (numpy's own meaning of a negative index would hide a write before the matrix)."""

    def __init__(self, emb):
        lead = emb.first - emb.guard * emb.itemsize
        n = (emb.buf.numel() - lead) // emb.itemsize
        self.flat = emb.buf.numpy()[lead: lead + n * emb.itemsize].view(emb.dtype)
        self.origin = emb.guard

    def __getitem__(self, key):
        return self.flat[self._shift(key)]

    def __setitem__(self, key, value):
        self.flat[self._shift(key)] = value

    def _shift(self, key):
        if isinstance(key, slice):
            assert key.step is None
            return slice(key.start + self.origin, key.stop + self.origin)
        return key + self.origin


@pytest.mark.parametrize("dtype,canary", [(np.uint8, CANARY_U8), (np.uint32, CANARY_F32), (np.float32, (np.inf, np.nan))])
@pytest.mark.parametrize("rows,cols,stride", [(7, 32, 32), (7, 32, 33), (5, 16, 32), (3, 33, 64), (1, 1, 1), (0, 32, 40), (1, 0, 0)])
@pytest.mark.parametrize("elem_offset", [0, 1, 3, 16])
def test_round_trip(dtype, canary, rows, cols, stride, elem_offset):
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(rows * 100 + cols)
    m = rng.integers(0, 200, (rows, cols)).astype(dtype)
    emb = embed(m, stride, elem_offset * dtype.itemsize, canary)
    assert emb.ptr % BASE_ALIGN == (elem_offset * dtype.itemsize) % BASE_ALIGN
    assert emb.guard >= GUARD_ROWS * stride
    got, problems = extract(emb)
    assert problems == []
    assert got.shape == (rows, cols) and got.dtype == dtype
    assert np.array_equal(got.view(f"u{dtype.itemsize}"), m.view(f"u{dtype.itemsize}"))
    # the address arithmetic a kernel does on (ptr, stride) lands on the payload
    base = emb.buf.data_ptr()
    raw = emb.buf.numpy()
    for r, c in ((0, 0), (rows - 1, cols - 1)):
        if rows and cols:
            at = emb.ptr + (r * stride + c) * dtype.itemsize - base
            assert raw[at: at + dtype.itemsize].tobytes() == m[r, c].tobytes()
            assert emb.row_ptr(r) == emb.ptr + r * stride * dtype.itemsize


def test_rejects_what_the_library_may_not_be_given():
    m = np.zeros((4, 8), np.float32)
    with pytest.raises(ValueError):
        embed(m, 7, 0, 0.0)            # stride below the column count
    with pytest.raises(ValueError):
        embed(m, 8, 2, 0.0)            # an f32 pointer that is not element-aligned
    embed(m.view(np.uint8).reshape(4, 32), 32, 3, 0)   # byte pointers may be anything


def write_rows(emb, matrix, stride, first_row=0):
    """A writer that believes the rows lie `stride` elements apart."""
    flat = host_view(emb)
    for r in range(matrix.shape[0]):
        at = (first_row + r) * stride
        flat[at: at + matrix.shape[1]] = matrix[r]


@pytest.mark.parametrize("dtype,canary", [(np.uint8, CANARY_U8), (np.uint32, CANARY_F32)])
def test_a_writer_with_the_wrong_stride_is_detected(dtype, canary):
    rows, cols, stride = 9, 32, 40
    want = np.arange(rows * cols).reshape(rows, cols).astype(dtype)
    blank = np.full((rows, cols), canary, dtype)
    # the right stride: payload arrives, no canary moves
    emb = embed(blank, stride, 0, canary)
    write_rows(emb, want, stride)
    got, problems = extract(emb)
    assert problems == [] and np.array_equal(got, want)
    # `cols` used where `stride` was meant: rows land early, in the padding of the rows before
    emb = embed(blank, stride, 0, canary)
    write_rows(emb, want, cols)
    got, problems = extract(emb)
    assert not np.array_equal(got, want)
    assert len(problems) == 1 and "row padding" in problems[0] and "row 0, column 32" in problems[0]
    # a stride that is too large runs past the last row
    emb = embed(blank, stride, 0, canary)
    write_rows(emb, want, stride + 8)
    got, problems = extract(emb)
    assert not np.array_equal(got, want) and any("behind the matrix" in p for p in problems)
    # one row too early
    emb = embed(blank, stride, 0, canary)
    write_rows(emb, want[:1], stride, first_row=-1)
    assert any("in front of the matrix" in p and "nearest: 9 elements" in p for p in extract(emb)[1])
    # a single element of padding, and a single byte outside everything
    emb = embed(blank, stride, 0, canary)
    host_view(emb)[3 * stride + cols + 5] = 1
    assert extract(emb)[1] == ["1 elements of row padding are wrong (first: row 3, column 37)"]
    emb = embed(blank, stride, 0, canary)
    emb.buf[emb.buf.numel() - 1] = 0
    assert extract(emb)[1] == ["bytes outside the guard rows changed"]


def test_a_reader_with_the_wrong_stride_sees_poison():
    """Inputs: the padding holds +inf and NaN, so a reduction that walks the rows `cols` apart meets them.  (The
    pattern is cycled in buffer order: a length that shares no factor with the stride puts both values in a column.)"""
    rows, cols, stride = 6, 5, 6
    m = np.arange(rows * cols, dtype=np.float32).reshape(rows, cols)
    emb = embed(m, stride, 4, (np.inf, np.nan, np.nan, np.inf, np.nan, np.inf, np.inf))
    flat = host_view(emb)
    right = np.stack([flat[r * stride: r * stride + cols] for r in range(rows)])
    wrong = np.stack([flat[r * cols: r * cols + cols] for r in range(rows)])
    assert np.array_equal(right, m)
    assert np.isinf(wrong).any() and np.isnan(wrong).any()
    pad = np.stack([flat[r * stride + cols: (r + 1) * stride] for r in range(rows)])
    assert np.isinf(pad).sum() + np.isnan(pad).sum() == pad.size
    # bit-for-bit comparison: the NaN canaries are equal to themselves, an intact buffer reports nothing
    assert extract(emb)[1] == []


def test_promised_padding():
    """stripe / configure_wrap promise the default symbol in the padding of the rows they write."""
    rows, cols, stride = 10, 33, 40
    emb = embed(np.full((rows, cols), CANARY_U8, np.uint8), stride, 1, CANARY_U8)
    flat = host_view(emb)
    for r in range(2, 7):
        flat[r * stride + cols: (r + 1) * stride] = 4
    assert extract(emb, padding=4, padded_rows=(2, 7))[1] == []
    assert "row 7" in extract(emb, padding=4, padded_rows=(2, 8))[1][0]
    assert "row 2" in extract(emb)[1][0]


def test_uncovered_pairs():
    axes = [(0, 1), ("a", "b"), (True, False)]
    full = [(x, y, z) for x in axes[0] for y in axes[1] for z in axes[2]]
    assert uncovered_pairs(full, axes) == []
    assert uncovered_pairs([(0, "a", True), (0, "b", False), (1, "a", False), (1, "b", True)], axes) == []
    assert uncovered_pairs([(0, "a", True), (1, "b", False)], axes[:2]) == [(0, 1, 0, "b"), (0, 1, 1, "a")]


def test_the_gpu_tables_are_pairwise_covers():
    """Every table of the GPU module names its axes; each pair of values of two axes meets in some case (pairs a
    table declares impossible excepted), and the number of cases is the number the module promises to have run."""
    import test_gpu_foreign_geometry as g
    assert 150 <= sum(len(table) for table, _, _ in g.TABLES.values()) <= 250
    for name, (table, axes, impossible) in g.TABLES.items():
        assert len(set(table)) == len(table), f"{name}: a case is listed twice"
        assert len(table) == g.EXPECTED_CASES[name], name
        if axes is None:            # a plain list of cases beside a table
            continue
        for row in table:
            assert len(row) == len(axes), (name, row)
            for value, axis in zip(row, axes):
                assert value in axis, (name, row, value)
        missing = [p for p in uncovered_pairs(table, axes) if not impossible(*p)]
        assert missing == [], (name, missing[:5])
