"""The host side of derived sets, no device: the BED reader (``io.read_bed``), ``io.resize_regions``, the argument table
of ``StripedSequenceSet.regions`` and ``RegionMap.to_source`` against brute force."""
import gzip

import numpy as np
import pytest

from lightmotif_amd import io as lmio
from lightmotif_amd import _ffi
from lightmotif_amd.lib import REGION_DTYPE, RegionMap, _region_args

import regions_rule as rr

NAMES = ["chr1", "chr2", "scaffold_3", "chr2"]     # (the second chr2 is never reached: the first of equal names wins)

BED = (b"browser position chr1:1-100\n"
       b"track name=peaks description=\"a test\"\n"
       b"# a comment\n"
       b"\n"
       b"chr1\t10\t20\n"
       b"chr2\t0\t5\tpeak_a\n"
       b"scaffold_3\t7\t9\tpeak_b\t960\t-\n"
       b"chr1\t100\t90\t.\t0\t+\n"
       b"   \n"
       b"chr2\t3\t4\twith space\t1\t.\n"
       b"chr1\t-5\t12\n")


def check_rows(bed):
    assert len(bed) == 6
    assert bed.records.tolist() == [0, 1, 2, 0, 1, 0] and bed.records.dtype == np.int64
    assert bed.starts.tolist() == [10, 0, 7, 100, 3, -5] and bed.ends.tolist() == [20, 5, 9, 90, 4, 12]
    assert bed.strands.tolist() == [0, 0, 1, 0, 0, 0] and bed.strands.dtype == np.uint8
    assert bed.names == [None, "peak_a", "peak_b", None, "with space", None]     # (a "." in column 4 is no name)
    assert bed.chroms == ["chr1", "chr2", "scaffold_3", "chr1", "chr2", "chr1"]
    assert bed.lines.tolist() == [5, 6, 7, 8, 10, 11]


def test_read_bed_rows_of_three_four_and_six_columns(tmp_path):
    check_rows(lmio.read_bed(BED, NAMES))
    path = tmp_path / "peaks.bed"
    path.write_bytes(BED)
    check_rows(lmio.read_bed(str(path), NAMES))
    check_rows(lmio.read_bed(path, NAMES))


def test_read_bed_is_gzip_transparent(tmp_path):
    check_rows(lmio.read_bed(gzip.compress(BED), NAMES))
    path = tmp_path / "peaks.bed.gz"
    path.write_bytes(gzip.compress(BED))
    check_rows(lmio.read_bed(str(path), NAMES))
    plain = tmp_path / "no_suffix"                   # the magic decides, not the name
    plain.write_bytes(gzip.compress(BED))
    check_rows(lmio.read_bed(str(plain), NAMES))


def test_read_bed_of_nothing():
    for data in (b"", b"\n\n", b"# only\ntrack x\nbrowser y\n"):
        bed = lmio.read_bed(data, NAMES)
        assert len(bed) == 0 and bed.records.shape == (0,) and bed.starts.dtype == np.int64


def test_read_bed_separated_by_blanks():
    bed = lmio.read_bed(b"chr2 1 2 name 0 -\n", NAMES)
    assert (bed.records.tolist(), bed.starts.tolist(), bed.ends.tolist(), bed.strands.tolist(), bed.names) == ([1], [1], [2], [1], ["name"])


@pytest.mark.parametrize("row, line, what", [
    (b"chrX\t1\t2\n", 3, "chrX"),                    # an unknown chromosome
    (b"chr1\t1\n", 3, "2 fields"),                   # too few columns
    (b"chr1\tone\t2\n", 3, "one"),                   # coordinates that are no integers
    (b"chr1\t1\t2.5\n", 3, "2.5"),
    (b"chr1\t1\t2\tname\t0\t*\n", 3, "*"),           # a strand that is none
])
def test_read_bed_names_the_line_of_a_bad_row(tmp_path, row, line, what):
    data = b"# head\nchr1\t0\t1\n" + row + b"chr1\t5\t6\n"
    with pytest.raises(ValueError) as e:
        lmio.read_bed(data, NAMES)
    assert f"BED:{line}:" in str(e.value) and what in str(e.value)
    path = tmp_path / "bad.bed"
    path.write_bytes(data)
    with pytest.raises(ValueError) as e:
        lmio.read_bed(str(path), NAMES)
    assert f"{path}:{line}:" in str(e.value)


def test_resize_regions():
    starts, ends = [10, 0, 7, 100, 5], [20, 5, 8, 90, 5]
    s, e = lmio.resize_regions(starts, ends, flank=3)
    assert s.tolist() == [7, -3, 4, 97, 2] and e.tolist() == [23, 8, 11, 93, 8] and s.dtype == e.dtype == np.int64
    s, e = lmio.resize_regions(starts, ends, flank=0)
    assert s.tolist() == starts and e.tolist() == ends
    for width in (0, 1, 4, 5, 200):
        s, e = lmio.resize_regions(starts, ends, width=width)
        for a, b, x, y in zip(starts, ends, s.tolist(), e.tolist()):
            mid = (a + b) // 2
            assert y - x == width and x == mid - width // 2            # the midpoint is symbol width // 2 of the window
    s, e = lmio.resize_regions([0], [3], width=200)
    assert (s.tolist(), e.tolist()) == ([-99], [101])                  # negative: the device clips
    s, e = lmio.resize_regions([], [], flank=5)
    assert s.shape == e.shape == (0,)
    for kw in ({}, {"flank": 1, "width": 2}):
        with pytest.raises(ValueError):
            lmio.resize_regions(starts, ends, **kw)
    with pytest.raises(ValueError):
        lmio.resize_regions([1, 2], [3], flank=1)
    with pytest.raises(ValueError):
        lmio.resize_regions([1], [3], width=-1)


def test_the_region_table_is_the_abi_struct():
    import ctypes as C
    assert REGION_DTYPE.itemsize == C.sizeof(_ffi.Region) == 32
    for name in ("record", "start", "end", "strand"):
        assert REGION_DTYPE.fields[name][1] == getattr(_ffi.Region, name).offset
    reg = _region_args([0, 2**63, 5], [-(2**63), 0, 7], [2**63 - 1, 1, 3], ["+", "-", "."])
    assert reg["record"].tolist() == [0, 2**63, 5] and reg["start"].tolist() == [-(2**63), 0, 7]
    assert reg["end"].tolist() == [2**63 - 1, 1, 3] and reg["strand"].tolist() == [0, 1, 0]
    assert _region_args([1, 2], [0, 0], [1, 1], None)["strand"].tolist() == [0, 0]
    assert _region_args([1, 2], [0, 0], [1, 1], [True, False])["strand"].tolist() == [1, 0]
    assert _region_args([1, 2], [0, 0], [1, 1], np.array([0, 1]))["strand"].tolist() == [0, 1]
    assert len(_region_args([], [], [])) == 0
    for bad in ([2, 0], ["x", "+"], [0.5, 1.0]):
        with pytest.raises((ValueError, TypeError)):
            _region_args([1, 2], [0, 0], [1, 1], bad)
    with pytest.raises(ValueError):
        _region_args([1, 2], [0], [1, 1])
    with pytest.raises(ValueError):
        _region_args([1, 2], [0, 0], [1, 1], ["+"])
    with pytest.raises(TypeError):
        _region_args([1], [0.5], [1])


def test_region_map_against_brute_force():
    rng = np.random.default_rng(11)
    lengths = [0, 30, 7, 55]
    symbols = [rng.integers(0, 5, n).astype(np.uint8) for n in lengths]
    n = 300
    records = rng.integers(0, 5, n)                  # (4: no such record)
    starts = rng.integers(-10, 60, n)
    ends = starts + rng.integers(-3, 40, n)
    strands = rng.integers(0, 2, n)
    pieces, taken = rr.extract(symbols, records, starts, ends, strands)
    assert (taken[:, 0] < 0).sum() == 0 and any(int(s) < 0 for s in starts) and any(int(e) > 55 for e in ends)   # clipped ones are there
    rmap = RegionMap(records, taken, ["-" if s else "+" for s in strands])
    assert len(rmap) == n
    checked = 0
    for i, piece in enumerate(pieces):
        for width in (1, 3, 8):
            for pos in range(0, len(piece) - width + 1):
                want = rr.to_source(records, taken, strands, i, pos, width)
                got = rmap.to_source(i, pos, width)
                assert (int(got[0]), int(got[1])) == want
                # and the window reads as the source window there, reverse-complemented on the minus strand
                src = symbols[want[0]][want[1]:want[1] + width]
                assert np.array_equal(piece[pos:pos + width], rr.COMPLEMENT[src[::-1]] if strands[i] else src)
                checked += 1
    assert checked > 2_000
    # arrays at once
    idx = np.array([i for i, p in enumerate(pieces) if len(p) >= 4][:50])
    rec, start = rmap.to_source(idx, np.ones(len(idx), dtype=np.int64), 3)
    for i, r, s in zip(idx.tolist(), rec.tolist(), start.tolist()):
        assert (r, s) == rr.to_source(records, taken, strands, i, 1, 3)
    with pytest.raises(ValueError):
        RegionMap([0, 1], np.zeros((3, 2)))
