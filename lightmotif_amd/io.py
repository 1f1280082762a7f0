"""JASPAR 2016 ("jaspar16") count-matrix reader and writer -- host-side text parsing that feeds
the GPU path.  Behaviour follows the reference's
lightmotif-io/src/jaspar16/{mod,parse}.rs:

    >MA0001.3\tAGL3                     header: id, optional description (parse.rs:84-105)
    A  [ 0  0 82 40 ... ]               one line per symbol, counts in brackets (parse.rs:40-51)

A symbol may not appear twice and all rows must have the same length
(parse.rs:53-78, ``InvalidData``).  Missing symbols (``N``) count zero.
"""
from __future__ import annotations

import gzip
import os
import re
from dataclasses import dataclass
from typing import Iterable, Iterator, Optional, TextIO, Union

import numpy as np

from .lib import CountMatrix, _symbols

_ROW = re.compile(r"^\s*(\S)\s+\[\s*([0-9\s]*?)\s*\]\s*$")


@dataclass
class Record:
    """jaspar16/mod.rs:33-65"""
    id: str
    description: Optional[str]
    matrix: CountMatrix


def read(file: Union[str, TextIO], *, protein: bool = False) -> Iterator[Record]:
    """Iterate over the records of a JASPAR-2016 formatted file (jaspar16/mod.rs:139)."""
    close = False
    if isinstance(file, (str, os.PathLike)):
        path = os.fspath(file)
        file = gzip.open(path, "rt") if path.endswith(".gz") else open(path, "r")
        close = True
    try:
        header, rows = None, []
        for line in file:
            if line.startswith(">"):
                if header is not None:
                    yield _build(header, rows, protein)
                header, rows = line, []
            elif line.strip():
                if header is None:
                    raise ValueError("matrix row before the first header")
                rows.append(line)
        if header is not None:
            yield _build(header, rows, protein)
    finally:
        if close:
            file.close()


def _build(header: str, rows: list, protein: bool) -> Record:
    parts = header[1:].strip().split(None, 1)   # id = up to the first whitespace (parse.rs:86-90)
    if not parts:
        raise ValueError("empty record header")
    ident = parts[0]
    desc = parts[1].strip() if len(parts) > 1 and parts[1].strip() else None
    sym = _symbols(protein)
    if not rows:
        raise ValueError(f"record {ident} has no matrix")
    counts, done, length = None, set(), None
    for line in rows:
        m = _ROW.match(line)
        if not m:
            raise ValueError(f"record {ident}: cannot parse matrix row {line!r}")
        letter, body = m.group(1), m.group(2)
        if letter not in sym:
            raise ValueError(f"record {ident}: invalid symbol {letter!r}")
        vals = [int(x) for x in body.split()]
        if letter in done:                       # parse.rs:62-64
            raise ValueError(f"record {ident}: duplicate symbol {letter!r}")
        if length is None:
            length = len(vals)
            counts = np.zeros((length, len(sym)), dtype=np.uint32)
        elif len(vals) != length:                # parse.rs:66-68
            raise ValueError(f"record {ident}: inconsistent row length")
        counts[:, sym.index(letter)] = vals
        done.add(letter)
    return Record(ident, desc, CountMatrix(counts, protein=protein))


@dataclass
class BedRegions:
    """The rows of a BED file, in file order: ``records`` (indices into the names they were read against), ``starts`` and
    ``ends`` (int64, 0-based and half-open as the file has them), ``strands`` (uint8, 1 for ``-``), ``names`` (column 4 or
    ``None``), ``chroms`` (column 1) and the 1-based ``lines`` they stood on."""
    records: np.ndarray
    starts: np.ndarray
    ends: np.ndarray
    strands: np.ndarray
    names: list
    chroms: list
    lines: np.ndarray

    def __len__(self) -> int:
        return len(self.chroms)


def _bed_lines(source) -> Iterator[str]:
    """The text lines of a BED file given as a path, as ``bytes`` or as an open handle; gzip is sniffed by its magic."""
    if isinstance(source, (str, os.PathLike)):
        with open(os.fspath(source), "rb") as fh:
            source = fh.read()
    if isinstance(source, (bytes, bytearray, memoryview)):
        data = bytes(source)
        if data[:2] == b"\x1f\x8b":
            data = gzip.decompress(data)
        yield from data.decode("utf-8", "replace").splitlines()
    else:
        for line in source:
            yield line.decode("utf-8", "replace") if isinstance(line, bytes) else line


def bed_rows(source, label: str = "BED") -> Iterator[tuple]:
    """``(line number, chrom, start, end, name or None, strand 0 / 1)`` per data row of a BED file: columns 1-3, the name
    (4; a lone ``.`` is no name) and the strand (6) when present.  ``track`` and ``browser`` lines, ``#`` lines and blank lines are skipped; fields
    are separated by tabs (or, in a file without tabs, by blanks).  ``ValueError`` names the line of a row with fewer than
    three columns, with coordinates that are not integers, or with a strand other than ``+``, ``-`` or ``.`` (a dot counts
    as plus)."""
    for number, line in enumerate(_bed_lines(source), 1):
        text = line.strip()
        if not text or text.startswith("#") or text.split(None, 1)[0] in ("track", "browser"):
            continue
        fields = text.split("\t") if "\t" in text else text.split()
        if len(fields) < 3:
            raise ValueError(f"{label}:{number}: expected `chrom start end`, found {len(fields)} fields")
        try:
            start, end = int(fields[1]), int(fields[2])
        except ValueError:
            raise ValueError(f"{label}:{number}: start `{fields[1]}` and end `{fields[2]}` are not integers") from None
        strand = fields[5].strip() if len(fields) > 5 else "."
        if strand not in ("+", "-", "."):
            raise ValueError(f"{label}:{number}: strand `{strand}` is not one of + - .")
        name = fields[3].strip() if len(fields) > 3 and fields[3].strip() not in ("", ".") else None   # ("." stands for no name)
        yield number, fields[0].strip(), start, end, name, 1 if strand == "-" else 0


def read_bed(path_or_bytes, names) -> BedRegions:
    """Reads a BED file (a path, or its bytes; gzip-transparent) against the records of a set: ``names[r]`` is the name of
    record ``r``, the first whitespace-delimited token of its FASTA header as ``fasta_names`` yields them (the first of
    equal names wins).  What comes back goes to ``StripedSequenceSet.regions`` as it is.  ``ValueError`` names the line of
    an unknown chromosome or a malformed row (``bed_rows``)."""
    label = os.fspath(path_or_bytes) if isinstance(path_or_bytes, (str, os.PathLike)) else "BED"
    index: dict = {}
    for r, name in enumerate(names):
        index.setdefault(name, r)
    rec, starts, ends, strands, labels, chroms, lines = [], [], [], [], [], [], []
    for number, chrom, start, end, name, strand in bed_rows(path_or_bytes, label):
        if chrom not in index:
            raise ValueError(f"{label}:{number}: no record is called `{chrom}`")
        rec.append(index[chrom]), starts.append(start), ends.append(end), strands.append(strand)
        labels.append(name), chroms.append(chrom), lines.append(number)
    return BedRegions(np.array(rec, dtype=np.int64), np.array(starts, dtype=np.int64), np.array(ends, dtype=np.int64),
                      np.array(strands, dtype=np.uint8), labels, chroms, np.array(lines, dtype=np.int64))


def resize_regions(starts, ends, flank: Optional[int] = None, width: Optional[int] = None):
    """``(starts, ends)`` as int64 arrays, either extended by ``flank`` symbols on both sides, or replaced by a window of
    ``width`` symbols centred on the midpoint ``(start + end) // 2`` -- ``[mid - width // 2, mid - width // 2 + width)``.
    Exactly one of the two; the results may be negative or lie past the record, the device clips them."""
    if (flank is None) == (width is None):
        raise ValueError("resize_regions: exactly one of flank and width")
    s, e = np.asarray(starts, dtype=np.int64), np.asarray(ends, dtype=np.int64)
    if s.shape != e.shape:
        raise ValueError(f"{s.size} starts against {e.size} ends")
    if flank is not None:
        return s - int(flank), e + int(flank)
    if int(width) < 0:
        raise ValueError("a window has no negative width")
    left = (s + e) // 2 - int(width) // 2
    return left, left + int(width)


def write(records: Iterable[Record], file: Union[str, TextIO]) -> None:
    """Writes records in the JASPAR-2016 format ``read`` parses: a header ``>id`` (tab, description) and one bracketed line
    of counts per symbol.  The default symbol's line (``N``) is written only when it holds a count: files of the format do not
    carry it, a missing line reads back as zeros, and the parsers (here and parse.rs:36-78) accept the line when present."""
    close = False
    if isinstance(file, (str, os.PathLike)):
        path = os.fspath(file)
        file = gzip.open(path, "wt") if path.endswith(".gz") else open(path, "w")
        close = True
    try:
        for rec in records:
            file.write(f">{rec.id}\t{rec.description}\n" if rec.description else f">{rec.id}\n")
            sym = _symbols(rec.matrix.protein)
            data = rec.matrix.data
            digits = max(1, len(str(int(data.max())))) if data.size else 1
            for s, letter in enumerate(sym):
                if s == len(sym) - 1 and not data[:, s].any():
                    continue
                file.write(f"{letter}  [ " + " ".join(f"{int(v):>{digits}}" for v in data[:, s]) + " ]\n")
    finally:
        if close:
            file.close()
