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
