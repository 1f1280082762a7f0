"""Host side of the device FASTA reader (lm_hip_seqset_from_fasta): the grammar stated in the header against
``scan_cli.read_fasta`` on plain inputs, the chunker that cuts a file at record starts, and the two new symbols.  No
device is needed."""
import gzip
import io
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from lightmotif_amd import _ffi, scan_cli
from lightmotif_amd.lib import fasta_names
from fasta_cases import PLAIN, fasta, parse, residues

ROOT = Path(__file__).resolve().parent.parent


@pytest.mark.parametrize("name", sorted(PLAIN))
def test_the_grammar_reads_plain_fasta_as_read_fasta_does(name):
    data = PLAIN[name]
    want = list(scan_cli.read_fasta(io.TextIOWrapper(io.BytesIO(data), encoding="ascii", newline=None)))
    spans, records = parse(data)
    assert fasta_names(data, spans) == [n for n, _ in want]
    assert records == [s.encode() for _, s in want]
    assert spans.dtype == np.uint64 and spans.shape == (len(want), 2)
    for begin, end in spans.tolist():                # a span is the header line without '>' and '\n'
        assert data[begin - 1:begin] == b">" and b"\n" not in data[begin:end]
        assert end == len(data) or data[end:end + 1] == b"\n"


def test_names_come_from_any_buffer():
    data = b">alpha one\r\n>\r\n>beta\n"
    spans, _ = parse(data)
    for buf in (data, bytearray(data), memoryview(data), np.frombuffer(data, dtype=np.uint8)):
        assert fasta_names(buf, spans) == ["alpha", "", "beta"]
    assert fasta_names(data, np.zeros((0, 2), dtype=np.uint64)) == []


def header_starts(chunk: bytes) -> int:
    return (1 if chunk.startswith(b">") else 0) + chunk.count(b"\n>")


def random_file(rng) -> bytes:
    recs = [(b"r%d some text" % i, residues(rng, int(rng.integers(0, 200)), b"ACGTN")) for i in range(int(rng.integers(1, 12)))]
    eol = b"\r\n" if rng.random() < 0.3 else b"\n"
    data = fasta(recs, width=int(rng.integers(1, 70)), eol=eol)
    if rng.random() < 0.3:
        data = b"text before\nthe first header\n" + data
    if rng.random() < 0.3:
        data = data.rstrip(b"\r\n")
    return data


def test_fasta_chunks_cut_at_record_starts(tmp_path):
    rng = np.random.default_rng(5)
    for case in range(60):
        data = random_file(rng)
        budgets = [1, 2, 3, 7, int(rng.integers(1, 64)), int(rng.integers(64, 400)), len(data) - 1, len(data), len(data) + 1, 1 << 20]
        for budget in budgets:
            if budget < 1:
                continue
            chunks = list(scan_cli.fasta_chunks(io.BytesIO(data), budget))
            assert b"".join(chunks) == data
            assert all(chunks)
            at = 0
            for i, chunk in enumerate(chunks):
                if i:
                    assert chunk[:1] == b">" and data[at - 1:at] == b"\n"
                if len(chunk) > budget:              # one record alone, longer than the budget
                    assert header_starts(chunk) == 1
                at += len(chunk)
            # what is cut is what is parsed: the records of the chunks are the records of the file
            assert [r for c in chunks for r in parse(c)[1]] == parse(data)[1]
        if case < 8:                                 # gzip delivers other block sizes: the cuts depend on the content alone
            plain, packed = tmp_path / "f.fa", tmp_path / "f.fa.gz"
            plain.write_bytes(data)
            with gzip.open(packed, "wb") as fh:
                fh.write(data)
            for budget in (1, 50, 300):
                with scan_cli._open_bytes(str(plain)) as a, scan_cli._open_bytes(str(packed)) as b:
                    assert list(scan_cli.fasta_chunks(a, budget)) == list(scan_cli.fasta_chunks(b, budget)) == \
                        list(scan_cli.fasta_chunks(io.BytesIO(data), budget))


def test_fasta_chunks_degenerate():
    assert list(scan_cli.fasta_chunks(io.BytesIO(b""), 10)) == []
    assert list(scan_cli.fasta_chunks(io.BytesIO(b"no header at all\nACGT\n"), 4)) == [b"no header at all\nACGT\n"]
    big = b">a\n" + b"ACGT" * 50_000 + b"\n>b\nAC\n"   # a record far longer than the read block's share
    assert list(scan_cli.fasta_chunks(io.BytesIO(big), 5)) == [big[:-6], b">b\nAC\n"]
    with pytest.raises(ValueError):
        list(scan_cli.fasta_chunks(io.BytesIO(b">a\n"), 0))


def test_the_symbols_are_declared_bound_and_exported():
    header = (ROOT / "include" / "lightmotif_hip.h").read_text()
    body = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", str(_ffi.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    for name in ("lm_hip_seqset_from_fasta", "lm_hip_fasta_tile_bytes"):
        assert re.search(r"\b%s\s*\(" % name, body)
        assert name in _ffi.SIGNATURES
        assert re.search(r" T %s$" % name, out, flags=re.M)
    assert "lm_hip_fasta_span" in body
    assert "main.rs:532-546" in header and "seq.rs:122-129" in header
    assert _ffi.lib().lm_hip_abi_version() == 1


def test_the_tile_size_needs_no_device():
    tile = _ffi.lib().lm_hip_fasta_tile_bytes()
    assert tile >= 256
