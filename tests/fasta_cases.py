"""The FASTA grammar of ``lm_hip_seqset_from_fasta`` (include/lightmotif_hip.h, csrc/fasta.hip) in plain Python, and the
inputs the host and GPU tests share.  Everything works on bytes."""
import numpy as np

SPACE = b"\t\n\x0b\x0c\r "                          # 0x09-0x0D and 0x20


def parse(data: bytes):
    """``(spans, records)``: per record the bytes ``[begin, end)`` of its header line (without the ``>`` and the ``\\n``; a
    ``\\r`` stays inside) as an ``(n, 2)`` uint64 array, and the record's residues as bytes."""
    data = bytes(data)
    spans, records = [], []
    pos = 0
    while pos < len(data):
        nl = data.find(b"\n", pos)
        end = len(data) if nl < 0 else nl            # the line is data[pos:end]
        if data[pos:pos + 1] == b">":
            spans.append((pos + 1, end))
            records.append(bytearray())
        elif records:
            records[-1] += data[pos:end].translate(None, SPACE)
        pos = end + 1
    return np.array(spans, dtype=np.uint64).reshape(-1, 2), [bytes(r) for r in records]


def lines(seq: bytes, width: int, eol: bytes = b"\n") -> bytes:
    return b"".join(seq[i:i + width] + eol for i in range(0, len(seq), width))


def residues(rng, n: int, alphabet: bytes = b"ACGT") -> bytes:
    return bytes(np.frombuffer(alphabet, dtype=np.uint8)[rng.integers(0, len(alphabet), n)])


def fasta(records, width: int = 60, eol: bytes = b"\n") -> bytes:
    """``records``: (header bytes, sequence bytes) pairs, ``width``-column lines."""
    return b"".join(b">" + h + eol + lines(s, width, eol) for h, s in records)


def land_at(rng, tail: bytes, at: int, mark: int = 0) -> bytes:
    """A text in which byte ``mark`` of ``tail`` stands at offset ``at``: a header and 60-column sequence lines in front
    of it (the last one sized to fit; a blank line if one byte is left), ``tail`` behind them."""
    head = b">pad\n"
    room = at - mark - len(head)
    assert room >= 0
    body = lines(residues(rng, room // 61 * 60), 60)
    if room % 61:
        body += residues(rng, room % 61 - 1) + b"\n"
    text = head + body + tail
    assert text[at] == tail[mark] and len(head + body) == at - mark
    return text


PLAIN = {                                            # inputs on which the grammar and scan_cli.read_fasta agree
    "unix": b">one first record\nACGTAC\nGTNNAC\n>two\nTTTT\n",
    "dos": b">one first record\r\nACGTAC\r\nGTNNAC\r\n>two\r\nTTTT\r\n",
    "blank_lines": b">one\n\nACGT\n\n\nAC\n>two\n\n",
    "no_final_newline": b">one\nACGT\n>two\nAC",
    "ends_in_header": b">one\nACGT\n>two",
    "consecutive_headers": b">a\n>b\n>c\nACGT\n>d\n>e\n",
    "junk_first": b"junk line\nACGT\n>one\nAC\n",
    "bare": b">\nACGT\n> \n>  name  rest\nGG\n",
    "only_headers": b">a\n>b\n>c\n",
    "tabs_in_header": b">id\tdescription here\nAC\n",
    "edge_space": b">one\n  ACGT  \n\tAC\t\n",
    "empty": b"",
    "junk_only": b"ACGT\nACGT\n",
    "gt_only": b">",
}
