"""Minimal command-line driver with the shape of ``lightmotif-cli``:

    python -m lightmotif_amd.scan_cli -m motifs.pwm[.gz] -s genome.fa[.gz] -o hits.tsv -P 1e-5

Behaviour follows lightmotif-cli/src/main.rs:
  * matrices: JASPAR-2016 count matrices -> ``to_freq(0.1).to_scoring(None)`` (main.rs:473-478);
  * threshold per motif: ``--pvalue`` through the MEME-style score distribution, or
    ``--rel-threshold`` (x max score) or ``--abs-threshold``; default p = 1e-5 (main.rs:479-489);
  * every FASTA record is encoded lossily, striped and given ``max_m`` wrap rows
    (main.rs:540-546) -- here on the device, from the raw text;
  * the FASTA container itself is parsed on the device as well (``--ingest device``, the default): the file is read in
    binary, cut at record starts into chunks of at most ``--batch-bases`` BYTES of FASTA text (``fasta_chunks``), and each
    chunk becomes a resident set through ``Pipeline.stripe_fasta_set`` -- the host never looks at a sequence line.
    ``--ingest host`` is the line-by-line reader ``read_fasta`` in front of ``Pipeline.stripe_ascii_set``, where
    ``--batch-bases`` counts bases.  On plain FASTA (ASCII, ``\\n`` or ``\\r\\n`` line ends, whitespace only at the ends of a
    sequence line) both write the same TSV, wherever the sets are cut.  They differ on whitespace INSIDE a sequence line
    (dropped on the device; a default symbol on the host), on a lone ``\\r`` used as a line end (no line end on the device;
    text mode makes it one) and on non-ASCII bytes (invalid residues on the device; a decoding matter on the host);
  * the reference fans (motif, sequence) pairs out to worker threads (main.rs:554-561); here
    records are gathered into sets of up to ``--batch-bases`` bases, each set is resident as one
    striped sequence, and all motifs x all records of a set go to the GPU as ONE call per strand
    (``Pipeline.scan_threshold_set``: windows that leave their record are cut on the device);
  * output: TSV ``seq_index seq_name motif_index motif_name pos strand score pvalue`` with
    1-based indices and the p-value in exponent notation (main.rs:527-531, 587-600).
    The reference writes hits in worker-completion order; this driver writes them grouped by
    sequence, then strand, then motif, then position.
``--best`` writes, instead of the hits above a threshold, ONE line per (sequence, strand, motif) that has a window: the
best window of the motif in that record, the lowest position among equal scores (``Pipeline.scan_best_set``); thresholds
play no part.
``--counts`` writes, instead of the hits themselves, how many there are: ONE line per (sequence, strand, motif) that has a
window, ``seq_index seq_name motif_index motif_name strand windows hits`` -- the windows of the motif in that record and
how many of them reach the motif's threshold (``Pipeline.scan_count_set``: no hit list is made).  It needs one of ``-P``,
``--abs-threshold``, ``--rel-threshold`` and excludes ``--best``, ``--matched`` and ``--site-matrices``.
``--sum-odds`` writes, instead of hits, the total affinity: ONE line per (sequence, strand, motif) that has a window,
``seq_index seq_name motif_index motif_name strand windows sum_odds log2_mean_odds`` -- the windows of the motif in that
record, the sum of ``2 ** score`` over them (``Pipeline.scan_sum_set``: no hit list is made; the scores are log2 odds) and
``log2(sum_odds / windows)``, both written with ``repr``.  Thresholds play no part; it excludes ``--best``, ``--counts``,
``--variants``, ``--matched`` and ``--site-matrices``.
``--refine N --refined PATH`` refines every motif on the input before the scan: N iterations of EM on the resident set
(``Pipeline.refine``: per iteration the total odds per record, then the expected site counts of all windows, both on the
device, then new matrices; ``--refine-model oops`` -- one site per record, the default -- or ``zoops``), from the forward
matrices as loaded and against the set's own background.  ``PATH`` receives one JASPAR-2016 record per motif: the expected
site counts of the last iteration, rounded to integers.  The input has to fit ONE resident set (``--batch-bases``).  The
scan then proceeds with the matrices as loaded: no other output changes.
``--pvalues device`` (the default) builds the score distributions of all motifs on the device
(``Pipeline.score_distributions``): the thresholds of ``-P`` come from one call, and the ``pvalue`` column of a set from one
call per strand on the set's hits.  ``--pvalues host`` is the per-motif, per-hit host code of ``dist.py``; the TSV is the
same byte for byte.
``--background sequences`` scores against the composition of the input instead of the uniform background: a first pass
over the FASTA file (with the chosen ``--ingest``) makes every chunk a resident set, adds its
``StripedSequenceSet.count_symbols()`` -- counted on the device -- into one total and drops the set; the background is
``background_from_counts(total)`` (abc.rs:441-456, the unknown symbol left out), the matrices are
``to_freq(0.1).to_scoring(background)`` (pwm/mod.rs:415-430), and thresholds and the ``pvalue`` column come from the
distributions of THOSE matrices.  The second pass scans as before.  ``--composition PATH`` writes, during the scan pass,
one TSV line per record: ``seq_index seq_name length`` and one count per symbol in alphabet order (``A C T G N``).
``--matched`` appends a ninth column ``matched``: the text of the hit's window, reverse-complemented for strand ``-`` (FIMO's
``matched_sequence``).  ``--site-matrices PATH`` writes one JASPAR-2016 record per motif with the counts over all its hits
in all sets (``CountMatrix::from_sequences`` of the ``matched`` strings, pwm/mod.rs:209-237); motifs without hits get zeros.
Both read the windows out of the resident set (``StripedSequenceSet.windows`` / ``count_sites``: one call per set and
strand; for ``-`` the count table of the reverse matrix's sites is reverse-complemented, pwm/mod.rs:313-321) -- with
``--ingest device`` the host never held the text -- and with ``--best`` the best windows are the sites.
``--variants PATH`` scores single-symbol variants instead of scanning (``Pipeline.scan_variant_hits_set``, one call per set
and strand).  The file is TSV ``seq_name  pos(1-based)  ref  alt`` with single letters; ``#`` lines and blank lines are
ignored.  ``-o`` receives one line per (variant, motif, strand) with a site on at least one allele -- the best window that
covers the position reaches the motif's threshold for ``ref`` or for ``alt`` --
``seq_index seq_name pos ref alt motif_index motif_name strand ref_pos ref_score alt_pos alt_score``, ordered by sequence,
then variant in file order, then strand, then motif; ``ref_pos`` / ``alt_pos`` are window starts as the hit table's ``pos``,
and an allele without a window prints ``.`` for both.  Exit status 2 with a message that names the line: a ``ref`` that is
not the resident symbol, multi-letter alleles, a non-numeric or zero ``pos`` or one behind the record's end, and, after the
pass, a ``seq_name`` no record carried.  It excludes ``--best``, ``--counts``, ``--matched`` and ``--site-matrices``.
``--regions BED`` scans regions of the records instead of the records: the FASTA is ingested as before, and each resident
set is replaced, before any scan, by the set of the BED rows that name one of its records, cut out on the device
(``StripedSequenceSet.regions``; ``-`` rows as reverse complements, coordinates clipped to the record).  ``--flank N``
extends every region by N symbols on both sides, ``--resize W`` centres a window of W symbols on its midpoint.  The output
is that of a run WITHOUT ``--regions`` on a FASTA file of the extracted regions: a region's record is called by its BED
name (column 4) or ``chrom:start-end`` -- the coordinates asked for, after ``--flank`` / ``--resize`` -- with ``(-)`` behind a
minus-strand region; positions are relative to the region as extracted; within a resident set the regions stand in file
order, and a row whose chromosome no record carries is exit status 2 after the pass.  It excludes ``--variants``
(variant coordinates would need remapping).
``--null order0|order1`` scans a CONTROL instead of the input: each resident set (after ``--regions``, if given) is replaced,
before any scan, by ``StripedSequenceSet.null`` of itself -- records of the same names and lengths drawn on the device.
``order0`` draws every record i.i.d. from its own composition (``N`` included); the generator numbers a record by its index
in the whole input, so the output does not depend on ``--batch-bases``.  ``order1`` fits ONE first-order Markov chain per
resident set, i.e. per ``--batch-bases`` chunk.  ``--null-seed N`` (default 0) seeds the generator.  It excludes
``--variants``, ``--matched`` and ``--site-matrices``, which ask about the real text.
``--reverse`` also scans the reverse-complement matrix and reports strand ``-``
(main.rs:343-362).  There is no CPU path: without a gfx950 device the scan fails.
"""
from __future__ import annotations

import argparse
import contextlib
import gzip
import itertools
import math
import sys
from typing import BinaryIO, Iterator, List, Optional, Sequence, TextIO, Tuple

import numpy as np

from . import io as lmio
from .lib import (DNA_SYMBOLS, CountMatrix, MotifBatch, Pipeline, ScoringMatrix, StripedSequence, StripedSequenceSet, background_from_counts,
                  fasta_names)

DEFAULT_BATCH_BASES = 100_000_000


def _open_text(path: str) -> TextIO:
    with open(path, "rb") as fh:                     # main.rs:424-436: sniff the gzip magic
        magic = fh.read(2)
    return gzip.open(path, "rt") if magic == b"\x1f\x8b" else open(path, "r")


def _open_bytes(path: str) -> BinaryIO:
    with open(path, "rb") as fh:                     # the same sniff, the bytes as they are
        magic = fh.read(2)
    return gzip.open(path, "rb") if magic == b"\x1f\x8b" else open(path, "rb")


def fasta_chunks(handle: BinaryIO, budget: int) -> Iterator[bytes]:
    """Cuts the bytes of a FASTA file into consecutive chunks that concatenate to the file.  Every chunk after the first
    starts at a ``>`` that follows a ``\\n``, i.e. at a record; a chunk holds at most ``budget`` bytes -- unless one record
    alone is longer, which then stands alone (text in front of the first header goes with the first record).  The cuts are
    found with ``bytes.find`` / ``rfind`` and depend on the content alone, not on how the handle delivers it."""
    if budget < 1:
        raise ValueError("the byte budget of a chunk must be positive")
    block = max(budget, 1 << 16)
    buf, eof, first = b"", False, True
    while True:
        while not eof and len(buf) <= budget + 1:    # a record start at byte `budget` shows in budget + 1 bytes
            more = handle.read(block)
            if more:
                buf += more
            else:
                eof = True
        if not buf:
            return
        if eof and len(buf) <= budget:
            cut = len(buf)
        else:
            i = buf.rfind(b"\n>", 0, budget + 1)      # the last record start the budget reaches
            if i < 0:                                # none: one record longer than the budget, up to the next start
                skip = first and buf[:1] != b">"
                at = 0
                while True:
                    i = buf.find(b"\n>", at)
                    if i >= 0 and skip:
                        skip, at = False, i + 1
                        continue
                    if i >= 0 or eof:
                        break
                    at = max(len(buf) - 1, at)
                    more = handle.read(block)
                    if more:
                        buf += more
                    else:
                        eof = True
            cut = i + 1 if i >= 0 else len(buf)
        yield buf[:cut]
        buf, first = buf[cut:], False


def read_fasta(handle: TextIO) -> Iterator[Tuple[str, str]]:
    """(name, sequence) per record; name = the header up to the first whitespace."""
    name, chunks = None, []
    for line in handle:
        if line.startswith(">"):
            if name is not None:
                yield name, "".join(chunks)
            head = line[1:].strip()
            name, chunks = (head.split()[0] if head else ""), []
        elif name is not None:
            chunks.append(line.strip())
    if name is not None:
        yield name, "".join(chunks)


def _fmt_score(x) -> str:                            # Rust `{}` of an f32: shortest round-trip digits
    return np.format_float_positional(np.float32(x), unique=True, trim="-")


def _fmt_exp(x) -> str:                              # Rust `{:e}` of an f32
    return np.format_float_scientific(np.float32(x), unique=True, trim="-", exp_digits=1).replace("e+", "e")


def thresholds_for(pssms: Sequence[ScoringMatrix], pvalue: Optional[float], rel: Optional[float],
                   absolute: Optional[float]) -> List[float]:
    out = []
    for p in pssms:
        if pvalue is not None:
            out.append(p.score_for_pvalue(pvalue))
        elif rel is not None:
            out.append(float(np.float32(p.max_score()) * np.float32(rel)))
        elif absolute is not None:
            out.append(float(absolute))
        else:
            out.append(p.score_for_pvalue(1e-5))
    return out


def scan_record(pli: Pipeline, seq: StripedSequence, pssms: Sequence[ScoringMatrix],
                thresholds: Sequence[float]):
    """Per motif: (positions ascending, scores) with ``score >= t`` and ``pos + M <= L`` (scan.rs:185-190)."""
    rows, length = seq.rows, len(seq)
    out = []
    for (coords, values), p in zip(pli.scan_threshold_batch(pssms, thresholds, seq), pssms):
        pos = coords[:, 1] * rows + coords[:, 0]
        keep = pos + len(p) <= length
        pos, values = pos[keep], values[keep]
        order = np.argsort(pos, kind="stable")
        out.append((pos[order], values[order]))
    return out


def batch_records(lengths: Sequence[int], budget: int) -> List[Tuple[int, int]]:
    """Cuts a list of record lengths into consecutive sets ``[first, end)`` of at most ``budget`` bases each, in order,
    every record in exactly one set.  A set is closed when the next record would take it over the budget -- unless it
    holds no base yet, so a record larger than the budget stands alone (with the empty records right in front of it)
    instead of being refused.  Empty records never close a set that still has room."""
    if budget < 1:
        raise ValueError("the base budget of a set must be positive")
    sets, first, bases = [], 0, 0
    for i, n in enumerate(lengths):
        if bases > 0 and bases + n > budget:
            sets.append((first, i))
            first, bases = i, 0
        bases += n
    if first < len(lengths):
        sets.append((first, len(lengths)))
    return sets


def scan_set(pli: Pipeline, seqset: StripedSequenceSet, batch: MotifBatch):
    """All motifs x all records of a set: ``(record, motif, position, score)`` arrays ordered by record, then motif, then
    position, and ``bounds`` with record r's hits at ``[bounds[r], bounds[r + 1])``."""
    res = pli.scan_threshold_set(batch, None, seqset)
    motif = np.repeat(np.arange(len(res), dtype=np.int64), np.asarray(res.counts, dtype=np.int64))
    rec, pos, score = res.hits["record"], res.hits["position"], res.hits["score"]
    order = np.argsort(rec, kind="stable")        # the list is (motif, record, position): a stable sort by record is all
    rec = rec[order]
    bounds = np.searchsorted(rec, np.arange(len(seqset) + 1))
    return motif[order], pos[order], score[order], bounds


def best_set(pli: Pipeline, seqset: StripedSequenceSet, batch: MotifBatch):
    """The best window of every motif in every record of a set, in the form of ``scan_set``: one entry per (record, motif)
    that has a window, ordered by record, then motif."""
    res = pli.scan_best_set(batch, seqset)
    rec, motif = np.nonzero(res.found.T)           # row-major over (record, motif): the order of the table
    bounds = np.searchsorted(rec, np.arange(len(seqset) + 1))
    return motif.astype(np.int64), res.position[motif, rec], res.score[motif, rec], bounds


def sites_by_motif(motif: np.ndarray, pos: np.ndarray, bounds: np.ndarray, n_motifs: int):
    """The hits of ``scan_set`` / ``best_set`` (ordered by record) as the sites ``windows`` and ``count_sites`` take: per motif
    a pair of (record, position) arrays, and ``order`` / ``starts`` with motif i's sites at ``order[starts[i]:starts[i + 1]]``
    of the hit arrays."""
    rec = np.repeat(np.arange(len(bounds) - 1, dtype=np.int64), np.diff(bounds))
    order = np.argsort(motif, kind="stable")
    starts = np.concatenate(([0], np.cumsum(np.bincount(motif, minlength=n_motifs)))).astype(np.int64)
    rec, pos = rec[order], pos[order]
    return [(rec[a:b], pos[a:b]) for a, b in zip(starts[:-1], starts[1:])], order, starts


def window_text(win: np.ndarray, reverse: bool) -> np.ndarray:
    """A ``(count, width)`` array of DNA symbol indices as ``count`` strings; ``reverse``: reverse-complemented."""
    if reverse:
        win = np.array([2, 3, 0, 1, 4], dtype=np.uint8)[win[:, ::-1]]
    letters = np.ascontiguousarray(np.frombuffer(DNA_SYMBOLS.encode("ascii"), dtype=np.uint8)[win])
    return letters.view(f"S{win.shape[1]}").reshape(-1).astype(str)


class VariantFileError(ValueError):
    """A line of the ``--variants`` file that cannot be used; the message names it."""


def read_variants(handle: TextIO, path: str) -> List[Tuple[int, str, int, int, int]]:
    """The ``--variants`` file: TSV ``seq_name  pos(1-based)  ref  alt``; ``#`` lines and blank lines are ignored.  Returns
    ``(line number, seq_name, pos, ref symbol, alt symbol)`` per variant, in file order; ``VariantFileError`` names the line
    of a multi-letter or unknown allele and of a non-numeric or zero ``pos``."""
    out = []
    for number, line in enumerate(handle, 1):
        text = line.strip()
        if not text or text.startswith("#"):
            continue
        fields = text.split()
        if len(fields) != 4:
            raise VariantFileError(f"{path}:{number}: expected `seq_name pos ref alt`, found {len(fields)} fields")
        name, pos, ref, alt = fields
        if not pos.isdigit() or int(pos) == 0:
            raise VariantFileError(f"{path}:{number}: pos `{pos}` is not a 1-based position")
        symbols = []
        for what, allele in (("ref", ref), ("alt", alt)):
            if len(allele) != 1:
                raise VariantFileError(f"{path}:{number}: {what} `{allele}` is not a single letter (indels and multi-symbol "
                                       "substitutions are out of scope)")
            if allele.upper() not in DNA_SYMBOLS:
                raise VariantFileError(f"{path}:{number}: {what} `{allele}` is not one of {DNA_SYMBOLS}")
            symbols.append(DNA_SYMBOLS.index(allele.upper()))
        out.append((number, name, int(pos), symbols[0], symbols[1]))
    return out


def variant_lines(pli: Pipeline, seqset: StripedSequenceSet, names: Sequence[str], first_index: int, by_name: dict, variants: Sequence,
                  batches: Sequence[Tuple[str, MotifBatch]], motif_names: Sequence[str], path: str, seen: set) -> List[str]:
    """The ``--variants`` lines of one resident set: every variant whose ``seq_name`` a record of the set carries goes to
    ``Pipeline.scan_variant_hits_set`` once per strand; lines by record, then variant in file order, then strand, then
    motif.  ``VariantFileError`` for a ``pos`` behind the record's end and for a ``ref`` that is not the resident symbol."""
    rec, which = [], []
    for r, name in enumerate(names):
        for vi in by_name.get(name, ()):
            rec.append(r)
            which.append(vi)
        if name in by_name:
            seen.add(name)
    if not rec:
        return []
    lengths = seqset.lengths
    pos = np.array([variants[vi][2] - 1 for vi in which], dtype=np.int64)
    alt = np.array([variants[vi][4] for vi in which], dtype=np.uint8)
    rec = np.array(rec, dtype=np.int64)
    for j in np.flatnonzero(pos >= lengths[rec]):
        number, name, p = variants[which[j]][:3]
        raise VariantFileError(f"{path}:{number}: pos {p} lies behind the end of `{name}` ({int(lengths[rec[j]])} symbols)")
    found = [(strand, pli.scan_variant_hits_set(batch, None, seqset, rec, pos, alt)) for strand, batch in batches]
    resident = found[0][1].ref_symbol
    for j in np.flatnonzero(resident != np.array([variants[vi][3] for vi in which], dtype=np.uint8)):
        number, name, p, ref = variants[which[j]][:4]
        raise VariantFileError(f"{path}:{number}: ref `{DNA_SYMBOLS[ref]}` disagrees with `{DNA_SYMBOLS[int(resident[j])]}` at "
                               f"position {p} of `{name}`")
    rows = []                                           # (variant of the set, strand, motif, line)
    for si, (strand, hits) in enumerate(found):
        for mi in range(len(hits)):
            for v, rs, as_, rp, ap_ in hits[mi].tolist():
                _, name, p, ref, a = variants[which[v]]
                sides = "\t".join(f"{q}\t{_fmt_score(s)}" if q >= 0 else ".\t." for q, s in ((rp, rs), (ap_, as_)))
                rows.append((v, si, mi, f"{first_index + int(rec[v]) + 1}\t{name}\t{p}\t{DNA_SYMBOLS[ref]}\t{DNA_SYMBOLS[a]}\t{mi + 1}\t"
                                         f"{motif_names[mi]}\t{strand}\t{sides}\n"))
    rows.sort(key=lambda row: row[:3])
    return [row[3] for row in rows]


NULL_ORDERS = {"order0": 0, "order1": 1}


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="lightmotif_amd.scan_cli", description=__doc__.split("\n\n")[0])
    ap.add_argument("-m", "--matrices", required=True, help="JASPAR-2016 count matrices (optionally gzipped)")
    ap.add_argument("-s", "--sequences", required=True, help="FASTA file (optionally gzipped)")
    ap.add_argument("-o", "--output", required=True, help="TSV file to write")
    group = ap.add_mutually_exclusive_group()
    group.add_argument("-P", "--pvalue", type=float)
    group.add_argument("--abs-threshold", type=float)
    group.add_argument("--rel-threshold", type=float)
    ap.add_argument("--reverse", action="store_true", help="also scan the reverse-complement matrices")
    ap.add_argument("--best", action="store_true",
                    help="write the best window of every motif in every record instead of the hits above a threshold")
    ap.add_argument("--counts", action="store_true",
                    help="write the number of hits of every motif in every record instead of the hits (needs -P, "
                         "--abs-threshold or --rel-threshold)")
    ap.add_argument("--sum-odds", action="store_true",
                    help="write the sum of 2 ** score over the windows of every motif in every record instead of the hits")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--batch-bases", type=int, default=DEFAULT_BATCH_BASES,
                    help="bases of sequence gathered into one resident set and scanned with one call per strand "
                         "(a longer record is a set of its own); with --ingest device: bytes of FASTA text per set")
    ap.add_argument("--ingest", choices=("device", "host"), default="device",
                    help="where the FASTA container is parsed: on the device from the file's bytes (default), or by the "
                         "line-by-line reader on the host")
    ap.add_argument("--pvalues", choices=("device", "host"), default="device",
                    help="where p-values become thresholds and scores become p-values: from score distributions built "
                         "on the device for all motifs at once (default), or motif by motif and hit by hit on the host")
    ap.add_argument("--background", choices=("uniform", "sequences"), default="uniform",
                    help="background frequencies of the scoring matrices and their score distributions: uniform (default), "
                         "or the composition of the input, counted on the device in a first pass over the file")
    ap.add_argument("--composition", metavar="PATH",
                    help="also write a TSV with one line per record: seq_index, seq_name, length and the count of every symbol")
    ap.add_argument("--matched", action="store_true",
                    help="append a column `matched`: the text of the hit's window, reverse-complemented for strand -")
    ap.add_argument("--site-matrices", metavar="PATH",
                    help="also write a JASPAR-2016 file with, per motif, the count matrix of all its hits' windows")
    ap.add_argument("--variants", metavar="PATH",
                    help="score single-symbol variants (TSV: seq_name, 1-based pos, ref, alt) instead of scanning: one line per "
                         "(variant, motif, strand) with a site on at least one allele")
    ap.add_argument("--null", choices=sorted(NULL_ORDERS),
                    help="scan a control instead of the input: every resident set is replaced by a set of the same names and lengths "
                         "drawn on the device -- order0: every record i.i.d. from its own composition (N included), so the output "
                         "does not depend on --batch-bases; order1: a first-order Markov chain, ONE chain fitted per resident set "
                         "(per --batch-bases chunk).  Excludes --variants, --matched and --site-matrices, which ask about the real text")
    ap.add_argument("--null-seed", type=int, default=0, metavar="N", help="with --null: the seed of the generator (default 0)")
    ap.add_argument("--regions", metavar="BED",
                    help="scan regions of the FASTA records instead of the records: a BED file (chrom, 0-based start, end, "
                         "optional name and strand), cut out of each resident set on the device")
    ap.add_argument("--refine", type=int, metavar="N",
                    help="before scanning, refine every motif on the input by N iterations of EM on the device (expected site "
                         "counts of all windows, then new matrices) and write the result to --refined; the input has to fit one "
                         "resident set (--batch-bases); the scan itself uses the matrices as loaded")
    ap.add_argument("--refine-model", choices=("oops", "zoops"), default="oops",
                    help="with --refine: one site per record (oops, default) or zero or one (zoops)")
    ap.add_argument("--refined", metavar="PATH",
                    help="with --refine: the JASPAR-2016 file of the refined motifs, per motif the expected site counts of the last "
                         "iteration rounded to integers")
    resize = ap.add_mutually_exclusive_group()
    resize.add_argument("--flank", type=int, metavar="N", help="with --regions: extend every region by N symbols on both sides")
    resize.add_argument("--resize", type=int, metavar="W", help="with --regions: a window of W symbols centred on every region's midpoint")
    return ap


def region_names(chroms: Sequence[str], starts: Sequence[int], ends: Sequence[int], strands: Sequence[int],
                 names: Sequence[Optional[str]]) -> List[str]:
    """What a region's record is called: its BED name, or ``chrom:start-end`` with the coordinates asked for (after
    ``--flank`` / ``--resize``, before clipping) and ``(-)`` behind a minus-strand region."""
    return [name if name is not None else f"{c}:{s}-{e}" + ("(-)" if strand else "")
            for c, s, e, strand, name in zip(chroms, starts, ends, strands, names)]


def log2_mean_odds(total: float, windows: int) -> float:
    """``log2(total / windows)`` of a ``--sum-odds`` line: -inf for a total of 0, +inf for one of +inf."""
    mean = total / windows
    return math.log2(mean) if 0.0 < mean < math.inf else (-math.inf if mean == 0.0 else mean)


def refined_counts(expected: np.ndarray) -> CountMatrix:
    """The count matrix ``--refined`` writes for a motif: its expected site counts rounded to the nearest integer (ties to
    even), the form the JASPAR-2016 format holds."""
    return CountMatrix(np.rint(expected).astype(np.uint32))


def hit_pvalues(dists, motif: np.ndarray, score: np.ndarray) -> np.ndarray:
    """The p-value of every hit of a set in one ``ScoreDistributions.pvalues`` call: the hits come ordered by record, the
    call takes them grouped by motif, so they are sorted by motif on the way in and put back on the way out."""
    order = np.argsort(motif, kind="stable")
    counts = np.bincount(motif, minlength=len(dists))
    out = np.empty(len(motif), dtype=np.float64)
    out[order] = dists.pvalues(counts, np.ascontiguousarray(score[order], dtype=np.float32))
    return out


def main(argv: Optional[Sequence[str]] = None) -> int:
    ap = build_parser()
    args = ap.parse_args(argv)

    print("Loading matrices")
    with _open_text(args.matrices) as fh:
        records = list(lmio.read(fh))
    lengths = [len(r.matrix) for r in records]
    print(f"Loaded {len(records)} matrices (M={min(lengths, default=0)}..{max(lengths, default=0)})")
    print("Preparing motifs")
    if args.batch_bases < 1:
        ap.error("--batch-bases must be positive")
    if args.counts:
        if args.pvalue is None and args.abs_threshold is None and args.rel_threshold is None:
            ap.error("--counts needs a threshold: one of -P, --abs-threshold, --rel-threshold")
        if args.best or args.matched or args.site_matrices:
            ap.error("--counts excludes --best, --matched and --site-matrices")
    if args.sum_odds and (args.best or args.counts or args.variants or args.matched or args.site_matrices):
        ap.error("--sum-odds excludes --best, --counts, --variants, --matched and --site-matrices")
    if args.null is not None and (args.variants or args.matched or args.site_matrices):
        ap.error("--null excludes --variants, --matched and --site-matrices: those ask about the real text")
    if args.null_seed < 0:
        ap.error("--null-seed is not negative")
    if (args.flank is not None or args.resize is not None) and not args.regions:
        ap.error("--flank and --resize need --regions")
    if args.regions and args.variants:
        ap.error("--regions excludes --variants: variant coordinates would have to be remapped to the regions")
    if (args.flank is not None and args.flank < 0) or (args.resize is not None and args.resize < 0):
        ap.error("--flank and --resize take a non-negative number of symbols")
    if (args.refine is None) != (args.refined is None):
        ap.error("--refine and --refined go together")
    if args.refine is not None and args.refine < 1:
        ap.error("--refine takes a positive number of iterations")
    bed_by_chrom: dict = {}
    if args.regions:
        try:
            rows = list(lmio.bed_rows(args.regions, args.regions))
        except (ValueError, OSError) as e:
            ap.error(str(e))
        if rows and (args.flank is not None or args.resize is not None):
            s, e = lmio.resize_regions([r[2] for r in rows], [r[3] for r in rows], flank=args.flank, width=args.resize)
            rows = [(r[0], r[1], int(a), int(b), r[4], r[5]) for r, a, b in zip(rows, s.tolist(), e.tolist())]
        for i, row in enumerate(rows):
            bed_by_chrom.setdefault(row[1], []).append((i,) + row)
    bed_seen: set = set()
    variants = None
    if args.variants:
        if args.best or args.counts or args.matched or args.site_matrices:
            ap.error("--variants excludes --best, --counts, --matched and --site-matrices")
        try:
            with _open_text(args.variants) as fh:
                variants = read_variants(fh, args.variants)
        except VariantFileError as e:
            ap.error(str(e))
    pli = Pipeline.hip(args.device)

    def sets() -> Iterator[Tuple[int, List[str], StripedSequenceSet]]:
        """One pass over the input, as it stands or -- with --null -- every set replaced by its control: same names, same
        lengths; the record number of the generator is the record's index in the whole input."""
        if args.null is None:
            yield from input_sets()
            return
        for first, names, seqset in input_sets():
            yield first, names, seqset.null(NULL_ORDERS[args.null], seed=args.null_seed, record_base=first)

    def input_sets() -> Iterator[Tuple[int, List[str], StripedSequenceSet]]:
        """One pass over the input: (index of the first record, names, resident set) per chunk -- of the FASTA records, or
        with --regions of the regions cut out of them."""
        if not args.regions:
            yield from record_sets()
            return
        first = 0
        bed_seen.clear()
        for _, names, seqset in record_sets():
            picked = []                                  # (row of the file, record of the set, start, end, name, strand)
            for r, name in enumerate(names):
                if name in bed_by_chrom and name not in bed_seen:     # (the first record of a name, as read_bed)
                    bed_seen.add(name)
                    picked.extend((i, r, s, e, label, strand) for i, _, _, s, e, label, strand in bed_by_chrom[name])
            if not picked:
                continue
            picked.sort()
            rec, starts, ends = [p[1] for p in picked], [p[2] for p in picked], [p[3] for p in picked]
            strands = [p[5] for p in picked]
            derived, _ = seqset.regions(rec, np.array(starts, dtype=np.int64), np.array(ends, dtype=np.int64),
                                        np.array(strands, dtype=np.uint8))
            yield first, region_names([names[r] for r in rec], starts, ends, strands, [p[4] for p in picked]), derived
            first += len(picked)

    def record_sets() -> Iterator[Tuple[int, List[str], StripedSequenceSet]]:
        """One pass over the FASTA file: (index of the first record, names, resident set) per chunk."""
        with (_open_bytes if args.ingest == "device" else _open_text)(args.sequences) as fasta:
            if args.ingest == "device":
                first = 0
                for chunk in fasta_chunks(fasta, args.batch_bases):
                    seqset = pli.stripe_fasta_set(chunk, lossy=True)
                    names = fasta_names(chunk, seqset.header_spans)
                    if names:
                        yield first, names, seqset
                    first += len(names)
            else:
                # the rule of batch_records, applied as the records stream in
                first, names, texts, bases = 0, [], [], 0
                for name, text in read_fasta(fasta):
                    if bases > 0 and bases + len(text) > args.batch_bases:
                        yield first, names, pli.stripe_ascii_set(texts, lossy=True)
                        first, names, texts, bases = first + len(names), [], [], 0
                    names.append(name)
                    texts.append(text)
                    bases += len(text)
                if names:
                    yield first, names, pli.stripe_ascii_set(texts, lossy=True)

    if args.background == "sequences":
        total = np.zeros(len(DNA_SYMBOLS), dtype=np.int64)
        for _, _, seqset in sets():
            total += seqset.count_symbols().sum(axis=0)
        try:
            background = background_from_counts(total, unknown=False)          # abc.rs:441-456
        except ValueError:
            ap.error(f"--background sequences: {args.sequences} holds no base to count")
        direct = [r.matrix.to_scoring(0.1, background) for r in records]       # pwm/mod.rs:240-258, 415-430
    else:
        direct = [r.matrix.normalize(0.1).log_odds() for r in records]
    dists = pli.score_distributions(direct) if args.pvalues == "device" else None
    if dists is not None and args.rel_threshold is None and args.abs_threshold is None:
        thresholds = dists.thresholds(1e-5 if args.pvalue is None else args.pvalue).tolist()   # main.rs:479-489
    else:
        thresholds = thresholds_for(direct, args.pvalue, args.rel_threshold, args.abs_threshold)
    strands = [("+", direct)]
    if args.reverse:
        strands.append(("-", [p.reverse_complement() for p in direct]))
    max_m = max(lengths, default=0)
    batches = [(strand, pli.prepare_batch(pssms, thresholds)) for strand, pssms in strands]
    if args.refine is not None:
        resident = list(itertools.islice(sets(), 2))
        if len(resident) > 1:
            ap.error("--refine works on one resident set: the input is larger than --batch-bases")
        refined = [r.matrix for r in records]
        if resident and records:
            _, _, seqset = resident[0]
            seqset.configure_wrap(max_m)
            _, _, expected = pli.refine(direct, seqset, args.refine, model=args.refine_model, return_counts=True)
            refined = [refined_counts(e) for e in expected.counts]
        lmio.write([lmio.Record(r.id, r.description, m) for r, m in zip(records, refined)], args.refined)
        print(f"Wrote {len(refined)} refined matrices to {args.refined}")
        del resident
    if variants is not None:
        by_name: dict = {}
        for vi, (_, name, _, _, _) in enumerate(variants):
            by_name.setdefault(name, []).append(vi)
        seen: set = set()
        n_lines = 0
        with open(args.output, "w") as out:
            out.write("seq_index\tseq_name\tpos\tref\talt\tmotif_index\tmotif_name\tstrand\tref_pos\tref_score\talt_pos\talt_score\n")
            try:
                for first, names, seqset in sets():
                    lines = variant_lines(pli, seqset, names, first, by_name, variants, batches, [r.id for r in records], args.variants,
                                          seen)
                    out.writelines(lines)
                    n_lines += len(lines)
            except VariantFileError as e:
                ap.error(str(e))
        for number, name, _, _, _ in variants:
            if name not in seen:
                ap.error(f"{args.variants}:{number}: no record is called `{name}`")
        print(f"Wrote {n_lines} lines to {args.output}")
        return 0
    n_hits = 0
    with contextlib.ExitStack() as files:
        out = files.enter_context(open(args.output, "w"))
        if args.counts:
            out.write("seq_index\tseq_name\tmotif_index\tmotif_name\tstrand\twindows\thits\n")
        elif args.sum_odds:
            out.write("seq_index\tseq_name\tmotif_index\tmotif_name\tstrand\twindows\tsum_odds\tlog2_mean_odds\n")
        else:
            out.write("seq_index\tseq_name\tmotif_index\tmotif_name\tpos\tstrand\tscore\tpvalue" + ("\tmatched" if args.matched else "") + "\n")
        site_totals = [np.zeros((m, len(DNA_SYMBOLS)), dtype=np.int64) for m in lengths] if args.site_matrices else None
        composition = files.enter_context(open(args.composition, "w")) if args.composition else None
        if composition is not None:
            composition.write("seq_index\tseq_name\tlength\t" + "\t".join(DNA_SYMBOLS) + "\n")

        def write_composition(first_index: int, names: List[str], seqset: StripedSequenceSet) -> None:
            table = seqset.count_symbols().tolist()
            for r, (name, length) in enumerate(zip(names, seqset.lengths.tolist())):
                composition.write(f"{first_index + r + 1}\t{name}\t{length}\t" + "\t".join(map(str, table[r])) + "\n")

        def write_counts(first_index: int, names: List[str], seqset: StripedSequenceSet) -> int:
            seqset.configure_wrap(max_m)                                   # main.rs:543
            tables = [(strand, pli.scan_count_set(batch, thresholds, seqset)) for strand, batch in batches]
            if composition is not None:
                write_composition(first_index, names, seqset)
            wrote = 0
            for r, name in enumerate(names):
                for strand, res in tables:
                    windows, hits = res.windows[:, r].tolist(), res.counts[:, 0, r].tolist()
                    for mi, (w, h) in enumerate(zip(windows, hits)):
                        if w > 0:
                            out.write(f"{first_index + r + 1}\t{name}\t{mi + 1}\t{records[mi].id}\t{strand}\t{w}\t{h}\n")
                            wrote += 1
            return wrote

        def write_sums(first_index: int, names: List[str], seqset: StripedSequenceSet) -> int:
            seqset.configure_wrap(max_m)                                   # main.rs:543
            tables = [(strand, pli.scan_sum_set(batch, seqset)) for strand, batch in batches]
            if composition is not None:
                write_composition(first_index, names, seqset)
            wrote = 0
            for r, name in enumerate(names):
                for strand, res in tables:
                    windows, sums = res.windows[:, r].tolist(), res.sums[:, r].tolist()
                    for mi, (w, total) in enumerate(zip(windows, sums)):
                        if w > 0:
                            out.write(f"{first_index + r + 1}\t{name}\t{mi + 1}\t{records[mi].id}\t{strand}\t{w}\t{total!r}\t"
                                      f"{log2_mean_odds(total, w)!r}\n")
                            wrote += 1
            return wrote

        def write_set(first_index: int, names: List[str], seqset: StripedSequenceSet) -> int:
            seqset.configure_wrap(max_m)                                   # main.rs:543
            found = [(strand, (best_set if args.best else scan_set)(pli, seqset, batch)) for strand, batch in batches]
            # either strand looks the DIRECT matrix's distribution up (main.rs:335)
            pvalues = [None if dists is None else hit_pvalues(dists, motif, score) for _, (motif, _, score, _) in found]
            if composition is not None:
                write_composition(first_index, names, seqset)
            # the windows of the hits, read out of the resident set: one call per strand, whatever the number of hits
            matched = [None] * len(found)
            if args.matched or site_totals is not None:
                for si, (strand, (motif, pos, _, bounds)) in enumerate(found):
                    sites, order, starts = sites_by_motif(motif, pos, bounds, len(records))
                    if args.matched:
                        matched[si] = np.empty(len(motif), dtype=object)
                        for mi, (win, _) in enumerate(seqset.windows(sites, lengths)):
                            matched[si][order[starts[mi]:starts[mi + 1]]] = window_text(win, strand == "-")
                    if site_totals is not None:
                        for total, mat in zip(site_totals, seqset.count_sites(sites, lengths)[0]):
                            total += (mat.reverse_complement() if strand == "-" else mat).data     # pwm/mod.rs:313-321
            wrote = 0
            for r, name in enumerate(names):
                for (strand, (motif, pos, score, bounds)), pvs, texts in zip(found, pvalues, matched):
                    a, b = int(bounds[r]), int(bounds[r + 1])
                    pv = [None] * (b - a) if pvs is None else pvs[a:b].tolist()
                    tail = [""] * (b - a) if texts is None else ["\t" + t for t in texts[a:b].tolist()]
                    for mi, p, s, q, t in zip(motif[a:b].tolist(), pos[a:b].tolist(), score[a:b].tolist(), pv, tail):
                        if q is None:
                            q = direct[mi].score_distribution.pvalue(s)   # main.rs:335: motif.dist
                        out.write(f"{first_index + r + 1}\t{name}\t{mi + 1}\t{records[mi].id}\t{p}\t{strand}\t{_fmt_score(s)}\t"
                                  f"{_fmt_exp(q)}{t}\n")
                    wrote += b - a
            return wrote

        for first, names, seqset in sets():
            n_hits += (write_counts if args.counts else write_sums if args.sum_odds else write_set)(first, names, seqset)
        for chrom, rows in bed_by_chrom.items():
            if chrom not in bed_seen:
                ap.error(f"{args.regions}:{rows[0][1]}: no record is called `{chrom}`")
        if site_totals is not None:
            if any(int(t.max(initial=0)) > 0xFFFFFFFF for t in site_totals):
                raise OverflowError("--site-matrices: a site count exceeds the u32 of a count matrix")
            lmio.write([lmio.Record(r.id, r.description, CountMatrix(t)) for r, t in zip(records, site_totals)], args.site_matrices)
    print(f"Wrote {n_hits} {'lines' if args.counts or args.sum_odds else 'hits'} to {args.output}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
