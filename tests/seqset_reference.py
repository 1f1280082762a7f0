"""A reference for scans over a sequence set that never touches the GPU library, and the seeded generator of the cases
the set fuzz (tests/test_gpu_seqset_fuzz.py) and the test that pins this reference (tests/test_seqset_reference.py) share.

The reference scores every window of the CONCATENATION of the records with one ``window_scores`` call per motif (M
sequential f32 adds from +0.0 in row order) and keeps position ``p`` when ``p + M <= end of the record holding p``
(``segment_rule``).  A window's score depends only on its M symbols, so a kept window scores bit for bit as it does in the
record alone.  From the kept windows come the hit list of a threshold and the best window per record.  Text goes to
symbols through a table of this file's own."""
from dataclasses import dataclass, field
from typing import List

import numpy as np

from fasta_cases import fasta, lines
from seqset_best_cases import window_scores
from seqset_rule import offsets_of, segment_rule

SYMBOLS = {False: b"ACTGN", True: b"ACDEFGHIKLMNPQRSTVWYX"}
JUNK = np.frombuffer(b"?*-.>acgtnx#\x80\xff", dtype=np.uint8)      # none of them a symbol or FASTA white space
RECORD_COUNTS = (0, 1, 2, 3, 7, 40, 300, 4097)                     # 4 097: offsets beyond the 4 095 records that fit LDS
THRESHOLD_KINDS = ("min", "median", "q99", "max", "above", "-inf", "+inf", "nan")
MATRIX_KINDS = ("normal", "ties", "finite_default", "neg_inf_cells")
OPTION_SETS = ({}, {"multi_motif": 0}, {"pair_prefilter": 0}, {"sort_hits": 0}, {"chunked_fused": 0}, {"tiled": 0})
FIRST_RNG_SEED = 310_000


def stride(k):
    """Floats per row of a scoring matrix: 8 for DNA, 24 for protein."""
    return 8 if k == 5 else 24


def symbol_table(protein, lossy):
    """256 entries: byte -> symbol index; any other byte becomes the last symbol with ``lossy`` and 255 without."""
    k = len(SYMBOLS[protein])
    table = np.full(256, k - 1 if lossy else 255, dtype=np.uint8)
    table[np.frombuffer(SYMBOLS[protein], dtype=np.uint8)] = np.arange(k, dtype=np.uint8)
    return table


def encode_text(raw, protein, lossy=True):
    return symbol_table(protein, lossy)[np.frombuffer(bytes(raw), dtype=np.uint8)]


@dataclass
class Case:
    seed: int
    protein: bool
    k: int
    cols: int
    wrap: int
    mats: List[np.ndarray]            # (M, stride) f32 each
    kinds: List[str]
    has_nan: bool
    lengths: np.ndarray               # int64, one per record
    symbols: List[np.ndarray]         # uint8 per record: what every builder must end up with
    texts: List[bytes]                # ASCII per record, junk bytes included
    fasta: bytes
    threshold_kinds: List[str]
    rows_per_stream: int
    prefilter: bool
    options: dict
    thresholds: List[float] = field(default_factory=list)   # filled by ``reference``

    @property
    def offsets(self):
        return offsets_of(self.lengths)

    @property
    def total(self):
        return int(self.lengths.sum())

    @property
    def has_window(self):
        """Some motif fits some record."""
        return len(self.lengths) > 0 and int(self.lengths.max()) >= min(p.shape[0] for p in self.mats)


def make_matrix(rng, m, k, kind):
    """The matrix kinds of tests/test_gpu_fuzz.py."""
    p = np.zeros((m, stride(k)), np.float32)
    p[:, :k] = rng.integers(-3, 4, (m, k)) if kind == "ties" else rng.normal(0, 2, (m, k))
    if kind != "finite_default":
        p[:, k - 1] = -np.inf
    if kind == "neg_inf_cells":
        p[:, :k][rng.random((m, k)) < 0.05] = -np.inf
    return p


def draw_case(seed):
    """Everything seed ``seed`` scans, drawn from ONE generator."""
    rng = np.random.default_rng(FIRST_RNG_SEED + seed)
    protein = seed % 5 == 2
    k = 21 if protein else 5
    ms = [int(m) for m in rng.integers(1, 41, int(rng.integers(1, 7)))]
    if seed % 7 == 4:
        ms[0] = int(rng.integers(37, 131))               # the generic best-hit kernel; long, chunked, generic scans
    kinds = [str(rng.choice(MATRIX_KINDS)) for _ in ms]
    mats = [make_matrix(rng, m, k, kind) for m, kind in zip(ms, kinds)]
    has_nan = seed % 13 == 6
    if has_nan:
        p = mats[int(rng.integers(0, len(mats)))]
        p[int(rng.integers(0, p.shape[0])), int(rng.integers(0, k - 1))] = np.nan
    cols = int(rng.choice([1, 3, 16, 33])) if seed % 4 == 0 else 32
    wrap = max(ms) - 1 + int(rng.integers(0, 3))

    n_records = int(rng.choice(RECORD_COUNTS))
    pool = sorted({0, 1, 2, cols - 1, cols, cols + 1, 31, 32, 33, 64, 200} | {m + d for m in ms for d in (-1, 0, 1)})
    lengths = rng.choice(pool, n_records).astype(np.int64)
    if seed % 3 == 0 and n_records:                      # a record that spans columns and several lanes' runs
        lengths[int(rng.integers(0, n_records))] = int(rng.integers(500, 6001))
    total = int(lengths.sum())
    sym = rng.integers(0, k - 1, total).astype(np.uint8)
    if seed % 3:
        sym[rng.random(total) < 0.02] = k - 1            # N / X
    text = np.frombuffer(SYMBOLS[protein], dtype=np.uint8)[sym]
    junk = np.flatnonzero(rng.random(total) < 0.005)
    text[junk] = rng.choice(JUNK, len(junk))

    width = int(rng.choice([1, 7, 60, 61, 4096]))
    eol = b"\r\n" if rng.random() < 0.5 else b"\n"
    offs = offsets_of(lengths)
    local = np.arange(total, dtype=np.int64) - np.repeat(offs[:-1].astype(np.int64), lengths)
    text[(local % width == 0) & (text == ord(">"))] = ord("?")     # a '>' that opens a line would open a record
    sym = symbol_table(protein, True)[text]                          # junk: the last symbol
    cuts = [int(x) for x in offs]
    texts = [text[a:b].tobytes() for a, b in zip(cuts[:-1], cuts[1:])]
    symbols = [sym[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
    blank = rng.random(n_records)
    parts = []
    for r, t in enumerate(texts):
        if blank[r] < 0.05 and len(t) > width:           # a blank line between two lines of the record
            head = width * (1 + (len(t) - 1) // width // 2)
            parts.append(b">rec%d fuzz" % r + eol + lines(t[:head], width, eol) + eol + lines(t[head:], width, eol))
        else:
            parts.append(fasta([(b"rec%d fuzz" % r, t)], width, eol))
        if blank[r] > 0.9:                               # ... and behind it
            parts.append(eol)
    threshold_kinds = [str(rng.choice(THRESHOLD_KINDS)) for _ in ms]
    rows_per_stream = int(rng.choice([0, 0, 7, 33, 1000]))
    options = OPTION_SETS[int(rng.integers(0, len(OPTION_SETS)))]
    return Case(seed, protein, k, cols, wrap, mats, kinds, has_nan, lengths, symbols, texts, b"".join(parts), threshold_kinds,
                rows_per_stream, bool(seed % 4), dict(options))


@dataclass
class MotifWindows:
    """The windows of one motif that lie inside a record, ascending in (record, position)."""
    record: np.ndarray                # int64
    position: np.ndarray              # int64, inside the record
    score: np.ndarray                 # f32

    def hits(self, t):
        """(records, positions, scores) with ``score >= float32(t)``; NaN is never a hit."""
        with np.errstate(invalid="ignore"):
            sel = self.score >= np.float32(t)
        return self.record[sel], self.position[sel], self.score[sel]

    def best(self, n_records):
        """(found, position, score) per record: the greatest score, NaN windows never competing, the lowest position among
        equals; found false, position -1 and score NaN where no non-NaN window fits."""
        found = np.zeros(n_records, dtype=bool)
        position = np.full(n_records, -1, dtype=np.int64)
        score = np.full(n_records, np.nan, dtype=np.float32)
        live = ~np.isnan(self.score)
        rec, pos, val = self.record[live], self.position[live], self.score[live]
        if len(rec):
            order = np.lexsort((pos, -val.astype(np.float64), rec))       # record, score descending, position
            rec, pos, val = rec[order], pos[order], val[order]
            first = np.flatnonzero(np.concatenate(([True], rec[1:] != rec[:-1])))
            found[rec[first]], position[rec[first]], score[rec[first]] = True, pos[first], val[first]
        return found, position, score


def motif_windows(weights, concatenation, offsets):
    m = weights.shape[0]
    scores = window_scores(weights, concatenation)
    rec, local, keep = segment_rule(offsets, np.arange(len(scores), dtype=np.uint64), m)
    return MotifWindows(rec[keep], local[keep], scores[keep])


def threshold_of(kind, scores):
    """A threshold of one kind from the f32 scores it is compared with, so that equality is exact."""
    if kind in ("-inf", "+inf", "nan"):
        return {"-inf": -np.inf, "+inf": np.inf, "nan": np.nan}[kind]
    v = np.sort(scores[~np.isnan(scores)])
    if not len(v):
        return 0.0
    if kind == "min":
        return float(v[0])
    if kind == "median":
        return float(v[(len(v) - 1) // 2])
    if kind == "q99":
        return float(v[int(0.99 * (len(v) - 1))])
    if kind == "max":
        return float(v[-1])
    assert kind == "above"
    return float(np.nextafter(v[-1], np.float32(np.inf)))


def reference(case):
    """Per motif the ``MotifWindows``; fills ``case.thresholds`` from them."""
    cat = np.concatenate(case.symbols) if case.symbols else np.zeros(0, np.uint8)
    offs = case.offsets
    out = [motif_windows(p, cat, offs) for p in case.mats]
    case.thresholds = [threshold_of(kind, w.score) for kind, w in zip(case.threshold_kinds, out)]
    return out


def pvalues_of(dist, scores):
    """``dist.pvalue`` (lightmotif_amd/dist.py) of many finite f32 scores at once: float64."""
    x = (np.asarray(scores, dtype=np.float32).astype(np.float64) - dist._rows * dist._offset) * dist._scale
    scaled = np.clip(np.sign(x) * np.floor(np.abs(x) + 0.5), -2.0 ** 62, 2.0 ** 62).astype(np.int64)   # (far outside the table)
    out = dist.sf[np.clip(scaled, 0, len(dist.sf) - 1)].astype(np.float64)
    out[scaled < dist.min_score] = 1.0
    out[scaled >= len(dist.sf)] = 0.0
    return out
