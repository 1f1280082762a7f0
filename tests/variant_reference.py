"""A reference for the effects of single-symbol variants on the motifs of a sequence set that never touches the GPU library,
and the seeded generator of the variants the GPU test (tests/test_gpu_variants.py) and the test that pins this reference
(tests/test_variant_reference.py) share.

The reference slices ``symbols[r][lo : hi + M]`` with ``lo = max(0, p - M + 1)`` and ``hi = min(p, L - M)`` -- the windows
that cover ``p`` and lie inside the record -- scores the slice with ``seqset_best_cases.window_scores`` (M sequential f32
adds from +0.0 in row order), replaces one byte and scores it again.  Each allele's best window follows ``best_of``: the
greatest score under f32 ``>``, NaN windows never competing, the lowest start among equals."""
from dataclasses import dataclass
from functools import lru_cache
from types import SimpleNamespace

import numpy as np

from seqset_best_cases import best_of, window_scores
from seqset_reference import draw_case

FIRST_RNG_SEED = 920_000
VARIANT_COUNTS = (1, 63, 64, 65, 257, 1500)
INVALID_SHARE = 0.035
NONE = 0xFFFFFFFF                       # LM_HIP_VARIANT_NONE


@dataclass
class Variants:
    record: np.ndarray                  # uint64
    position: np.ndarray                # uint64
    alt: np.ndarray                     # uint8
    valid: np.ndarray                   # bool: record < records, position < L, alt < k

    def __len__(self):
        return len(self.record)

    def take(self, index):
        return Variants(self.record[index], self.position[index], self.alt[index], self.valid[index])


@dataclass
class Effects:
    ref_score: np.ndarray               # (n, V) f32, NaN for none
    alt_score: np.ndarray
    ref_back: np.ndarray                # (n, V) int64, position - start; NONE for none
    alt_back: np.ndarray
    ref_symbol: np.ndarray              # (V,) uint8, 0xFF for an invalid variant
    valid: np.ndarray                   # (V,) bool
    has_window: np.ndarray              # (n, V) bool: valid and L >= M

    def position(self, variants, side):
        """Record-relative window starts, -1 for none."""
        back = getattr(self, side + "_back")
        none = back == NONE
        return np.where(none, -1, variants.position.astype(np.int64).reshape(1, -1) - np.where(none, 0, back))


def validity(lengths, k, record, position, alt):
    lengths = np.asarray(lengths, dtype=np.uint64)
    ok = record < np.uint64(len(lengths))
    safe = np.minimum(record, np.uint64(max(len(lengths) - 1, 0))).astype(np.int64)
    length = lengths[safe] if len(lengths) else np.zeros(len(record), dtype=np.uint64)
    return ok & (position < length) & (alt < k)


def small_case(mats, symbols, protein=False):
    """What ``reference`` reads of a case, for hand-made inputs."""
    return SimpleNamespace(mats=mats, symbols=[np.asarray(s, dtype=np.uint8) for s in symbols], k=21 if protein else 5,
                           lengths=np.array([len(s) for s in symbols], dtype=np.int64), protein=protein)


def variants_of(case, record, position, alt):
    record, position = np.asarray(record, dtype=np.uint64), np.asarray(position, dtype=np.uint64)
    alt = np.asarray(alt, dtype=np.uint8)
    return Variants(record, position, alt, validity(case.lengths, case.k, record, position, alt))


def draw_variants(case, seed=None):
    """The variants seed ``case.seed`` asks about, drawn from ONE generator of their own."""
    rng = np.random.default_rng(FIRST_RNG_SEED + (case.seed if seed is None else seed))
    v = int(rng.choice(VARIANT_COUNTS))
    n, k = len(case.lengths), case.k
    ms = [p.shape[0] for p in case.mats]
    record = np.zeros(v, dtype=np.uint64)
    position = np.zeros(v, dtype=np.uint64)
    alt = rng.integers(0, k, v).astype(np.uint8)
    for i in range(v):
        if n == 0:
            record[i], position[i] = int(rng.integers(0, 2)), int(rng.integers(0, 3))
            continue
        r = int(rng.integers(0, n))
        length = int(case.lengths[r])
        record[i] = r
        if length == 0:
            position[i] = int(rng.integers(0, 2))
            continue
        if rng.random() < 0.5:
            pool = sorted({x for m in ms for x in (0, 1, m - 2, m - 1, m, length - m - 1, length - m, length - m + 1, length - 2,
                                                   length - 1) if 0 <= x < length})
            position[i] = int(rng.choice(pool))
        else:
            position[i] = int(rng.integers(0, length))
        if rng.random() < INVALID_SHARE:
            kind = int(rng.integers(0, 4))
            if kind == 0:
                record[i] = n + int(rng.integers(0, 2))
            elif kind == 1:
                position[i] = length + int(rng.integers(0, 2))
            elif kind == 2:
                alt[i] = k + int(rng.integers(0, 3))
            else:
                position[i] = (1 << 63) + int(rng.integers(0, 4))
    return Variants(record, position, alt, validity(case.lengths, k, record, position, alt))


def windows_of(p, length, m):
    """(lo, hi): the starts of the windows of a motif of ``m`` rows that cover ``p`` inside a record of ``length`` symbols;
    hi < lo when there are none."""
    return max(0, p - m + 1), min(p, length - m)


def side(weights, piece, lo, p):
    found, start, score = best_of(window_scores(weights, piece))
    return (np.float32(score), p - (lo + start)) if found else (np.float32(np.nan), NONE)


def reference(case, variants):
    n, v = len(case.mats), len(variants)
    out = Effects(np.full((n, v), np.nan, np.float32), np.full((n, v), np.nan, np.float32), np.full((n, v), NONE, np.int64),
                  np.full((n, v), NONE, np.int64), np.full(v, 0xFF, np.uint8), variants.valid.copy(), np.zeros((n, v), dtype=bool))
    for j in np.flatnonzero(variants.valid):
        r, p, a = int(variants.record[j]), int(variants.position[j]), int(variants.alt[j])
        symbols = case.symbols[r]
        out.ref_symbol[j] = symbols[p]
        for i, weights in enumerate(case.mats):
            m = weights.shape[0]
            lo, hi = windows_of(p, len(symbols), m)
            if hi < lo:
                continue
            out.has_window[i, j] = True
            piece = np.array(symbols[lo:hi + m])
            out.ref_score[i, j], out.ref_back[i, j] = side(weights, piece, lo, p)
            piece[p - lo] = a
            out.alt_score[i, j], out.alt_back[i, j] = side(weights, piece, lo, p)
    return out


def kept(effects, i, t):
    """Indices of the variants motif ``i`` keeps at threshold ``t``: a site on at least one allele (f32 ``>=``)."""
    with np.errstate(invalid="ignore"):
        return np.flatnonzero((effects.ref_score[i] >= np.float32(t)) | (effects.alt_score[i] >= np.float32(t)))


@lru_cache(maxsize=None)
def case_of(seed):
    """(case, variants, effects) of a seed, computed once and shared by the tests of a session; never written to."""
    case = draw_case(seed)
    variants = draw_variants(case)
    return case, variants, reference(case, variants)
