"""Test helper: f32 scoring matrices at the edges of the format, and the thresholds that go with them.

Each regime is a small generator with a fixed seed (tests/test_extreme_weights_cpu.py checks on the CPU that every
construction produces the edge it is named after; tests/test_gpu_extreme_weights.py runs every score route on them
against the C oracle).  The matrices follow the layout of ``ScoringMatrix`` data: ``(M, stride(K, 4))`` f32 with the
default symbol (N / X) in column K - 1.
"""
import numpy as np

from oracle import c_oracle as co

FLT_MAX = float(np.finfo(np.float32).max)
TINY = float(np.nextafter(np.float32(0), np.float32(1)))  # the smallest subnormal, 2^-149
BIG = 3e38                                                 # two of these overflow f32, one does not

# (regime, variant): variant "" where the regime has only one form
REGIMES = [
    ("overflow_inf", "ninf_head"),     # -inf N column; the overflowing rows open the motif
    ("overflow_inf", "finite_tail"),   # finite N column; the overflowing rows close the motif
    ("overflow_nan", "first"),         # NaN at cell (0, 0): the first-cell rule of the argmax
    ("overflow_nan", "inner"),         # NaN elsewhere, cell (0, 0) finite
    ("near_overflow", "below"),        # sum of row max |w| just under the prefilter's no-overflow limit
    ("near_overflow", "above"),        # ... just over it
    ("wide_range", ""),
    ("subnormal", "pure"),
    ("subnormal", "mixed"),
    ("signed_zero", ""),
    ("tiny_range", ""),
]


def regime_id(regime, variant):
    return f"{regime}-{variant}" if variant else regime


def min_length(regime):
    """Shortest motif a regime is defined for (an overflow needs two adds, a NaN after one needs a third; one weight
    alone has no rounding error to swamp the step)."""
    return {"overflow_inf": 2, "overflow_nan": 3, "tiny_range": 2}.get(regime, 1)


def no_overflow_limit(m):
    """The prefilter's limit on the sum of the rows' largest finite |w| (csrc/pssm_tables.hpp, build_prefilter): below it no
    partial sum of a window can round to +-inf."""
    return FLT_MAX / (1.0 + (m + 1) * 2.0 ** -23)


def abs_sum(pssm, k):
    """Sum over the rows of the largest finite |w| (-inf stands for the row minimum and does not count)."""
    w = np.asarray(pssm[:, :k], np.float64)
    w = np.where(np.isneginf(w), 0.0, np.abs(w))
    return float(w.max(axis=1).sum())


def prefilter_sound(pssm, k):
    """Whether build_pssm_tables (csrc/pssm_tables.hpp) gives this matrix prefilter images: an independent restatement of
    build_prefilter's conditions, which tests/cpp/test_pssm_tables.cpp checks on the builder itself."""
    w = np.asarray(pssm[:, :k], np.float64)
    if w.shape[0] < 1 or np.isnan(w).any() or np.isposinf(w).any():
        return False
    fin = np.where(np.isneginf(w), np.nan, w)
    if np.isnan(fin).all(axis=1).any():
        return False
    rng = float(np.nansum(np.nanmax(fin, axis=1) - np.nanmin(fin, axis=1)))
    m = w.shape[0]
    return rng > 0 and abs_sum(pssm, k) * (1.0 + (m + 1) * 2.0 ** -23) < FLT_MAX


def kmer_bound(pssm, k):
    """Sequential f32 sum of the row maxima from 0.0 (best_kmer_score): the greatest score any window can have."""
    b = np.float32(0.0)
    with np.errstate(over="ignore", invalid="ignore"):
        for row in np.asarray(pssm[:, :k], np.float32):
            best = row[0]
            for x in row[1:]:
                best = x if x > best else best
            b = np.float32(b + best)
    return b


def make_pssm(regime, variant, m, k, seed=0):
    rng = np.random.default_rng([hash_regime(regime, variant), m, k, seed])
    n = k - 1  # real symbols; column k - 1 is N / X
    p = np.zeros((m, co.stride(k, 4)), np.float32)
    p[:, :n] = rng.normal(0, 2, (m, n))
    p[:, n] = -np.inf
    if regime == "overflow_inf":
        # rows r, r + 1: w[A] = 3e38 -> A A overflows; row r + 2: w[A] = -3e38 (A A A: real sum ~3e38, f32 +inf) and
        # w[C] = 1e38 (A A C: +inf and a real sum of 7e38, above every finite threshold)
        r = overflow_row(regime, variant, m)
        p[r, 0] = p[r + 1, 0] = BIG
        if m >= 3:
            p[r + 2, 0] = -BIG
            p[r + 2, 1] = 1e38
        if variant.startswith("finite"):
            p[:, n] = rng.normal(0, 1, m)
    elif regime == "overflow_nan":
        # rows 0, 1: w[A] = 3e38 -> A A is +inf; row 2 N = -inf -> A A N is NaN (+inf + -inf)
        p[0, 0] = p[1, 0] = BIG
    elif regime == "near_overflow":
        # every row's largest |w| positive, so that the best windows come close to FLT_MAX
        w = rng.normal(0, 1, (m, n))
        j = np.abs(w).argmax(axis=1)
        w[np.arange(m), j] = np.abs(w[np.arange(m), j])
        scale = 1.0 - 2.0 ** -20 if variant == "below" else 1.0 + 2.0 ** -20
        w *= no_overflow_limit(m) * scale / np.abs(w).max(axis=1).sum()
        p[:, :n] = w
    elif regime == "wide_range":
        j = rng.integers(0, n, m)
        p[np.arange(m), j] = 1e30 * rng.choice([1.0, 1.25, 1.5], m)  # few distinct big terms: ties
    elif regime == "subnormal":
        p[:, :n] = rng.integers(-300, 301, (m, n)) * np.float32(1e-42)  # |sums| < 2^-126 up to M = 37
        if variant == "mixed":  # normal weights just above the subnormal range: partial sums cross into it
            mask = rng.random((m, n)) < 0.5
            normal = rng.choice([-1.0, 1.0], (m, n)) * rng.uniform(1.2e-38, 4e-38, (m, n))
            p[:, :n] = np.where(mask, normal.astype(np.float32), p[:, :n])
    elif regime == "signed_zero":
        p[:, :k] = np.where(rng.random((m, k)) < 0.5, np.float32(-0.0), np.float32(0.0))
        p[0, :k] = -0.0
    elif regime == "tiny_range":
        base = np.float32(1000.0)
        steps = rng.integers(-1, 2, (m, n))  # 1000 and its two neighbours
        p[:, :n] = np.float32(base) + steps * np.spacing(base)
    else:
        raise ValueError(regime)
    return p


def hash_regime(regime, variant):
    return sum((i + 1) * ord(c) for i, c in enumerate(regime + "/" + variant))


def make_sequence(regime, variant, length, k, m, seed=0):
    """Random symbols with ~2 % N / X.  The overflow regimes plant windows (no N / X inside) whose overflowing rows
    read A A A / A A C (overflow_inf) or A A N (overflow_nan), and overflow_nan fixes what cell (0, 0) holds."""
    rng = np.random.default_rng([hash_regime(regime, variant), length, k, m, seed, 7])
    enc = rng.integers(0, k - 1, length).astype(np.uint8)
    enc[rng.random(length) < 0.02] = k - 1
    if regime in ("overflow_inf", "overflow_nan") and length >= 2 * m + 8:
        r = overflow_row(regime, variant, m)
        tails = [(0, 0, 0), (0, 0, 1)] if regime == "overflow_inf" else [(0, 0, k - 1)]
        for i, pos in enumerate(rng.integers(m + 1, length - m, max(length // 500, 8))):
            enc[pos:pos + m] = rng.integers(0, k - 1, m)
            tail = tails[i % len(tails)][: m - r]
            enc[pos + r:pos + r + len(tail)] = tail
        if regime == "overflow_nan":
            enc[:m] = rng.integers(0, k - 1, m)
            enc[:3] = (0, 0, k - 1) if variant == "first" else (1, 0, 0)
    return enc


def overflow_row(regime, variant, m):
    """First of the motif rows that carry the overflowing weights."""
    return m - 3 if regime == "overflow_inf" and variant.endswith("tail") and m >= 3 else 0


def thresholds(scores, cols, pssm, k, extra=()):
    """The edge thresholds of every case, and for a quantile and the maximum s of the realised finite scores: s and
    its two f32 neighbours; then the window bound B (best_kmer_score) and the next float above it."""
    ts = [np.nan, np.inf, -np.inf, 0.0, -0.0, FLT_MAX, -FLT_MAX, TINY]
    fin = np.sort(scores[:, :cols][np.isfinite(scores[:, :cols])].ravel())
    if fin.size:
        for s in (fin[int(0.99 * (fin.size - 1))], fin[-1]):
            s = np.float32(s)
            ts += [float(s), float(np.nextafter(s, np.float32(np.inf))), float(np.nextafter(s, np.float32(-np.inf)))]
    b = kmer_bound(pssm, k)
    if np.isfinite(b):
        ts += [float(b), float(np.nextafter(b, np.float32(np.inf)))]
    ts += list(extra)
    return ts


def quantile_threshold(scores, cols):
    """A realised finite score that some cells reach (None when no score is finite)."""
    fin = np.sort(scores[:, :cols][np.isfinite(scores[:, :cols])].ravel())
    return float(fin[int(0.99 * (fin.size - 1))]) if fin.size else None


def extra_thresholds(regime):
    # overflow_inf: above the real sum of A A A (~3e38), below that of A A C (~7e38)
    return (3.2e38,) if regime == "overflow_inf" else ()


def prefilter_td(pssm, k, t):
    """The discrete threshold the fused threshold route derives from ``t`` (score_threshold.hip, mirror of its map
    with the offset / factor / error bound of build_prefilter, csrc/pssm_tables.hpp); a value below 1 means the route cannot be taken."""
    w = np.asarray(pssm[:, :k], np.float64)
    fin = np.where(np.isneginf(w), np.nan, w)
    lo, hi = np.nanmin(fin, axis=1), np.nanmax(fin, axis=1)
    m = w.shape[0]
    factor = float((hi - lo).sum()) / 32000.0
    emax = m * 2.0 ** -24 * abs_sum(pssm, k) * 1.5
    return np.floor((float(np.float32(t)) - float(lo.sum())) / factor) - np.ceil(emax / factor) - 1.0


def discrete_weights(pssm, k):
    """The u16 weights of the images build_pssm_tables packs (csrc/pssm_tables.hpp, build_prefilter: ceil((w - row min) / factor), at least the guard's +1 on exact
    multiples; -inf -> 0), computed whether or not the matrix passes the no-overflow limit."""
    w = np.asarray(pssm[:, :k], np.float64)
    fin = np.where(np.isneginf(w), np.nan, w)
    lo, hi = np.nanmin(fin, axis=1), np.nanmax(fin, axis=1)
    factor = float((hi - lo).sum()) / 32000.0
    v = np.where(np.isneginf(w), 0.0, (w - lo[:, None]) / factor)
    q = np.ceil(v)
    q = np.where(np.isneginf(w), 0.0, np.where(q < v + 1e-9, q + 1, q))
    return q.astype(np.int64)


# ---- the candidate route of the fused argmax: planted +inf windows its sample misses ------------------------------

PLANT_M, PLANT_LENGTH, PLANT_COLS = 13, 101_000_000, 32
SAMPLE_ROWS = 8   # argmax_plan.hpp: kSampleRows (one row per half-wave of a 256-thread block)


def sampled_rows(rows, num_cus=256):
    """Rows the candidate route's sample scores for a lone job (argmax_plan.hpp, sample_geometry, restated here: chunks of
    SAMPLE_ROWS rows spread evenly, about 1/1024 of the rows, at most 8 per CU)."""
    nchunks = min(max(rows // 1024 // SAMPLE_ROWS, 32), num_cus * 8)
    stride = (rows - SAMPLE_ROWS) // (nchunks - 1)
    return (np.arange(nchunks)[:, None] * stride + np.arange(SAMPLE_ROWS)[None, :]).ravel(), stride


def planted_argmax_pssm(overflow):
    """M = 13: rows 0-11 carry w[A] = 3e37 (twelve A overflow: 3.6e38), row 12 w[A] = -3e38, so an all-A window scores
    +inf in f32 while its real sum (~0.6e38) lies far below the sample's bound (~3e38, windows with 10-11 A).  Every
    other weight but T's (below) is distinct, ~1e36, so the sample's bound is no huge tie.  ``overflow`` False: w[A] = 2.5e37 and -3e37
    -- the same shape under the no-overflow limit, which the candidate route serves."""
    rng = np.random.default_rng([101, int(overflow)])
    m, k = PLANT_M, 5
    p = np.zeros((m, co.stride(k, 4)), np.float32)
    p[:, :4] = rng.uniform(0.5, 1.5, (m, 4)) * rng.choice([-1.0, 1.0], (m, 4)) * 1e36
    p[:12, 0] = 3e37 if overflow else 2.5e37
    p[12, 0] = -3e38 if overflow else -3e37
    # T is the minimum of rows 0-11: the image counts the N after a planted run as that minimum, so the windows that
    # start inside the run and read the N (real score -inf) stay unflagged like the run itself; the scan re-scores
    # whole flagged row ranges, and a flagged neighbour would have the planted window re-scored too
    p[:12, 2] = -3e38 if overflow else -2.5e37
    p[:, 4] = -np.inf
    return p


def planted_argmax_sequence(num_cus=256):
    """101 Mbp of ACGT without any run of 12 A, then 8 planted runs of 13 A, each followed by an N: the window at the run
    is all A (+inf with the overflowing matrix), the one a row later reads 12 A then N (+inf + -inf = NaN, never the
    maximum).  So the only +inf windows are the planted ones.  They sit half-way between sampled chunks, in the last
    gaps of the range, so the last of them in row-major order -- the reference's argmax -- is one the sample misses."""
    m, length, cols = PLANT_M, PLANT_LENGTH, PLANT_COLS
    rng = np.random.default_rng(101)
    enc = rng.integers(0, 4, length, dtype=np.uint8)
    for _ in range(3):   # break every run of 12 A (breaking one cannot make another)
        a = (enc == 0).astype(np.int32)
        c = np.concatenate(([0], np.cumsum(a)))
        starts = np.nonzero(c[12:] - c[:-12] == 12)[0]
        if starts.size == 0:
            break
        enc[starts + 6] = 1
    rows = -(-length // cols)
    _, stride = sampled_rows(rows, num_cus)
    nchunks = (rows - SAMPLE_ROWS) // stride + 1
    plants = []
    for i, col in enumerate((3, 30, 11, 25, 17, 8, 21, 29)):
        row = (nchunks - 9 + i) * stride + stride // 2
        pos = col * rows + row
        enc[pos - 1] = 1
        enc[pos:pos + m] = 0
        enc[pos + m] = 4
        plants.append((row, col))
    return enc, plants


def window_bounds(enc, d, rows, cells):
    """Discrete sums of the windows at the (row, col) cells under the image's weights ``d`` (M x K)."""
    pos = np.asarray([c * rows + r for r, c in cells])
    m = d.shape[0]
    return sum(d[j][enc[pos + j]] for j in range(m))


def unflagged_near(enc, pssm, cell, bound, k=5, reach=64):
    """Whether the image of real sums (without the no-overflow limit) flags no window within ``reach`` rows of ``cell``
    in any column at the candidate route's threshold for the sample bound ``bound``: the scan re-scores whole flagged row
    ranges, so a flagged neighbour would expose the cell too."""
    rows = -(-len(enc) // PLANT_COLS)
    r0, _ = cell
    cells = [(r, c) for r in range(r0 - reach, r0 + reach + 1) for c in range(PLANT_COLS)]
    return bool((window_bounds(enc, discrete_weights(pssm, k), rows, cells) < prefilter_td(pssm, k, bound)).all())
