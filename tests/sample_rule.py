"""The sampling rule of ``lm_hip_seqset_sample`` restated in numpy: the only source of expected values for the tests of
csrc/sample.hip.  Philox4x32-10 with its rounds in ``uint64``; thresholds in f64; one uniform per symbol.

``u(seed, R, j)`` is output word ``j & 3`` of the block with key ``(lo32(seed), hi32(seed))`` and counter
``(lo32(j >> 2), lo32(R), hi32(R), hi32(j >> 2))``.  ``T[s] = floor(c_s / c_{K-1} * 2^32)`` over the running f64 sum of the
f32 row; ``draw(T, u) = #{s < K - 1 : u >= T[s]}``."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """``counter``: four uint64 arrays (or scalars) holding 32-bit words; ``key``: two Python ints.  Returns four uint64 arrays."""
    c0, c1, c2, c3 = [np.atleast_1d(np.asarray(c, dtype=np.uint64)) & MASK for c in counter]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2                   # 32 x 32 -> 64 bits: no wrap in uint64
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ np.uint64(k0), p1 & MASK, (p0 >> S32) ^ c3 ^ np.uint64(k1), p0 & MASK
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def uniforms(seed, R, n):
    """``u(seed, R, j)`` for ``j = 0 .. n - 1`` as uint64 values below 2^32."""
    seed, R = int(seed) % (1 << 64), int(R) % (1 << 64)
    if n == 0:
        return np.zeros(0, dtype=np.uint64)
    q = np.arange((n + 3) // 4, dtype=np.uint64)
    out = philox4x32_10((q & MASK, np.uint64(R & 0xFFFFFFFF), np.uint64(R >> 32), q >> S32), (seed & 0xFFFFFFFF, seed >> 32))
    return np.stack(out, axis=1).reshape(-1)[:n]


def valid(row):
    row = np.asarray(row, dtype=np.float32)
    return bool(np.isfinite(row).all() and (row >= 0).all() and row.astype(np.float64).sum() > 0)


def thresholds(row):
    """``T[0 .. K - 1)`` as uint64 values in [0, 2^32]."""
    c = np.cumsum(np.asarray(row, dtype=np.float32).astype(np.float64))       # sequential, in index order
    return np.floor(c[:-1] / c[-1] * 4294967296.0).astype(np.uint64)


def draw(T, u):
    return (np.asarray(u, dtype=np.uint64)[:, None] >= np.asarray(T, dtype=np.uint64)[None, :]).sum(axis=1).astype(np.uint8)


def record_order0(row, seed, R, n):
    return draw(thresholds(row), uniforms(seed, R, n))


def record_order1(initial, transitions, seed, R, n):
    k = len(initial)
    transitions = np.asarray(transitions, dtype=np.float32).reshape(k, k)
    T0 = thresholds(initial)
    rows = [thresholds(t) if t.astype(np.float64).sum() > 0 else T0 for t in transitions]
    u = uniforms(seed, R, n)
    # every state's successor at every position, then the chain itself
    step = np.stack([draw(T, u) for T in rows], axis=0) if n else np.zeros((k, 0), dtype=np.uint8)
    out = np.zeros(n, dtype=np.uint8)
    if n:
        x = int(draw(T0, u[:1])[0])
        out[0] = x
        for j in range(1, n):
            x = int(step[x, j])
            out[j] = x
    return out


def sample(lengths, frequencies, transitions=None, seed=0, record_base=0):
    """The records of the rule: ``frequencies`` is ``(k,)`` or ``(records, k)``."""
    f = np.asarray(frequencies, dtype=np.float32)
    out = []
    for r, n in enumerate(lengths):
        row = f if f.ndim == 1 else f[r]
        n = int(n)
        if n == 0:
            out.append(np.zeros(0, dtype=np.uint8))
        elif transitions is None:
            out.append(record_order0(row, seed, record_base + r, n))
        else:
            out.append(record_order1(row, transitions, seed, record_base + r, n))
    return out


def count_pairs(records, k):
    table = np.zeros((k, k), dtype=np.int64)
    for rec in records:
        rec = np.asarray(rec, dtype=np.int64)
        a, b = rec[:-1], rec[1:]
        keep = (a < k) & (b < k)
        np.add.at(table, (a[keep], b[keep]), 1)
    return table


def markov_from_counts(symbol_counts, pair_counts, pseudocount=0.0, unknown=False):
    """``lightmotif_amd.markov_from_counts`` restated."""
    sym = np.asarray(symbol_counts, dtype=np.int64)
    sym = sym.sum(axis=0) if sym.ndim == 2 else sym.copy()
    k = sym.size
    if not unknown:
        sym[-1] = 0
    initial = sym.astype(np.float32) / np.float32(sym.sum())
    pairs = np.asarray(pair_counts, dtype=np.int64).reshape(k, k)
    keep = np.ones((k, k), dtype=bool)
    if not unknown:
        keep[-1, :] = False
        keep[:, -1] = False
    # entries and row totals in f64 (exact for counts below 2^53), ONE conversion to f32 each, one f32 divide
    table = np.where(keep, pairs.astype(np.float64) + float(pseudocount), 0.0)
    transitions = np.zeros((k, k), dtype=np.float32)
    for a in range(k):
        total = np.float32(sum(float(x) for x in table[a]))
        if total > 0:
            transitions[a] = table[a].astype(np.float32) / total
    return initial, transitions
