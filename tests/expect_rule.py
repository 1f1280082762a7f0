"""The rule of the expected site counts of a set (``lm_hip_seqset_expected_counts``) in numpy and Python integers, shared
by tests/test_expect_host.py, tests/test_gpu_seqset_expect.py and tests/test_gpu_expect_cli.py.  The window scores, the
planted edge records and the consensus matrix come from tests/seqset_best_cases.py.

Per motif (``M`` rows, scale ``s``) and record ``r`` with gain ``g``: every window ``p`` with ``p + M <= len(r)`` scores
``v`` (M sequential f32 adds), ``e = 2 ** fl32(s * v)``, ``z = min(e * g, 1.0)`` in f64 (a NaN score or a NaN product
contributes nothing), ``q = rint(z * 2 ** F)`` to nearest even with ``F = min(40, 62 - bit_length(N))``, ``N`` the
positions of the set, and ``Q[j][symbol(p + j)] += q`` in exact integers.  The table is ``Q * 2 ** -F``."""
import numpy as np

from seqset_best_cases import consensus_matrix, edge_records, window_scores  # noqa: F401  (shared with the users of this file)


def frac_bits_of(positions):
    return min(40, 62 - int(positions).bit_length())


def quanta_of(scores, scale, gain, frac_bits):
    """The integer weight of every window of one record from its f32 scores: a list of Python ints."""
    out = []
    with np.errstate(invalid="ignore", over="ignore"):
        x = np.float32(scale) * np.asarray(scores, dtype=np.float32)           # one f32 multiply
    for t in x.tolist():
        if t != t:
            out.append(0)
            continue
        try:
            e = 2.0 ** t
        except OverflowError:
            e = float("inf")
        with np.errstate(invalid="ignore", over="ignore"):
            zz = float(np.float64(e) * np.float64(gain))
        if zz != zz:
            out.append(0)
            continue
        z = min(zz, 1.0)
        out.append(int(round(z * 2.0 ** frac_bits)))                           # round(): to nearest, ties to even
    return out


def expected_quanta(weights, records_sym, gains, scale=1.0, k=5, frac_bits=None):
    """``Q`` of one motif: an ``(M, k)`` array of Python ints (dtype object), and the windows of the motif in the set."""
    m = weights.shape[0]
    f = frac_bits_of(sum(len(s) for s in records_sym)) if frac_bits is None else frac_bits
    q_tab = np.zeros((m, k), dtype=object)
    q_tab[:] = 0
    windows = 0
    for sym, g in zip(records_sym, gains):
        sym = np.asarray(sym, dtype=np.int64)
        scores = window_scores(weights, sym)
        windows += len(scores)
        for p, q in enumerate(quanta_of(scores, scale, g, f)):
            if q:
                for j in range(m):
                    q_tab[j, sym[p + j]] += q
    return q_tab, windows


def expected_counts(mats, records_sym, gains, scales=None, k=5):
    """Per motif ``(E, Q, windows)``: the float64 table ``Q * 2 ** -F``, the integers and the motif's window count; and F."""
    f = frac_bits_of(sum(len(s) for s in records_sym))
    out = []
    for i, w in enumerate(mats):
        q_tab, windows = expected_quanta(w, records_sym, gains[i], 1.0 if scales is None else scales[i], k, f)
        e = np.asarray([[float(int(c)) * 2.0 ** -f for c in row] for row in q_tab], dtype=np.float64).reshape(w.shape[0], k)
        out.append((e, q_tab, windows))
    return out, f


def planted_case(seed=7, records=200, length=60, m=10, mutate=0.10):
    """The set of the EM tests: ``records`` random DNA records of ``length`` bases, a ``m``-mer planted in each at a random
    place with ``mutate`` of its letters replaced.  Returns (word, texts)."""
    rng = np.random.default_rng(seed)
    letters = list("ACGT")
    while True:
        word = "".join(rng.choice(letters, m))
        if len(set(word)) == 4 and all(word[:i] != word[-i:] for i in range(1, m)):
            break
    texts = []
    for _ in range(records):
        site = list(word)
        for j in range(m):
            if rng.random() < mutate:
                site[j] = str(rng.choice([c for c in letters if c != word[j]]))
        at = int(rng.integers(0, length - m + 1))
        body = list(rng.choice(letters, length))
        body[at:at + m] = site
        texts.append("".join(body))
    return word, texts


def flattened_start(word, protein=False):
    """The start of the EM tests: the consensus of ``word`` flattened towards the background, as float counts (M, 5):
    0.4 for the consensus letter, 0.2 for every other one."""
    from seqset_best_cases import DNA_SYMBOLS
    counts = np.full((len(word), 5), 0.2, dtype=np.float64)
    counts[:, 4] = 0.0
    for j, c in enumerate(word):
        counts[j, DNA_SYMBOLS.index(c)] = 0.4
    return counts


def rule_em(weights, records_sym, iterations, to_scoring, scale=1.0):
    """OOPS EM with the rule alone: per iteration Z per record (``math.fsum`` of the rule's terms), gains ``1 / Z``,
    ``expected_quanta`` and ``to_scoring(E)`` -> the next (M, >= 5) weights.  Returns (weights, log2-likelihoods before every
    iteration and after the last)."""
    import math
    f = frac_bits_of(sum(len(s) for s in records_sym))
    lls = []

    def z_of(w):
        out = []
        for sym in records_sym:
            x = np.float32(scale) * window_scores(w, sym)
            out.append(math.fsum(2.0 ** t for t in x[~np.isnan(x)].astype(np.float64).tolist()))
        return out

    for _ in range(iterations):
        z = z_of(weights)
        lls.append(sum(math.log2(v) for v in z if v > 0))
        gains = [1.0 / v if v > 0 and math.isfinite(v) else 0.0 for v in z]
        q_tab, _ = expected_quanta(weights, records_sym, gains, scale, 5, f)
        e = np.asarray([[float(int(c)) * 2.0 ** -f for c in row] for row in q_tab], dtype=np.float64)
        weights = to_scoring(e)
    lls.append(sum(math.log2(v) for v in z_of(weights) if v > 0))
    return weights, lls
