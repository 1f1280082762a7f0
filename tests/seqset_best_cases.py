"""What the tests of the best hit per record (tests/test_gpu_seqset_best.py, tests/test_cpp_seqset_best.py) share: the
window scores of a record computed on the host in the reference's add order, the rule that picks a record's best window,
and the planted edge cases."""
import numpy as np

DNA_SYMBOLS = "ACTGN"


def window_scores(weights, symbols):
    """f32 scores of every window of one record: M sequential adds from +0.0 in row order (pli/mod.rs:96-105).
    ``weights`` is (M, >= K) f32, ``symbols`` the record's symbol indices."""
    m = weights.shape[0]
    n = len(symbols) - m + 1
    if n <= 0:
        return np.zeros(0, np.float32)
    symbols = np.asarray(symbols, dtype=np.int64)
    acc = np.zeros(n, np.float32)
    with np.errstate(invalid="ignore"):
        for j in range(m):
            acc = acc + weights[j, symbols[j:j + n]].astype(np.float32)
    return acc


def best_of(scores):
    """(found, position, score) of one record from its window scores: the greatest score under f32 `>`, NaN windows
    never competing, the lowest position among equals."""
    idx = np.flatnonzero(~np.isnan(scores))
    if not len(idx):
        return False, -1, np.float32(np.nan)
    pos = int(idx[int(np.argmax(scores[idx]))])          # argmax takes the first maximum; all -inf: the first window
    return True, pos, np.float32(scores[pos])


def consensus_matrix(consensus, n_weight, stride=8):
    """+2 for the consensus base, -2 for the others, ``n_weight`` for N."""
    m = len(consensus)
    p = np.zeros((m, stride), np.float32)
    p[:, :4] = -2.0
    p[:, 4] = n_weight
    for j, c in enumerate(consensus):
        p[j, DNA_SYMBOLS.index(c)] = 2.0
    return p


def encode(text):
    return np.asarray([DNA_SYMBOLS.index(c) for c in text], dtype=np.int64)


def edge_records(seed=3, m=12):
    """The planted records of the edge test: (consensus, records, notes); notes maps a label to record indices."""
    rng = np.random.default_rng(seed)
    while True:
        consensus = "".join(rng.choice(list("ACGT"), m))
        if all(consensus[:i] != consensus[-i:] for i in range(1, m)) and len(set(consensus)) > 1:
            break

    def bg(n):
        while True:
            s = "".join(rng.choice(list("ACGT"), n))
            if consensus not in s:
                return s

    records, notes = [], {"split": [], "planted": {}}
    for split in range(1, m):                                   # a consensus across a junction, at every split point
        records.append(bg(40) + consensus[:split])
        records.append(consensus[split:] + bg(25))
        notes["split"].append((len(records) - 2, len(records) - 1))
    records.append(bg(33) + consensus)                          # ends on the last base of the record
    notes["planted"][len(records) - 1] = 33
    records.append(consensus + bg(17))                          # starts on the first base
    notes["planted"][len(records) - 1] = 0
    records.append(bg(20))
    records.append("")                                          # an empty record between two others
    notes["empty"] = len(records) - 1
    records.append(consensus)                                   # a record that is exactly the motif
    notes["planted"][len(records) - 1] = 0
    records.append(bg(9) + consensus + bg(14) + consensus + bg(5))   # planted twice: the lower position
    notes["planted"][len(records) - 1] = 9
    records.append(consensus[0] * 40)                           # one repeated base: every window ties
    notes["repeat"] = len(records) - 1
    records.append(bg(50) + consensus[: m - 3])                 # the last record: its tail window runs into the padding
    notes["last"] = len(records) - 1
    return consensus, records, notes
