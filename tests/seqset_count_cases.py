"""What the tests of the hit counts per record (tests/test_gpu_seqset_count.py, tests/test_seqset_count_host.py,
tests/test_cpp_seqset_count.py) share: the rule that counts a record's windows at a cut-off.  The window scores, the
planted edge records and the consensus matrix come from tests/seqset_best_cases.py."""
import numpy as np


def count_of(scores, t):
    """Windows of one record that reach ``t``: ``score >= t`` in f32, so a NaN window never counts, an -inf window counts
    at ``t = -inf`` alone and a NaN threshold counts nothing."""
    with np.errstate(invalid="ignore"):
        return int(np.count_nonzero(np.asarray(scores, dtype=np.float32) >= np.float32(t)))


def counts_of(mats, records_sym, cuts, window_scores):
    """``(motifs, levels, records)`` uint32 from sums made on the host in the reference's add order; ``cuts`` is
    ``(motifs, levels)``."""
    cuts = np.asarray(cuts, dtype=np.float32).reshape(len(mats), -1)
    out = np.zeros((len(mats), cuts.shape[1], len(records_sym)), dtype=np.uint32)
    for mi, p in enumerate(mats):
        for ri, sym in enumerate(records_sym):
            scores = window_scores(p, sym)
            for li in range(cuts.shape[1]):
                out[mi, li, ri] = count_of(scores, cuts[mi, li])
    return out
