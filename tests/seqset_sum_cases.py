"""What the tests of the total odds per record (tests/test_gpu_seqset_sum.py, tests/test_seqset_sum_host.py) share: the
rule that sums a record's windows.  The window scores, the planted edge records and the consensus matrix come from
tests/seqset_best_cases.py."""
import math

import numpy as np

from seqset_best_cases import consensus_matrix, edge_records, window_scores  # noqa: F401  (shared with the users of this file)

TOLERANCE = 2.0 ** -21     # relative, of a cell against ``sum_of``: the fraction x - rint(x) is exact, the hardware exp2 is
                           # documented at 1 ulp (2^-23 on [1, 2)), all terms are positive so the sum inherits the terms'
                           # relative error, and the f64 accumulation adds n * 2^-53: four times that


def sum_of(scores, scale=1.0):
    """The total odds of one record from its f32 window scores: ``2 ** fl32(scale * v)`` in f64 over the windows, a NaN
    window adding nothing; an -inf window adds 0 and a +inf window makes the sum +inf."""
    return math.fsum(2.0 ** float(np.float32(scale) * np.float32(v)) for v in scores if v == v)


def sums_of(mats, records_sym, scales=None):
    """``(motifs, records)`` float64 of ``sum_of`` over sums made on the host in the reference's add order."""
    out = np.zeros((len(mats), len(records_sym)), dtype=np.float64)
    for mi, p in enumerate(mats):
        s = np.float32(1.0 if scales is None else scales[mi])
        for ri, sym in enumerate(records_sym):
            with np.errstate(invalid="ignore", over="ignore"):
                x = s * window_scores(p, sym)                       # f32 * f32: one f32 multiply
            out[mi, ri] = math.fsum(2.0 ** t for t in x[~np.isnan(x)].astype(np.float64).tolist())
    return out


def close(got, want, tol=TOLERANCE):
    """Every cell within ``tol`` relative of the rule; cells of 0 and of +inf exactly."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    plain = np.isfinite(want) & (want != 0)
    with np.errstate(invalid="ignore"):
        return bool(np.array_equal(got[~plain], want[~plain]) and np.all(np.abs(got[plain] - want[plain]) <= tol * want[plain]))
