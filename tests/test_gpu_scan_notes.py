"""The five threshold scans with MORE THAN ONE GROUP PER NOTE (scan_stream.hpp: groups_per_note > 1), on an input that
takes seconds.

A scan keeps at most 64 flag bits ("notes") per stream, so a stream of more than 64 groups puts G > 1 groups under one
bit, and the rows that get re-scored exactly come from the note -> row-range rule (scan_stream.hpp: note_rows).  The
planner grants such streams only to inputs of tens of millions of rows or to large batches; the other tests stay at
G = 1.  This one takes the batch road.  Its premise, by plan_c32's rule (score_plan.hip):

  * one sequence of 32 * 66 000 - 11 symbols = 66 000 rows of 32 columns, ``rows_per_stream`` = 1024;
  * one ``scan_threshold_batch`` call with 2 x CU count jobs of one length, which form ONE group of jobs, so each job is
    asked for ``want_streams = max(CUs * 128 / jobs, 64) = 64`` streams; 66 000 / 1024 = 64.4 >= 64, so the requested 1024
    rows per stream stand and T = q * step + first with q = (1024 + step / 2) / step:
      - DNA, M = 7: the ring of the pair scans and MP of the one-symbol scan are 8 -> q = 128, 129 groups, G = 3
        (43 notes, all full; T = 1026 for the pair scans, 1025 for the one-symbol scan);
      - protein, M = 4: MP = 4 -> q = 256, 257 groups, G = 5, 52 notes of which the last holds 2 groups (T = 1025);
        the protein pair scan has ring 8 -> 129 groups, G = 3 (T = 1026);
    66 000 is no multiple of either T, so the last stream of every job is the shifted one.

The jobs cycle over 8 distinct matrices and, per matrix, over two thresholds taken from realised scores: the maximum,
and one that leaves between 1 and 10 000 hits (checked on the oracle's output: a condition on the inputs).  Expected
hits are ``co.threshold`` of the oracle's score matrix, per distinct (matrix, threshold); every job's ordered
coordinates and score bits are compared.  Each route is asserted through ``launch_tally()``."""
from functools import lru_cache

import numpy as np
import pytest
import torch

import lightmotif_amd as lm
from oracle import c_oracle as co
from test_gpu_batch_routes import bits, make_enc, make_matrix

pytestmark = pytest.mark.gpu

LENGTH = 32 * 66_000 - 11
ROWS_PER_STREAM = 1024
NMATS = 8

# (alphabet size, M, options) -> the registry row the scans must run on: (family, wide, M, slot)
ROUTES = {
    "dna-default": (5, 7, {}, ("pre2_multi", 0, 7, "")),
    "dna-multi_motif=0": (5, 7, {"multi_motif": 0}, ("pre2", 0, 7, "")),
    "dna-pair_prefilter=0": (5, 7, {"pair_prefilter": 0}, ("pre", 0, 7, "")),
    "protein-default": (21, 4, {}, ("preblk", 1, 4, "")),
    "protein-block_prefilter=0": (21, 4, {"block_prefilter": 0}, ("pre", 1, 4, "")),
    "protein-pair_prefilter_protein=1": (21, 4, {"pair_prefilter_protein": 1}, ("pre2_protein", 1, 4, "")),
}


@lru_cache(maxsize=None)
def reference(k, m):
    """The sequence, 8 matrices and, per matrix, two (threshold, expected coordinates, expected values): computed once
    per alphabet and shared by its three routes."""
    rng = np.random.default_rng([7_100, k, m])
    enc = make_enc(rng, LENGTH, k, 0.02)
    mats = [make_matrix(rng, m, k) for _ in range(NMATS)]
    ref = co.stripe(enc, 32, k)
    co.configure_wrap(ref, m - 1)
    expected = []
    for p in mats:
        want = co.score_rows(ref, p)[0]
        assert want.shape[0] == 66_000
        fin = np.sort(want[np.isfinite(want)])
        per_matrix = []
        for t in (float(fin[-1]), float(fin[-2_000])):
            rc = co.threshold(want, 32, t).astype(np.int64).reshape(-1, 2)
            assert 1 <= len(rc) <= 10_000, (k, m, t, len(rc))
            per_matrix.append((t, rc, want[rc[:, 0], rc[:, 1]].copy()))
        expected.append(per_matrix)
    return enc, mats, expected


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_scan_with_several_groups_per_note(route):
    k, m, options, row = ROUTES[route]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    jobs = 2 * cus
    # the premise (see the module's docstring): 64 streams per job are enough, and the sequence has them at 1024 rows each
    assert cus * 128 // jobs <= 64 and 66_000 // ROWS_PER_STREAM >= 64
    enc, mats, expected = reference(k, m)
    pli = lm.Pipeline.hip(0)
    try:
        pli.set_option("tally_launches", 1)
        pli.set_rows_per_stream(ROWS_PER_STREAM)
        for name, value in options.items():
            pli.set_option(name, value)
        seq = pli.stripe(lm.EncodedSequence(enc, protein=k == 21), 32)
        seq.configure_wrap(m - 1)
        handles = [lm.ScoringMatrix(p, protein=k == 21) for p in mats]
        which = [(i % NMATS, (i // NMATS) % 2) for i in range(jobs)]   # job -> (matrix, threshold)
        pli.launch_tally()
        hits = pli.scan_threshold_batch([handles[a] for a, _ in which], [expected[a][b][0] for a, b in which], seq)
        tally = pli.launch_tally()
        assert set(tally) == {row}, (route, sorted(tally))
        assert len(hits) == jobs
        for i, (a, b) in enumerate(which):
            t, rc, values = expected[a][b]
            coords, got = hits[i]
            assert np.array_equal(coords, rc), (route, i, a, t, len(coords), len(rc))
            assert np.array_equal(bits(got), bits(values)), (route, i, a, t)
    finally:
        pli.close()
