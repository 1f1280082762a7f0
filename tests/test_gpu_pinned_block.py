"""The users of the context's pinned staging block (lm_internal.hpp: the kPin* layout) back to back on ONE context.

Every route that returns something small to the host goes through that block, each through its own region; the other GPU
tests run one route per context or per test.  Stale bytes a region's previous tenant left behind are what a mistake in the
layout shows as, so this test cycles three times, in a fixed order, through every delivery mode and compares each result
with the oracle exactly (scores bit for bit, coordinates as integers):

 1. fused argmax of one job at C = 32: the exact kernel's wavefront records folded by the host (kPinFoldRecords), then with
    option host_fold = 0 the record its last workgroup writes and the generation word the host polls (kPinRecord);
 2. fused argmax of one job at C = 1: the tiled store kernel's records, folded by the host (kPinFoldRecords);
 3. fused threshold batch of both motifs, a few dozen hits each (kPinUploadHead, kPinHitStaging);
 4. Scanner.max: the window walk (kPinScanMaxState) and, over a sequence of 2^20 cells, the candidate list (kPinCounters,
    kPinListHead);
 5. score_discrete of a 256-row block (kPinU8Out);
 6. score_into + argmax + threshold on a handle (the handle's own records; kPinCounters);
 7. fused argmax batch of both motifs (kPinArgmaxBatch: results and the FinalizeJob table, finalize launch).

The shapes (2 048 rows at C = 32, M = 8 and 20) are the smallest that still take each mode.  At C = 1 that is 2^16 cells
(score_plan.hip: chunked_ok; 4 096 positions go cell by cell through score_generic<1>, which leaves no records), and the
M = 20 motif in every cycle: a motif of up to 9 rows over that many rows may be settled by the suffix route instead.

The three single-launch argmax forms read what the kernel wrote by polling pinned memory (the records' generation halves, or
the generation word behind the record) and fall back to a stream synchronisation after 2^20 unanswered polls, which gives
the right answer too.  So a host that polls the wrong word is told from one that polls the right one by time alone: 2^20
polls of a load and a `pause` cost at least a few milliseconds (1 ms at an impossible 1 ns each), the call itself costs tens of
microseconds.  Each form is therefore called five times and the fastest call must stay under kPollBound = 1 ms.
"""
import time

import numpy as np
import pytest

import lightmotif_amd as lm
from oracle import c_oracle as co
from oracle import np_oracle as no

pytestmark = pytest.mark.gpu
WRAP = 20
kPollBound = 1e-3  # seconds: see the module docstring


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_every_tenant_of_the_pinned_block_back_to_back_on_one_context():
    pli = lm.Pipeline.hip(0)
    rng = np.random.default_rng(0x9B10C)
    enc32 = rng.integers(0, 4, 2048 * 32 - 11, dtype=np.uint8)
    enc1 = rng.integers(0, 4, 66_001, dtype=np.uint8)
    ref32, ref1 = co.stripe(enc32, 32, 5), co.stripe(enc1, 1, 5)
    assert ref32.rows == 2048 and ref1.rows == 66_001
    seq32, seq1 = pli.stripe(lm.EncodedSequence(enc32), 32), pli.stripe(lm.EncodedSequence(enc1), 1)
    encbig = rng.integers(0, 4, 32768 * 32 - 5, dtype=np.uint8)      # 2^20 cells: Scanner.max goes by candidate list
    refbig, seqbig = co.stripe(encbig, 32, 5), pli.stripe(lm.EncodedSequence(encbig), 32)
    assert refbig.rows == 32768
    for ref, seq in ((ref32, seq32), (ref1, seq1), (refbig, seqbig)):
        co.configure_wrap(ref, WRAP)
        seq.configure_wrap(WRAP)

    # the references, computed once
    motifs = []
    for m in (8, 20):
        p = np.zeros((m, 8), np.float32)
        p[:, :4] = rng.normal(0, 2, (m, 4))
        p[:, 4] = -np.inf
        want32, _ = co.score_rows(ref32, p)
        want1, _ = co.score_rows(ref1, p)
        finite = np.sort(want32[:, :32][np.isfinite(want32[:, :32])])
        t = float(finite[-30])
        hits = [tuple(map(int, rc)) for rc in co.threshold(want32, 32, t)]
        assert 24 <= len(hits) <= 60
        w, factor, _, offset = no.to_discrete(p, 5)
        d_sat = no.score_rows_u8_saturating(ref32.data, 32, len(enc32), w, 0, ref32.rows)
        pssm = lm.ScoringMatrix(p)
        dm = pssm.to_discrete()
        d_wrap, _ = co.score_rows_u8(ref32, dm.data)
        ts = float(np.quantile(finite, 0.999))
        smax = no.scanner_max_strict(want32, d_sat, 32, ts, lambda x: no.discrete_scale(x, factor, offset), 256)
        assert smax is not None
        wantbig, _ = co.score_rows(refbig, p)
        dbig = no.score_rows_u8_saturating(refbig.data, 32, len(encbig), w, 0, refbig.rows)
        tsbig = float(np.quantile(wantbig[:, :32][np.isfinite(wantbig[:, :32])], 0.999))
        smaxbig = no.scanner_max_strict(wantbig, dbig, 32, tsbig, lambda x: no.discrete_scale(x, factor, offset), 256)
        assert smaxbig is not None
        motifs.append(dict(m=m, pssm=pssm, dm=dm, want32=want32, want1=want1, t=t, hits=hits, d_sat=d_sat, d_wrap=d_wrap,
                           ts=ts, smax=smax, tsbig=tsbig, smaxbig=smaxbig, am32=co.argmax(want32, 32), am1=co.argmax(want1, 1)))

    def check_argmax(got, want, am, what):
        assert got is not None and got[0] == am, (what, got, am)
        assert bits(np.float32(got[1])) == bits(want[am]), (what, got, want[am])

    def polled_argmax(mo, seq, want, am, kernel, what):
        """A single-launch argmax form, five times: right every time, and not by way of the synchronising fall-back."""
        fastest = float("inf")
        for _ in range(5):
            t0 = time.perf_counter()
            got = pli.score_argmax(mo["pssm"], seq)
            fastest = min(fastest, time.perf_counter() - t0)
            check_argmax(got, mo[want], mo[am], what)
            assert pli.last_kernel == kernel, (what, pli.last_kernel)
        assert fastest < kPollBound, (what, fastest)

    scores = lm.StripedScores.empty(pli, 32)
    for cycle in range(3):
        a, b = motifs[cycle % 2], motifs[(cycle + 1) % 2]
        # 1. one job at C = 32: host-folded records, then the polled record
        polled_argmax(a, seq32, "want32", "am32", f"score_c32<{a['m']},1>", (cycle, "host records"))
        pli.set_option("host_fold", 0)
        try:
            polled_argmax(b, seq32, "want32", "am32", f"score_c32<{b['m']},1>", (cycle, "polled record"))
        finally:
            pli.set_option("host_fold", 1)
        # 2. one job at C = 1: tiled store + host fold
        polled_argmax(motifs[1], seq1, "want1", "am1", "score_tiled+host_fold", (cycle, "C = 1"))
        # 3. threshold batch of both motifs
        batch = pli.scan_threshold_batch([a["pssm"], b["pssm"]], [a["t"], b["t"]], seq32)
        for (coords, values), mo in zip(batch, (a, b)):
            assert [tuple(map(int, rc)) for rc in coords] == mo["hits"], (cycle, mo["m"])
            assert np.array_equal(bits(values), bits([mo["want32"][rc] for rc in mo["hits"]])), (cycle, mo["m"])
        # 4. Scanner.max
        for seq, ts, smax, kernel in ((seq32, a["ts"], a["smax"], "scanmax_find"),
                                      (seqbig, a["tsbig"], a["smaxbig"], "score_c32_prefilter2+scanmax_gate")):
            hit = lm.Scanner(a["pssm"], seq, threshold=ts).max()
            assert hit is not None and (hit.position, bits(np.float32(hit.score))) == (smax[0], bits(smax[1])), (cycle, hit, smax)
            assert pli.last_kernel == kernel, (cycle, pli.last_kernel)
        # 5. a Scanner block of u8 scores
        r0 = 256 * (1 + cycle)
        for saturate, want in ((True, b["d_sat"]), (False, b["d_wrap"])):
            got, _ = pli.score_discrete(b["dm"], seq32, rows=range(r0, r0 + 256), saturate=saturate)
            assert np.array_equal(got[:, :32], want[r0:r0 + 256, :32]), (cycle, saturate)
        # 6. score_into + argmax + threshold on a handle
        pli.score_into(b["pssm"], seq32, scores)
        assert pli.argmax(scores) == b["am32"], cycle
        assert bits(np.float32(pli.max(scores))) == bits(b["want32"][b["am32"]]), cycle
        assert pli.threshold(scores, b["t"]) == b["hits"], cycle
        assert np.array_equal(bits(scores.matrix()[:, :32]), bits(b["want32"][:, :32])), cycle
        # 7. argmax batch of both motifs
        got = pli.scan_argmax_batch([a["pssm"], b["pssm"]], seq32)
        for g, mo in zip(got, (a, b)):
            check_argmax(g, mo["want32"], mo["am32"], (cycle, "batch", mo["m"]))
