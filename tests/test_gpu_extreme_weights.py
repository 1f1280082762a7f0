"""Every score route on f32 matrices at the edges of the format, bit for bit against the C oracle.

The regimes (tests/extreme_weights.py; their constructions are checked on the CPU by test_extreme_weights_cpu.py):
windows that overflow to +inf whose real sum lies below the threshold, +inf + -inf = NaN (at cell (0, 0) and
elsewhere), sums of row maxima just under and over the prefilter's no-overflow limit, one weight near 1e30 per row,
subnormal weights, signed zeros and weights within an ulp of 1000.  Thresholds: NaN, +-inf, +-0, +-FLT_MAX, the
smallest subnormal, realised scores and their f32 neighbours, the window bound B (best_kmer_score) and just above it.

The fused routes scan a 16-bit image of the matrix and re-score what it flags; that image is sound only while no
partial sum can overflow (pssm_tables.hpp, build_prefilter).  Each parametrisation forces its route through a pipeline with
its own options and checks ``last_kernel`` after a threshold the route can serve: the prefilter kernel where a sound
image exists and the threshold maps into its range (mirrored by extreme_weights.prefilter_td), never otherwise."""
import os
import re

import numpy as np
import pytest
import torch

import extreme_weights as xw
import lightmotif_amd as lm
from host_walk import scanner_max_strict_host
from oracle import c_oracle as co

pytestmark = pytest.mark.gpu
LENGTH = 20_000

# route: (context options, alphabet size K, motif lengths, column count, kernel of the fused threshold when the prefilter
# serves it; None = the route has no prefilter scan)
ROUTES = {
    "store": ({}, 5, (1, 8, 31), 32, "score_c32_prefilter2"),
    "store_no_track": ({"track_argmax": 0}, 21, (2, 17), 32, "score_c32_prefilter_blk"),
    "exact": ({"prefilter": 0}, 5, (1, 12, 31), 32, None),
    "single": ({"pair_prefilter": 0}, 5, (3, 17), 32, "score_c32_prefilter"),
    "pair": ({}, 5, (2, 3, 7), 32, "score_c32_prefilter2"),
    "no_skip": ({"skip_unreachable": 0}, 5, (7, 12), 32, "score_c32_prefilter2"),
    "no_suffix": ({"suffix_argmax": 0}, 5, (8,), 32, "score_c32_prefilter2"),
    "drop_last": ({}, 5, (20, 24, 36), 32, "score_c32_prefilter2"),
    "no_drop_last": ({"drop_last": 0}, 5, (24,), 32, "score_c32_prefilter2"),
    "protein_block": ({}, 21, (3, 12), 32, "score_c32_prefilter_blk"),
    "protein_bytes": ({"block_prefilter": 0}, 21, (8,), 32, "score_c32_prefilter"),
    "protein_pair": ({"pair_prefilter_protein": 1}, 21, (7, 20), 32, "score_c32_prefilter2"),
    "long": ({}, 5, (37, 64, 128), 32, "score_c32_prefilter2"),
    "long_cellwise": ({"chunked_fused": 0}, 5, (37, 128), 32, "score_c32_prefilter2"),
    "generic_c1": ({}, 5, (3, 12), 1, None),
    "tiled_c16": ({}, 21, (7, 36), 16, None),
    "generic_c33": ({"tiled": 0}, 5, (1, 20), 33, None),
}

_PIPES = {}


def pipeline(options):
    key = tuple(sorted(options.items()))
    if key not in _PIPES:
        p = lm.Pipeline.hip(0)
        for name, value in options.items():
            p.set_option(name, value)
        _PIPES[key] = p
    return _PIPES[key]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(a, b):
    """Bit for bit, except that any NaN equals any NaN: the NaN of +inf + -inf carries the adding unit's default NaN,
    whose bits are the hardware's choice and which nothing in the reference can observe (every comparison with a NaN
    is false)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(bits(a[~na]), bits(b[~nb]))


def rc_list(a):
    return [tuple(map(int, rc)) for rc in a]


def oracle_case(enc, pssm_np, k, cols):
    m = pssm_np.shape[0]
    s = co.stripe(enc, cols, k)
    co.configure_wrap(s, max(m - 1, 0))
    want, mi = co.score_rows(s, pssm_np)
    return s, want, mi


def fast_expected(fast, pssm_np, k, t):
    return fast is not None and t is not None and xw.prefilter_sound(pssm_np, k) and xw.prefilter_td(pssm_np, k, t) >= 1


def ceil4(m):
    return -(-m // 4) * 4


def store_kernels(m, cols, options):
    """Names the store kernel of score_into may carry (score_store.hip: C = 32 with the table padded to 4 rows or not,
    one slice of a long motif, slices beyond 64 rows; other column counts tiled or generic)."""
    if cols == 32:
        if m <= 36:
            return {f"score_c32<{m},0>", f"score_c32<{ceil4(m)},0>"}
        return {f"score_c32<{ceil4(m)},0>"} if m <= 64 else {"score_c32_sliced"}
    if cols == 16 and m <= 36:   # the C = 32 kernels also store C = 16
        return {f"score_c32<{m},0>", f"score_c32<{ceil4(m)},0>"}
    return {"score_tiled"} if options.get("tiled", 1) else {"score_generic<0>"}


def exact_threshold_kernels(m, cols, options):
    """Names of the fused threshold without a prefilter scan: the exact C = 32 kernel up to 64 rows (C = 16: that family
    or the generic kernel), the generic kernel for other column counts (these sequences are below the chunked route's 2^16 cells) and, with chunked_fused off,
    for motifs beyond the exact kernels; None = the chunked route (its chunks go through the store kernels)."""
    if cols == 16 and m <= 36:
        return {f"score_c32<{m},2>", "score_generic<2>"}
    if cols != 32:
        return {"score_generic<2>"}
    if m <= 64:
        return {f"score_c32<{m if m <= 36 else ceil4(m)},2>"}
    return None if options.get("chunked_fused", 1) else {"score_generic<2>"}


def check_case(pli, regime, variant, k, m, cols, fast, options, length=LENGTH):
    protein = k == 21
    pssm_np = xw.make_pssm(regime, variant, m, k)
    enc = xw.make_sequence(regime, variant, length, k, m)
    s, want, want_mi = oracle_case(enc, pssm_np, k, cols)
    seq = pli.stripe(lm.EncodedSequence(enc, protein=protein), cols)
    seq.configure_wrap(max(m - 1, 0))
    pssm = lm.ScoringMatrix(pssm_np, protein=protein)
    ctx = (regime, variant, k, m, cols)

    # score_into, then the materialised Maximum / Threshold
    scores = lm.StripedScores.empty(pli, cols)
    pli.score_rows_into(pssm, seq, range(0, seq.rows), scores)
    got = scores.matrix()
    assert got.shape == want.shape and scores.max_index == want_mi
    assert same(got[:, :cols], want[:, :cols]), ("scores", ctx, pli.last_kernel)
    assert pli.last_kernel in store_kernels(m, cols, options), ("store kernel", ctx, pli.last_kernel)
    want_am = co.argmax(want, cols)
    wmax = co.max_(want, cols)
    assert pli.argmax(scores) == want_am, ctx
    gmax = pli.max(scores)
    assert (gmax is None) == (wmax is None)
    if wmax is not None:
        assert same(gmax, wmax), ctx

    # fused argmax
    fused = pli.score_argmax(pssm, seq)
    assert fused is not None and fused[0] == want_am, ("fused argmax", ctx, fused, want_am, pli.last_kernel)
    assert same(fused[1], want[want_am]), ("fused argmax value", ctx, pli.last_kernel)

    # thresholds: materialised and fused, row-major order, values bit for bit
    for t in xw.thresholds(want, cols, pssm_np, k, xw.extra_thresholds(regime)):
        wrc = rc_list(co.threshold(want, cols, t))        # (NaN: `x >= NaN` selects nothing, as the reference's `>=`)
        assert pli.threshold(scores, t) == wrc, ("threshold", ctx, t)
        frc, fval = pli.score_threshold(pssm, seq, t)
        assert frc == wrc, ("fused threshold", ctx, t, pli.last_kernel, len(frc), len(wrc))
        assert np.array_equal(bits(fval), bits([want[r, c] for r, c in wrc])), ("fused values", ctx, t)
    # which kernel the fused threshold takes at a realised score (a store call first resets last_kernel), and how many
    # motif rows its scan read (the drop-last form reads M - 1 when the last row carries at most a quarter of the bound)
    tq = xw.quantile_threshold(want, cols)
    pli.score_rows_into(pssm, seq, range(0, seq.rows), scores)
    pli.score_threshold(pssm, seq, tq)
    kernel, scanned = pli.last_kernel, pli.last_scan_info[0]
    if fast_expected(fast, pssm_np, k, tq):
        assert kernel == fast, ("route not reached", ctx, kernel)
        if fast == "score_c32_prefilter2" and k == 5 and m >= 20 and m % 4 == 0 and m <= 36:
            d = xw.discrete_weights(pssm_np, k)
            td = min(xw.prefilter_td(pssm_np, k, tq), 65535)
            drop = options.get("drop_last", 1) and 4 * d[-1].max() <= td
            assert scanned == (m - 1 if drop else m), ("drop-last form", ctx, scanned, drop)
    else:
        assert not kernel.startswith("score_c32_prefilter"), ("prefilter without a sound image", ctx, kernel)
        names = exact_threshold_kernels(m, cols, options)
        if names is None:
            assert kernel != "score_generic<2>", ("chunked route not taken", ctx, kernel)
        else:
            assert kernel in names, ("exact route", ctx, kernel, names)


CASES = [(route, r, v, m) for route, (_, _, lengths, _, _) in ROUTES.items() for r, v in xw.REGIMES
         for m in lengths if m >= xw.min_length(r)]


@pytest.mark.parametrize("route,regime,variant,m", CASES,
                         ids=[f"{route}-{xw.regime_id(r, v)}-M{m}" for route, r, v, m in CASES])
def test_route_against_the_oracle(route, regime, variant, m):
    options, k, _, cols, fast = ROUTES[route]
    if fast == "score_c32_prefilter2" and m == 1:
        fast = "score_c32_prefilter"   # one row: no pair to look up
    pli = pipeline(options)
    check_case(pli, regime, variant, k, m, cols, fast, options)


# ---- an unaligned device pointer: the one-symbol scan with byte loads -----------------------------------------------

UNALIGNED = [(r, v) for r, v in xw.REGIMES if r != "overflow_nan"]


@pytest.mark.parametrize("regime,variant", UNALIGNED, ids=[xw.regime_id(r, v) for r, v in UNALIGNED])
def test_unaligned_sequence_pointer(regime, variant):
    k, m, cols = 5, 12, 32
    pli = pipeline({})
    pssm_np = xw.make_pssm(regime, variant, m, k)
    enc = xw.make_sequence(regime, variant, LENGTH, k, m)
    s, want, _ = oracle_case(enc, pssm_np, k, cols)
    rows = want.shape[0]
    total = rows + m - 1
    host = np.ascontiguousarray(s.data[:total, :cols])
    buf = torch.zeros(total * cols + 8, dtype=torch.uint8, device="cuda:0")
    buf[1:1 + total * cols] = torch.from_numpy(host.reshape(-1)).to("cuda:0")
    ptr = buf.data_ptr() + 1
    pssm = lm.ScoringMatrix(pssm_np)
    tq = xw.quantile_threshold(want, cols)
    for t in [tq] + xw.thresholds(want, cols, pssm_np, k, xw.extra_thresholds(regime)):
        wrc = rc_list(co.threshold(want, cols, t))
        got = pli.score_threshold_dptr(pssm, ptr, total, cols, cols, m - 1, len(enc), 0, rows, t)
        assert rc_list(got[0]) == wrc, (regime, variant, t, pli.last_kernel)
        assert np.array_equal(bits(got[1]), bits([want[r, c] for r, c in wrc]))
        if t is tq:
            if fast_expected("score_c32_prefilter", pssm_np, k, t):
                assert pli.last_kernel == "score_c32_prefilter", pli.last_kernel
            else:
                assert not pli.last_kernel.startswith("score_c32_prefilter"), pli.last_kernel
    am = pli.score_argmax_dptr(pssm, ptr, total, cols, cols, m - 1, len(enc), 0, rows)
    assert am[0] == co.argmax(want, cols)


# ---- batches: several motifs of one length per launch --------------------------------------------------------------

BATCH = [(r, v, m, multi) for r, v in xw.REGIMES for m in ((8, 12) if r != "tiny_range" else (12,)) for multi in (1, 0)]


@pytest.mark.parametrize("regime,variant,m,multi", BATCH,
                         ids=[f"{xw.regime_id(r, v)}-M{m}-multi{multi}" for r, v, m, multi in BATCH])
def test_batch_against_the_oracle(regime, variant, m, multi):
    k, cols = 5, 32
    pli = pipeline({"multi_motif": multi})
    enc = xw.make_sequence(regime, variant, LENGTH, k, m)
    mats = [xw.make_pssm(regime, variant, m, k, seed) for seed in range(3)]
    wants = [oracle_case(enc, p, k, cols)[1] for p in mats]
    seq = pli.stripe(lm.EncodedSequence(enc), cols)
    seq.configure_wrap(m - 1)
    pssms = [lm.ScoringMatrix(p) for p in mats]
    am = pli.scan_argmax_batch(pssms, seq)
    for i, want in enumerate(wants):
        wa = co.argmax(want, cols)
        assert am[i][0] == wa and same(am[i][1], want[wa]), (i, am[i], wa, pli.last_kernel)
    per_motif = [xw.thresholds(w, cols, p, k, xw.extra_thresholds(regime)) for w, p in zip(wants, mats)]
    for j in range(max(len(t) for t in per_motif)):
        ts = [t[min(j, len(t) - 1)] for t in per_motif]
        hits = pli.scan_threshold_batch(pssms, ts, seq)
        if j == 8:   # each motif at a realised score of its own: one group, the pair scan (multi-motif passes) or exact
            fast = [fast_expected("score_c32_prefilter2", p, k, t) for p, t in zip(mats, ts)]
            if all(fast):
                assert pli.last_kernel == ("score_c32_prefilter2_multi" if multi else "score_c32_prefilter2"), pli.last_kernel
            elif not any(fast):
                assert pli.last_kernel == f"score_c32<{m},2>", pli.last_kernel
        for i, want in enumerate(wants):
            coords, values = hits[i]
            wrc = rc_list(co.threshold(want, cols, ts[i]))
            assert rc_list(coords) == wrc, (i, ts[i], pli.last_kernel, len(coords), len(wrc))
            assert np.array_equal(bits(values), bits([want[r, c] for r, c in wrc]))


# ---- Scanner: positions / scores against the f32 oracle, max() against the host walk --------------------------------

SCAN = [(r, v, m) for r, v in xw.REGIMES for m in (max(xw.min_length(r), 3), 20)]


@pytest.mark.parametrize("regime,variant,m", SCAN, ids=[f"{xw.regime_id(r, v)}-M{m}" for r, v, m in SCAN])
def test_scanner(regime, variant, m):
    k, cols = 5, 32
    pli = pipeline({})
    pssm_np = xw.make_pssm(regime, variant, m, k)
    enc = xw.make_sequence(regime, variant, LENGTH, k, m)
    _, want, _ = oracle_case(enc, pssm_np, k, cols)
    seq = pli.stripe(lm.EncodedSequence(enc), cols)
    seq.configure_wrap(m - 1)
    pssm = lm.ScoringMatrix(pssm_np)
    by_pos = want[:, :cols].T.reshape(-1)[: len(enc) - m + 1]
    tq = xw.quantile_threshold(want, cols)
    pli.score(pssm, seq)   # (resets last_kernel to a store kernel)
    for t in [tq, xw.FLT_MAX, 3.2e38, 0.0, xw.TINY]:
        sc = lm.Scanner(pssm, seq, threshold=t)
        if t is tq:
            sc.positions
            assert pli.last_kernel.startswith("score_c32_prefilter") == fast_expected("score_c32_prefilter2", pssm_np, k, t), \
                pli.last_kernel
        wpos = np.nonzero(by_pos >= np.float32(t))[0]
        assert sc.positions.tolist() == wpos.tolist(), (t, pli.last_kernel)
        assert np.array_equal(bits(sc.scores), bits(by_pos[wpos]))

    def walk(fn):
        try:
            hit = fn()
            return None if hit is None else (hit.position, int(bits([hit.score])[0]))
        except IndexError:   # a candidate window past the matrix: the reference panics there, both walks refuse
            return "IndexError"
    for sat in (True, False):
        got = walk(lambda: lm.Scanner(pssm, seq, threshold=tq).max(sat))
        host = walk(lambda: scanner_max_strict_host(lm.Scanner(pssm, seq, threshold=tq), sat))
        assert got == host, (sat, got, host)


# ---- the suffix route of the fused argmax (sparse form: a threshold scan at t = B over the last rows) ----------------

SUFFIX = [(r, v) for r, v in xw.REGIMES if r in ("overflow_inf", "near_overflow", "wide_range", "subnormal")]


@pytest.mark.parametrize("regime,variant", SUFFIX, ids=[xw.regime_id(r, v) for r, v in SUFFIX])
def test_suffix_argmax(regime, variant):
    """DNA M = 8 over 2.2 Mbp: the best k-mer is expected ~32 times, so the fused argmax scans only a suffix of the
    rows at t = B (score_argmax.hip: argmax_by_suffix, by argmax_plan.hpp: suffix_choice) when B is finite and the prefilter is sound."""
    k, m, cols = 5, 8, 32
    pssm_np = xw.make_pssm(regime, variant, m, k)
    enc = xw.make_sequence(regime, variant, 2_200_000, k, m)
    enc[enc == k - 1] = 0   # no N: every k-mer is as frequent as in the suffix model
    _, want, _ = oracle_case(enc, pssm_np, k, cols)
    wa = co.argmax(want, cols)
    for options in ({}, {"suffix_argmax": 0}):
        pli = pipeline(options)
        seq = pli.stripe(lm.EncodedSequence(enc), cols)
        seq.configure_wrap(m - 1)
        pssm = lm.ScoringMatrix(pssm_np)
        got = pli.score_argmax(pssm, seq)
        assert got[0] == wa and same(got[1], want[wa]), (options, got, wa, pli.last_kernel)
        b = xw.kmer_bound(pssm_np, k)
        if not options and xw.prefilter_sound(pssm_np, k) and np.isfinite(b) and want[wa] == b:
            assert pli.last_kernel == "score_c32_prefilter2", pli.last_kernel   # the suffix's threshold scan


# ---- the candidate route of the fused argmax (>= 100 M cells) -------------------------------------------------------

TRACE = re.compile(r"candidate-route argmax: (\d+) jobs, (\d+) candidates \(room (\d+)\), (\d+) hits \(room (\d+)\)")


def test_candidate_route_argmax_at_101_mbp(capfd):
    """The reference's argmax is a planted +inf window whose real sum (~0.6e38) lies below the sample's bound: an image
    of real sums cannot flag it (checked here on the host with the image's own arithmetic), so the overflowing matrix
    must take the exact kernel.  The same shape under the no-overflow limit must settle on the candidate route."""
    k, m, cols = 5, xw.PLANT_M, xw.PLANT_COLS
    num_cus = torch.cuda.get_device_properties(0).multi_processor_count
    enc, plants = xw.planted_argmax_sequence(num_cus)
    s = co.stripe(enc, cols, k)
    co.configure_wrap(s, m - 1)
    sample, _ = xw.sampled_rows(s.rows, num_cus)
    pli = pipeline({})
    seq = pli.stripe(lm.EncodedSequence(enc), cols)
    seq.configure_wrap(m - 1)
    os.environ["LM_HIP_TRACE"] = "1"
    try:
        for overflow in (True, False):
            pssm_np = xw.planted_argmax_pssm(overflow)
            assert xw.prefilter_sound(pssm_np, k) == (not overflow)
            want, _ = co.score_rows(s, pssm_np)
            wa = co.argmax(want, cols)
            assert np.isposinf(want[wa]) == overflow and (wa == max(plants) or not overflow)
            bound = want[sample, :cols]
            assert not np.isnan(bound).any() and not np.isposinf(bound).any()   # (-inf: T + T)
            if overflow:   # the image without the limit would not flag the answer at the sample's bound
                assert xw.unflagged_near(enc, pssm_np, wa, float(np.max(bound[np.isfinite(bound)])))
            capfd.readouterr()
            got = pli.score_argmax(lm.ScoringMatrix(pssm_np), seq)
            trace = capfd.readouterr().err
            assert got[0] == wa and same(got[1], want[wa]), (overflow, got, wa, want[wa], trace)
            found = TRACE.search(trace)
            if overflow:
                assert found is None, trace   # no sound image: the exact kernel
            else:   # the route settled the job: neither list was truncated
                assert found is not None, trace
                _, ncand, ccap, nhits, cap = map(int, found.groups())
                assert ncand <= ccap and 0 < nhits <= cap, trace
            del want, bound
    finally:
        del os.environ["LM_HIP_TRACE"]
