#!/usr/bin/env python3
"""Many motifs x many short records: what a resident sequence set saves over the per-record loop.

Three ways to produce the same hit lists, timed on one MI355X in ONE process, alternating, after a warm-up:

  A  the loop the CLI ran before sequence sets existed: per record ``stripe_ascii`` + ``configure_wrap`` +
     ``scan_threshold_batch`` (prepared ``MotifBatch``) + the ``pos + M <= L`` cut and the sort on the host;
  B  ``stripe_ascii_set`` + ``scan_threshold_set`` on the same records (one upload, one call, the cut on the device);
  C  ``stripe_ascii`` + ``scan_threshold_batch`` on the plain concatenation: no segment pass, no offsets -- the floor
     B cannot beat (its hit list is NOT the answer: it holds the windows that straddle records).

Cases: (i) 2 000 records x 500 bp x 64 JASPAR motifs, (ii) 50 000 records x 200 bp x all 2 346 matrices of
tests/golden/JASPAR2024.pwm.gz; thresholds at p = 1e-5.  Reports median and spread (min, max) of every way, the ratios
A/B and B/C, the share of call C that its tail takes (re-score + order + host, ``lm_hip_ctx_last_phases_ms``), and the
sustained shader clock.  ``python tools/seqset_bench.py [--case i|ii|both] [--runs 7] [--out profiles/seqset_bench.json]``

``--best`` measures the best-hit-per-record matrix instead (``measure_best``; 2 000 records x 500 bp x 8 motifs, the set
resident, the calls alone timed) and writes ``profiles/seqset_best_bench.json``:

  A'  ``scan_threshold_set`` at thresholds of -inf + the reduction per (motif, record) in numpy: the cheapest single
      call that gave the answer before ``scan_best_set`` existed (a 16-byte hit for every window of every motif);
  B'  ``scan_best_set``;
  C'  ``scan_argmax_batch`` over the plain concatenation: the bare fused argmax, no segmentation -- not the answer.

``--count`` measures the hits per (motif, record) on the same set at p = 1e-1 ... 1e-5 (``measure_count``: the list plus a
``bincount`` per motif, ``scan_count_set``, and ``scan_best_set`` as the walk's floor) and writes
``profiles/seqset_count_bench.json``.

``--sum`` measures the total odds per (motif, record) on the same set (``measure_sum``: the list at -inf plus ``exp2`` and a
sum per record on the host, ``scan_sum_set``, and ``scan_count_set`` as the walk with the cheapest reducer; then
``scan_sum_set`` and ``scan_count_set`` on 2 000 records x 50 000 bp, where a record spans many lane runs and the merge of the
partial sums has work) and writes ``profiles/seqset_sum_bench.json``.

``--best --per-length`` / ``--count --per-length`` time the walk kernels one motif length at a time (``measure_per_length``:
the same resident set, 8 seeded random motifs of one length M per call, M = 1 ... 36, 40 and 70, medians of ``--runs``)
and write the series to ``--out``; ``--combine-ab P1 N1 P2 N2`` turns four such files per reduction -- parent, new,
parent, new, each run with ``LM_HIP_LIBRARY`` pointing at its build -- into ``profiles/seqset_walk_ab.json``: per
reduction the margin (the largest relative difference between the two parent series at any length) and, per length, the
ratio of the new medians to the parent's.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

import lightmotif_amd as lm  # noqa: E402
from lightmotif_amd import io as lmio  # noqa: E402

CASES = {"i": (2_000, 500, 64), "ii": (50_000, 200, None)}


def load_motifs(count=None, pvalue=1e-5):
    recs = list(lmio.read(ROOT / "tests" / "golden" / "JASPAR2024.pwm.gz"))
    if count is not None:                         # spread over the file: all motif lengths take part
        recs = [recs[i] for i in np.linspace(0, len(recs) - 1, count).astype(int)]
    pssms = [r.matrix.normalize(0.1).log_odds() for r in recs]
    return pssms, [p.score_for_pvalue(pvalue) for p in pssms]


def make_records(n, length, seed=5):
    rng = np.random.default_rng(seed)
    text = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n * length)]
    return [text[i * length:(i + 1) * length] for i in range(n)], text


def run_loop(pli, records, batch, lengths, max_m):
    """A: returns the number of hits (the lists are built and dropped, as the CLI consumes them record by record)."""
    total = 0
    for text in records:
        seq = pli.stripe_ascii(text, lossy=True)
        seq.configure_wrap(max_m)
        rows, n = seq.rows, len(seq)
        res = pli.scan_threshold_batch(batch, None, seq)
        for (coords, values), m in zip(res, lengths):
            pos = coords[:, 1] * rows + coords[:, 0]
            keep = pos + m <= n
            pos, values = pos[keep], values[keep]
            order = np.argsort(pos, kind="stable")
            pos, values = pos[order], values[order]
            total += len(pos)
    return total


def run_set(pli, joined, offsets, batch, max_m):
    """B"""
    seqset = pli.stripe_ascii_set(joined, lossy=True, offsets=offsets)
    seqset.configure_wrap(max_m)
    return pli.scan_threshold_set(batch, None, seqset).total


def run_plain(pli, joined, batch, max_m):
    """C"""
    seq = pli.stripe_ascii(joined, lossy=True)
    seq.configure_wrap(max_m)
    return pli.scan_threshold_batch(batch, None, seq).total


def timed(fn):
    t0 = time.perf_counter()
    n = fn()
    return (time.perf_counter() - t0) * 1e3, n


def measure(pli, n_records, length, n_motifs, runs=7, warmup=2, with_loop=True, loop_records=None):
    """`loop_records`: A runs over the first so many records only and its time is scaled to all of them (the loop is
    per record by construction; 50 000 records x 2 346 motifs spend minutes in its host code alone)."""
    pssms, ts = load_motifs(n_motifs)
    batch = pli.prepare_batch(pssms, ts)
    lengths = [len(p) for p in pssms]
    max_m = max(lengths)
    records, joined = make_records(n_records, length)
    offsets = np.arange(n_records + 1, dtype=np.uint64) * np.uint64(length)
    ways = {"B": lambda: run_set(pli, joined, offsets, batch, max_m), "C": lambda: run_plain(pli, joined, batch, max_m)}
    if with_loop:
        ways["A"] = lambda: run_loop(pli, records[:loop_records] if loop_records else records, batch, lengths, max_m)
    times = {k: [] for k in ways}
    hits = {}
    for it in range(warmup + runs):
        for k in sorted(ways):                    # alternating: A, B, C, A, B, C ...
            if k != "A":
                # steady state: the library sizes a call's hit list and its ordering from the previous call on the
                # context.  The CLI scans set after set of similar size; here the previous call would be the last tiny
                # record of A (or the other way's list), so every timed B / C call follows an untimed one of its own kind
                ways[k]()
            ms, n = timed(ways[k])
            hits[k] = n
            if it >= warmup:
                times[k].append(ms)
    # the tail's share of call C, from the library's own phase clocks
    pli.set_option("time_scan", 1)
    run_plain(pli, joined, batch, max_m)
    phases = pli.last_phases_ms
    pli.set_option("time_scan", 0)
    out = {"records": n_records, "record_length": length, "motifs": len(pssms), "runs": runs, "warmup": warmup, "hits": hits,
           "ms": {k: {"median": statistics.median(v), "min": min(v), "max": max(v), "all": [round(x, 3) for x in v]}
                  for k, v in times.items()}}
    med = {k: out["ms"][k]["median"] for k in times}
    if "A" in med and loop_records and loop_records < n_records:
        out["A_measured_on_records"] = loop_records
        out["A_scaled_median_ms"] = med["A"] * n_records / loop_records
        med["A"] = out["A_scaled_median_ms"]
    if "A" in med:
        out["A_over_B"] = med["A"] / med["B"]
    out["B_over_C"] = med["B"] / med["C"]
    if phases and phases[0] >= 0:
        tail = sum(max(x, 0.0) for x in phases[1:])
        out["C_phases_ms"] = [round(float(x), 4) for x in phases]
        out["C_tail_share"] = tail / (tail + phases[0]) if tail + phases[0] > 0 else None
    return out


def reduce_hits(res, n_records):
    """A': (found, position, score) of shape (motifs, records) from a ``SetHits`` that holds every window: per record the
    greatest score and the first position holding it (the lists are ascending in (record, position))."""
    n = len(res)
    found = np.zeros((n, n_records), dtype=bool)
    position = np.full((n, n_records), -1, dtype=np.int64)
    score = np.full((n, n_records), np.nan, dtype=np.float32)
    for mi in range(n):
        rec, pos, val = res[mi]
        keep = ~np.isnan(val)                     # NaN windows never compete
        rec, pos, val = rec[keep], pos[keep], val[keep]
        if not len(rec):
            continue
        starts = np.flatnonzero(np.concatenate(([True], rec[1:] != rec[:-1])))
        best = np.maximum.reduceat(val, starts)
        seg = np.cumsum(np.concatenate(([0], (rec[1:] != rec[:-1]).astype(np.int64))))
        at = np.flatnonzero(val == best[seg])     # ascending: the first of a record is its lowest position
        first = at[np.concatenate(([True], rec[at][1:] != rec[at][:-1]))]
        found[mi, rec[first]] = True
        position[mi, rec[first]] = pos[first]
        score[mi, rec[first]] = val[first]
    return found, position, score


def measure_best(pli, n_records, length, n_motifs, runs=5, warmup=1):
    """A', B', C' (module docstring) on one resident set, alternating, medians of `runs` after `warmup`; the answers of A'
    and B' are compared first."""
    pssms, _ = load_motifs(n_motifs)
    lengths = [len(p) for p in pssms]
    max_m = max(lengths)
    _, joined = make_records(n_records, length)
    offsets = np.arange(n_records + 1, dtype=np.uint64) * np.uint64(length)
    seqset = pli.stripe_ascii_set(joined, lossy=True, offsets=offsets)
    seqset.configure_wrap(max_m)
    plain = pli.stripe_ascii(joined, lossy=True)
    plain.configure_wrap(max_m)
    dense = pli.prepare_batch(pssms, [-np.inf] * len(pssms))
    batch = pli.prepare_batch(pssms)

    kernels = set()

    def way_a():
        res = pli.scan_threshold_set(dense, None, seqset)
        return res.total, reduce_hits(res, n_records)

    def way_b():
        res = pli.scan_best_set(batch, seqset)
        kernels.add(res.last_kernel)
        return res.found.size, (res.found, res.position, res.score)

    def way_c():
        return len(pli.scan_argmax_batch(pssms, plain)), None

    (hits_a, a), (_, b) = way_a(), way_b()
    same = bool(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and
                np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32)))
    ways = {"A": way_a, "B": way_b, "C": way_c}
    times = {k: [] for k in ways}
    for it in range(warmup + runs):
        for k in sorted(ways):
            if k == "A":
                ways[k]()                         # steady state, as in measure(): the hit list is sized from the call before
            t0 = time.perf_counter()
            ways[k]()
            if it >= warmup:
                times[k].append((time.perf_counter() - t0) * 1e3)
    out = {"records": n_records, "record_length": length, "motifs": len(pssms), "motif_lengths": lengths, "runs": runs,
           "warmup": warmup, "answers_equal": same, "windows": int(hits_a), "found": int(b[0].sum()), "kernel": sorted(kernels),
           "ms": {k: {"median": statistics.median(v), "min": min(v), "max": max(v), "all": [round(x, 3) for x in v]}
                  for k, v in times.items()}}
    out["A_over_B"] = out["ms"]["A"]["median"] / out["ms"]["B"]["median"]
    out["B_over_C"] = out["ms"]["B"]["median"] / out["ms"]["C"]["median"]
    return out


def main_best(a):
    pli = lm.Pipeline.hip(0)
    res = measure_best(pli, 2_000, 500, 8, runs=a.runs, warmup=2)
    out = a.out if a.out != str(ROOT / "profiles" / "seqset_bench.json") else str(ROOT / "profiles" / "seqset_best_bench.json")
    result = {"tool": "tools/seqset_bench.py --best", "device": "MI355X (gfx950)", "case": res}
    Path(out).parent.mkdir(parents=True, exist_ok=True)
    Path(out).write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps({"A_over_B": res["A_over_B"], "B_over_C": res["B_over_C"], "answers_equal": res["answers_equal"], "wrote": out}))
    return 0 if res["answers_equal"] else 1


COUNT_PVALUES = (1e-1, 1e-2, 1e-3, 1e-4, 1e-5)
COUNT_LEVELS3 = (1e-1, 1e-2, 1e-3)


def count_hits(res, n_records, cuts=None):
    """A: ``(motifs, levels, records)`` counts from a ``SetHits``: per motif one ``bincount`` of the record column (with
    ``cuts`` -- ``(motifs, levels)`` thresholds -- one per level, over the hits that reach it)."""
    n = len(res)
    out = np.zeros((n, 1 if cuts is None else cuts.shape[1], n_records), dtype=np.uint32)
    for mi in range(n):
        rec, _, val = res[mi]
        if cuts is None:
            out[mi, 0] = np.bincount(rec, minlength=n_records)
        else:
            for li in range(cuts.shape[1]):
                out[mi, li] = np.bincount(rec[val >= cuts[mi, li]], minlength=n_records)
    return out


def alternate(ways, runs, warmup, untimed_first=("A",)):
    """Medians of `runs` alternating calls of every way after `warmup` rounds; the ways of `untimed_first` follow an
    untimed call of their own kind (the hit list is sized from the call before, as in measure())."""
    times = {k: [] for k in ways}
    for it in range(warmup + runs):
        for k in sorted(ways):
            if k in untimed_first:
                ways[k]()
            t0 = time.perf_counter()
            ways[k]()
            if it >= warmup:
                times[k].append((time.perf_counter() - t0) * 1e3)
    return {k: {"median": statistics.median(v), "min": min(v), "max": max(v), "all": [round(x, 3) for x in v]} for k, v in times.items()}


def measure_count(pli, n_records, length, n_motifs, runs=5, warmup=1):
    """Hits per (motif, record) at p = 1e-1 ... 1e-5 on one resident set, three legs per p, alternating, medians of `runs`
    after `warmup`, the answers of A and B compared first:

      A   ``scan_threshold_set`` at the thresholds + one ``bincount`` per motif: the cheapest way before ``scan_count_set``;
      B   ``scan_count_set`` with one level;
      C   ``scan_best_set`` of the same motifs: the same walk with another reduction, so B / C is the price of counting.

    ``three_levels``: ``scan_count_set`` at (1e-1, 1e-2, 1e-3) in one call (B3) against the list at 1e-1 plus the three
    counts on the host (A3).  ``crossover_p``: the largest p of the sweep at which A is faster than B (None: nowhere)."""
    pssms, _ = load_motifs(n_motifs)
    lengths = [len(p) for p in pssms]
    max_m = max(lengths)
    _, joined = make_records(n_records, length)
    offsets = np.arange(n_records + 1, dtype=np.uint64) * np.uint64(length)
    seqset = pli.stripe_ascii_set(joined, lossy=True, offsets=offsets)
    seqset.configure_wrap(max_m)
    dists = pli.score_distributions(pssms)
    batch = pli.prepare_batch(pssms)
    kernels = set()

    def way_c():
        return pli.scan_best_set(batch, seqset)

    sweep = []
    for p in COUNT_PVALUES:
        ts = dists.thresholds(p)
        listed = pli.prepare_batch(pssms, ts)

        def way_a():
            return count_hits(pli.scan_threshold_set(listed, None, seqset), n_records)

        def way_b():
            res = pli.scan_count_set(batch, ts, seqset)
            kernels.add(res.last_kernel)
            return res.counts

        a, b = way_a(), way_b()
        ms = alternate({"A": way_a, "B": way_b, "C": way_c}, runs, warmup)
        sweep.append({"p": p, "answers_equal": bool(np.array_equal(a, b)), "hits": int(b.sum(dtype=np.int64)), "ms": ms,
                      "A_over_B": ms["A"]["median"] / ms["B"]["median"], "B_over_C": ms["B"]["median"] / ms["C"]["median"]})

    cuts = np.stack([dists.thresholds(p) for p in COUNT_LEVELS3], axis=1)
    loosest = pli.prepare_batch(pssms, cuts.min(axis=1))

    def way_a3():
        return count_hits(pli.scan_threshold_set(loosest, None, seqset), n_records, cuts)

    def way_b3():
        return pli.scan_count_set(batch, cuts, seqset).counts

    a3, b3 = way_a3(), way_b3()
    ms3 = alternate({"A": way_a3, "B": way_b3}, runs, warmup)
    three = {"p": list(COUNT_LEVELS3), "answers_equal": bool(np.array_equal(a3, b3)), "ms": {"A3": ms3["A"], "B3": ms3["B"]},
             "A3_over_B3": ms3["A"]["median"] / ms3["B"]["median"]}
    a_wins = [row["p"] for row in sweep if row["ms"]["A"]["median"] < row["ms"]["B"]["median"]]
    windows = int(sum(max(0, length - m + 1) for m in lengths)) * n_records
    return {"records": n_records, "record_length": length, "motifs": len(pssms), "motif_lengths": lengths, "runs": runs, "warmup": warmup,
            "windows": windows, "kernel": sorted(kernels), "answers_equal": all(r["answers_equal"] for r in sweep) and three["answers_equal"],
            "sweep": sweep, "three_levels": three, "crossover_p": max(a_wins) if a_wins else None}


def main_count(a):
    pli = lm.Pipeline.hip(0)
    res = measure_count(pli, 2_000, 500, 8, runs=a.runs, warmup=2)
    out = a.out if a.out != str(ROOT / "profiles" / "seqset_bench.json") else str(ROOT / "profiles" / "seqset_count_bench.json")
    result = {"tool": "tools/seqset_bench.py --count", "device": "MI355X (gfx950)", "case": res}
    Path(out).parent.mkdir(parents=True, exist_ok=True)
    Path(out).write_text(json.dumps(result, indent=1) + "\n")
    for row in res["sweep"]:
        print(json.dumps({"p": row["p"], "hits": row["hits"], "A_ms": round(row["ms"]["A"]["median"], 3), "B_ms": round(row["ms"]["B"]["median"], 3),
                          "C_ms": round(row["ms"]["C"]["median"], 3), "A_over_B": round(row["A_over_B"], 2), "B_over_C": round(row["B_over_C"], 2)}))
    print(json.dumps({"A3_over_B3": res["three_levels"]["A3_over_B3"], "crossover_p": res["crossover_p"], "answers_equal": res["answers_equal"],
                      "wrote": out}))
    return 0 if res["answers_equal"] else 1


def host_sums(res, n_records):
    """Leg A of measure_sum: ``(motifs, records)`` f64 from a ``SetHits`` at -inf -- ``2 ** score`` of every window in f64
    and one weighted ``bincount`` per motif."""
    out = np.zeros((len(res), n_records), dtype=np.float64)
    for mi in range(len(res)):
        rec, _, val = res[mi]
        out[mi] = np.bincount(rec, weights=np.exp2(val.astype(np.float64)), minlength=n_records)
    return out


def measure_sum(pli, n_records, length, n_motifs, runs=5, warmup=1, long_length=50_000):
    """Total odds per (motif, record) on one resident set, three legs, alternating, medians of `runs` after `warmup`:

      A   ``scan_threshold_set`` at -inf + ``np.exp2`` + one weighted ``bincount`` per motif: the only way before
          ``scan_sum_set`` (a 16-byte hit for every window of every motif);
      B   ``scan_sum_set``;
      C   ``scan_count_set`` at one level (p = 1e-3): the same walk with the cheapest reducer, so B / C is the price of the
          exponential, the f64 add and the merge.

    ``worst_relative_error``: B against A's f64 sums of ``2 ** score`` (the f64 rule; A's own rounding is n * 2^-53).
    ``long``: B and C on `n_records` records of `long_length` bp (None: skipped), where every record spans many lane runs."""
    pssms, _ = load_motifs(n_motifs)
    lengths = [len(p) for p in pssms]
    max_m = max(lengths)
    dists = pli.score_distributions(pssms)
    cuts = dists.thresholds(1e-3)
    batch = pli.prepare_batch(pssms)
    everything = pli.prepare_batch(pssms, [-np.inf] * len(pssms))
    kernels = set()

    def legs(seqset):
        def way_a():
            return host_sums(pli.scan_threshold_set(everything, None, seqset), n_records)

        def way_b():
            res = pli.scan_sum_set(batch, seqset)
            kernels.add(res.last_kernel)
            return res.sums

        def way_c():
            return pli.scan_count_set(batch, cuts, seqset).counts
        return way_a, way_b, way_c

    _, joined = make_records(n_records, length)
    offsets = np.arange(n_records + 1, dtype=np.uint64) * np.uint64(length)
    seqset = pli.stripe_ascii_set(joined, lossy=True, offsets=offsets)
    seqset.configure_wrap(max_m)
    way_a, way_b, way_c = legs(seqset)
    a, b = way_a(), way_b()
    worst = float(np.max(np.abs(b - a) / a))
    repeat_equal = way_b().tobytes() == b.tobytes()
    ms = alternate({"A": way_a, "B": way_b, "C": way_c}, runs, warmup)
    windows = int(sum(max(0, length - m + 1) for m in lengths)) * n_records
    out = {"records": n_records, "record_length": length, "motifs": len(pssms), "motif_lengths": lengths, "runs": runs, "warmup": warmup,
           "windows": windows, "ms": ms, "A_over_B": ms["A"]["median"] / ms["B"]["median"], "B_over_C": ms["B"]["median"] / ms["C"]["median"],
           "worst_relative_error": worst, "tolerance": 2.0 ** -21, "within_tolerance": worst <= 2.0 ** -21, "repeat_bit_identical": repeat_equal}
    if long_length:
        del seqset
        _, joined = make_records(n_records, long_length)
        offsets = np.arange(n_records + 1, dtype=np.uint64) * np.uint64(long_length)
        seqset = pli.stripe_ascii_set(joined, lossy=True, offsets=offsets)
        seqset.configure_wrap(max_m)
        _, way_b, way_c = legs(seqset)
        first = way_b()
        ms_long = alternate({"B": way_b, "C": way_c}, runs, warmup, untimed_first=())
        out["long"] = {"records": n_records, "record_length": long_length, "ms": ms_long,
                       "B_over_C": ms_long["B"]["median"] / ms_long["C"]["median"], "repeat_bit_identical": way_b().tobytes() == first.tobytes(),
                       "ns_per_window": {k: v["median"] * 1e6 / (sum(max(0, long_length - m + 1) for m in lengths) * n_records)
                                         for k, v in ms_long.items()}}
    out["kernel"] = sorted(kernels)
    return out


def main_sum(a):
    pli = lm.Pipeline.hip(0)
    res = measure_sum(pli, 2_000, 500, 8, runs=a.runs, warmup=2)
    out = a.out if a.out != str(ROOT / "profiles" / "seqset_bench.json") else str(ROOT / "profiles" / "seqset_sum_bench.json")
    Path(out).parent.mkdir(parents=True, exist_ok=True)
    Path(out).write_text(json.dumps({"tool": "tools/seqset_bench.py --sum", "device": "MI355X (gfx950)", "case": res}, indent=1) + "\n")
    print(json.dumps({"A_ms": round(res["ms"]["A"]["median"], 3), "B_ms": round(res["ms"]["B"]["median"], 3), "C_ms": round(res["ms"]["C"]["median"], 3),
                      "A_over_B": round(res["A_over_B"], 2), "B_over_C": round(res["B_over_C"], 2), "worst_relative_error": res["worst_relative_error"]}))
    if "long" in res:
        print(json.dumps({"long_B_ms": round(res["long"]["ms"]["B"]["median"], 3), "long_C_ms": round(res["long"]["ms"]["C"]["median"], 3),
                          "long_B_over_C": round(res["long"]["B_over_C"], 2)}))
    print(json.dumps({"within_tolerance": res["within_tolerance"], "repeat_bit_identical": res["repeat_bit_identical"], "wrote": out}))
    return 0 if res["within_tolerance"] and res["repeat_bit_identical"] else 1


PER_LENGTH_MS = tuple(range(1, 37)) + (40, 70)


def measure_per_length(pli, which, n_records=2_000, length=500, n_motifs=8, runs=15, warmup=2):
    """Median ms of one ``scan_best_set`` / ``scan_count_set`` (one level, about 3 sigma of the random weights) call per
    motif length on the resident set of the other modes."""
    from lightmotif_amd.lib import stride as lm_stride
    _, joined = make_records(n_records, length)
    offsets = np.arange(n_records + 1, dtype=np.uint64) * np.uint64(length)
    seqset = pli.stripe_ascii_set(joined, lossy=True, offsets=offsets)
    seqset.configure_wrap(max(PER_LENGTH_MS))
    out = {}
    for m in PER_LENGTH_MS:
        rng = np.random.default_rng(7_000 + m)
        mats = []
        for _ in range(n_motifs):
            p = np.zeros((m, lm_stride(5, 4)), np.float32)
            p[:, :5] = rng.normal(0, 2, (m, 5))
            mats.append(lm.ScoringMatrix(p))
        batch = pli.prepare_batch(mats)
        cuts = np.full(n_motifs, 6.0 * np.sqrt(m), dtype=np.float32)
        call = (lambda: pli.scan_best_set(batch, seqset)) if which == "best" else (lambda: pli.scan_count_set(batch, cuts, seqset))
        times = []
        for it in range(warmup + runs):
            t0 = time.perf_counter()
            res = call()
            if it >= warmup:
                times.append((time.perf_counter() - t0) * 1e3)
        out[str(m)] = {"median": statistics.median(times), "min": min(times), "max": max(times), "kernel": res.last_kernel}
    return out


def main_per_length(a):
    which = "best" if a.best else "count"
    if a.out == str(ROOT / "profiles" / "seqset_bench.json"):
        raise SystemExit("--per-length: name the series' file with --out (one of the four --combine-ab reads)")
    res = measure_per_length(lm.Pipeline.hip(0), which, runs=a.runs)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps({"tool": f"tools/seqset_bench.py --{which} --per-length", "reduction": which, "runs": a.runs,
                                       "ms": res}, indent=1) + "\n")
    print(json.dumps({"reduction": which, "lengths": len(res), "wrote": a.out}))
    return 0


def main_combine_ab(a):
    """a.combine_ab: per reduction four files, parent, new, parent, new ("best:p1,n1,p2,n2 count:...")."""
    out = a.out if a.out != str(ROOT / "profiles" / "seqset_bench.json") else str(ROOT / "profiles" / "seqset_walk_ab.json")
    result = {"tool": "tools/seqset_bench.py --combine-ab", "reductions": {}}
    ok = True
    for spec in a.combine_ab:
        which, _, files = spec.partition(":")
        files = files.split(",")
        if which not in ("best", "count") or len(files) != 4:
            raise SystemExit(f"--combine-ab: `{spec}` is not best:P1,N1,P2,N2 or count:P1,N1,P2,N2")
        p1, n1, p2, n2 = [json.loads(Path(f).read_text())["ms"] for f in files]
        med = lambda s, m: s[m]["median"]
        margin = max(abs(med(p1, m) - med(p2, m)) / min(med(p1, m), med(p2, m)) for m in p1)
        parent = {m: statistics.median([med(p1, m), med(p2, m)]) for m in p1}
        new = {m: statistics.median([med(n1, m), med(n2, m)]) for m in p1}
        ratios = {m: new[m] / parent[m] for m in p1}
        worst = max(ratios, key=ratios.get)
        result["reductions"][which] = {"series": {"parent_1": p1, "new_1": n1, "parent_2": p2, "new_2": n2}, "margin": margin,
                                       "ratio_new_over_parent": ratios, "worst_length": int(worst), "worst_ratio": ratios[worst],
                                       "within_margin": ratios[worst] <= 1.0 + margin}
        ok = ok and ratios[worst] <= 1.0 + margin
        print(json.dumps({"reduction": which, "margin": round(margin, 4), "worst_length": int(worst), "worst_ratio": round(ratios[worst], 4)}))
    Path(out).write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps({"within_margin": ok, "wrote": out}))
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="both", choices=["i", "ii", "both"])
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--runs-ii", dest="loop_runs_ii", type=int, default=5, help="runs of case (ii)")
    ap.add_argument("--loop-records-ii", type=int, default=500, help="records the loop of case (ii) runs over (scaled to 50 000)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "seqset_bench.json"))
    ap.add_argument("--best", action="store_true", help="the best hit per record (measure_best) -> profiles/seqset_best_bench.json")
    ap.add_argument("--count", action="store_true", help="hits per (motif, record) (measure_count) -> profiles/seqset_count_bench.json")
    ap.add_argument("--sum", action="store_true", help="total odds per (motif, record) (measure_sum) -> profiles/seqset_sum_bench.json")
    ap.add_argument("--per-length", action="store_true", help="with --best / --count: one call per motif length (measure_per_length) -> --out")
    ap.add_argument("--combine-ab", nargs="+", metavar="REDUCTION:P1,N1,P2,N2", help="per-length files of an A/B session -> --out")
    a = ap.parse_args()
    if a.combine_ab:
        return main_combine_ab(a)
    if a.per_length and (a.best or a.count):
        return main_per_length(a)
    if a.best:
        return main_best(a)
    if a.count:
        return main_count(a)
    if a.sum:
        return main_sum(a)
    pli = lm.Pipeline.hip(0)
    result = {"tool": "tools/seqset_bench.py", "device": "MI355X (gfx950)", "cases": {}}
    for name in (["i", "ii"] if a.case == "both" else [a.case]):
        n_records, length, n_motifs = CASES[name]
        runs = a.runs if name == "i" else max(a.loop_runs_ii, 1)
        warm = 2 if name == "i" else 1
        res = measure(pli, n_records, length, n_motifs, runs=runs, warmup=warm, loop_records=a.loop_records_ii if name == "ii" else None)
        result["cases"][name] = res
        print(name, json.dumps({k: res[k] for k in ("A_over_B", "B_over_C", "C_tail_share", "hits") if k in res}), flush=True)
    try:
        joined = make_records(2_000, 500)[1]
        pssms, ts = load_motifs(64)
        batch = pli.prepare_batch(pssms, ts)
        clock = pli.sustained_clock_mhz(lambda: run_plain(pli, joined, batch, max(len(p) for p in pssms)))
        result["sustained_clock_mhz"] = clock if isinstance(clock, (int, float)) else list(clock) if clock is not None else None
    except Exception as exc:  # a diagnostic: the timings stand without it
        result["sustained_clock_mhz"] = f"unavailable: {exc}"
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps({"wrote": a.out}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
