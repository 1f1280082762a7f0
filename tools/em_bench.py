#!/usr/bin/env python
"""The E-step of motif EM on a resident set, three roads, written to ``profiles/em_bench.json``.

Cases: 2 000 records x 500 bp with 1, 8 and 64 JASPAR motifs, and 100 000 records x 200 bp with 8 motifs.  Per case, after
a warm-up, the legs alternate and each reports median, min, max and all times of ``--runs`` repeats:

  A        the host road: ``scan_threshold_set`` at -inf (every window a hit), ``StripedSequenceSet.windows`` of the hits,
           ``np.exp2`` and one ``np.add.at`` per motif -- the only way to the expected counts before
           ``expected_counts_set`` (timed on the small cases only, and with fewer repeats: it takes seconds);
  B_flat   ``expected_counts_set`` at a flat first-iteration matrix (all weights 0: every window is live and pays the
           scatter of its M symbols), gains 1 / windows;
  B_loaded ``expected_counts_set`` at the matrices as loaded with OOPS gains: nearly every posterior quantises to 0 and
           is skipped;
  C        ``scan_sum_set`` of the same job: the same walk with one f64 add per window instead of the scatter.

A's table is compared with B's (B_loaded, the same matrices and gains) within the bound of the tests."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(Path(__file__).resolve().parent))

import lightmotif_amd as lm  # noqa: E402
from seqset_bench import load_motifs, make_records  # noqa: E402

CASES = ((2_000, 500, 1, True), (2_000, 500, 8, True), (2_000, 500, 64, False), (100_000, 200, 8, False))


def timed(call, runs, warmup):
    for _ in range(warmup):
        call()
    out = []
    for _ in range(runs):
        t0 = time.perf_counter()
        call()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "all": [round(x, 3) for x in v]}


def host_road(pli, everything, seqset, pssms, gains, k=5):
    """Leg A: per motif the (M, k) float64 table from the list of every window."""
    hits = pli.scan_threshold_set(everything, None, seqset)
    out = []
    for mi, ((rec, _, val), (win, valid)) in enumerate(zip(hits, seqset.windows(hits, pssms))):
        z = np.minimum(np.exp2(val.astype(np.float64)) * gains[mi][rec], 1.0)
        table = np.zeros((len(pssms[mi]), k), dtype=np.float64)
        for j in range(len(pssms[mi])):
            np.add.at(table[j], win[:, j], z)
        out.append(table)
    return out


def measure(pli, n_records, length, n_motifs, with_host, runs, warmup):
    pssms, _ = load_motifs(n_motifs)
    lengths = [len(p) for p in pssms]
    _, joined = make_records(n_records, length)
    offsets = np.arange(n_records + 1, dtype=np.uint64) * np.uint64(length)
    seqset = pli.stripe_ascii_set(joined, lossy=True, offsets=offsets)
    seqset.configure_wrap(max(lengths))
    batch = pli.prepare_batch(pssms)
    flat = [lm.ScoringMatrix(np.zeros_like(p.data)) for p in pssms]
    flat_batch = pli.prepare_batch(flat)
    sums = pli.scan_sum_set(batch, seqset)
    gains = lm.posterior_gains(sums)
    flat_gains = lm.posterior_gains(pli.scan_sum_set(flat_batch, seqset))
    windows = int(sums.windows.sum())

    loaded = pli.expected_counts_set(batch, seqset, gains)
    first = pli.expected_counts_set(flat_batch, seqset, flat_gains)
    live = {"flat": windows, "loaded": None}
    ways = {"B_flat": lambda: pli.expected_counts_set(flat_batch, seqset, flat_gains),
            "B_loaded": lambda: pli.expected_counts_set(batch, seqset, gains),
            "C": lambda: pli.scan_sum_set(batch, seqset)}
    times = {k: [] for k in ways}
    for it in range(warmup + runs):                                # the legs alternate
        for k in sorted(ways):
            t = timed(ways[k], 1, 0)
            if it >= warmup:
                times[k] += t
    out = {"records": n_records, "record_length": length, "motifs": len(pssms), "motif_lengths": lengths, "runs": runs, "warmup": warmup,
           "windows": windows, "frac_bits": loaded.frac_bits, "kernel": loaded.kernel, "ms": {k: summary(v) for k, v in times.items()},
           "repeat_bit_identical": all(a.tobytes() == b.tobytes() for a, b in zip(pli.expected_counts_set(batch, seqset, gains).counts, loaded.counts)),
           "flat_row_total": float(first.counts[0].sum(axis=1)[0]), "loaded_row_total": float(loaded.counts[0].sum(axis=1)[0])}
    if with_host:
        everything = pli.prepare_batch(pssms, [-np.inf] * len(pssms))
        a = host_road(pli, everything, seqset, pssms, gains)
        unit = 2.0 ** -loaded.frac_bits
        worst = max(float(np.max(np.abs(x - y) / (2.0 ** -21 * x + (windows / len(pssms) + 1) * unit))) for x, y in zip(a, loaded.counts))
        out["ms"]["A"] = summary(timed(lambda: host_road(pli, everything, seqset, pssms, gains), max(3, runs // 5), 1))
        out["A_worst_error_over_bound"] = worst
        out["A_over_B_loaded"] = out["ms"]["A"]["median"] / out["ms"]["B_loaded"]["median"]
    for k in ("B_flat", "B_loaded"):
        out[k + "_over_C"] = out["ms"][k]["median"] / out["ms"]["C"]["median"]
        out[k + "_ns_per_window"] = out["ms"][k]["median"] * 1e6 / windows
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "em_bench.json"))
    a = ap.parse_args()
    pli = lm.Pipeline.hip(0)
    cases = []
    for n_records, length, n_motifs, with_host in CASES:
        res = measure(pli, n_records, length, n_motifs, with_host, a.runs, a.warmup)
        cases.append(res)
        print(json.dumps({"records": n_records, "length": length, "motifs": n_motifs,
                          **{k + "_ms": round(v["median"], 3) for k, v in res["ms"].items()},
                          "B_flat_over_C": round(res["B_flat_over_C"], 2), "B_loaded_over_C": round(res["B_loaded_over_C"], 2)}), flush=True)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps({"tool": "tools/em_bench.py", "device": "MI355X (gfx950)", "cases": cases}, indent=1) + "\n")
    print(json.dumps({"wrote": a.out}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
