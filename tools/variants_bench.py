#!/usr/bin/env python3
"""Single-symbol variants of a resident set against all motifs (csrc/variants.hip) against the cheapest route before it,
timed on one MI355X in ONE process, every leg warmed up first.

Set: 2 000 records x 500 bp, resident.  100 000 variants, uniform over records, positions and the four bases.

  A    ``Pipeline.scan_variants_set``: the dense call, the first 64 JASPAR motifs x all variants
  A'   ``Pipeline.scan_variant_hits_set`` at the p = 1e-4 thresholds: all 2 346 JASPAR matrices x both strands x all variants
  B    the route before: ``StripedSequenceSet.windows`` reads the neighbourhoods [p - W + 1, p + W - 1] back and numpy scores
       every covering window of every motif for both alleles (vectorised over the variants, M sequential f32 adds per window,
       strict ``>`` over ascending starts).  ``windows`` refuses a window that leaves its record, so B only takes the variants
       at least W - 1 symbols from both record ends (W = the longest of the 64 motifs); ``A_on_B_variants`` is the dense call
       on exactly those, and B's result is compared with it bit for bit in the warm-up run.

Medians of ``--runs`` runs that take the legs in turn, after ``--warmup`` runs of each, with min and max as the spread; every
time is a host clock around calls that end in a stream synchronisation.

``--only dense|hits`` runs that leg alone (for a profiler).  ``--merge-kernel-stats DIR`` / ``--merge-pmc DIR`` add the kernels'
times (``rocprofv3 --kernel-trace --stats``) and their LDS bank-conflict cycles (a counters-only ``rocprofv3 --pmc`` run of its
own) from the CSV files under DIR to the JSON: tools/prof_variants.sh makes all three runs.

    python tools/variants_bench.py [--runs 7] [--out profiles/variants_bench.json]
"""
from __future__ import annotations

import argparse
import csv
import glob
import json
import platform
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

JASPAR = ROOT / "tests" / "golden" / "JASPAR2024.pwm.gz"
NONE = 0xFFFFFFFF


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "runs": len(ms)}


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def cpu_name():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return platform.processor()


def host_route(seqset, pssms, rec, pos, alt):
    """B: (ref_score, alt_score, ref_back, alt_back), each (motifs, variants), for variants whose neighbourhood of the
    longest motif lies inside the record."""
    w = max(len(p) for p in pssms)
    (nb, valid), = seqset.windows([(rec, pos)], [2 * w - 1], [-(w - 1)])
    assert valid.all(), "B only takes variants at least W - 1 symbols from both record ends"
    nb = nb.astype(np.int64)
    n, v = len(pssms), len(rec)
    out = [np.full((n, v), np.nan, np.float32), np.full((n, v), np.nan, np.float32), np.full((n, v), NONE, np.uint32),
           np.full((n, v), NONE, np.uint32)]
    alt = alt.astype(np.int64)
    with np.errstate(invalid="ignore"):
        for i, p in enumerate(pssms):
            weights, m = p.data, len(p)
            for back in range(m - 1, -1, -1):                   # ascending start
                win = nb[:, w - 1 - back:w - 1 - back + m]
                r, a = np.zeros(v, np.float32), np.zeros(v, np.float32)
                for j in range(m):
                    x = weights[j, win[:, j]]
                    r = r + x
                    a = a + (weights[j, alt] if j == back else x)
                for score, best, where in ((r, out[0][i], out[2][i]), (a, out[1][i], out[3][i])):
                    take = ~np.isnan(score) & ~(score <= best)  # strictly greater, or the first
                    best[take], where[take] = score[take], back
    return out


def merge_kernel_stats(result, directory):
    rows = {}
    for path in glob.glob(str(Path(directory) / "**" / "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            if "lm::variants::" in row["Name"]:
                name = row["Name"][row["Name"].index("lm::variants::") + len("lm::variants::"):].split("(")[0]
                rows[name] = {"calls": int(row["Calls"]), "average_us": float(row["AverageNs"]) / 1e3, "min_us": float(row["MinNs"]) / 1e3,
                              "max_us": float(row["MaxNs"]) / 1e3}
    leg = Path(directory).name
    result.setdefault("kernels", {"source": "rocprofv3 --kernel-trace --stats around `--only dense` and `--only hits`, a run of its own each"})
    result["kernels"][leg] = rows


def merge_pmc(result, directory):
    acc = {}
    for path in glob.glob(str(Path(directory) / "**" / "*counter_collection.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            if "lm::variants::" in row["Kernel_Name"]:
                name = row["Kernel_Name"][row["Kernel_Name"].index("lm::variants::") + len("lm::variants::"):].split("(")[0]
                acc.setdefault(name, {}).setdefault(row["Counter_Name"], []).append(float(row["Counter_Value"]))
    table = {}
    for name, counters in acc.items():
        table[name] = {c: sum(v) / len(v) for c, v in counters.items()}
        table[name]["launches"] = max(len(v) for v in counters.values())
        if table[name].get("SQ_LDS_IDX_ACTIVE"):
            table[name]["bank_conflict_share_of_lds_active"] = table[name].get("SQ_LDS_BANK_CONFLICT", 0.0) / table[name]["SQ_LDS_IDX_ACTIVE"]
    result["lds_counters"] = {"source": "rocprofv3 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE around `--only dense`, counters only; mean per launch",
                              **table}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--b-runs", type=int, default=3, help="B takes seconds per run: it joins the first of the runs only")
    ap.add_argument("--records", type=int, default=2_000)
    ap.add_argument("--length", type=int, default=500)
    ap.add_argument("--variants", type=int, default=100_000)
    ap.add_argument("--motifs", type=int, default=64)
    ap.add_argument("--pvalue", type=float, default=1e-4)
    ap.add_argument("--only", choices=("dense", "hits"))
    ap.add_argument("--merge-kernel-stats", metavar="DIR", action="append", default=[])
    ap.add_argument("--merge-pmc", metavar="DIR")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "variants_bench.json"))
    args = ap.parse_args(argv)

    if args.merge_kernel_stats or args.merge_pmc:
        result = json.loads(Path(args.out).read_text())
        for directory in args.merge_kernel_stats:
            merge_kernel_stats(result, directory)
        if args.merge_pmc:
            merge_pmc(result, args.merge_pmc)
        Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
        print(json.dumps({k: result.get(k) for k in ("kernels", "lds_counters")}))
        return 0

    import torch
    pli = lm.Pipeline.hip(0)
    rng = np.random.default_rng(1)
    motifs = list(lmio.read(str(JASPAR)))
    direct = [r.matrix.normalize(0.1).log_odds() for r in motifs]
    few = direct[:args.motifs]
    letters = np.frombuffer(b"ACTG", dtype=np.uint8)
    seqset = pli.stripe_ascii_set([letters[rng.integers(0, 4, args.length, dtype=np.uint8)] for _ in range(args.records)], lossy=True)
    rec = rng.integers(0, args.records, args.variants).astype(np.int64)
    pos = rng.integers(0, args.length, args.variants).astype(np.int64)
    alt = rng.integers(0, 4, args.variants).astype(np.uint8)
    w = max(len(p) for p in few)
    inner = np.flatnonzero((pos >= w - 1) & (pos <= args.length - w))
    both = direct + [p.reverse_complement() for p in direct]
    thresholds = pli.score_distributions(direct).thresholds(args.pvalue).tolist()
    batch = pli.prepare_batch(both, thresholds + thresholds)
    few_batch = pli.prepare_batch(few)

    def dense(index=slice(None)):
        return pli.scan_variants_set(few_batch, seqset, rec[index], pos[index], alt[index])

    def hits():
        return pli.scan_variant_hits_set(batch, None, seqset, rec, pos, alt)

    if args.only:
        leg = dense if args.only == "dense" else hits
        for _ in range(args.warmup + args.runs):
            leg()
        print(json.dumps({"only": args.only, "calls": args.warmup + args.runs, "last_kernel": pli.last_kernel}))
        return 0

    result = {"machine": {"gpu": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName,
                          "compute_units": torch.cuda.get_device_properties(0).multi_processor_count, "hip": torch.version.hip,
                          "cpu": cpu_name(), "torch": torch.__version__},
              "runs": args.runs, "warmup": args.warmup,
              "set": {"records": len(seqset), "bases": seqset.total_length},
              "variants": args.variants,
              "B_restriction": f"`windows` cannot clip a neighbourhood at a record's end, so B (and A_on_B_variants) take only the "
                               f"{len(inner)} of {args.variants} variants at least W - 1 = {w - 1} symbols from both record ends"}
    legs = {key: [] for key in ("A_dense", "A_on_B_variants", "A_prime_hits", "B_windows_numpy")}
    kept = 0
    for run in range(-args.warmup, args.runs):
        t_a, _ = timed(dense)
        t_ab, got = timed(lambda: dense(inner))
        t_hits, sparse = timed(hits)
        t_b, want = timed(lambda: host_route(seqset, few, rec[inner], pos[inner], alt[inner])) if run < args.b_runs else (None, None)
        if run < 0:
            for name, x in zip(("ref_score", "alt_score", "ref_back", "alt_back"), want):
                assert got.raw[name].tobytes() == x.tobytes(), f"B's {name} differs from A's"
            continue
        kept = sparse.total
        for key, ms in zip(legs, (t_a, t_ab, t_hits, t_b)):
            if ms is not None:
                legs[key].append(ms)
    result.update({key: summary(ms) for key, ms in legs.items()})
    med = {key: result[key]["median_ms"] for key in legs}
    result["A"] = {"motifs": len(few), "longest_motif": w, "pairs": len(few) * args.variants,
                   "pairs_per_s": len(few) * args.variants / med["A_dense"] * 1e3}
    result["A_prime"] = {"motifs": len(both), "pvalue": args.pvalue, "pairs": len(both) * args.variants, "kept": kept,
                         "pairs_per_s": len(both) * args.variants / med["A_prime_hits"] * 1e3}
    result["B_over_A_on_B_variants"] = med["B_windows_numpy"] / med["A_on_B_variants"]
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
