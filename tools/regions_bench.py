#!/usr/bin/env python3
"""From a resident set of contigs and a table of regions to a resident set of the regions: three legs over the same source.

  A  the only road before ``lm_hip_seqset_from_regions``: ``StripedSequenceSet.windows`` reads the regions back to the
     host (one "motif" per distinct width), minus-strand regions are reverse-complemented there, and
     ``Pipeline.stripe_set`` uploads them again
  B  ``StripedSequenceSet.regions``: the gather on the device (csrc/regions.hip)
  C  a device-to-device copy of as many bytes as the result holds (``torch.Tensor.copy_``), the floor

The sets of A and B are compared first (record lengths and every record's symbols); then A/B and B/C alternate and the
medians and [min, max] are reported.  Two workloads: regions scattered over a genome-like source (a few percent of it),
and a tiling of the whole source, where every source byte is gathered once and the column walk of the striped matrix
re-reads each 32-byte sector about 32 times.  ``python tools/regions_bench.py`` writes profiles/regions_bench.json.
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch                                                       # (before the library: leg C copies with it)

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import lightmotif_amd as lm                                        # noqa: E402

COMPLEMENT = np.arange(256, dtype=np.uint8)
COMPLEMENT[[0, 1, 2, 3]] = [2, 3, 0, 1]                            # abc.rs:174-185 on symbol bytes


def make_source(pli, n_contigs, contig_len, seed=7):
    rng = np.random.default_rng(seed)
    text = rng.choice(5, n_contigs * contig_len, p=[0.245, 0.245, 0.245, 0.245, 0.02]).astype(np.uint8)
    return pli.stripe_set([lm.EncodedSequence(text[r * contig_len:(r + 1) * contig_len]) for r in range(n_contigs)])


def scattered(n_contigs, contig_len, n_regions, region_len, seed=8):
    """``n_regions`` regions of ``region_len`` symbols inside random contigs, every second one on the minus strand."""
    rng = np.random.default_rng(seed)
    rec = rng.integers(0, n_contigs, n_regions)
    starts = rng.integers(0, contig_len - region_len + 1, n_regions)
    return rec, starts, starts + region_len, (np.arange(n_regions) % 2).astype(np.uint8)


def tiling(n_contigs, contig_len, region_len):
    """Every contig cut into consecutive regions of ``region_len`` symbols (the last one shorter), plus strand."""
    starts = np.arange(0, contig_len, region_len)
    rec = np.repeat(np.arange(n_contigs), len(starts))
    starts = np.tile(starts, n_contigs)
    return rec, starts, np.minimum(starts + region_len, contig_len), np.zeros(len(rec), dtype=np.uint8)


def by_read_back(pli, source, rec, starts, ends, strands):
    """Leg A: windows -> host reverse complement -> stripe_set."""
    widths = ends - starts
    kinds = np.unique(widths)
    sites = [(rec[widths == w], starts[widths == w]) for w in kinds]
    pieces = [None] * len(rec)
    for w, (win, valid) in zip(kinds.tolist(), source.windows(sites, kinds.tolist())):
        assert valid.all()
        idx = np.flatnonzero(widths == w)
        minus = strands[idx] == 1
        win[minus] = COMPLEMENT[win[minus][:, ::-1]]
        for i, row in zip(idx.tolist(), win):
            pieces[i] = lm.EncodedSequence(row)
    return pli.stripe_set(pieces)


def measure(pli, n_contigs, contig_len, n_regions, region_len, runs=5, warmup=1, tile=False):
    source = make_source(pli, n_contigs, contig_len)
    rec, starts, ends, strands = tiling(n_contigs, contig_len, region_len) if tile else scattered(n_contigs, contig_len, n_regions, region_len)
    nbytes = int((ends - starts).sum())
    src = torch.empty(max(nbytes, 1), dtype=torch.uint8, device="cuda:0")
    dst = torch.empty_like(src)

    def way_a():
        return by_read_back(pli, source, rec, starts, ends, strands)

    def way_b():
        return source.regions(rec, starts, ends, strands)[0]

    def way_c():
        dst.copy_(src)
        torch.cuda.synchronize()

    set_a, set_b = way_a(), way_b()
    same = bool(len(set_a) == len(set_b) == len(rec) and set_a.total_length == set_b.total_length == nbytes and
                set_a.rows == set_b.rows and np.array_equal(set_a.lengths, set_b.lengths) and
                all(np.array_equal(x.data, y.data) for x, y in zip(set_a.records(), set_b.records())))
    del set_a, set_b
    ways = {"A": way_a, "B": way_b, "C": way_c}
    times = {k: [] for k in ways}
    for it in range(warmup + runs):
        for k in ("A", "B", "B", "C"):                 # alternating: A/B, then B/C
            t0 = time.perf_counter()
            ways[k]()
            if it >= warmup:
                times[k].append((time.perf_counter() - t0) * 1e3)
    out = {"workload": "tiling" if tile else "scattered", "contigs": n_contigs, "contig_length": contig_len, "regions": int(len(rec)),
           "region_length": region_len, "minus_strand": int(strands.sum()), "source_bytes": n_contigs * contig_len, "result_bytes": nbytes,
           "runs": runs, "warmup": warmup, "sets_equal": same, "last_kernel": pli.last_kernel,
           "ms": {k: {"median": statistics.median(v), "min": min(v), "max": max(v), "all": [round(x, 3) for x in v]}
                  for k, v in times.items()}}
    out["A_over_B"] = out["ms"]["A"]["median"] / out["ms"]["B"]["median"]
    out["B_over_C"] = out["ms"]["B"]["median"] / out["ms"]["C"]["median"]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--contigs", type=int, default=20)
    ap.add_argument("--contig-length", type=int, default=5_000_000)
    ap.add_argument("--regions", type=int, default=100_000)
    ap.add_argument("--region-length", type=int, default=500)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "regions_bench.json"))
    a = ap.parse_args()
    pli = lm.Pipeline.hip(0)
    cases = [measure(pli, a.contigs, a.contig_length, a.regions, a.region_length, a.runs, a.warmup),
             measure(pli, a.contigs, a.contig_length, 0, a.region_length, a.runs, a.warmup, tile=True)]
    result = {"tool": "tools/regions_bench.py", "device": "MI355X (gfx950)", "cases": cases}
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps({"cases": [{k: c[k] for k in ("workload", "result_bytes", "A_over_B", "B_over_C", "sets_equal")} for c in cases],
                      "wrote": a.out}))
    return 0 if all(c["sets_equal"] for c in cases) else 1


if __name__ == "__main__":
    sys.exit(main())
