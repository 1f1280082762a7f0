#!/usr/bin/env python3
"""From a resident set to its control, a null set of the same record lengths and composition: three legs over the same set.

  A  the only road before ``lm_hip_seqset_sample``: per record ``numpy.random.Generator.choice`` with the record's own
     composition on the host, then ``Pipeline.stripe_set`` (a host generator plus the whole result as an upload)
  B  ``StripedSequenceSet.null(order)``: counted, fitted and drawn on the device (csrc/sample.hip, csrc/pairs.hip)
  C  a device-to-device copy of as many bytes as the result holds (``torch.Tensor.copy_``), the floor

Three models -- order 0 with one model for all records (``Pipeline.sample_set`` on the set's background; A draws with that
one background), order 0 with per-record models (``null(0)``), order 1 (``null(1)``; A has no first-order generator and
draws i.i.d., so A is a LOWER bound of the host road there) -- on two shapes.  A/B and B/C alternate; medians and [min, max]
are reported, and with the option ``time_scan`` the draw kernels' own time between two events on the stream.
``python tools/null_bench.py`` writes profiles/null_bench.json.
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

MODELS = ("order0_shared", "order0_per_record", "order1")


def make_source(pli, records, length, seed=7):
    rng = np.random.default_rng(seed)
    gc = rng.uniform(0.35, 0.65, records)                          # every record its own composition
    out = []
    for r in range(records):
        p = np.array([(1 - gc[r]) / 2, gc[r] / 2, (1 - gc[r]) / 2, gc[r] / 2, 0.0]) * 0.99
        p[4] = 0.01
        out.append(lm.EncodedSequence(rng.choice(5, length, p=p).astype(np.uint8)))
    return pli.stripe_set(out)


def by_host(pli, lengths, models, seed):
    """Leg A: numpy draws every record, stripe_set uploads them."""
    rng = np.random.default_rng(seed)
    shared = models.ndim == 1
    return pli.stripe_set([lm.EncodedSequence(rng.choice(5, int(n), p=models if shared else models[r]).astype(np.uint8))
                           for r, n in enumerate(lengths)])


def measure(pli, records, length, model="order0_per_record", runs=5, warmup=1):
    source = make_source(pli, records, length)
    lengths = source.lengths
    counts = source.count_symbols().astype(np.float64)
    per_record = counts / counts.sum(axis=1, keepdims=True)
    shared = counts.sum(axis=0) / counts.sum()
    nbytes = int(lengths.sum())
    src = torch.empty(max(nbytes, 1), dtype=torch.uint8, device="cuda:0")
    dst = torch.empty_like(src)
    background = source.background(unknown=True)
    step = [0]

    def way_a():
        step[0] += 1
        return by_host(pli, lengths, shared if model == "order0_shared" else per_record, step[0])

    def way_b():
        step[0] += 1
        if model == "order0_shared":
            return pli.sample_set(lengths, background, seed=step[0])
        return source.null(1 if model == "order1" else 0, seed=step[0])

    def way_c():
        dst.copy_(src)
        torch.cuda.synchronize()

    # what both roads make is a set of the same geometry and, within sampling error, the same composition
    set_a, set_b = way_a(), way_b()
    ca, cb = set_a.count_symbols().sum(axis=0).astype(np.float64), set_b.count_symbols().sum(axis=0).astype(np.float64)
    if model == "order1":                              # a chain fitted without the default symbol draws none: compare the rest
        ca[-1] = cb[-1] = 0
    ca, cb = ca / ca.sum(), cb / cb.sum()
    alike = bool(len(set_a) == len(set_b) == records and set_a.rows == set_b.rows and np.array_equal(set_a.lengths, set_b.lengths) and
                 np.abs(ca - cb).max() < 0.01)
    kernel = pli.last_kernel
    del set_a, set_b
    ways = {"A": way_a, "B": way_b, "C": way_c}
    times = {k: [] for k in ways}
    for it in range(warmup + runs):
        for k in ("A", "B", "B", "C"):                 # alternating: A/B, then B/C
            t0 = time.perf_counter()
            ways[k]()
            if it >= warmup:
                times[k].append((time.perf_counter() - t0) * 1e3)
    # the draw kernels alone, between two events on the library's stream
    pli.set_option("time_scan", 1)
    draw = []
    for _ in range(warmup + runs):
        way_b()
        draw.append(pli.last_scan_kernel_ms)
    pli.set_option("time_scan", 0)
    draw = [x for x in draw[warmup:] if x is not None]
    out = {"model": model, "records": records, "record_length": length, "result_bytes": nbytes, "runs": runs, "warmup": warmup,
           "sets_alike": alike, "draw_kernel": kernel,
           "ms": {k: {"median": statistics.median(v), "min": min(v), "max": max(v), "all": [round(x, 3) for x in v]}
                  for k, v in times.items()}}
    if draw:
        out["draw_kernels_ms"] = {"median": statistics.median(draw), "min": min(draw), "max": max(draw), "all": [round(x, 4) for x in draw]}
        out["draw_ns_per_symbol"] = statistics.median(draw) * 1e6 / max(nbytes, 1)
    out["A_over_B"] = out["ms"]["A"]["median"] / out["ms"]["B"]["median"]
    out["B_over_C"] = out["ms"]["B"]["median"] / out["ms"]["C"]["median"]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "null_bench.json"))
    a = ap.parse_args()
    pli = lm.Pipeline.hip(0)
    cases = [measure(pli, records, length, model, a.runs, a.warmup)
             for records, length in ((2_000, 5_000), (100_000, 500)) for model in MODELS]
    result = {"tool": "tools/null_bench.py", "device": "MI355X (gfx950)", "cases": cases}
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps({"cases": [{k: c.get(k) for k in ("model", "records", "record_length", "A_over_B", "B_over_C", "draw_ns_per_symbol",
                                                        "sets_alike")} for c in cases], "wrote": a.out}))
    return 0 if all(c["sets_alike"] for c in cases) else 1


if __name__ == "__main__":
    sys.exit(main())
