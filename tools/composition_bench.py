#!/usr/bin/env python3
"""Symbol counts of resident sequences: the host route a user had before against the device (csrc/composition.hip), timed
on one MI355X in ONE process, every shape warmed up first.

  A    what a user did before: ``np.asarray(seq)`` of the resident matrix (the copy over the link) and one ``np.bincount``
       per record
  B    the new call: ``StripedSequence.count_symbols`` / ``StripedSequenceSet.count_symbols``
  C    ``StripedSequence.copy()`` of a sequence of the same length.  It is the library's own copy of a resident matrix --
       which goes through the host (download, upload, symbol check), not a pass on the device
  C'   a device-to-device copy of as many bytes as the matrix holds (``torch.Tensor.clone``): the bare pass over the same
       bytes at 2 B of traffic per position that B, which reads 1 B per position, is held against

Shapes: one sequence of 1 Gbp; one record of 100 Mbp; 2 000 x 50 000 bp; 2 000 x 500 bp; 50 000 x 200 bp;
1 000 000 x 40 bp (``--scale`` shrinks them all for a rehearsal).  Every time is a host clock around calls that end in a
stream synchronisation; median and spread (min, max) over the runs, the ratios from the medians.  With ``--phases`` B is
also run with the context option ``time_scan``, which puts events between its passes
(``lm_hip_ctx_last_phases_ms``): block pass, scan, prefix pass + differences.  B's table is compared with A's in the run.

    python tools/composition_bench.py [--runs 10] [--host-runs 2] [--out profiles/composition_bench.json]
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

SHAPES = [("seq_1gbp", None, 1_000_000_000), ("set_1x100mbp", 1, 100_000_000), ("set_2000x50000", 2_000, 50_000),
          ("set_2000x500", 2_000, 500), ("set_50000x200", 50_000, 200), ("set_1000000x40", 1_000_000, 40)]


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "runs": len(ms)}


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def random_text(rng, n):
    """ASCII of skewed DNA with 1 % N, made in pieces (a 1 Gbp draw in one go needs 8 GB for the indices)."""
    out = np.empty(n, dtype=np.uint8)
    letters = np.frombuffer(b"AAACCTTTGGN", dtype=np.uint8)
    for a in range(0, n, 1 << 26):
        b = min(n, a + (1 << 26))
        out[a:b] = letters[rng.integers(0, len(letters), b - a, dtype=np.uint8)]
    return out


def host_counts(striped, offsets, k):
    """A: the matrix over the link, then numpy -- positions in order are the rows of the (columns, rows) view.  (bincount
    widens its input to 8 bytes per symbol: records beyond 64 Mbp are counted in pieces.)"""
    flat = np.asarray(striped).reshape(-1)[:int(offsets[-1])]
    out = np.zeros((len(offsets) - 1, k), dtype=np.int64)
    for r in range(len(offsets) - 1):
        for a in range(int(offsets[r]), int(offsets[r + 1]), 1 << 26):
            out[r] += np.bincount(flat[a:min(a + (1 << 26), int(offsets[r + 1]))], minlength=k)
    return out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-runs", type=int, default=2)
    ap.add_argument("--scale", type=float, default=1.0, help="multiplies every shape's total (a rehearsal at 0.001)")
    ap.add_argument("--phases", action="store_true", help="also time B's passes with events (option time_scan)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "composition_bench.json"))
    args = ap.parse_args(argv)

    import torch
    pli = lm.Pipeline.hip(0)
    rng = np.random.default_rng(1)
    result = {"runs": args.runs, "warmup": args.warmup, "scale": args.scale, "shapes": {}}
    copies = {}    # total -> C, C'
    for name, records, size in SHAPES:
        if records is None:
            total = max(int(size * args.scale), 1)
            offsets = np.array([0, total], dtype=np.uint64)
        else:
            n = max(int(records * (args.scale if records > 1 else 1)), 1)
            per = max(int(size * args.scale), 1) if records == 1 else size
            total, offsets = n * per, np.arange(n + 1, dtype=np.uint64) * np.uint64(per)
        text = random_text(rng, total)
        # the same bytes as a single sequence: A's download, C, and (for the first shape) B itself
        single = pli.stripe_ascii(text, lossy=True)
        target = single if records is None else pli.stripe_ascii_set(text, lossy=True, offsets=offsets)
        del text
        entry = {"records": len(offsets) - 1, "bases": total}

        for _ in range(args.warmup):
            got = target.count_symbols()
        entry["B_device"] = summary([timed(target.count_symbols)[0] for _ in range(args.runs)])
        if args.phases:
            pli.set_option("time_scan", 1)
            phases = []
            for _ in range(args.runs):
                target.count_symbols()
                phases.append(pli.last_phases_ms)
            pli.set_option("time_scan", 0)
            entry["B_phases_ms"] = {key: statistics.median(p[i] for p in phases)
                                    for i, key in enumerate(("count_blocks", "scan", "count_prefix_and_diff"))}

        host = []
        for _ in range(args.host_runs):
            ms, want = timed(lambda: host_counts(single, offsets, 5))
            host.append(ms)
        assert np.array_equal(np.atleast_2d(got), want), f"{name}: the device's table differs from numpy's"
        entry["A_host"] = summary(host)

        if total not in copies:
            for _ in range(min(args.warmup, 1)):
                single.copy()
            c = summary([timed(single.copy)[0] for _ in range(max(args.host_runs, 3))])
            nbytes = single.rows * single.stride
            src = torch.empty(nbytes, dtype=torch.uint8, device="cuda:0")

            def clone():
                dst = src.clone()
                torch.cuda.synchronize()
                return dst
            for _ in range(args.warmup):
                clone()
            copies[total] = (c, summary([timed(clone)[0] for _ in range(args.runs)]))
            del src
        entry["C_copy"], entry["C_device_copy"] = copies[total]
        b = entry["B_device"]["median_ms"]
        entry["A_over_B"] = entry["A_host"]["median_ms"] / b
        entry["B_over_C"] = b / entry["C_copy"]["median_ms"]
        entry["B_over_C_device"] = b / entry["C_device_copy"]["median_ms"]
        entry["B_gbp_per_s"] = total / b / 1e6
        result["shapes"][name] = entry
        print(name, json.dumps(entry), flush=True)
        del single, target

    shapes = result["shapes"]
    result["B_one_record_over_B_2000_records_at_100mbp"] = (shapes["set_1x100mbp"]["B_device"]["median_ms"]
                                                            / shapes["set_2000x50000"]["B_device"]["median_ms"])
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
