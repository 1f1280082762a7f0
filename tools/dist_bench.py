#!/usr/bin/env python3
"""Score distributions: the host code of lightmotif_amd/dist.py against the device (csrc/dist.hip), on the 2 346
matrices of tests/golden/JASPAR2024.pwm.gz, timed on one MI355X in ONE process after a warm-up.

  A    ``dist.ScoreDistribution(pssm)`` + ``.score(1e-5)`` for every motif: what ``scan_cli -P`` paid before its first launch
  B    ``Pipeline.score_distributions`` (``lm_hip_dists_create``) + ``.thresholds(1e-5)`` (``lm_hip_dists_scores``): the
       first call of the process (code object load and allocations included) and the later ones
  A'   the Python loop ``dist.pvalue(score)`` over about one million scores, the distributions already built
  B'   ``ScoreDistributions.pvalues`` (``lm_hip_dists_pvalues``) of the same scores: upload, kernel and read-back

A' / B' run on two inputs: random scores, the same number for every motif, and the hits of a real scan (``--scan-mbp``
of random DNA at p = 1e-5, whatever number of hits that gives).  Every time is a host clock around calls that end in a
stream synchronisation; median and spread (min, max) over ``--runs`` are reported, the ratios from the medians.  The
device's thresholds and p-values are compared with the host's, bit for bit, in the same run.

    python tools/dist_bench.py [--runs 5] [--host-runs 3] [--scan-mbp 40] [--out profiles/dist_bench.json]
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
from lightmotif_amd.dist import ScoreDistribution  # noqa: E402


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "runs": len(ms)}


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def host_build(pssms, pvalue):
    dists = [ScoreDistribution(p) for p in pssms]
    return dists, np.array([d.score(pvalue) for d in dists], dtype=np.float32)


def host_pvalues(dists, counts, scores):
    out, at = np.empty(len(scores)), 0
    for d, c in zip(dists, counts.tolist()):
        for s in scores[at:at + c].tolist():
            out[at] = d.pvalue(s)
            at += 1
    return out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--host-runs", type=int, default=3)
    ap.add_argument("--scores", type=int, default=1_000_000, help="random scores of A' / B'")
    ap.add_argument("--scan-mbp", type=float, default=40.0, help="random DNA scanned for the real hits of A' / B'")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "dist_bench.json"))
    args = ap.parse_args(argv)

    pli = lm.Pipeline.hip(0)
    pssms = [r.matrix.normalize(0.1).log_odds() for r in lmio.read(ROOT / "tests" / "golden" / "JASPAR2024.pwm.gz")]
    n = len(pssms)
    result = {"motifs": n, "rows": int(sum(len(p) for p in pssms)), "pvalue": 1e-5,
              "table_bytes": 8 * (1000 * int(sum(len(p) for p in pssms)) + n)}

    # B first: the first call of the process is the cold one
    def device_build():
        d = pli.score_distributions(pssms)
        return d, d.thresholds(1e-5)
    for p in pssms:                                 # (the matrices' device tables are not part of either side)
        p._device(pli)
    pli.sync()
    cold_ms, (dists, t_dev) = timed(device_build)
    warm = []
    for _ in range(args.runs):
        del dists
        ms, (dists, t_again) = timed(device_build)
        warm.append(ms)
        assert t_again.tobytes() == t_dev.tobytes()
    create_only, scores_only = [], []
    for _ in range(args.runs):
        del dists
        ms, dists = timed(lambda: pli.score_distributions(pssms))
        create_only.append(ms)
        scores_only.append(timed(lambda: dists.thresholds(1e-5))[0])
    result["B_device_cold"] = {"ms": cold_ms}
    result["B_device"] = summary(warm)
    result["B_create_alone"] = summary(create_only)
    result["B_scores_alone"] = summary(scores_only)

    host = []
    for _ in range(args.host_runs):
        ms, (hdists, t_host) = timed(lambda: host_build(pssms, 1e-5))
        host.append(ms)
    assert np.array_equal(t_host, t_dev), "thresholds differ between host and device"
    result["A_host"] = summary(host)
    result["A_over_B"] = result["A_host"]["median_ms"] / result["B_device"]["median_ms"]
    result["A_over_B_cold"] = result["A_host"]["median_ms"] / cold_ms

    rng = np.random.default_rng(1)
    inputs = {}
    per = max(args.scores // n, 1)
    inputs["random"] = (np.full(n, per, dtype=np.uintp), rng.uniform(-25.0, 20.0, per * n).astype(np.float32))
    text = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, int(args.scan_mbp * 1e6))]
    seqset = pli.stripe_ascii_set(text, lossy=True, offsets=np.array([0, text.size], dtype=np.uint64))
    seqset.configure_wrap(max(len(p) for p in pssms))
    hits = pli.scan_threshold_set(pli.prepare_batch(pssms, t_dev), None, seqset)
    inputs["scan"] = (hits.counts, np.ascontiguousarray(hits.hits["score"]))
    result["scan_bases"], result["scan_hits"] = int(text.size), int(hits.total)
    del seqset
    for name, (counts, scores) in inputs.items():
        dev = []
        for _ in range(args.runs + 1):
            ms, p_dev = timed(lambda: dists.pvalues(counts, scores))
            dev.append(ms)
        host = []
        for _ in range(args.host_runs):
            ms, p_host = timed(lambda: host_pvalues(hdists, counts, scores))
            host.append(ms)
        assert np.array_equal(p_dev, p_host), f"p-values differ between host and device ({name})"
        result[f"pvalues_{name}"] = {"scores": int(scores.size), "A_host": summary(host), "B_device_first": {"ms": dev[0]},
                                     "B_device": summary(dev[1:]),
                                     "A_over_B": statistics.median(host) / statistics.median(dev[1:])}
    # the strided read of the hit list itself, as a caller holding lm_hip_set_hit records makes it
    result["pvalues_scan"]["B_device_strided"] = summary([timed(lambda: dists.pvalues(hits))[0] for _ in range(args.runs)])

    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
