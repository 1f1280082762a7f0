#!/usr/bin/env python3
"""Hit windows read back out of a resident set (csrc/sites.hip) against the host route, timed on one MI355X in ONE process,
every leg warmed up first.  The set is built from FASTA bytes on the device, as ``scan_cli`` builds it: the host holds no
record, so the host route starts with the parse.

Shape 1  2 000 records x 5 000 bp, the first 64 JASPAR motifs, the sites = the hits of ``scan_threshold_set`` at p = 1e-4:
         the text of every hit's window and the count matrix of every motif's hits.
Shape 2  every record of the same set read back (``StripedSequenceSet.records()``).

  A   the host: the FASTA text parsed (``scan_cli.read_fasta``) and encoded record by record, then per motif one numpy
      fancy-index gather of the windows and one ``np.add.at`` into the table.  Reported in parts; ``A`` is their sum, and
      ``A_without_parse`` leaves the parse out (a host that kept the encoded records)
  B   the device calls: ``windows`` + ``count_sites`` of the hit list as it came back (shape 1), ``records()`` (shape 2)
  C   a device-to-device copy of as many bytes as the windows hold (``torch.Tensor.clone``)

Medians of ``--runs`` (7) runs that take A, B and C in turn, after ``--warmup`` runs of each; every time is a host clock
around calls that end in a stream synchronisation.  B's windows and tables are compared with A's in the run.

    python tools/sites_bench.py [--runs 7] [--out profiles/sites_bench.json]
"""
from __future__ import annotations

import argparse
import io
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
from lightmotif_amd import scan_cli  # noqa: E402

JASPAR = ROOT / "tests" / "golden" / "JASPAR2024.pwm.gz"


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "runs": len(ms)}


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def make_fasta(rng, records, length):
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    parts = []
    for r in range(records):
        seq = letters[rng.integers(0, 4, length, dtype=np.uint8)].tobytes()
        parts.append(b">rec%d\n" % r + b"".join(seq[i:i + 70] + b"\n" for i in range(0, length, 70)))
    return b"".join(parts)


def host_parse(text):
    """The records as the host gets them: the line-by-line reader, then one lossy encode per record."""
    return [lm.EncodedSequence.encode_lossy(seq).data for _, seq in scan_cli.read_fasta(io.StringIO(text))]


def host_windows(symbols, hits, widths):
    cat = np.concatenate(symbols)
    offsets = np.concatenate(([0], np.cumsum([len(s) for s in symbols]))).astype(np.int64)
    return [cat[(offsets[rec] + pos)[:, None] + np.arange(w)] for (rec, pos, _), w in zip(hits, widths)]


def host_counts(windows, widths):
    out = []
    for win, w in zip(windows, widths):
        table = np.zeros((w, 5), dtype=np.int64)
        np.add.at(table, (np.tile(np.arange(w), len(win)), win.reshape(-1)), 1)
        out.append(table)
    return out


def cpu_name():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return platform.processor()


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--records", type=int, default=2_000)
    ap.add_argument("--length", type=int, default=5_000)
    ap.add_argument("--motifs", type=int, default=64)
    ap.add_argument("--pvalue", type=float, default=1e-4)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "sites_bench.json"))
    args = ap.parse_args(argv)

    import torch
    pli = lm.Pipeline.hip(0)
    rng = np.random.default_rng(1)
    motifs = list(lmio.read(str(JASPAR)))[:args.motifs]
    pssms = [r.matrix.normalize(0.1).log_odds() for r in motifs]
    widths = [len(p) for p in pssms]
    data = make_fasta(rng, args.records, args.length)
    text = data.decode("ascii")
    seqset = pli.stripe_fasta_set(data, lossy=True)
    seqset.configure_wrap(max(widths))
    thresholds = pli.score_distributions(pssms).thresholds(args.pvalue).tolist()
    hits = pli.scan_threshold_set(pli.prepare_batch(pssms, thresholds), None, seqset)
    per_motif = [hits[i] for i in range(len(hits))]
    window_bytes = int(sum(int(c) * w for c, w in zip(hits.counts, widths)))
    result = {"machine": {"gpu": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName,
                          "compute_units": torch.cuda.get_device_properties(0).multi_processor_count, "hip": torch.version.hip, "cpu": cpu_name(), "torch": torch.__version__},
              "runs": args.runs, "warmup": args.warmup,
              "set": {"records": len(seqset), "bases": seqset.total_length, "fasta_bytes": len(data)},
              "shapes": {}}

    def clone_of(nbytes):
        src = torch.empty(max(nbytes, 1), dtype=torch.uint8, device="cuda:0")

        def clone():
            dst = src.clone()
            torch.cuda.synchronize()
            return dst
        return clone

    # ---- shape 1: the hits' windows and the motifs' count matrices --------------------------------------------------
    legs = {key: [] for key in ("A_parse_encode", "A_gather", "A_add_at", "B_windows", "B_count_sites", "C_device_copy")}
    clone = clone_of(window_bytes)
    for run in range(-args.warmup, args.runs):
        t_parse, symbols = timed(lambda: host_parse(text))
        t_gather, want_windows = timed(lambda: host_windows(symbols, per_motif, widths))
        t_add, want_tables = timed(lambda: host_counts(want_windows, widths))
        t_windows, got_windows = timed(lambda: seqset.windows(hits, pssms))
        t_counts, (got_mats, used) = timed(lambda: seqset.count_sites(hits, pssms))
        t_copy, _ = timed(clone)
        if run < 0:
            assert all(v.all() and np.array_equal(g, w) for (g, v), w in zip(got_windows, want_windows)), "windows differ from the host's"
            assert all(np.array_equal(m.data, t) for m, t in zip(got_mats, want_tables)), "tables differ from the host's"
            assert np.array_equal(used, np.asarray(hits.counts, dtype=np.int64))
            continue
        for key, ms in zip(legs, (t_parse, t_gather, t_add, t_windows, t_counts, t_copy)):
            legs[key].append(ms)
    entry = {"motifs": len(pssms), "hits": hits.total, "window_bytes": window_bytes, "pvalue": args.pvalue}
    entry.update({key: summary(ms) for key, ms in legs.items()})
    med = {key: entry[key]["median_ms"] for key in legs}
    entry["A_ms"] = med["A_parse_encode"] + med["A_gather"] + med["A_add_at"]
    entry["A_without_parse_ms"] = med["A_gather"] + med["A_add_at"]
    entry["B_ms"] = med["B_windows"] + med["B_count_sites"]
    entry["A_over_B"] = entry["A_ms"] / entry["B_ms"]
    entry["A_without_parse_over_B"] = entry["A_without_parse_ms"] / entry["B_ms"]
    entry["B_windows_over_C"] = med["B_windows"] / med["C_device_copy"]
    result["shapes"]["hits_2000x5000x64"] = entry
    print("hits", json.dumps(entry), flush=True)

    # ---- shape 2: every record read back ------------------------------------------------------------------------------
    legs = {key: [] for key in ("A_parse_encode", "B_records", "C_device_copy")}
    clone = clone_of(seqset.total_length)
    for run in range(-args.warmup, args.runs):
        t_parse, symbols = timed(lambda: host_parse(text))
        t_records, got = timed(seqset.records)
        t_copy, _ = timed(clone)
        if run < 0:
            assert len(got) == len(symbols) and all(np.array_equal(g.data, w) for g, w in zip(got, symbols)), "records differ"
            continue
        for key, ms in zip(legs, (t_parse, t_records, t_copy)):
            legs[key].append(ms)
    entry = {"records": len(seqset), "bytes": seqset.total_length}
    entry.update({key: summary(ms) for key, ms in legs.items()})
    med = {key: entry[key]["median_ms"] for key in legs}
    entry["A_over_B"] = med["A_parse_encode"] / med["B_records"]
    entry["B_over_C"] = med["B_records"] / med["C_device_copy"]
    entry["B_gb_per_s"] = seqset.total_length / med["B_records"] / 1e6
    result["shapes"]["records_2000x5000"] = entry
    print("records", json.dumps(entry), flush=True)

    # one record of the whole length: the same bytes as ONE window, where nothing but the kernel and the copy back remain
    one = pli.stripe_ascii_set([np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, seqset.total_length, dtype=np.uint8)]], lossy=True)
    for _ in range(args.warmup):
        one.record(0)
    ms = [timed(lambda: one.record(0))[0] for _ in range(args.runs)]
    copy = [timed(clone)[0] for _ in range(args.runs)]
    entry = {"bytes": one.total_length, "B_record": summary(ms), "C_device_copy": summary(copy)}
    entry["B_over_C"] = entry["B_record"]["median_ms"] / entry["C_device_copy"]["median_ms"]
    entry["B_gb_per_s"] = one.total_length / entry["B_record"]["median_ms"] / 1e6
    result["shapes"]["one_record"] = entry
    print("one_record", json.dumps(entry), flush=True)

    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
