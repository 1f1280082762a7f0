#!/usr/bin/env python3
"""From the bytes of a FASTA file to a resident sequence set: three roads over the same in-memory file (60-column lines).

  A  ``scan_cli.read_fasta`` over a text wrapper of the bytes, then ``Pipeline.stripe_ascii_set``: the line loop on the
     host, the only road before ``lm_hip_seqset_from_fasta``
  B  ``Pipeline.stripe_fasta_set``: the container parsed on the device (csrc/fasta.hip)
  C  ``Pipeline.stripe_ascii`` of the residues joined beforehand: the same bases without a container, the floor

The sets of A and B are compared first (record lengths, and a scan that lists every symbol); then the roads alternate
and their medians are reported.  ``python tools/fasta_ingest_bench.py`` writes profiles/fasta_ingest_bench.json.
"""
import argparse
import io
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import lightmotif_amd as lm                                        # noqa: E402
from lightmotif_amd import scan_cli                                # noqa: E402
from lightmotif_amd.lib import fasta_names, stride as lm_stride    # noqa: E402


def make_fasta(n_records, record_len, width=60, seed=7):
    """(the file's bytes, the joined residues, the record names)"""
    rng = np.random.default_rng(seed)
    bases = np.frombuffer(b"ACGTN", dtype=np.uint8)[rng.choice(5, n_records * record_len, p=[0.245, 0.245, 0.245, 0.245, 0.02])]
    full, rest = divmod(record_len, width)
    parts, names = [], []
    for r in range(n_records):
        rec = bases[r * record_len:(r + 1) * record_len]
        body = np.full((full, width + 1), ord("\n"), dtype=np.uint8)
        body[:, :width] = rec[:full * width].reshape(full, width)
        names.append(f"rec{r}")
        parts += [f">rec{r} synthetic record\n".encode(), body.tobytes()]
        if rest:
            parts += [rec[full * width:].tobytes(), b"\n"]
    return b"".join(parts), bases, names


def measure(pli, n_records, record_len, runs=5, warmup=1):
    data, joined, names = make_fasta(n_records, record_len)
    one = np.zeros((1, lm_stride(5, 4)), np.float32)
    one[0, :5] = np.arange(1, 6, dtype=np.float32)
    probe = [lm.ScoringMatrix(one)]

    def way_a():
        records = list(scan_cli.read_fasta(io.TextIOWrapper(io.BytesIO(data), encoding="ascii")))
        return [n for n, _ in records], pli.stripe_ascii_set([s for _, s in records], lossy=True)

    def way_b():
        seqset = pli.stripe_fasta_set(data, lossy=True)
        return fasta_names(data, seqset.header_spans), seqset

    def way_c():
        return None, pli.stripe_ascii(joined, lossy=True)

    def shown(seqset):
        hits = pli.scan_threshold_set(probe, [-np.inf], seqset)
        return [seqset.lengths.tobytes()] + [np.ascontiguousarray(hits.hits[f]).tobytes() for f in ("record", "position", "score")]

    (names_a, set_a), (names_b, set_b) = way_a(), way_b()
    same = bool(names_a == names_b == names and len(set_a) == len(set_b) == n_records and
                set_a.total_length == set_b.total_length == joined.size and shown(set_a) == shown(set_b))
    del set_a, set_b
    ways = {"A": way_a, "B": way_b, "C": way_c}
    times = {k: [] for k in ways}
    for it in range(warmup + runs):
        for k in sorted(ways):
            t0 = time.perf_counter()
            ways[k]()
            if it >= warmup:
                times[k].append((time.perf_counter() - t0) * 1e3)
    out = {"records": n_records, "record_length": record_len, "line_width": 60, "fasta_bytes": len(data), "bases": int(joined.size),
           "runs": runs, "warmup": warmup, "sets_equal": same,
           "ms": {k: {"median": statistics.median(v), "min": min(v), "max": max(v), "all": [round(x, 3) for x in v]}
                  for k, v in times.items()}}
    out["A_over_B"] = out["ms"]["A"]["median"] / out["ms"]["B"]["median"]
    out["B_over_C"] = out["ms"]["B"]["median"] / out["ms"]["C"]["median"]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--records", type=int, default=2_000)
    ap.add_argument("--record-length", type=int, default=50_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "fasta_ingest_bench.json"))
    a = ap.parse_args()
    pli = lm.Pipeline.hip(0)
    cases = [measure(pli, 2_000, 5_000, a.runs, a.warmup)]
    if (a.records, a.record_length) != (2_000, 5_000):
        cases.append(measure(pli, a.records, a.record_length, a.runs, a.warmup))
    result = {"tool": "tools/fasta_ingest_bench.py", "device": "MI355X (gfx950)", "cases": cases}
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps({"cases": [{k: c[k] for k in ("fasta_bytes", "A_over_B", "B_over_C", "sets_equal")} for c in cases], "wrote": a.out}))
    return 0 if all(c["sets_equal"] for c in cases) else 1


if __name__ == "__main__":
    sys.exit(main())
