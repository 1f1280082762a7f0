#!/usr/bin/env python3
"""Host share of the fused calls, library A against library B on one box: the fused threshold call at 1 Mbp / 100 Mbp /
1 Gbp (M = 20, p = 1e-5), the fused argmax at 1 Gbp, the configs[0] small argmax (C ABI, C = 32 and C = 1) and the
2 346-motif x 100 Mbp threshold and argmax batches, and creating + destroying the device handles of those 2 346 matrices
(pssm_create_jaspar).  Every round starts a fresh child process per library in the order
A, B, A (LM_HIP_LIBRARY selects the library; the second A is the A/A control); a child warms every call up once and
reports the median wall time of each.  The table holds, per call, the medians over the rounds of A and B, their
difference, and the A/A differences (of the medians, and the largest of a round).

    tools/build_prev.sh <rev>     # where git is: makes lightmotif_amd/csrc/liblightmotif_hip_prev.so
    python tools/lib_ab_calls.py [--a <lib>] [--b <lib>] [--rounds 7] [--json profiles/<name>.json]      # GPU box"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "lightmotif_amd" / "csrc"


def child():
    import numpy as np
    import torch
    sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tools"))
    import lightmotif_amd as lm
    from lightmotif_amd import _ffi, io as lmio
    from bench_configs import motif, resident_sequence

    def med(fn, reps, warm=1, setup=None):
        """Median wall time of `fn` in us; `setup` runs before every repetition, untimed, and hands `fn` its argument."""
        ts = []
        for rep in range(warm + reps):
            args = (setup(),) if setup else ()
            t0 = time.perf_counter(); fn(*args); ts.append(time.perf_counter() - t0)
        return round(float(np.median(ts[warm:])) * 1e6, 2)

    torch.cuda.set_device(0)
    pli = lm.Pipeline.hip(0, stream=torch.cuda.current_stream().cuda_stream)
    out = {}
    m = 20
    pssm = motif(np.random.default_rng(m), m)
    thr = pssm.score_for_pvalue(1e-5)
    for length, reps in ((1_000_000, 400), (100_000_000, 200), (1_000_000_000, 60)):
        seq, rows = resident_sequence(pli, length, 5, m - 1, 11)
        out[f"threshold_{length}"] = med(lambda: pli.score_threshold_dptr(pssm, seq.data_ptr(), rows + m - 1, 32, 32, m - 1, length, 0, rows, thr), reps, 3)
        if length == 1_000_000_000:
            out[f"argmax_{length}"] = med(lambda: pli.score_argmax_dptr(pssm, seq.data_ptr(), rows + m - 1, 32, 32, m - 1, length, 0, rows), reps, 3)
        del seq
    # configs[0] (tools/c1_latency.py): the fused call through bare ctypes
    p1 = lm.Pipeline.hip(0)
    enc = np.random.default_rng(0xEC011).integers(0, 4, 464_165, dtype=np.uint8)
    small = lm.create(["GTTGACCTTATCAAC", "GTTGATCCAGTCAAC"]).counts.normalize(0.1).log_odds()
    for cols in (32, 1):
        s = p1.stripe(lm.EncodedSequence(enc), cols); s.configure(small)
        slen, swrap, srows, sstride, scols, sptr = s._info()
        found, best, val = C.c_int(0), _ffi.Coords(), C.c_float(0)
        hc, hp = p1._h, small._device(p1)
        out[f"c1_argmax_C{cols}"] = med(lambda: p1._L.lm_hip_score_argmax_f32_dptr(hc, hp, sptr, srows + swrap, sstride, scols, swrap, slen, 0, srows,
                                                                                  C.byref(found), C.byref(best), C.byref(val)), 2000, 200)
    # configs[2]: 2 346 JASPAR motifs x 100 Mbp
    pssms = [r.matrix.normalize(0.1).log_odds() for r in lmio.read(ROOT / "tests" / "golden" / "JASPAR2024.pwm.gz")]
    length, wrap = 100_000_000, max(len(p) for p in pssms) - 1
    enc_seq, rows = resident_sequence(pli, length, 5, wrap, 33)
    seq = pli.upload(enc_seq.cpu().numpy(), length, wrap, 32)
    batch = pli.prepare_batch(pssms, [p.score_for_pvalue(1e-5) for p in pssms])
    out["c3_threshold_batch"] = med(lambda: pli.scan_threshold_batch(batch, None, seq), 12, 2)
    out["c3_argmax_batch"] = med(lambda: pli.scan_argmax_batch(pssms, seq), 12, 2)
    # the device handles of those matrices, created and destroyed on a fresh pipeline
    def create_destroy(p):
        handles = []
        for q in pssms:
            h = C.c_void_p()
            _ffi.check(p._L.lm_hip_pssm_create(p._h, q.data.ctypes.data, q.data.shape[0], q.data.shape[1], q.k, C.byref(h)))
            handles.append(h)
        for h in handles:
            p._L.lm_hip_pssm_destroy(h)
    out["pssm_create_jaspar"] = med(create_destroy, 5, 1, setup=lambda: lm.Pipeline.hip(0))
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--a", default=str(CSRC / "liblightmotif_hip_prev.so"))
    ap.add_argument("--b", default=str(CSRC / "liblightmotif_hip.so"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    if a.child:
        return child()
    import numpy as np
    runs = {"A": [], "B": [], "A2": []}
    for rnd in range(a.rounds):
        for label, lib in (("A", a.a), ("B", a.b), ("A2", a.a)):
            r = subprocess.run([sys.executable, __file__, "--child"], env=dict(os.environ, LM_HIP_LIBRARY=lib), timeout=240,
                               stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            line = [x for x in r.stdout.splitlines() if x.startswith("RESULT ")]
            if r.returncode != 0 or not line:  # nothing more is started on the device after a failure
                sys.exit(f"round {rnd} {label} ({lib}) failed with status {r.returncode}:\n{r.stdout[-2000:]}")
            runs[label].append(json.loads(line[0][7:]))
            print(rnd, label, line[0][7:], flush=True)
    table = {}
    for call in runs["A"][0]:
        A, B, A2 = (np.array([r[call] for r in runs[k]]) for k in ("A", "B", "A2"))
        row = {"A_us": float(np.median(A)), "B_us": float(np.median(B)), "A_again_us": float(np.median(A2))}
        row["B_minus_A_us"] = round(row["B_us"] - row["A_us"], 2)
        row["AA_median_diff_us"] = round(abs(row["A_again_us"] - row["A_us"]), 2)
        row["AA_largest_round_diff_us"] = round(float(np.max(np.abs(A2 - A))), 2)
        row["within_AA_spread"] = bool(abs(row["B_minus_A_us"]) <= row["AA_largest_round_diff_us"])
        table[call] = row
        print(call, row, flush=True)
    if a.json:
        Path(a.json).write_text(json.dumps({"what": __doc__.split("\n\n")[0], "A": os.path.relpath(a.a, ROOT), "B": os.path.relpath(a.b, ROOT),
                                            "rounds": a.rounds, "calls": table, "per_round": runs}, indent=1) + "\n")


if __name__ == "__main__":
    main()
