#!/usr/bin/env python3
"""One call of each fused route, for a launch count under `rocprofv3 --kernel-trace --stats` (two libraries side by side:
LM_HIP_LIBRARY, then tools/kernel_stats_diff.py): fused threshold, fused argmax and Scanner::max of one length-20 motif at
100 Mbp, and the threshold and argmax batches of the first 64 JASPAR motifs.  Prints a digest of the results.  GPU box only."""
import hashlib
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tools"))
import lightmotif_amd as lm  # noqa: E402
from lightmotif_amd import io as lmio  # noqa: E402
from bench_configs import motif, resident_sequence  # noqa: E402

torch.cuda.set_device(0)
pli = lm.Pipeline.hip(0)
length, m = 100_000_000, 20
pssm = motif(np.random.default_rng(m), m)
pssms = [r.matrix.normalize(0.1).log_odds() for r in lmio.read(ROOT / "tests" / "golden" / "JASPAR2024.pwm.gz")][:64]
wrap = max(max(len(p) for p in pssms), m) - 1
enc, rows = resident_sequence(pli, length, 5, wrap, 11)
seq = pli.upload(enc.cpu().numpy(), length, wrap, 32)
thr = pssm.score_for_pvalue(1e-5)
res = []
res.append([np.asarray(x).tobytes() for x in pli.score_threshold(pssm, seq, thr)]); k1 = pli.last_kernel
res.append(repr(pli.score_argmax(pssm, seq))); k2 = pli.last_kernel
hit = lm.Scanner(pssm, seq, threshold=thr).max(); k3 = pli.last_kernel
res.append(repr((hit.position, hit.score) if hit else None))
bh = pli.scan_threshold_batch(pssms, [p.score_for_pvalue(1e-5) for p in pssms], seq)
res.append([(np.asarray(c).tobytes(), np.asarray(v).tobytes()) for c, v in bh])
res.append(repr(pli.scan_argmax_batch(pssms, seq)))
print("kernels:", k1, "|", k2, "|", k3, "| digest", hashlib.sha1(repr(res).encode()).hexdigest()[:16])
