"""The device-pointer entry points at strides and alignments that are not the natural ones.

`*_dptr` functions and `lm_hip_seq_adopt_dptr` take raw pointers and take `seq_stride`, `out_stride`, `stride`
independently of `cols`; the library picks its kernel from those values and from the pointers' alignment
(include/lightmotif_hip.h, "pointers, strides and alignment").  Whatever fails one of its tests falls through to
byte-load, tiled, generic or cell-by-cell code -- the code an embedder with a torch view at a storage offset, a row
shard of a wider buffer or a matrix with rows wider than 32 runs first.  Every case here places its matrices with
tests/foreign_geometry.py (canary rows around them, canaries in the row padding), compares the results with the C
oracle on the NATURAL layout bit for bit (the numpy oracle for saturating u8 sums), requires every canary to survive,
and checks the launch tally of the call against the contract: no unrolled C = 32 / scan / u8 kernel off the natural
strides, no dword-load kernel on a sequence pointer that is not 4-byte aligned, and in the aligned, natural control
of each family the fast kernel itself -- so that no case passes by testing the fall-back twice.

Rules: pointers are element-aligned (f32: a multiple of 4; bytes: anything); strides are never below the natural
stride nor below `cols`, so code that ignored a stride would still read and write inside the buffers -- no case is
meant to fault, and none may be added that could.  No tolerances.  The tables are pairwise covers of their axes
(tests/test_foreign_geometry_helper.py checks that without a GPU), written out so that a reader sees what runs;
`test_every_case_ran` asserts the counts."""
import collections
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import lightmotif_amd as lm
from foreign_geometry import CANARY_F32, CANARY_U8, embed, extract
from host_walk import scanner_max_strict_host
from lightmotif_amd import _ffi
from oracle import c_oracle as co
from oracle import np_oracle as no

pytestmark = pytest.mark.gpu

ROWS = 584                      # nine 64-row streams and a ragged tail (tests/test_gpu_store_pairs.py)
DEV = "cuda"
POISON_F32 = (np.inf, np.nan, np.nan, np.inf, np.nan, np.inf, np.inf)   # row padding of reduction inputs
TRACK_FOLD_DEFAULT = 8 << 20

# ---- the tables ----------------------------------------------------------------------------------------------------
# motif labels: alphabet (D: DNA, K = 5; P: protein, K = 21) and length.  D7: the zero-padded table (M % 4 != 0);
# D20: dword loads and paired stores; D36: the last unrolled length; D40: the long family; D72: the very long family;
# D100: slices with in-place continuation.  Fused scans: D8, D20 and D24 (the last two drop the last row), D40 and
# D100 (chunked).  `rows`: "all" = (0, rows), "inner" = (3, rows - 5).

# lm_hip_score_f32_dptr at C = 32: (motif, seq byte offset, seq_stride, out offset in floats, out_stride, rows)
SCORE_F32_AXES = (("D7", "D20", "D36", "D40", "D72", "D100", "P12"), (0, 1, 2, 3), (32, 33, 40, 64), (0, 1, 2), (32, 33, 40),
                  ("all", "inner"))
SCORE_F32 = [
    ("D7", 0, 32, 0, 32, "all"), ("D20", 0, 32, 0, 32, "all"), ("D36", 0, 32, 0, 32, "all"), ("D40", 0, 32, 0, 32, "all"),
    ("D72", 0, 32, 0, 32, "all"), ("D100", 0, 32, 0, 32, "all"), ("P12", 0, 32, 0, 32, "all"),          # the controls
    ("D20", 1, 64, 2, 33, "inner"), ("D40", 3, 40, 1, 40, "inner"), ("P12", 2, 33, 2, 40, "all"),
    ("D36", 2, 33, 1, 33, "inner"), ("D72", 1, 40, 1, 32, "all"), ("D72", 3, 64, 0, 33, "all"),
    ("D7", 1, 33, 0, 40, "inner"), ("D100", 3, 33, 2, 32, "inner"), ("P12", 0, 32, 1, 33, "inner"),
    ("D7", 2, 64, 1, 32, "inner"), ("D7", 0, 40, 2, 33, "all"), ("D72", 2, 32, 2, 40, "inner"),
    ("D36", 0, 64, 2, 40, "all"), ("D100", 2, 40, 0, 40, "all"), ("D40", 2, 64, 2, 33, "inner"),
    ("D20", 0, 33, 1, 40, "all"), ("D100", 1, 32, 1, 33, "inner"), ("P12", 1, 64, 1, 33, "inner"),
    ("D20", 3, 40, 0, 40, "inner"), ("P12", 3, 32, 1, 40, "all"), ("D36", 3, 40, 1, 32, "inner"),
    ("D40", 1, 33, 0, 33, "inner"), ("D36", 1, 33, 2, 40, "all"), ("P12", 1, 40, 2, 33, "all"),
    ("D100", 1, 64, 1, 32, "inner"), ("D72", 0, 33, 0, 40, "all"), ("D7", 3, 32, 1, 33, "all"),
    ("D20", 2, 40, 0, 40, "all"),
    # natural strides at every sequence offset (the byte-load members of the family) and at unaligned outputs
    ("D7", 1, 32, 0, 32, "all"), ("D20", 2, 32, 1, 32, "inner"), ("D36", 3, 32, 2, 32, "all"), ("D40", 1, 32, 0, 32, "inner"),
    ("D72", 2, 32, 1, 32, "all"), ("D100", 3, 32, 2, 32, "inner"), ("P12", 1, 32, 0, 32, "all"), ("D20", 0, 32, 1, 32, "all"),
    ("D100", 0, 32, 2, 32, "all"),
]

# ... at other column counts, a list: (cols, motif, seq byte offset, seq_stride, out offset, out_stride, rows).
# C = 16: the 16-column kernel at offset 0, which must step aside at offset 1 (dword loads) and off its strides;
# C = 33: stride 64 in (the natural one) and 48 out.
SCORE_F32_OTHER = [
    (16, "D20", 0, 32, 0, 16, "all"), (16, "D20", 1, 32, 0, 16, "all"), (16, "D7", 0, 32, 1, 16, "inner"),
    (16, "D20", 0, 40, 2, 24, "inner"), (33, "D20", 0, 64, 0, 48, "all"), (33, "D40", 1, 64, 1, 48, "inner"),
]

# lm_hip_score_rows_into + lm_hip_argmax / lm_hip_max on an adopted sequence, track_argmax on:
# (motif, (seq byte offset, seq_stride), rows, track_fold_cells: "fold0" = 0, "default")
SCORE_HANDLE_AXES = (("D7", "D20", "D40", "D100", "P12"), ((0, 32), (1, 32), (0, 40), (3, 64)), ("all", "inner"),
                     ("fold0", "default"))
SCORE_HANDLE = [
    ("D7", (0, 32), "all", "default"), ("D20", (0, 32), "all", "fold0"), ("D40", (0, 32), "all", "default"),
    ("D100", (0, 32), "all", "fold0"), ("P12", (0, 32), "all", "default"),                                # the controls
    ("D100", (3, 64), "inner", "default"), ("P12", (0, 40), "inner", "fold0"), ("D20", (1, 32), "inner", "default"),
    ("D7", (1, 32), "all", "fold0"), ("D40", (3, 64), "inner", "fold0"), ("D20", (0, 40), "all", "default"),
    ("D7", (0, 32), "inner", "default"), ("D7", (3, 64), "all", "fold0"), ("P12", (3, 64), "inner", "default"),
    ("D7", (0, 40), "all", "default"), ("D100", (0, 40), "all", "fold0"), ("P12", (1, 32), "all", "default"),
    ("D40", (0, 40), "all", "default"), ("D20", (3, 64), "inner", "default"), ("D100", (1, 32), "inner", "fold0"),
    ("D40", (1, 32), "all", "fold0"),
]

# fused argmax, its shard form with first_cell_rule = 0, fused threshold at the 0.999 quantile and at -inf:
# (op, motif, seq byte offset, seq_stride, prefilter, rows, protein options: "b" = block_prefilter on,
#  "p" = pair_prefilter_protein on, "-" = off)
FUSED_AXES = (("argmax", "shard0", "thr_q", "thr_ninf"), ("D8", "D20", "D24", "D40", "D100", "P12"), (0, 1, 2, 3),
              (32, 33, 40, 64), (1, 0), ("all", "inner"), ("bp", "b-", "-p", "--"))
FUSED = [
    ("argmax", "D8", 0, 32, 1, "all", "bp"), ("shard0", "D8", 0, 32, 0, "all", "bp"), ("thr_q", "D20", 0, 32, 1, "all", "bp"),
    ("thr_ninf", "D20", 0, 32, 0, "all", "bp"), ("argmax", "D24", 0, 32, 1, "all", "bp"), ("shard0", "D24", 0, 32, 0, "all", "bp"),
    ("thr_q", "D40", 0, 32, 1, "all", "bp"), ("thr_ninf", "D40", 0, 32, 0, "all", "bp"), ("argmax", "D100", 0, 32, 1, "all", "bp"),
    ("shard0", "D100", 0, 32, 0, "all", "bp"), ("thr_q", "P12", 0, 32, 1, "all", "bp"),
    ("thr_ninf", "P12", 0, 32, 0, "all", "bp"),                                                          # the controls
    ("shard0", "D20", 1, 64, 1, "inner", "b-"), ("thr_q", "D100", 2, 40, 0, "inner", "--"), ("argmax", "P12", 3, 33, 0, "inner", "-p"),
    ("thr_ninf", "D8", 3, 40, 1, "all", "-p"), ("thr_ninf", "D24", 2, 33, 1, "all", "--"), ("argmax", "D40", 1, 64, 0, "all", "--"),
    ("thr_q", "D24", 3, 64, 0, "inner", "b-"), ("shard0", "D40", 2, 32, 0, "inner", "-p"), ("thr_q", "D8", 1, 33, 0, "inner", "bp"),
    ("argmax", "D20", 2, 40, 0, "all", "b-"), ("thr_ninf", "D100", 0, 64, 1, "inner", "-p"), ("shard0", "D20", 3, 32, 1, "all", "--"),
    ("shard0", "D100", 0, 33, 1, "inner", "b-"), ("thr_ninf", "P12", 1, 32, 1, "all", "b-"), ("thr_q", "D24", 1, 40, 0, "all", "-p"),
    ("shard0", "P12", 0, 40, 0, "inner", "--"), ("argmax", "D8", 2, 64, 1, "all", "bp"), ("thr_ninf", "D40", 3, 40, 0, "inner", "bp"),
    ("thr_ninf", "P12", 2, 64, 0, "all", "--"), ("argmax", "D20", 0, 33, 0, "inner", "-p"), ("argmax", "D40", 1, 33, 0, "all", "b-"),
    ("thr_ninf", "D100", 1, 40, 1, "all", "--"), ("shard0", "D8", 0, 33, 0, "all", "b-"), ("thr_q", "D8", 0, 64, 1, "all", "--"),
    ("thr_ninf", "D100", 3, 64, 0, "inner", "bp"),
    # natural stride, unaligned: the scans that load bytes
    ("thr_q", "D20", 1, 32, 1, "all", "bp"), ("argmax", "D24", 2, 32, 1, "inner", "bp"), ("thr_q", "P12", 3, 32, 1, "inner", "bp"),
    ("argmax", "D100", 1, 32, 1, "all", "bp"),
    # more controls: every scan of the prefilter where it is fast -- the DNA pair scan at each length, and the
    # protein scans under each setting of the two options (block scan, one symbol per byte load, pair scan)
    ("thr_q", "D8", 0, 32, 1, "all", "bp"), ("thr_q", "D24", 0, 32, 1, "all", "bp"), ("thr_q", "D100", 0, 32, 1, "all", "bp"),
    ("thr_q", "P12", 0, 32, 1, "all", "b-"), ("thr_q", "P12", 0, 32, 1, "all", "-p"), ("thr_q", "P12", 0, 32, 1, "all", "--"),
]

# ... with a NaN weight that makes the FIRST cell of the scored block NaN (and a quarter of the others): the
# first-cell rule answers (0, 0) / NaN, the shard form skips it.  A list: (op, motif, seq byte offset, seq_stride, rows)
FUSED_NAN = [
    ("argmax", "D20", 0, 32, "all"), ("shard0", "D20", 0, 32, "inner"), ("argmax", "D20", 1, 32, "inner"),
    ("shard0", "D20", 0, 40, "all"), ("argmax", "D40", 2, 64, "all"), ("shard0", "D40", 3, 33, "inner"),
]

# lm_hip_score_u8_dptr: (M, saturate, seq byte offset, seq_stride, out byte offset, out_stride, rows)
SCORE_U8_AXES = ((12, 40), (1, 0), (0, 1, 2, 3), (32, 33, 40, 64), (0, 1, 3), (32, 37), ("all", "inner"))
SCORE_U8 = [
    (12, 1, 0, 32, 0, 32, "all"), (12, 0, 0, 32, 0, 32, "all"), (40, 1, 0, 32, 0, 32, "all"), (40, 0, 0, 32, 0, 32, "all"),  # controls
    (40, 0, 1, 64, 1, 37, "inner"), (12, 1, 3, 40, 3, 37, "inner"), (12, 1, 2, 33, 1, 32, "inner"), (40, 0, 2, 33, 3, 37, "all"),
    (12, 1, 1, 64, 3, 32, "all"), (40, 0, 3, 40, 1, 32, "all"), (40, 1, 0, 32, 1, 37, "inner"), (12, 1, 2, 40, 0, 37, "inner"),
    (40, 0, 3, 33, 0, 37, "inner"), (40, 1, 2, 32, 3, 32, "all"), (40, 0, 1, 64, 0, 37, "inner"), (12, 0, 0, 64, 3, 32, "inner"),
    (40, 1, 0, 33, 3, 32, "inner"), (40, 1, 3, 64, 3, 37, "inner"), (40, 1, 2, 64, 1, 32, "inner"), (12, 1, 1, 32, 0, 32, "inner"),
    (40, 0, 1, 33, 1, 37, "all"), (12, 1, 3, 32, 1, 32, "all"), (12, 1, 0, 40, 1, 32, "all"), (40, 1, 1, 40, 3, 32, "all"),
    (40, 0, 3, 32, 0, 32, "all"), (12, 0, 2, 32, 0, 32, "all"),          # natural strides, an unaligned sequence alone
    (12, 1, 0, 40, 0, 32, "all"), (40, 0, 0, 33, 0, 32, "inner"), (12, 0, 1, 64, 0, 32, "all"),
    (40, 1, 2, 40, 0, 32, "all"),                                        # a foreign sequence stride alone
]

# reductions over f32: ((cols, rows), pointer offset in elements, stride - cols, values).  12 295 or 12 320 cells: three
# 4096-cell threshold chunks and a ragged piece, more than one 8192-cell span of argmax_flat; the last two shapes have
# ncells % 4 == 3.  Every case runs argmax, max, the shard argmax with the first-cell rule on and off, and threshold
# at a tied value, at -0.0, at -inf and above the maximum.
SHAPES = ((32, 385), (5, 2459), (1, 12295))
REDUCE_F32_AXES = (SHAPES, (0, 1, 2, 3), (0, 1, 8), ("ties", "nan2", "specials", "nan00", "neginf"))
REDUCE_F32 = [
    ((32, 385), 0, 0, "ties"), ((5, 2459), 0, 0, "nan2"), ((1, 12295), 0, 0, "specials"),               # flat, aligned
    ((1, 12295), 1, 8, "ties"), ((5, 2459), 1, 1, "specials"), ((32, 385), 2, 8, "specials"), ((1, 12295), 2, 1, "nan2"),
    ((5, 2459), 3, 8, "nan00"), ((32, 385), 3, 1, "neginf"), ((32, 385), 1, 0, "nan00"), ((5, 2459), 2, 0, "neginf"),
    ((1, 12295), 0, 1, "nan00"), ((1, 12295), 0, 8, "neginf"), ((5, 2459), 3, 0, "ties"), ((32, 385), 3, 8, "nan2"),
    ((1, 12295), 2, 1, "ties"), ((1, 12295), 3, 0, "specials"), ((32, 385), 1, 8, "neginf"), ((32, 385), 2, 1, "nan00"),
    ((32, 385), 1, 0, "nan2"),
]
# ... and over u8 (argmax and threshold): "ties" = small values, "top" = many cells at 255; the padding holds 255
REDUCE_U8_AXES = (SHAPES, (0, 1, 2, 3), (0, 1, 8), ("ties", "top"))
REDUCE_U8 = [
    ((32, 385), 0, 0, "ties"), ((32, 385), 2, 8, "top"), ((5, 2459), 1, 0, "top"), ((1, 12295), 1, 8, "ties"),
    ((5, 2459), 2, 1, "ties"), ((1, 12295), 3, 1, "top"), ((5, 2459), 3, 8, "ties"), ((1, 12295), 0, 1, "top"),
    ((32, 385), 1, 1, "top"), ((1, 12295), 2, 0, "ties"), ((5, 2459), 0, 8, "ties"), ((32, 385), 3, 0, "top"),
]

# lm_hip_encode_dptr: (source byte offset, destination byte offset, length, alphabet, mode).  "*_bad": the text holds
# invalid bytes -- two where the length allows, one in the 16-byte body and one in the byte tail of an aligned call
ENCODE_AXES = ((0, 1, 5, 16), (0, 1, 5, 16), (0, 1, 15, 16, 17, 4099), ("D", "P"), ("strict", "lossy", "strict_bad", "lossy_bad"))
ENCODE = [
    (0, 0, 4099, "D", "strict"), (0, 0, 4099, "P", "strict_bad"), (16, 16, 4099, "D", "lossy_bad"), (5, 1, 0, "P", "lossy"),
    (16, 5, 17, "P", "strict"), (1, 5, 15, "D", "lossy"), (1, 16, 16, "P", "strict"), (5, 1, 16, "D", "strict_bad"),
    (1, 1, 1, "P", "lossy_bad"), (0, 16, 1, "D", "lossy"), (5, 0, 15, "P", "lossy_bad"), (0, 5, 16, "D", "lossy_bad"),
    (16, 0, 17, "D", "lossy"), (1, 16, 17, "D", "strict_bad"), (5, 5, 1, "P", "strict_bad"), (16, 1, 15, "D", "strict"),
    (1, 0, 0, "D", "strict"), (0, 1, 17, "P", "lossy_bad"), (5, 5, 4099, "D", "lossy"), (5, 16, 1, "P", "strict"),
    (0, 16, 15, "D", "strict_bad"), (16, 0, 16, "P", "strict_bad"), (16, 5, 0, "D", "strict"), (16, 0, 1, "P", "lossy_bad"),
    (0, 16, 0, "D", "strict"), (1, 1, 4099, "P", "strict"), (5, 16, 17, "P", "strict_bad"), (1, 5, 16, "D", "lossy"),
]
BAD_AT = {1: (0,), 15: (3, 14), 16: (3, 15), 17: (5, 16), 4099: (4090, 4097)}
# ... a strict call whose only invalid byte lies in the byte tail, a list: (source offset, destination offset, length,
# alphabet, index of the byte)
ENCODE_TAIL = [(0, 0, 17, "D", 16), (0, 0, 4099, "P", 4097), (16, 16, 4099, "D", 4096), (1, 0, 4099, "D", 4098)]

# lm_hip_stripe_dptr and lm_hip_configure_wrap_dptr: (cols, d_data byte offset, stride: "nat" = lm_hip_stride(cols, 1),
# "+1", "+4" beyond it, or 64, length, wrap: none, 19 or three more than the row count, op: "stripe" = one call with the
# wrap, "stripe+wrap" = stripe without, then configure_wrap)
STRIPE_AXES = ((32, 16, 33), (0, 1, 4), ("nat", "+1", "+4", "64"), (31, 1000, 18677), ("none", "19", "big"), ("stripe", "stripe+wrap"))
STRIPE = [
    (32, 0, "nat", 18677, "19", "stripe"), (16, 0, "nat", 18677, "19", "stripe+wrap"), (32, 1, "64", 1000, "big", "stripe+wrap"),
    (16, 4, "+1", 31, "big", "stripe"), (33, 0, "+4", 1000, "none", "stripe"), (33, 4, "+4", 31, "19", "stripe+wrap"),
    (33, 1, "+1", 18677, "none", "stripe+wrap"), (32, 4, "64", 31, "none", "stripe"), (16, 1, "+1", 1000, "19", "stripe"),
    (33, 0, "nat", 31, "big", "stripe"), (16, 4, "nat", 1000, "none", "stripe+wrap"), (16, 1, "+4", 18677, "big", "stripe+wrap"),
    (16, 0, "64", 18677, "19", "stripe"), (32, 1, "+1", 31, "19", "stripe+wrap"), (32, 4, "+4", 18677, "none", "stripe"),
    (16, 0, "+1", 18677, "19", "stripe"), (16, 1, "nat", 1000, "19", "stripe"),
]

# lm_hip_seq_adopt_dptr: ((byte offset, stride), group of calls), the full product
ADOPT_AXES = (((0, 32), (1, 32), (0, 40)), ("score_into", "batches", "scanner", "discrete", "housekeeping"))
ADOPTED = [(place, group) for place in ADOPT_AXES[0] for group in ADOPT_AXES[1]]


def _never(*_):
    return False


# name -> (table, axes or None for a plain list, pairs of axis values that cannot meet)
TABLES = {
    "score_f32": (SCORE_F32, SCORE_F32_AXES, _never),
    "score_f32_other": (SCORE_F32_OTHER, None, _never),
    "score_handle": (SCORE_HANDLE, SCORE_HANDLE_AXES, _never),
    "fused": (FUSED, FUSED_AXES, _never),
    "fused_nan": (FUSED_NAN, None, _never),
    "score_u8": (SCORE_U8, SCORE_U8_AXES, _never),
    "reduce_f32": (REDUCE_F32, REDUCE_F32_AXES, _never),
    "reduce_u8": (REDUCE_U8, REDUCE_U8_AXES, _never),
    # (an empty text holds no invalid byte)
    "encode": (ENCODE, ENCODE_AXES, lambda i, j, a, b: (i, j) == (2, 4) and a == 0 and b.endswith("bad")),
    "encode_tail": (ENCODE_TAIL, None, _never),
    # (the natural stride of 33 columns IS 64)
    "stripe": (STRIPE, STRIPE_AXES, lambda i, j, a, b: (i, j) == (0, 2) and a == 33 and b == "64"),
    "adopted": (ADOPTED, ADOPT_AXES, _never),
}
EXPECTED_CASES = {"score_f32": 44, "score_f32_other": 6, "score_handle": 21, "fused": 47, "fused_nan": 6, "score_u8": 30,
                  "reduce_f32": 20, "reduce_u8": 12, "encode": 28, "encode_tail": 4, "stripe": 17, "adopted": 15}

RAN = collections.Counter()                       # cases that ran to their last assertion, per table
SEEN = collections.defaultdict(collections.Counter)   # (table, "control" | "natural" | "foreign") -> last_kernel -> cases


def case_id(case):
    return "-".join("x".join(map(str, v)) if isinstance(v, tuple) else str(v) for v in case)


def cases(name):
    return pytest.mark.parametrize("case", TABLES[name][0], ids=case_id)


# ---- shared inputs and references, computed once -----------------------------------------------------------------

def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def differing(got, want):
    """Cells in which two arrays differ (every cell when the shapes do): `assert differing(a, b) == 0` fails with a
    number in place of two matrices."""
    got, want = np.asarray(got), np.asarray(want)
    return int((got != want).sum()) if got.shape == want.shape else max(got.size, want.size, 1)


class Checks:
    """The result checks and the route check of a case are independent: both run, and a case that fails both says so."""

    def __init__(self):
        self.failed = []

    def __call__(self, what):
        return _Check(self, what)

    def done(self):
        assert not self.failed, "\n".join(self.failed)


class _Check:
    def __init__(self, checks, what):
        self.checks, self.what = checks, what

    def __enter__(self):
        return self

    def __exit__(self, kind, error, trace):
        if kind is not None and issubclass(kind, AssertionError):
            self.checks.failed.append(f"[{self.what}] {error}")
            return True
        return False


@pytest.fixture(scope="module")
def tp():
    """A pipeline of the module's own that counts the registry rows it launches."""
    p = lm.Pipeline.hip(0)
    p.set_option("tally_launches", 1)
    return p


def motif_shape(label):
    return (21 if label[0] == "P" else 5), int(label[1:])


@functools.lru_cache(maxsize=None)
def weights(label):
    k, m = motif_shape(label)
    rng = np.random.default_rng(7919 * m + k)
    p = np.zeros((m, co.stride(k, 4)), np.float32)
    p[:, :k] = rng.normal(0, 2, (m, k))
    p[:, k - 1] = -np.inf
    return p


@functools.lru_cache(maxsize=None)
def motif(label):
    return lm.ScoringMatrix(weights(label), protein=label[0] == "P")


@functools.lru_cache(maxsize=None)
def sequence(k, cols):
    """(encoded symbols, the oracle's striped matrix with 127 wrap rows): `ROWS` rows, a padded tail of 11 cells.  The
    first m - 1 wrap rows are the wrap rows of configure_wrap(m - 1)."""
    length = ROWS * cols - 11
    rng = np.random.default_rng(1000 * k + cols)
    enc = rng.integers(0, k, length, dtype=np.uint8)
    enc[rng.random(length) < 0.99] %= (k - 1)      # a few N / X: some windows score -inf
    ref = co.stripe(enc, cols, k)
    co.configure_wrap(ref, 127)
    assert ref.rows == ROWS
    return enc, ref


@functools.lru_cache(maxsize=None)
def oracle_scores(label, cols):
    """The oracle's score matrix of the whole row range on the natural layout (read-only: shared between cases)."""
    k, _ = motif_shape(label)
    want, mi = co.score_rows(sequence(k, cols)[1], weights(label))
    want.setflags(write=False)
    return want, mi


def row_range(rows_id):
    return (0, ROWS) if rows_id == "all" else (3, ROWS - 5)


def embed_sequence(k, cols, m, stride, offset, spare_rows=0):
    """The striped matrix with m - 1 wrap rows at a foreign place.  Padding, guard rows and spare rows hold a VALID symbol:
    a kernel that walks the rows with the wrong stride computes wrong scores, it does not leave the weight tables."""
    _, ref = sequence(k, cols)
    live = ref.data[: ROWS + m - 1, :cols]
    if spare_rows:
        live = np.concatenate([live, np.full((spare_rows, cols), k - 2, np.uint8)])
    return embed(live, stride, offset, k - 2, device=DEV)


def untouched(emb, original=None):
    """An input buffer after the call: no canary moved, and the payload is what was put there."""
    payload, problems = extract(emb)
    assert problems == [], problems
    if original is not None:
        assert differing(payload.view(np.uint8), np.ascontiguousarray(original).view(np.uint8)) == 0


# ---- the route contract ------------------------------------------------------------------------------------------------

FAST_FAMILIES = {"c32", "pre", "preblk", "pre2", "pre2_protein", "pre2_multi", "u8", "u8_pairs"}
DWORD_FAMILIES = {"preblk", "pre2", "pre2_protein", "pre2_multi", "u8_pairs"}
DWORD_SLOTS = {"STORE_QL", "STORE_C16", "STORE_TRACK"}


def loads_dwords(row):
    family, _, m, slot = row
    return family in DWORD_FAMILIES or (family == "c32" and (slot in DWORD_SLOTS or m > 36))


def check_route(table, tp, tally, *, seq_offset, natural, control, must=None, no_u8=False, kernel=None):
    """The launch tally of one call against the contract, independently of the results."""
    kernel = kernel or tp.last_kernel
    fast = sorted(r for r in tally if r[0] in FAST_FAMILIES)
    if not natural:
        assert fast == [], (kernel, "an unrolled kernel ran off its strides", fast)
    if seq_offset % 4:
        assert [r for r in fast if loads_dwords(r)] == [], (kernel, "a dword-load kernel ran on an unaligned sequence", fast)
    if no_u8:
        assert [r for r in fast if r[0] in ("u8", "u8_pairs")] == [], (kernel, "a u8 kernel ran on an unaligned score matrix", fast)
    if control:
        assert natural and seq_offset % 4 == 0
        assert fast != [], (kernel, "the control did not take the fast kernel", tally)
        if must is not None:
            assert any(must(r) for r in fast), (kernel, "the control did not take ITS fast kernel", fast)
    SEEN[table, "control" if control else "natural" if natural and seq_offset % 4 == 0 else "foreign"][kernel] += 1


def tallied(tp, call):
    """Runs `call` between two reads of the launch tally: (its result, the rows it launched)."""
    torch.cuda.synchronize()            # the embeddings were filled on torch's stream, the pipeline runs on its own
    tp.launch_tally()
    result = call()
    tp.sync()
    return result, tp.launch_tally()


# ---- 1. lm_hip_score_f32_dptr ---------------------------------------------------------------------------------------

def store_must(label, cols):
    """The fast row the aligned, natural store of this motif is promised (the header's table of shapes)."""
    k, m = motif_shape(label)
    if cols == 16:
        return lambda r: r[3] == "STORE_C16"
    if m <= 36:
        return lambda r: r == ("c32", int(k > 16), (m + 3) // 4 * 4, "STORE_QL")
    if m <= 88:
        return lambda r: r[0] == "c32" and r[2] == (m + 3) // 4 * 4 and r[3] == "STORE_QL"
    return lambda r: r[0] == "c32" and r[3] == "CONTINUE"


def run_score_f32(table, tp, cols, label, seq_off, seq_stride, out_off, out_stride, rows_id):
    k, m = motif_shape(label)
    want, want_mi = oracle_scores(label, cols)
    a, b = row_range(rows_id)
    seq = embed_sequence(k, cols, m, seq_stride, seq_off)
    out = embed(np.full((b - a, cols), CANARY_F32, np.uint32), out_stride, 4 * out_off, CANARY_F32, device=DEV)
    (orow, mi), tally = tallied(tp, lambda: tp.score_dptr(motif(label), seq.ptr, ROWS + m - 1, seq_stride, cols, m - 1,
                                                          ROWS * cols - 11, a, b, out.ptr, out_stride))
    got, problems = extract(out)
    print(table, label, tp.last_kernel, sorted(tally))
    checks = Checks()
    with checks("results"):
        assert problems == [], (tp.last_kernel, problems)       # row padding counts as canary (pli/mod.rs:103)
        assert (orow, mi) == (b - a, want_mi)
        assert differing(got, bits(want[a:b, :cols])) == 0, tp.last_kernel
        untouched(seq)
    natural = seq_stride == 32 and out_stride == cols
    with checks("route"):
        check_route(table, tp, tally, seq_offset=seq_off, natural=natural,
                    control=natural and seq_off == 0 and out_off == 0 and rows_id == "all", must=store_must(label, cols))
    checks.done()
    RAN[table] += 1


@cases("score_f32")
def test_score_f32(tp, case):
    run_score_f32("score_f32", tp, 32, *case)


@cases("score_f32_other")
def test_score_f32_other_columns(tp, case):
    cols, label, seq_off, seq_stride, out_off, out_stride, rows_id = case
    run_score_f32("score_f32_other", tp, cols, label, seq_off, seq_stride, out_off, out_stride, rows_id)


@cases("score_handle")
def test_score_rows_into_on_an_adopted_sequence(tp, case):
    label, (seq_off, seq_stride), rows_id, fold = case
    k, m = motif_shape(label)
    want, want_mi = oracle_scores(label, 32)
    a, b = row_range(rows_id)
    block = np.ascontiguousarray(want[a:b])
    emb = embed_sequence(k, 32, m, seq_stride, seq_off)
    seq = tp.adopt_sequence(emb.ptr, ROWS, m - 1, 32, seq_stride, ROWS * 32 - 11, protein=k == 21, keepalive=emb)
    scores = lm.StripedScores.empty(tp, 32)
    tp.set_track_argmax(True)
    tp.set_option("track_fold_cells", 0 if fold == "fold0" else TRACK_FOLD_DEFAULT)
    try:
        _, tally = tallied(tp, lambda: tp.score_rows_into(motif(label), seq, range(a, b), scores))
        kernel = tp.last_kernel
        print("score_handle", label, kernel, sorted(tally))
        best = tp.argmax(scores)                     # the tracked maximum where the store kernel left one
        top = tp.max(scores)
        got = scores.matrix()
    finally:
        tp.set_option("track_fold_cells", TRACK_FOLD_DEFAULT)
    checks = Checks()
    with checks("results"):
        assert got.shape == block.shape and scores.max_index == want_mi
        assert differing(bits(got[:, :32]), bits(block[:, :32])) == 0, kernel
        assert best == co.argmax(block, 32), kernel
        assert bits([top])[0] == bits([block[best]])[0]
        assert tp.argmax_handle_shard(scores, False)[0] == best     # no NaN here: the shard rule changes nothing
        untouched(emb)
    natural = seq_stride == 32
    # below track_fold_cells one launch stores and tracks, from it on the store leaves block maxima (the padded table
    # and the long family included); the sliced D100 tracks nothing
    slot = "STORE_ARGMAX" if fold == "fold0" else "STORE_TRACK"
    must = (lambda r: r[0] == "c32" and r[3] == "CONTINUE") if m > 64 else (lambda r: r[0] == "c32" and r[3] == slot)
    with checks("route"):
        check_route("score_handle", tp, tally, seq_offset=seq_off, natural=natural,
                    control=natural and seq_off == 0 and rows_id == "all", must=must, kernel=kernel)
    checks.done()
    RAN["score_handle"] += 1


# ---- 2. the fused forms -----------------------------------------------------------------------------------------------

def last_maximum_without_first_cell_rule(block, cols):
    """Maximum::argmax (pli/mod.rs:135-155) without its `scores[0][0] is NaN` branch: the greatest cell, NaN cells never
    candidates, the last one in (row, col) order among equals."""
    live = block[:, :cols]
    with np.errstate(invalid="ignore"):
        top = np.max(live[~np.isnan(live)])
        r, c = np.argwhere(live == top)[-1]
    return int(r), int(c)


def run_fused(table, tp, op, label, p, pssm, want, seq_off, seq_stride, rows_id, control, must=None):
    k, m = motif_shape(label)
    a, b = row_range(rows_id)
    block = np.ascontiguousarray(want[a:b])
    seq = embed_sequence(k, 32, m, seq_stride, seq_off)
    args = (pssm, seq.ptr, ROWS + m - 1, seq_stride, 32, m - 1, ROWS * 32 - 11, a, b)
    checks = Checks()
    if op in ("argmax", "shard0"):
        got, tally = tallied(tp, lambda: tp.score_argmax_dptr(*args, first_cell_rule=op == "argmax"))
        kernel = tp.last_kernel
        where = co.argmax(block, 32) if op == "argmax" else last_maximum_without_first_cell_rule(block, 32)
        with checks("results"):
            assert got is not None and got[0] == where, (kernel, got, where)
            assert bits([got[1]])[0] == bits([block[where]])[0], (kernel, got, block[where])
    else:
        finite = np.sort(block[:, :32][np.isfinite(block[:, :32])])
        t = float(finite[int(0.999 * (finite.size - 1))]) if op == "thr_q" else float("-inf")
        (coords, values), tally = tallied(tp, lambda: tp.score_threshold_dptr(*args, t))
        kernel = tp.last_kernel
        where = co.threshold(block, 32, t)
        assert len(where) == (b - a) * 32 if op == "thr_ninf" else 0 < len(where) < 200
        with checks("results"):
            assert differing(np.asarray(coords).reshape(-1, 2), where.astype(np.int64)) == 0, kernel   # coordinates AND order
            assert differing(bits(values), bits(block[where[:, 0], where[:, 1]])) == 0, kernel
    print(table, op, label, kernel, sorted(tally))
    with checks("results"):
        untouched(seq)
    with checks("route"):
        check_route(table, tp, tally, seq_offset=seq_off, natural=seq_stride == 32, control=control, must=must)
    checks.done()
    RAN[table] += 1


@cases("fused")
def test_fused(tp, case):
    op, label, seq_off, seq_stride, prefilter, rows_id, popt = case
    want, _ = oracle_scores(label, 32)
    tp.set_prefilter(bool(prefilter))
    tp.set_option("block_prefilter", popt[0] == "b")
    tp.set_option("pair_prefilter_protein", popt[1] == "p")
    try:
        # a threshold far up the tail goes through the discrete prefilter: pairs of symbols for DNA; for protein the
        # pair scan where its option is on, else 4-row symbol blocks, else one byte per lane and row
        scan = None
        if op == "thr_q" and prefilter:
            scan = "pre2" if label[0] == "D" else "pre2_protein" if popt[1] == "p" else "preblk" if popt[0] == "b" else "pre"
        run_fused("fused", tp, op, label, weights(label), motif(label), want, seq_off, seq_stride, rows_id,
                  control=seq_off == 0 and seq_stride == 32 and rows_id == "all",
                  must=None if scan is None else lambda r: r[0] == scan)
    finally:
        tp.set_prefilter(True)
        tp.set_option("block_prefilter", 1)
        tp.set_option("pair_prefilter_protein", 0)


@cases("fused_nan")
def test_fused_with_a_nan_first_cell(tp, case):
    op, label, seq_off, seq_stride, rows_id = case
    k, m = motif_shape(label)
    enc, ref = sequence(k, 32)
    a, _ = row_range(rows_id)
    p = weights(label).copy()
    p[0, enc[a]] = np.nan          # cell (0, 0) of the block is the window at position a (column 0, row a)
    want, _ = co.score_rows(ref, p)
    assert np.isnan(want[a, 0]) and 0.1 < np.isnan(want[:, :32]).mean() < 0.5
    run_fused("fused_nan", tp, op, label, p, lm.ScoringMatrix(p), want, seq_off, seq_stride, rows_id, control=False)


# ---- 3. lm_hip_score_u8_dptr ------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def discrete(m):
    """Weights whose sums straddle 255, so that the saturating and the wrapping flavour differ in about half the cells."""
    rng = np.random.default_rng(131 * m)
    w = rng.integers(0, 530 // m + 1, (m, 5), dtype=np.uint8)
    _, ref = sequence(5, 32)
    wrap, _ = co.score_rows_u8(ref, w)
    sat = no.score_rows_u8_saturating(ref.data, 32, ROWS * 32 - 11, w, 0, ROWS)
    differ = (wrap[:, :32] != sat).mean()
    assert 0.2 < differ < 0.8, differ
    return lm.DiscreteMatrix(w, 1.0, np.zeros(m, np.float32), 0.0), np.ascontiguousarray(wrap[:, :32]), sat


@cases("score_u8")
def test_score_u8(tp, case):
    m, saturate, seq_off, seq_stride, out_off, out_stride, rows_id = case
    dm, want_wrap, want_sat = discrete(m)
    want = want_sat if saturate else want_wrap
    a, b = row_range(rows_id)
    seq = embed_sequence(5, 32, m, seq_stride, seq_off)
    out = embed(np.full((b - a, 32), CANARY_U8, np.uint8), out_stride, out_off, CANARY_U8, device=DEV)
    (orow, mi), tally = tallied(tp, lambda: tp.score_u8_dptr(dm, seq.ptr, ROWS + m - 1, seq_stride, 32, m - 1, ROWS * 32 - 11,
                                                             a, b, out.ptr, out_stride, saturate=bool(saturate)))
    got, problems = extract(out)
    print("score_u8", case, tp.last_kernel, sorted(tally))
    checks = Checks()
    with checks("results"):
        assert problems == [], (tp.last_kernel, problems)
        assert (orow, mi) == (b - a, ROWS * 32 - 11 + 1 - m)
        assert differing(got, want[a:b]) == 0, tp.last_kernel
        untouched(seq)
    natural = seq_stride == 32 and out_stride == 32
    # DNA on an aligned matrix: two symbols per lookup, motifs beyond 36 rows in slices of that kernel
    with checks("route"):
        check_route("score_u8", tp, tally, seq_offset=seq_off, natural=natural, no_u8=out_off % 4 != 0,
                    control=natural and seq_off == 0 and out_off == 0 and rows_id == "all", must=lambda r: r[0] == "u8_pairs")
    checks.done()
    RAN["score_u8"] += 1


# ---- 4. reductions ----------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def reduce_values(shape, kind):
    cols, rows = shape
    rng = np.random.default_rng(rows + 17 * len(kind))
    x = rng.integers(-3, 4, (rows, cols)).astype(np.float32)       # ties everywhere: the LAST maximal cell must win
    n = x.size
    if kind == "nan2":
        x.reshape(-1)[rng.choice(n, n // 50, replace=False)] = np.nan
        x[0, 0] = 1.0                                                # (the first cell is "nan00"'s business)
    elif kind == "specials":
        flat = x.reshape(-1)
        where = rng.choice(n, 40, replace=False)
        flat[where[:10]] = np.inf                                    # several +inf: the last of them wins
        flat[where[10:20]] = -np.inf
        flat[where[20:40]] = -0.0
    elif kind == "nan00":
        x.reshape(-1)[rng.choice(n, n // 50, replace=False)] = np.nan
        x[0, 0] = np.nan
    elif kind == "neginf":
        x[:] = -np.inf
    x.setflags(write=False)
    return x


def c_argmax(tp, emb, rows, stride, cols):
    found, best, value = C.c_int(0), _ffi.Coords(), C.c_float(0)
    _ffi.check(tp._L.lm_hip_argmax_f32_dptr(tp._h, C.c_void_p(emb.ptr), rows, stride, cols, C.byref(found), C.byref(best),
                                            C.byref(value)))
    return ((best.row, best.col), np.float32(value.value)) if found.value else None


def c_max(tp, emb, rows, stride, cols):
    found, value = C.c_int(0), C.c_float(0)
    _ffi.check(tp._L.lm_hip_max_f32_dptr(tp._h, C.c_void_p(emb.ptr), rows, stride, cols, C.byref(found), C.byref(value)))
    return np.float32(value.value) if found.value else None


@cases("reduce_f32")
def test_reductions_f32(tp, case):
    (cols, rows), offset, extra, kind = case
    x = reduce_values((cols, rows), kind)
    stride = cols + extra
    emb = embed(x, stride, 4 * offset, POISON_F32, device=DEV)    # +inf and NaN in the padding: reading it changes the answer
    torch.cuda.synchronize()
    tp.launch_tally()
    # Maximum::argmax / max with the first-cell rule (the oracle), and the shard form with the rule off
    where = co.argmax(x, cols)
    got = c_argmax(tp, emb, rows, stride, cols)
    assert got is not None and got[0] == where and bits([got[1]])[0] == bits([x[where]])[0], (got, where, x[where])
    assert bits([c_max(tp, emb, rows, stride, cols)])[0] == bits([co.max_(x, cols)])[0] == bits([x[where]])[0]
    on = tp.argmax_dptr(emb.ptr, rows, stride, cols, first_cell_rule=True)
    assert on[0] == where and bits([on[1]])[0] == bits([x[where]])[0]
    off = tp.argmax_dptr(emb.ptr, rows, stride, cols, first_cell_rule=False)
    where_off = last_maximum_without_first_cell_rule(x, cols)
    assert off[0] == where_off and bits([off[1]])[0] == bits([x[where_off]])[0], (off, where_off)
    assert (where_off != where) == (kind == "nan00")             # the two rules part exactly where the first cell is NaN
    # Threshold::threshold: a tied value, -0.0, -inf, above the maximum
    finite = x[np.isfinite(x)]
    tied = float(np.median(finite)) if finite.size else 0.0
    above = float(finite.max()) + 1.0 if finite.size and not np.isinf(x).any() else float("inf")
    for t in (tied, -0.0, float("-inf"), above):
        want = co.threshold(x, cols, t).astype(np.int64)
        if t == above and kind != "specials":
            assert len(want) == 0
        if t == float("-inf"):
            assert len(want) == x.size - np.isnan(x).sum()
        got = tp.threshold_dptr(emb.ptr, rows, stride, cols, t)
        assert differing(np.asarray(got).reshape(-1, 2), want) == 0, (t, len(got), len(want))
    tp.sync()
    assert tp.launch_tally() == {}                                 # no registry kernel has any business here
    untouched(emb, x)
    RAN["reduce_f32"] += 1


@cases("reduce_u8")
def test_reductions_u8(tp, case):
    (cols, rows), offset, extra, kind = case
    rng = np.random.default_rng(rows + extra)
    x = rng.integers(0, 7, (rows, cols)).astype(np.uint8)
    if kind == "top":
        x.reshape(-1)[rng.choice(x.size, x.size // 20, replace=False)] = 255
    stride = cols + extra
    emb = embed(x, stride, offset, 255, device=DEV)
    torch.cuda.synchronize()
    tp.launch_tally()
    r, c = np.argwhere(x == x.max())[-1]                           # pli/mod.rs:135-155: the last maximal cell
    assert tp.argmax_u8_dptr(emb.ptr, rows, stride, cols) == ((int(r), int(c)), int(x.max()))
    for t in sorted({0, 3, int(x.max()), min(int(x.max()) + 1, 255), 255}):
        got = tp.threshold_u8_dptr(emb.ptr, rows, stride, cols, t)
        assert differing(np.asarray(got).reshape(-1, 2), np.argwhere(x >= t)) == 0, t
    tp.sync()
    assert tp.launch_tally() == {}
    untouched(emb, x)
    RAN["reduce_u8"] += 1


# ---- 5. layout ----------------------------------------------------------------------------------------------------------

LETTERS = {"D": b"ACTGN", "P": b"ACDEFGHIKLMNPQRSTVWYX"}


def encode_call(tp, alphabet, src, length, lossy, dst):
    bad = C.c_size_t(2 ** 62)
    status = tp._L.lm_hip_encode_dptr(tp._h, alphabet.encode(), C.c_void_p(src.ptr), length, int(lossy), C.c_void_p(dst.ptr),
                                      C.byref(bad))
    return status, bad.value


def run_encode(tp, src_off, dst_off, length, alphabet, lossy, bad_at):
    rng = np.random.default_rng(length + 31 * src_off + dst_off)
    text = np.frombuffer(LETTERS[alphabet], np.uint8)[rng.integers(0, len(LETTERS[alphabet]), length)].copy()
    for i in bad_at:
        text[i] = ord("#") if i % 2 else ord("a")                  # Symbol::from_ascii knows upper case only
    src = embed(text.reshape(1, length), length, src_off, ord("Z"), device=DEV)
    dst = embed(np.full((1, length), CANARY_U8, np.uint8), length, dst_off, CANARY_U8, device=DEV)
    torch.cuda.synchronize()
    status, bad = encode_call(tp, alphabet, src, length, lossy, dst)
    got, problems = extract(dst)
    assert problems == [], problems                                   # nothing past the last byte, nothing before the first
    untouched(src, text.reshape(1, length))
    if bad_at and not lossy:
        assert status == _ffi.ERR_INVALID_SYMBOL and bad == min(bad_at), (status, bad, bad_at)   # pli/mod.rs:63: the FIRST
    else:
        assert status == _ffi.OK, _ffi.last_error()
        assert differing(got[0], co.encode(text.tobytes(), alphabet, lossy=bool(lossy))) == 0

@cases("encode")
def test_encode(tp, case):
    src_off, dst_off, length, alphabet, mode = case
    run_encode(tp, src_off, dst_off, length, alphabet, mode.startswith("lossy"), BAD_AT[length] if mode.endswith("bad") else ())
    RAN["encode"] += 1


@cases("encode_tail")
def test_encode_invalid_byte_in_the_tail(tp, case):
    src_off, dst_off, length, alphabet, at = case
    run_encode(tp, src_off, dst_off, length, alphabet, False, (at,))
    RAN["encode_tail"] += 1


@cases("stripe")
def test_stripe_and_configure_wrap(tp, case):
    cols, offset, stride_id, length, wrap_id, op = case
    natural = co.stride(cols, 1)
    stride = {"nat": natural, "+1": natural + 1, "+4": natural + 4, "64": 64}[stride_id]
    rows = -(-length // cols)
    wrap = {"none": 0, "19": 19, "big": rows + 3}[wrap_id]
    rng = np.random.default_rng(length + cols)
    enc = rng.integers(0, 5, length, dtype=np.uint8)
    ref = co.stripe(enc, cols, 5)
    co.configure_wrap(ref, wrap)
    assert ref.data.shape[0] == rows + wrap
    d_enc = torch.from_numpy(enc).to(DEV)
    data = embed(np.full((rows + wrap, cols), CANARY_U8, np.uint8), stride, offset, CANARY_U8, device=DEV)
    torch.cuda.synchronize()
    tp.launch_tally()
    if op == "stripe":
        tp.stripe_dptr(d_enc.data_ptr(), length, cols, 4, wrap, data.ptr, stride)
    else:
        tp.stripe_dptr(d_enc.data_ptr(), length, cols, 4, 0, data.ptr, stride)
        tp.sync()
        _, problems = extract(data, padding=4, padded_rows=(0, rows))
        assert problems == [], ("stripe wrote beyond its rows", problems)
        tp.configure_wrap_dptr(data.ptr, rows, stride, cols, wrap, 4)
    tp.sync()
    assert tp.launch_tally() == {}
    # the live bytes are the oracle's; every byte from `cols` to `stride - 1` of every written row is the default
    # symbol, as the header promises; nothing outside the rows is written
    got, problems = extract(data, padding=4)
    assert problems == [], problems
    assert differing(got, ref.data[:, :cols]) == 0
    RAN["stripe"] += 1


# ---- 6. adopted handles ----------------------------------------------------------------------------------------------

SPARE_ROWS = 60
BATCH = ("D20", "D20b", "D20c", "D13")     # three motifs of one length (the multi-motif pass) and one odd one


@functools.lru_cache(maxsize=None)
def batch_motif(label):
    if label in ("D20", "D13"):
        return weights(label), motif(label)
    p = weights("D20").copy()
    p[:, :4] = np.roll(p[:, :4], 1 + "bc".index(label[-1]), axis=1)
    return p, lm.ScoringMatrix(p)


def adopted_pair(tp, offset, stride):
    """The same sequence with 19 wrap rows twice: adopted at a foreign place, and in a handle the library owns."""
    enc, ref = sequence(5, 32)
    emb = embed_sequence(5, 32, 20, stride, offset, spare_rows=SPARE_ROWS)
    adopted = tp.adopt_sequence(emb.ptr, ROWS, 19, 32, stride, len(enc), keepalive=emb, capacity_rows=ROWS + 19 + SPARE_ROWS)
    owned = tp.upload(ref.data[: ROWS + 19], len(enc), 19, 32)
    assert (adopted.rows, adopted.wrap, adopted.stride, adopted.data_ptr) == (ROWS, 19, stride, emb.ptr)
    return emb, adopted, owned


@cases("adopted")
def test_adopted_sequence(tp, case):
    (offset, stride), group = case
    enc, ref = sequence(5, 32)
    length = len(enc)
    emb, adopted, owned = adopted_pair(tp, offset, stride)
    want, want_mi = oracle_scores("D20", 32)
    pssm = motif("D20")
    torch.cuda.synchronize()
    tp.launch_tally()
    grown = False
    checks, tally, kernel = Checks(), None, None
    with checks("results"):
        if group == "score_into":
            for seq in (adopted, owned):
                scores = lm.StripedScores.empty(tp, 32)
                tp.score_into(pssm, seq, scores)
                assert scores.max_index == want_mi
                assert differing(bits(scores.matrix()[:, :32]), bits(want[:, :32])) == 0, tp.last_kernel
                assert tp.argmax(scores) == co.argmax(want, 32)
                if seq is adopted:
                    tally, kernel = tp.launch_tally(), tp.last_kernel
        elif group == "batches":
            mats = [batch_motif(label) for label in BATCH]
            wants = [co.score_rows(ref, p)[0] for p, _ in mats]
            ts = [float(np.sort(w[:, :32].ravel())[-60]) for w in wants]
            for seq in (adopted, owned):
                hits = tp.scan_threshold_batch([m for _, m in mats], ts, seq)
                if seq is adopted:
                    tally, kernel = tp.launch_tally(), tp.last_kernel
                best = tp.scan_argmax_batch([m for _, m in mats], seq)
                for i, w in enumerate(wants):
                    where = co.threshold(w, 32, ts[i])
                    assert differing(np.asarray(hits[i][0]).reshape(-1, 2), where.astype(np.int64)) == 0, (i, tp.last_kernel)
                    assert differing(bits(hits[i][1]), bits(w[where[:, 0], where[:, 1]])) == 0
                    at = co.argmax(w, 32)
                    assert best[i][0] == at and bits([best[i][1]])[0] == bits([w[at]])[0]
                if seq is adopted:
                    tally.update(tp.launch_tally())
                    kernel = tp.last_kernel
        elif group == "scanner":
            t = float(np.sort(want[:, :32].ravel())[-80])
            by_pos = want[:, :32].T.reshape(-1)[: length - 19]
            at = np.nonzero(by_pos >= np.float32(t))[0]
            results = []
            for seq in (adopted, owned):
                scanner = lm.Scanner(pssm, seq, threshold=t)
                assert scanner.positions.tolist() == at.tolist()
                assert differing(bits(scanner.scores), bits(by_pos[at])) == 0
                tops = []
                for saturate in (True, False):                          # Scanner::max, both flavours of the u8 sums
                    hit = lm.Scanner(pssm, seq, threshold=t).max(saturate)
                    tops.append(None if hit is None else (hit.position, bits([hit.score])[0]))
                results.append(tops)
                if seq is adopted:
                    tally, kernel = tp.launch_tally(), tp.last_kernel
            # the reference's walk (scan.rs:200-249) on the host, over the downloaded matrices
            walked = [scanner_max_strict_host(lm.Scanner(pssm, owned, threshold=t), saturate) for saturate in (True, False)]
            assert results[0] == results[1] == [None if h is None else (h.position, bits([h.score])[0]) for h in walked]
            assert results[0][0] is not None
        elif group == "discrete":
            dm, want_wrap, want_sat = discrete(12)
            for seq in (adopted, owned):
                for saturate, w8 in ((True, want_sat), (False, want_wrap)):
                    got, mi = tp.score_discrete(dm, seq, saturate=saturate)
                    assert mi == length + 1 - 12 and np.array_equal(got[:, :32], w8), (saturate, tp.last_kernel)
                    part, _ = tp.score_discrete(dm, seq, rows=range(3, ROWS - 5), saturate=saturate)
                    assert differing(part[:, :32], w8[3: ROWS - 5]) == 0
                if seq is adopted:
                    tally, kernel = tp.launch_tally(), tp.last_kernel
        else:
            counts = np.bincount(enc, minlength=5)
            assert adopted.count_symbols().tolist() == owned.count_symbols().tolist() == counts.tolist()
            before = adopted.matrix()                                   # lm_hip_seq_download: (rows + wrap) x stride bytes
            assert before.shape == (ROWS + 19, stride) and np.array_equal(before[:, :32], ref.data[: ROWS + 19, :32])
            assert (before[:, 32:] == 3).all()                          # the caller's padding, as the caller left it
            adopted.configure_wrap(19 + SPARE_ROWS)                     # grows inside the capacity, in the caller's buffer
            owned.configure_wrap(19 + SPARE_ROWS)
            grown = True
            assert adopted.wrap == 19 + SPARE_ROWS and adopted.data_ptr == emb.ptr
            after = adopted.matrix()
            assert differing(after[:, :32], ref.data[: ROWS + 19 + SPARE_ROWS, :32]) == 0
            assert differing(after[:, :32], owned.matrix()[:, :32]) == 0
            with pytest.raises(_ffi.LightmotifHipError) as err:
                adopted.configure_wrap(20 + SPARE_ROWS)                 # one row more than the buffer has
            assert err.value.status == _ffi.ERR_CAPACITY
            long_want, _ = oracle_scores("D72", 32)                     # a motif that needs the new wrap rows
            scores = lm.StripedScores.empty(tp, 32)
            tp.score_into(motif("D72"), adopted, scores)
            assert differing(bits(scores.matrix()[:, :32]), bits(long_want[:, :32])) == 0, tp.last_kernel
            tally, kernel = tp.launch_tally(), tp.last_kernel
    if tally is None:        # a result check failed before the tally was read: what the adopted handle launched so far
        tally, kernel = tp.launch_tally(), tp.last_kernel
    print("adopted", case, kernel, sorted(tally))
    # the buffer around the matrix: configure_wrap writes every wrap row anew, padding included (the default symbol)
    with checks("results"):
        _, problems = extract(emb, padding=4, padded_rows=(ROWS, ROWS + 19 + SPARE_ROWS) if grown else (0, 0))
        assert problems == [], problems
    with checks("route"):
        check_route("adopted", tp, tally, seq_offset=offset, natural=stride == 32, control=(offset, stride) == (0, 32),
                    kernel=kernel)
    checks.done()
    RAN["adopted"] += 1


# ---- the count ------------------------------------------------------------------------------------------------------

CASE_TESTS = {"score_f32": "test_score_f32", "score_f32_other": "test_score_f32_other_columns",
              "score_handle": "test_score_rows_into_on_an_adopted_sequence", "fused": "test_fused",
              "fused_nan": "test_fused_with_a_nan_first_cell", "score_u8": "test_score_u8", "reduce_f32": "test_reductions_f32",
              "reduce_u8": "test_reductions_u8", "encode": "test_encode", "encode_tail": "test_encode_invalid_byte_in_the_tail",
              "stripe": "test_stripe_and_configure_wrap", "adopted": "test_adopted_sequence"}


def test_every_case_ran(request):
    """No case is skipped: every collected case of this module reached its last assertion (a failed case is missing
    here too), and the tables hold the numbers of cases they are documented to hold."""
    for name, (table, _, _) in TABLES.items():
        assert len(table) == EXPECTED_CASES[name], name
    assert 150 <= sum(EXPECTED_CASES.values()) <= 250
    for (table, kind), kernels in sorted(SEEN.items()):
        print(f"{table:16s} {kind:8s} " + ", ".join(f"{k} x{n}" for k, n in sorted(kernels.items())))
    selected = collections.Counter()
    for item in request.session.items:
        if item.module is request.module and hasattr(item, "callspec"):
            for name, (table, _, _) in TABLES.items():
                if item.callspec.params.get("case") in table and item.function.__name__ == CASE_TESTS[name]:
                    selected[name] += 1
    assert dict(RAN) == dict(selected), (dict(RAN), dict(selected))
    if sum(selected.values()) == sum(EXPECTED_CASES.values()):      # the module ran whole
        assert dict(RAN) == EXPECTED_CASES
