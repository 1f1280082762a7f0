"""The rows the build promises (CPU tier): ``Pipeline.registry_rows()`` reads every non-null cell of the kernel registry
(csrc/score_plan.hip) and of the best-hit table (csrc/seqset_best.hip) out of the tables themselves; here the same set is
derived independently, from the four length limits of csrc/score_kernels.hpp and the rules of the instantiation units
restated in Python.  A row that disappears from the build -- a unit not compiled, an ``if constexpr`` that turns false, a
table entry overwritten -- fails here without a GPU.  What each row computes is tests/test_gpu_registry_sweep.py's part."""
import re
from collections import Counter
from pathlib import Path

import lightmotif_amd as lm

CSRC = Path(__file__).resolve().parent.parent / "lightmotif_amd" / "csrc"
SLOTS = ("STORE", "ARGMAX", "THRESHOLD", "STORE_QL", "STORE_ARGMAX", "CONTINUE", "STORE_C16", "STORE_TRACK")


def limit(name):
    """``constexpr int <name> = <value>;`` of score_kernels.hpp."""
    return int(re.search(rf"constexpr int {name} = (\d+);", (CSRC / "score_kernels.hpp").read_text()).group(1))


FAST, LONG, STORE, PAIR = (limit(n) for n in ("kMaxFastM", "kMaxLongM", "kMaxStoreM", "kMaxPairM"))


def prefilter2_multi(m):
    """score_prefilter2.hpp: motifs per pass of the multi-motif pair scan, from the pairs of a group ((m | 3) + 1) / 2."""
    npair = ((m | 3) + 1) // 2
    return 4 if npair <= 8 else 2 if npair <= 16 else 1


def expected_rows():
    rows = set()
    for m in range(1, FAST + 1):                        # score_inst.hip: every length, both alphabet widths
        for wide in (0, 1):
            slots = ["STORE", "ARGMAX", "THRESHOLD", "STORE_ARGMAX", "CONTINUE"]
            if m % 4 == 0:
                slots += ["STORE_QL", "STORE_C16", "STORE_TRACK"]
            rows |= {("c32", wide, m, s) for s in slots}
            rows |= {("pre", wide, m, ""), ("u8", wide, m, "")}
        rows |= {("preblk", 1, m, ""), ("best_fused", 0, m, "")}
        if m >= 2:
            rows |= {("pre2", 0, m, ""), ("pre2_protein", 1, m, ""), ("u8_pairs", 0, m, "")}
            if prefilter2_multi(m) > 1:
                rows.add(("pre2_multi", 0, m, ""))
    for m in range(FAST + 1, LONG + 1):                 # score_long_inst.hip: padded lengths, dword loads only
        if m % 4 == 0:
            for wide in (0, 1):
                rows |= {("c32", wide, m, s) for s in ("STORE", "STORE_QL", "ARGMAX", "THRESHOLD", "STORE_ARGMAX", "CONTINUE",
                                                       "STORE_TRACK")}
    for m in range(LONG + 1, STORE + 1):                # score_xlong_inst.hip: the plain store alone
        if m % 8 == 0:
            for wide in (0, 1):
                rows |= {("c32", wide, m, "STORE"), ("c32", wide, m, "STORE_QL")}
    rows |= {("pre2", 0, m, "") for m in range(FAST + 1, PAIR + 1)}   # score_long_inst.hip and score_pair_inst.hip
    return rows


def test_limits_are_the_documented_ones():
    assert (FAST, LONG, STORE, PAIR) == (36, 64, 88, 128)
    assert lm._ffi.SLOTS == SLOTS                       # the binding's slot names, in the order of SLOT_* (score_kernels.hpp)
    enum = re.search(r"enum : int \{ SLOT_STORE = MODE_STORE,(.*?)kRegistrySlots \}", (CSRC / "score_kernels.hpp").read_text(), re.S)
    assert ["STORE"] + re.findall(r"SLOT_([A-Z0-9_]+)", enum.group(1)) == list(SLOTS)


def test_promised_rows_are_the_rows_the_rules_give():
    got = lm.Pipeline.registry_rows()
    want = expected_rows()
    assert set(got) - want == set(), sorted(set(got) - want)
    assert want - set(got) == set(), sorted(want - set(got))
    assert all(v != 0 for v in got.values())
    per_family = Counter(key[0] for key in got)
    assert per_family == {"c32": 5 * 36 * 2 + 3 * 9 * 2 + 7 * 7 * 2 + 2 * 3 * 2, "pre": 72, "preblk": 36, "pre2": 127,
                          "pre2_protein": 35, "pre2_multi": sum(prefilter2_multi(m) > 1 for m in range(2, 37)), "u8": 72,
                          "u8_pairs": 35, "best_fused": 36}
    assert len(got) == 967


def test_rows_that_share_a_kernel_are_the_long_stores_alone():
    """STORE and STORE_QL of the long and very long families are one function; every other row has a kernel of its own."""
    got = lm.Pipeline.registry_rows()
    by_id = {}
    for key, ident in got.items():
        by_id.setdefault(ident, []).append(key)
    shared = sorted(sorted(keys) for keys in by_id.values() if len(keys) > 1)
    want = sorted([("c32", wide, m, "STORE"), ("c32", wide, m, "STORE_QL")]
                  for wide in (0, 1) for m in list(range(40, 65, 4)) + [72, 80, 88])
    assert shared == want
    assert len(by_id) == len(got) - len(want)


def test_needs_no_device_and_the_tally_needs_a_context():
    import ctypes as C
    from lightmotif_amd import _ffi
    L = _ffi.lib()
    n = C.c_size_t(0)
    assert L.lm_hip_registry_rows(None, 0, C.byref(n)) == _ffi.OK and n.value == 967
    few = (_ffi.RegistryRow * 3)()
    assert L.lm_hip_registry_rows(few, 3, C.byref(n)) == _ffi.OK and n.value == 967      # a short buffer: filled, not overrun
    assert [(_ffi.FAMILIES[r.family], r.wide, r.m, r.slot) for r in few] == [("c32", 0, 1, 0), ("c32", 0, 1, 1), ("c32", 0, 1, 2)]
    assert L.lm_hip_registry_rows(None, 3, C.byref(n)) == _ffi.ERR_BAD_ARGS
    assert L.lm_hip_ctx_launch_tally(None, None, 0, C.byref(n)) == _ffi.ERR_BAD_ARGS
