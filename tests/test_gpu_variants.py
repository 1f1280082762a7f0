"""Single-symbol variants of a resident set against all motifs: ``Pipeline.scan_variants_set`` / ``scan_variant_hits_set``
(``lm_hip_seqset_variant_effects`` / ``lm_hip_seqset_variant_hits``, csrc/variants.hip) against tests/variant_reference.py,
which tests/test_variant_reference.py pins on the CPU.  Every comparison is exact: scores as uint32 views where a window
was found and with ``isnan`` where none, ``back``, ``ref_symbol`` and ``valid`` as they are.  The options ``variant_chunk``
and ``variant_lds_bytes`` make small calls cross chunk boundaries and take the kernel that reads global memory."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import lightmotif_amd as lm
from lightmotif_amd import _ffi
from lightmotif_amd.lib import VARIANT_DTYPE, VARIANT_EFFECT_DTYPE

import seqset_reference as sr
import variant_reference as vr
from variant_reference import small_case, variants_of

pytestmark = pytest.mark.gpu

SEEDS = range(0, 40)


@contextlib.contextmanager
def options(pli, **values):
    for name, value in values.items():
        pli.set_option(name, value)
    try:
        yield
    finally:
        for name in values:
            pli.set_option(name, 0)


def make_set(pli, symbols, protein=False, cols=32):
    return pli.stripe_set([lm.EncodedSequence(np.asarray(s, dtype=np.uint8), protein=protein) for s in symbols], columns=cols,
                          protein=protein)


def random_variants(case, count, seed):
    rng = np.random.default_rng(seed)
    n = len(case.lengths)
    record = rng.integers(0, n, count)
    position = (rng.random(count) * case.lengths[record]).astype(np.int64)
    return variants_of(case, record, position, rng.integers(0, case.k, count))


def assert_scores(got, want, what):
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    assert got.shape == want.shape, what
    none = np.isnan(want)
    assert np.array_equal(np.isnan(got), none), what
    assert np.array_equal(got.view(np.uint32)[~none], want.view(np.uint32)[~none]), what


def assert_dense(res, case, variants, effects, what):
    assert res.shape == (len(case.mats), len(variants)), what
    assert_scores(res.ref_score, effects.ref_score, (what, "ref_score"))
    assert_scores(res.alt_score, effects.alt_score, (what, "alt_score"))
    assert np.array_equal(res.raw["ref_back"].astype(np.int64), effects.ref_back), (what, "ref_back")
    assert np.array_equal(res.raw["alt_back"].astype(np.int64), effects.alt_back), (what, "alt_back")
    assert np.array_equal(res.ref_position, effects.position(variants, "ref")), (what, "ref_position")
    assert np.array_equal(res.alt_position, effects.position(variants, "alt")), (what, "alt_position")
    assert np.array_equal(res.ref_symbol, effects.ref_symbol), (what, "ref_symbol")
    assert np.array_equal(res.valid, effects.valid), (what, "valid")


def pooled_threshold(kind, effects, i):
    return sr.threshold_of(kind, np.concatenate([effects.ref_score[i], effects.alt_score[i]]))


def assert_hits(hits, case, variants, effects, thresholds, what):
    assert len(hits) == len(case.mats), what
    ref_pos, alt_pos = effects.position(variants, "ref"), effects.position(variants, "alt")
    for i, t in enumerate(thresholds):
        keep = vr.kept(effects, i, t)
        got = hits[i]
        assert int(hits.counts[i]) == len(keep) == len(got), (what, i, t)
        assert np.array_equal(got["variant"], keep), (what, i, t)
        assert_scores(got["ref_score"], effects.ref_score[i, keep], (what, i, t))
        assert_scores(got["alt_score"], effects.alt_score[i, keep], (what, i, t))
        assert np.array_equal(got["ref_position"], ref_pos[i, keep]) and np.array_equal(got["alt_position"], alt_pos[i, keep]), (what, i, t)
    assert hits.total == int(hits.counts.sum())
    assert np.array_equal(hits.ref_symbol, effects.ref_symbol) and np.array_equal(hits.valid, effects.valid), what


def run_both(pli, case, variants, effects, what, cols=32, kinds=None, seqset=None):
    """The dense call and the hits call of one case against the reference; -> (seqset, pssms, dense result)."""
    seqset = seqset or make_set(pli, case.symbols, case.protein, cols)
    pssms = [lm.ScoringMatrix(p, protein=case.protein) for p in case.mats]
    res = pli.scan_variants_set(pssms, seqset, variants.record, variants.position, variants.alt)
    assert_dense(res, case, variants, effects, what)
    kinds = kinds or [sr.THRESHOLD_KINDS[i % len(sr.THRESHOLD_KINDS)] for i in range(len(pssms))]
    thresholds = [pooled_threshold(kind, effects, i) for i, kind in enumerate(kinds)]
    hits = pli.scan_variant_hits_set(pssms, thresholds, seqset, variants.record, variants.position, variants.alt)
    assert_hits(hits, case, variants, effects, thresholds, what)
    return seqset, pssms, res


# ---- the seeded cases ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", SEEDS)
def test_random_set(pli, seed):
    """cols 1 / 3 / 16 / 33 / 32, protein, M = 1 ... 130, 4 097 records, records of 0 / 1 / 2 symbols, neighbourhoods across
    record and column boundaries; every threshold kind over the seeds; the same bytes again behind configure_wrap."""
    case, variants, effects = vr.case_of(seed)
    kinds = [sr.THRESHOLD_KINDS[(seed + i) % len(sr.THRESHOLD_KINDS)] for i in range(len(case.mats))]
    seqset, pssms, res = run_both(pli, case, variants, effects, seed, cols=case.cols, kinds=kinds)
    seqset.configure_wrap(case.wrap + 1)
    again = pli.scan_variants_set(pssms, seqset, variants.record, variants.position, variants.alt)
    assert res.raw.tobytes() == again.raw.tobytes() and np.array_equal(res.ref_symbol, again.ref_symbol)


# ---- hand-made cases ---------------------------------------------------------------------------------------------------

def dna_matrix(rng, m, kind="normal"):
    return sr.make_matrix(rng, m, 5, kind)


def dna_records(rng, lengths):
    return [rng.integers(0, 5, n).astype(np.uint8) for n in lengths]


def test_one_row_motifs_and_single_windows(pli):
    """M = 1; L = M (one window); L = 2M - 1 with p = M - 1 (all M windows)."""
    rng = np.random.default_rng(1)
    for m in (1, 2, 7, 36, 37):
        case = small_case([dna_matrix(rng, m, "ties"), dna_matrix(rng, 1)], dna_records(rng, [m, 2 * m - 1, 1, m + 1]))
        rec = np.concatenate([np.full(m, 0), np.full(2 * m - 1, 1), [2], np.arange(m + 1) * 0 + 3])
        pos = np.concatenate([np.arange(m), np.arange(2 * m - 1), [0], np.arange(m + 1)])
        variants = variants_of(case, rec, pos, rng.integers(0, 5, len(rec)))
        effects = vr.reference(case, variants)
        centre = m + (m - 1)
        assert effects.has_window[0, :centre + m].all() and (effects.ref_back[0, :m] == np.arange(m)).all()   # one window: back = p
        if m > 1:
            assert vr.windows_of(m - 1, 2 * m - 1, m) == (0, m - 1) and variants.position[centre] == m - 1
        _, _, res = run_both(pli, case, variants, effects, ("single", m))
        assert res.last_kernel == "variant_effects"


def test_neighbourhoods_across_columns(pli):
    """A 200-symbol set at cols = 32 has 7 rows: every neighbourhood of a 12-row motif crosses columns of the matrix."""
    rng = np.random.default_rng(2)
    case = small_case([dna_matrix(rng, 12), dna_matrix(rng, 5, "neg_inf_cells")], dna_records(rng, [90, 60, 50]))
    rec = np.repeat(np.arange(3), [90, 60, 50])
    pos = np.concatenate([np.arange(90), np.arange(60), np.arange(50)])
    variants = variants_of(case, rec, pos, rng.integers(0, 5, 200))
    seqset, _, _ = run_both(pli, case, variants, vr.reference(case, variants), "columns")
    assert seqset.rows == 7


@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, 257])
def test_variant_counts(pli, count):
    rng = np.random.default_rng(3)
    case = small_case([dna_matrix(rng, 9), dna_matrix(rng, 20, "ties")], dna_records(rng, [40, 0, 25, 300]))
    variants = random_variants(case, count, 30 + count)
    _, _, res = run_both(pli, case, variants, vr.reference(case, variants), ("count", count))
    assert res.last_kernel == ("variant_effects" if count else "")


def test_seventy_motifs_cross_a_group(pli):
    rng = np.random.default_rng(4)
    mats = [dna_matrix(rng, int(m), "ties" if i % 3 == 0 else "normal") for i, m in enumerate(rng.integers(1, 25, 70))]
    case = small_case(mats, dna_records(rng, [64, 3, 150]))
    variants = random_variants(case, 130, 41)
    run_both(pli, case, variants, vr.reference(case, variants), "groups")


@pytest.mark.parametrize("chunk", [1, 7])
def test_chunks_of_variants(pli, chunk):
    """Chunk boundaries inside the list; duplicates and unsorted input stay in caller order."""
    rng = np.random.default_rng(5)
    case = small_case([dna_matrix(rng, 6), dna_matrix(rng, 40), dna_matrix(rng, 3, "ties")], dna_records(rng, [50, 41, 7]))
    base = random_variants(case, 23, 51)
    order = rng.permutation(np.concatenate([np.arange(23), np.arange(0, 23, 2)]))
    variants = base.take(order)
    effects = vr.reference(case, variants)
    whole = pli.scan_variants_set([lm.ScoringMatrix(p) for p in case.mats], make_set(pli, case.symbols), variants.record,
                                  variants.position, variants.alt)
    with options(pli, variant_chunk=chunk):
        _, _, res = run_both(pli, case, variants, effects, ("chunk", chunk), kinds=["median", "-inf", "q99"])
    assert res.raw.tobytes() == whole.raw.tobytes()
    for a, b in zip(np.flatnonzero(order == 4), np.flatnonzero(order == 4)[1:]):       # a duplicate: the same cells twice
        assert res.raw[:, a].tobytes() == res.raw[:, b].tobytes()


def test_tables_from_global_memory(pli):
    """One motif whose table exceeds the LDS budget: ``variant_effects_global``; the same bytes as from LDS."""
    rng = np.random.default_rng(6)
    case = small_case([dna_matrix(rng, 4), dna_matrix(rng, 30), dna_matrix(rng, 5, "ties")], dna_records(rng, [70, 33, 30]))
    variants = random_variants(case, 100, 61)
    effects = vr.reference(case, variants)
    _, _, lds = run_both(pli, case, variants, effects, "lds")
    assert lds.last_kernel == "variant_effects"
    with options(pli, variant_lds_bytes=256):                # 31 * 5 floats = 620 bytes: the 30-row motif alone leaves LDS
        _, _, mixed = run_both(pli, case, variants, effects, "mixed")
    assert mixed.last_kernel == "variant_effects_global" and mixed.raw.tobytes() == lds.raw.tobytes()
    with options(pli, variant_lds_bytes=16):                 # every motif
        _, _, glob = run_both(pli, case, variants, effects, "global")
    assert glob.last_kernel == "variant_effects_global" and glob.raw.tobytes() == lds.raw.tobytes()


def test_neighbourhoods_beyond_lds(pli):
    """A 300-row motif: 599 bytes per lane are read from the scratch block, not from LDS; with a protein alphabet too."""
    rng = np.random.default_rng(7)
    for protein in (False, True):
        k = 21 if protein else 5
        mats = [sr.make_matrix(rng, 300, k, "normal"), sr.make_matrix(rng, 130, k, "ties"), sr.make_matrix(rng, 2, k, "normal")]
        records = [rng.integers(0, k, n).astype(np.uint8) for n in (700, 299, 300, 140)]
        case = small_case(mats, records, protein)
        variants = random_variants(case, 90, 71)
        effects = vr.reference(case, variants)
        assert effects.has_window[0].any() and not effects.has_window[0].all()
        run_both(pli, case, variants, effects, ("long", protein))
        with options(pli, variant_lds_bytes=16):
            run_both(pli, case, variants, effects, ("long global", protein))


def test_motifs_without_a_window_anywhere(pli):
    """A motif longer than every record never reaches the device: none everywhere, the resident symbols all the same."""
    rng = np.random.default_rng(8)
    case = small_case([dna_matrix(rng, 50), dna_matrix(rng, 8), dna_matrix(rng, 41)], dna_records(rng, [40, 12]))
    variants = random_variants(case, 30, 81)
    effects = vr.reference(case, variants)
    assert not effects.has_window[0].any() and not effects.has_window[2].any() and effects.has_window[1].any()
    run_both(pli, case, variants, effects, "dead")
    alone = small_case([case.mats[0]], case.symbols)
    _, _, res = run_both(pli, alone, variants, vr.reference(alone, variants), "all dead")
    assert res.last_kernel == "variant_gather"


def test_calls_repeat_byte_for_byte(pli):
    case, variants, effects = vr.case_of(9)
    seqset = make_set(pli, case.symbols, case.protein, case.cols)
    pssms = [lm.ScoringMatrix(p, protein=case.protein) for p in case.mats]
    thresholds = [pooled_threshold("median", effects, i) for i in range(len(pssms))]
    args = (seqset, variants.record, variants.position, variants.alt)
    dense = [pli.scan_variants_set(pssms, *args).raw.tobytes() for _ in range(2)]
    sparse = [pli.scan_variant_hits_set(pssms, thresholds, *args) for _ in range(2)]
    assert dense[0] == dense[1]
    assert sparse[0].hits.tobytes() == sparse[1].hits.tobytes() and np.array_equal(sparse[0].counts, sparse[1].counts)
    seqset.configure_wrap(140)
    assert pli.scan_variants_set(pssms, *args).raw.tobytes() == dense[0]
    assert pli.scan_variant_hits_set(pssms, thresholds, *args).hits.tobytes() == sparse[0].hits.tobytes()


def test_letters_and_batches(pli):
    """``alts`` as letters go through the strict table; a prepared batch brings its thresholds."""
    rng = np.random.default_rng(10)
    case = small_case([dna_matrix(rng, 8)], dna_records(rng, [30, 20]))
    seqset = make_set(pli, case.symbols)
    pssms = [lm.ScoringMatrix(case.mats[0])]
    rec, pos = [0, 1, 1, 0], [3, 0, 19, 29]
    by_index = pli.scan_variants_set(pssms, seqset, rec, pos, [0, 3, 4, 2])
    for letters in ("AGNT", b"AGNT"):
        assert pli.scan_variants_set(pssms, seqset, rec, pos, letters).raw.tobytes() == by_index.raw.tobytes()
    with pytest.raises(lm.InvalidSymbol):
        pli.scan_variants_set(pssms, seqset, rec, pos, "AGnT")
    with pytest.raises(ValueError):
        pli.scan_variants_set(pssms, seqset, rec, pos[:3], "AGNT")
    batch = pli.prepare_batch(pssms, [-np.inf])
    hits = pli.scan_variant_hits_set(batch, None, seqset, rec, pos, "AGNT")
    assert hits.total == 4 and np.array_equal(hits[0]["variant"], np.arange(4))
    with pytest.raises(ValueError):
        pli.scan_variant_hits_set(pssms, None, seqset, rec, pos, "AGNT")
    with pytest.raises(ValueError):                          # a protein matrix against a DNA set
        pli.scan_variants_set([lm.ScoringMatrix(sr.make_matrix(rng, 4, 21, "normal"), protein=True)], seqset, rec, pos, "AGNT")
    empty = pli.scan_variants_set([], seqset, rec, pos, "AGNT")
    assert empty.shape == (0, 4) and np.array_equal(empty.ref_symbol, [case.symbols[r][p] for r, p in zip(rec, pos)])


# ---- statuses ----------------------------------------------------------------------------------------------------------

def test_statuses(pli):
    L = _ffi.lib()
    rng = np.random.default_rng(11)
    case = small_case([dna_matrix(rng, 8), dna_matrix(rng, 3)], dna_records(rng, [30, 20]))
    seqset = make_set(pli, case.symbols)
    batch = pli.prepare_batch([lm.ScoringMatrix(p) for p in case.mats], [0.0, 0.0])
    protein = pli.prepare_batch([lm.ScoringMatrix(sr.make_matrix(rng, 4, 21, "normal"), protein=True)], [0.0])
    v = np.zeros(3, dtype=VARIANT_DTYPE)
    v["position"] = [1, 2, 3]
    out = np.zeros((2, 3), dtype=VARIANT_EFFECT_DTYPE)
    ref = np.zeros(3, dtype=np.uint8)
    counts = np.full(2, 99, dtype=np.uintp)
    ptr = C.c_void_p(1)

    def dense(ctx=pli._h, handles=batch.handles, n=2, s=seqset._h, variants=v.ctypes.data, nv=3, effects=out.ctypes.data, symbols=ref.ctypes.data):
        return L.lm_hip_seqset_variant_effects(ctx, handles, n, s, variants, nv, effects, symbols)

    def sparse(ctx=pli._h, handles=batch.handles, ts=batch.thresholds, n=2, s=seqset._h, variants=v.ctypes.data, nv=3,
               cnt=counts.ctypes.data, hits=C.byref(ptr), symbols=ref.ctypes.data):
        return L.lm_hip_seqset_variant_hits(ctx, handles, ts, n, s, variants, nv, cnt, hits, symbols)

    def refused(status, want=_ffi.ERR_BAD_ARGS):
        assert status == want and _ffi.last_error()

    assert dense() == _ffi.OK and dense(symbols=None) == _ffi.OK
    refused(dense(ctx=None))
    refused(dense(s=None))
    refused(dense(ctx=None, n=0, nv=0))
    refused(dense(s=None, n=0, nv=0))
    refused(dense(handles=None))
    refused(dense(effects=None))
    refused(dense(variants=None))
    refused(dense(handles=protein.handles, n=1))
    assert dense(variants=None, nv=0) == _ffi.OK
    assert dense(handles=None, n=0, effects=None) == _ffi.OK
    refused(sparse(ctx=None))
    refused(sparse(s=None, n=0, nv=0))
    refused(sparse(handles=None))
    refused(sparse(ts=None))
    refused(sparse(cnt=None))
    refused(sparse(hits=None))
    refused(sparse(variants=None))
    refused(sparse(handles=protein.handles, ts=protein.thresholds, n=1))
    assert sparse(variants=None, nv=0) == _ffi.OK                      # nothing launched: counts zeroed, no list
    assert counts.tolist() == [0, 0] and ptr.value is None
    ptr.value = 1
    assert sparse(handles=None, ts=None, n=0, cnt=None) == _ffi.OK and ptr.value is None
    for bad in (-1, 2.0 ** 33, float("nan")):
        with pytest.raises(lm.LightmotifHipError):
            pli.set_option("variant_chunk", bad)
    for bad in (-1, 24577, float("nan")):
        with pytest.raises(lm.LightmotifHipError):
            pli.set_option("variant_lds_bytes", bad)
