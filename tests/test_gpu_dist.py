"""Score distributions on the device (csrc/dist.hip: lm_hip_dists_*, Pipeline.score_distributions) against the host code
they stand in for, lightmotif_amd/dist.py (pwm/dist.rs:129-225): survival functions, parameters, thresholds and p-values
are compared on their f64 / f32 BITS (np.array_equal), never within a tolerance."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

import lightmotif_amd as lm
from lightmotif_amd import _ffi, scan_cli
from lightmotif_amd import dist as lmdist
from lightmotif_amd.lib import SET_HIT_DTYPE, BatchHits, SetHits

pytestmark = pytest.mark.gpu

JASPAR = Path(__file__).parent / "golden" / "JASPAR2024.pwm.gz"
NINF = -np.inf


@pytest.fixture(scope="module")
def jaspar():
    return list(lm.io.read(JASPAR))


def ma0045():
    """dist.rs:246-270, the matrix of tests/test_io_dist.py"""
    return lm.CountMatrix({
        "A": [3, 7, 9, 3, 11, 11, 11, 3, 4, 3, 8, 8, 9, 9, 11, 2],
        "C": [5, 0, 1, 6, 0, 0, 0, 3, 1, 4, 5, 1, 0, 5, 0, 7],
        "T": [2, 4, 3, 1, 0, 1, 1, 6, 1, 1, 0, 1, 3, 0, 0, 5],
        "G": [4, 3, 1, 4, 3, 2, 2, 2, 8, 6, 1, 4, 2, 0, 3, 0],
    }).normalize(pseudocount=0.25).log_odds()


def dna(rng, m, lo=-6.0, hi=2.0, background=None):
    w = rng.uniform(lo, hi, (m, 5)).astype(np.float32)
    w[:, 4] = NINF
    return lm.ScoringMatrix(w, background)


def crafted():
    rng = np.random.default_rng(2024)
    out = {}
    out["m1"] = lm.ScoringMatrix(np.array([[-1.5, 0.25, 1.0, 2.0, NINF]], np.float32))      # uniform background: sf steps of 1/4
    out["m2"] = dna(rng, 2)
    out["all_equal"] = lm.ScoringMatrix(np.full((3, 5), 1.25, np.float32))                   # small = large - 1
    hole = dna(rng, 3).data[:, :5].copy()
    hole[1, :] = NINF
    out["row_of_ninf"] = lm.ScoringMatrix(hole)                                             # an all-zero table
    out["zero_background"] = dna(rng, 6, background=np.array([0.5, 0.0, 0.3, 0.2, 0.0], np.float32))
    w = rng.uniform(-7.0, 2.5, (5, 5)).astype(np.float32)
    w[0, 0], w[3, 2], w[:, 4] = -7.3, 2.9, NINF                                             # offset -8, scale floor(1000 / 10.9) = 91
    out["negative_offset"] = lm.ScoringMatrix(w)
    bg = rng.uniform(0.01, 1.0, 21)
    bg[20] = 0.0
    pw = rng.uniform(-5.0, 3.0, (12, 21)).astype(np.float32)
    pw[:, 20] = NINF
    pw[4, 7] = pw[9, 0] = NINF
    out["protein12"] = lm.ScoringMatrix(pw, (bg / bg.sum()).astype(np.float32), protein=True)
    for m in (36, 37, 64):
        out[f"dna{m}"] = dna(rng, m)
    return out


class Batch:
    """One mixed batch (DNA and protein together), its device distributions and the host oracle of every motif, made once."""

    def __init__(self, pli, jaspar):
        named = {"ma0045": ma0045()}
        for i in range(0, len(jaspar), 97):
            named[f"jaspar{i}_pc0.1"] = jaspar[i].matrix.normalize(0.1).log_odds()
            named[f"jaspar{i}_pc0"] = jaspar[i].matrix.normalize(0.0).log_odds()              # -inf weights
        named.update(crafted())
        self.names, self.pssms = list(named), list(named.values())
        self.oracle = [lmdist.ScoreDistribution(p) for p in self.pssms]
        self.dists = pli.score_distributions(self.pssms)

    def index(self, name):
        return self.names.index(name)


@pytest.fixture(scope="module")
def batch(pli, jaspar):
    return Batch(pli, jaspar)


def test_tables_equal_the_host_code_bit_for_bit(batch):
    d = batch.dists
    assert len(d) == len(batch.pssms) == 1 + 2 * 25 + 10
    assert {p.protein for p in batch.pssms} == {False, True}
    for i, (name, o) in enumerate(zip(batch.names, batch.oracle)):
        assert d.rows[i] == len(batch.pssms[i]), name
        assert d.scale[i] == o._scale and d.offset[i] == o._offset, name
        assert (d.min_score[i], d.max_score[i]) == (o.min_score, o.max_score), name
        sf = d.sf(i)
        assert sf.dtype == np.float64 and np.array_equal(sf, o.sf), name
    # what the crafted cases are there for
    i = batch.index("all_equal")
    assert d.max_score[i] == 3000 and d.min_score[i] == 0 and d.sf(i)[3000] == 1.0
    i = batch.index("row_of_ninf")
    assert not d.sf(i).any() and d.min_score[i] == d.max_score[i] == 0
    i = batch.index("negative_offset")
    assert d.offset[i] == -8 and d.scale[i] == 91
    assert any(np.isneginf(batch.pssms[batch.index(n)].data[:, :4]).any() for n in batch.names if n.endswith("_pc0"))


def test_distribution_object_answers_like_the_host_one(batch):
    for name in ("ma0045", "protein12", "m1"):
        i = batch.index(name)
        got, want = batch.dists.distribution(i), batch.oracle[i]
        for s in (-3.0, 0.5, 8.7708, 12.6648, 1e9, -1e9):
            assert got.pvalue(s) == want.pvalue(s)
        for p in (1e-5, 3e-4, 0.5, 1.0, 0.0):
            assert got.score(p) == want.score(p)
        assert got.min_pvalue() == want.min_pvalue()


def test_thresholds(batch):
    d = batch.dists
    for p in (1e-5, 1e-3, 0.3, 1.0, 0.0, 1.5, -1.0, 1e-300):
        got = d.thresholds(p)
        assert got.dtype == np.float32 and got.shape == (len(d),)
        want = np.array([o.score(p) for o in batch.oracle], dtype=np.float32)
        assert np.array_equal(got, want), p
    # p-values that EQUAL table entries: which index of a run of equal values comes back is the probe sequence's choice
    i = batch.index("m1")
    assert sorted(set(batch.oracle[i].sf.tolist())) == [0.25, 0.5, 0.75, 1.0]
    for p in (0.25, 0.5):
        assert d.thresholds(p)[i] == np.float32(batch.oracle[i].score(p))
    for pick in (lambda o: o.min_score, lambda o: o.max_score, lambda o: (o.min_score + o.max_score) // 2,
                 lambda o: len(o.sf) // 3, lambda o: 0, lambda o: len(o.sf) - 1, lambda o: max(o.max_score - 7, 0)):
        ps = np.array([o.sf[pick(o)] for o in batch.oracle])
        want = np.array([o.score(float(p)) for o, p in zip(batch.oracle, ps)], dtype=np.float32)
        assert np.array_equal(d.thresholds(ps), want)


def neighbours(x):
    x = np.float32(x)
    return [np.nextafter(x, np.float32(-np.inf)), x, np.nextafter(x, np.float32(np.inf))]


def expected_pvalue(o, s):
    """dist.py for finite scores; for the others the rule of dist.rs:77-101 with Rust's `as i32` (dist.py's int() raises there)"""
    s = np.float32(s)
    if np.isfinite(s):
        return o.pvalue(float(s))
    if np.isnan(s):
        return 1.0 if o.min_score > 0 else float(o.sf[0])
    return 0.0 if s > 0 else 1.0


def scores_for(rng, o):
    lo, hi = o.unscale(0), o.unscale(len(o.sf) - 1)
    out = rng.uniform(lo - 2.0, hi + 2.0, 40).astype(np.float32).tolist()
    mid = (o.min_score + o.max_score) // 2
    for j in {o.min_score - 1, o.min_score, o.min_score + 1, mid, mid + 1, o.max_score - 1, o.max_score, o.max_score + 1,
              0, 1, len(o.sf) - 2, len(o.sf) - 1, len(o.sf)}:
        if j >= 0:
            out += neighbours(o.unscale(j))
    out += [-1e6, 1e6, -3e38, 3e38, np.inf, -np.inf, np.nan]
    return np.array(out, dtype=np.float32)


def test_pvalues(batch):
    rng = np.random.default_rng(7)
    d = batch.dists
    per = [scores_for(rng, o) for o in batch.oracle]
    for i in (0, 5, 6, len(per) - 1):                                      # counts with zeros, at the ends and in the middle
        per[i] = np.zeros(0, np.float32)
    counts = np.array([len(s) for s in per])
    flat = np.concatenate(per)
    want = np.array([expected_pvalue(o, s) for o, ss in zip(batch.oracle, per) for s in ss], dtype=np.float64)
    assert {0.0, 1.0} <= set(want.tolist()) and ((want > 0) & (want < 1)).sum() > 1000

    got = d.pvalues(counts, flat)                                          # a plain f32 array: stride 4
    assert got.dtype == np.float64 and np.array_equal(got, want)
    hits = np.zeros(flat.size, dtype=SET_HIT_DTYPE)                        # the score column of lm_hip_set_hit
    hits["score"] = flat
    assert hits["score"].strides == (C.sizeof(_ffi.SetHit),)
    assert np.array_equal(d.pvalues(SetHits(hits, counts.astype(np.uintp))), want)
    assert np.array_equal(d.pvalues(BatchHits(np.zeros((flat.size, 2), np.int64), flat, counts.astype(np.uintp))), want)
    assert d.pvalues(np.zeros(len(d), np.uintp), np.zeros(0, np.float32)).shape == (0,)
    with pytest.raises(ValueError):
        d.pvalues(counts, flat[:-1])


def test_whole_jaspar_batch_and_repeatability(pli, jaspar):
    pssms = [r.matrix.normalize(0.1).log_odds() for r in jaspar]
    assert len(pssms) == 2346
    a = pli.score_distributions(pssms)
    ta = a.thresholds(1e-5)
    want = np.array([p.score_for_pvalue(1e-5) for p in pssms], dtype=np.float32)
    assert np.array_equal(ta, want)
    assert pli.last_kernel == "dist_scores"
    b = pli.score_distributions(pli.prepare_batch(pssms))                  # a MotifBatch is taken as well
    assert np.array_equal(b.thresholds(1e-5).view(np.uint32), ta.view(np.uint32))
    for name in ("scale", "offset", "min_score", "max_score", "rows"):
        assert np.array_equal(getattr(a, name), getattr(b, name))
    rng = np.random.default_rng(3)
    counts = rng.integers(0, 40, len(pssms))
    scores = rng.uniform(-20, 20, int(counts.sum())).astype(np.float32)
    pa = a.pvalues(counts, scores)
    assert pa.tobytes() == b.pvalues(counts, scores).tobytes()
    for i in range(0, len(pssms), 199):
        sf = a.sf(i)
        assert sf.tobytes() == b.sf(i).tobytes()
        assert np.array_equal(sf, pssms[i].score_distribution.sf)
    starts = np.concatenate(([0], np.cumsum(counts)))
    for i in range(0, len(pssms), 199):
        o = pssms[i].score_distribution
        assert pa[starts[i]:starts[i + 1]].tolist() == [o.pvalue(float(s)) for s in scores[starts[i]:starts[i + 1]]]


def test_misuse(pli, batch):
    L = _ffi.lib()
    ok = np.zeros((2, 5), np.float32)
    for bad in (np.nan, np.inf):
        w = ok.copy()
        w[1, 2] = bad
        with pytest.raises(lm.LightmotifHipError) as e:
            pli.score_distributions([batch.pssms[0], lm.ScoringMatrix(w)])
        assert e.value.status == _ffi.ERR_BAD_ARGS
    with pytest.raises(lm.LightmotifHipError) as e:
        pli.score_distributions([lm.ScoringMatrix(np.full((2, 5), NINF, np.float32))])
    assert e.value.status == _ffi.ERR_BAD_ARGS

    d = batch.dists
    n = len(d)
    assert L.lm_hip_dists_len(d._h) == n
    assert L.lm_hip_dists_info(d._h, n, None, None, None, None, None, None) == _ffi.ERR_BAD_ARGS
    assert L.lm_hip_dists_info(d._h, n - 1, None, None, None, None, None, None) == _ffi.OK
    sf_len = C.c_size_t(0)
    assert L.lm_hip_dists_info(d._h, 0, None, None, None, None, None, C.byref(sf_len)) == _ffi.OK
    assert sf_len.value == 1000 * len(batch.pssms[0]) + 1
    buf = np.zeros(sf_len.value, np.float64)
    assert L.lm_hip_dists_sf(pli._h, d._h, n, buf.ctypes.data, buf.size) == _ffi.ERR_BAD_ARGS
    assert L.lm_hip_dists_sf(pli._h, d._h, 0, buf.ctypes.data, buf.size - 1) == _ffi.ERR_CAPACITY
    assert L.lm_hip_dists_sf(pli._h, d._h, 0, buf.ctypes.data, buf.size) == _ffi.OK
    assert np.array_equal(buf, batch.oracle[0].sf)

    empty = pli.score_distributions([])                                    # n == 0: a valid, empty object
    assert len(empty) == 0 and L.lm_hip_dists_len(empty._h) == 0
    assert empty.thresholds(1e-5).shape == (0,) and empty.pvalues([], np.zeros(0, np.float32)).shape == (0,)
    h = C.c_void_p()
    assert L.lm_hip_dists_create(pli._h, None, 0, None, C.byref(h)) == _ffi.OK and h.value
    assert L.lm_hip_dists_destroy(h) == _ffi.OK


def test_cli_device_pvalues_write_the_same_bytes(tmp_path, jaspar):
    rng = np.random.default_rng(11)
    mats = tmp_path / "motifs.pwm"
    with open(mats, "w") as fh:
        for r in jaspar[:20]:
            fh.write(f">{r.id}\t{r.description}\n")
            for col, sym in ((0, "A"), (1, "C"), (3, "G"), (2, "T")):      # the matrix holds A C T G N (abc.rs:106-108)
                fh.write(f"{sym}  [ " + " ".join(str(int(x)) for x in r.matrix.data[:, col]) + " ]\n")
    fasta = tmp_path / "records.fa"
    with open(fasta, "w") as fh:
        for i, n in enumerate((300, 0, 5, 450, 120)):
            fh.write(f">rec{i} a test record\n")
            s = "".join(rng.choice(list("ACGTN"), n, p=[0.24, 0.24, 0.24, 0.24, 0.04] if n > 30 else [0.25, 0.25, 0.25, 0.25, 0]))
            for j in range(0, n, 60):
                fh.write(s[j:j + 60] + "\n")
    outs = {}
    for extra in ((), ("--best",)):
        for where in ("device", "host"):
            out = tmp_path / f"hits_{where}{'_best' if extra else ''}.tsv"
            argv = ["-m", str(mats), "-s", str(fasta), "-o", str(out), "-P", "1e-2", "--reverse", "--pvalues", where, *extra]
            assert scan_cli.main(argv) == 0
            outs[where, extra] = out.read_bytes()
        assert outs["device", extra] == outs["host", extra]
        assert outs["device", extra].count(b"\n") > 20
