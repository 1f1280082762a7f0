"""Host pieces of the device score distributions (no GPU): the alternate constructor of ``dist.ScoreDistribution`` that
``ScoreDistributions.distribution`` fills from a downloaded table, the CLI's ``--pvalues`` switch, and the new unit in the
build."""
import numpy as np
import pytest

import lightmotif_amd as lm
from lightmotif_amd import _ffi, build, scan_cli
from lightmotif_amd.dist import ScoreDistribution


def matrices():
    rng = np.random.default_rng(5)
    w = rng.uniform(-6, 2, (9, 5)).astype(np.float32)
    w[:, 4] = -np.inf
    w[2, 1] = -np.inf
    p = rng.uniform(-4, 3, (3, 21)).astype(np.float32)
    p[:, 20] = -np.inf
    return [lm.ScoringMatrix(w), lm.ScoringMatrix(p, protein=True),
            lm.ScoringMatrix(np.full((2, 5), 0.5, np.float32))]


@pytest.mark.parametrize("which", range(3))
def test_distribution_rebuilt_from_its_parts_answers_alike(which):
    want = ScoreDistribution(matrices()[which])
    got = ScoreDistribution.from_parts(want.sf.copy(), want._scale, want._offset, want._rows, want.min_score, want.max_score)
    lo, hi = want.unscale(0), want.unscale(len(want.sf) - 1)
    for s in np.linspace(lo - 3, hi + 3, 101).astype(np.float32):
        assert got.pvalue(s) == want.pvalue(s) and got.scale(s) == want.scale(s)
    for p in (0.0, 1e-300, 1e-5, 1e-3, 0.25, 0.5, 1.0, 2.0, -1.0, float(want.sf[want.max_score]), float(want.sf[len(want.sf) // 2])):
        assert got.score(p) == want.score(p)
    assert got.min_pvalue() == want.min_pvalue()
    assert got.unscale(17) == want.unscale(17)
    with pytest.raises(ValueError):
        ScoreDistribution.from_parts(want.sf[:-1], want._scale, want._offset, want._rows, want.min_score, want.max_score)


def test_cli_parser_takes_pvalues():
    ap = scan_cli.build_parser()
    base = ["-m", "m.pwm", "-s", "s.fa", "-o", "o.tsv"]
    assert ap.parse_args(base).pvalues == "device"
    assert ap.parse_args(base + ["--pvalues", "host"]).pvalues == "host"
    assert ap.parse_args(base + ["--pvalues", "device", "-P", "1e-4"]).pvalue == 1e-4
    with pytest.raises(SystemExit):
        ap.parse_args(base + ["--pvalues", "elsewhere"])


def test_hit_pvalues_regroups_by_motif():
    """The CLI hands its record-ordered hits to ONE pvalues call grouped by motif and puts the answers back in place."""
    class Fake:
        def __len__(self):
            return 4

        def pvalues(self, counts, scores):
            assert counts.tolist() == [2, 0, 3, 1] and scores.dtype == np.float32
            motif = np.repeat(np.arange(4), counts)
            return motif * 100.0 + scores
    motif = np.array([2, 0, 3, 2, 0, 2])
    score = np.array([1, 2, 3, 4, 5, 6], np.float32)
    assert scan_cli.hit_pvalues(Fake(), motif, score).tolist() == [201, 2, 303, 204, 5, 206]


def test_unit_and_symbols_are_declared():
    assert "dist.hip" in build.UNITS and "dist.hip" not in build.UNIT_FLAGS      # no looser float flags than the rest
    assert (build.CSRC / "dist.hip").exists()
    for name in ("create", "len", "info", "sf", "scores", "pvalues", "destroy"):
        assert f"lm_hip_dists_{name}" in _ffi.SIGNATURES
    assert "ScoreDistributions" in lm.__all__
