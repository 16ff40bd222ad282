"""CPU self-test of tests/lambda_tier_cases.py: the input builders, the clamp-band precondition and the score-scale ladder run
against the fp64 oracle alone for every case tests/test_lambda_tiers_gpu.py will use, so a case that cannot meet its precondition is
found before any GPU time is spent.  Also: the scheme table of the oracle and of the device package name the same schemes."""
import math

import pytest
import torch

import lambda_tier_cases as LT
import ltr_oracle as O


def test_scheme_tables_agree():
    """A ninth weighing scheme cannot arrive untested: the tier tests parametrise over O.SCHEMES, the kernels dispatch on SCHEME_IDS."""
    from ltr_mi355x.functional import SCHEME_IDS
    assert set(O.SCHEMES) == set(SCHEME_IDS), set(O.SCHEMES) ^ set(SCHEME_IDS)
    assert len(O.SCHEMES) == len(set(O.SCHEMES))
    assert sorted(SCHEME_IDS.values()) == list(range(len(SCHEME_IDS)))       # one template instance each, no id shared


def test_required_cross_product_is_complete():
    cases = LT.tier_cases()
    assert len(set(cases)) == len(cases)
    have = {(c.variant, c.S, c.scheme, c.opt) for c in cases}
    for scheme in O.SCHEMES:
        for S in LT.TIER_S:
            for variant in ("plain", "padded"):
                for opt in LT.REQUIRED_OPTS:
                    assert (variant, S, scheme, opt) in have
        for S in LT.FULL_S:
            for variant in ("flat_labels", "tied_scores", "softmaxed"):
                assert any((variant, S, scheme, opt) in have for opt in LT.OPTS)
            for opt in LT.EXTRA_OPTS:
                assert any((v, S, scheme, opt) in have for v in LT.VARIANTS)
        for S in LT.CLAMPED_S:
            assert ("clamped", S, scheme, LT.REQUIRED_OPTS[0]) in have
    for S in LT.RAGGED_S:
        assert any(c.B == 5 and c.S == S for c in cases)
    assert all(c.B == (3 if c.S <= 512 else 2) or (c.B == 5 and c.S in LT.RAGGED_S) for c in cases)


@pytest.mark.parametrize("scheme", list(O.SCHEMES))
def test_every_case_meets_its_precondition(scheme):
    """build() asserts an empty clamp band; the scale is the FIRST rung of the ladder that empties it (never a later one), 2 for the
    schemes outside LADDER_SCHEMES; inputs are fp32, finite, and carry what their variant promises."""
    n = 0
    for c in LT.tier_cases():
        if c.scheme != scheme:
            continue
        s, y, kw = LT.build(c)
        n += 1
        assert s.dtype == torch.float32 and y.dtype == torch.float32 and s.shape == y.shape == (c.B, c.S)
        assert bool(torch.isfinite(s).all())
        if c.variant == "softmaxed":
            assert c.scale is None and not bool((y == LT.PAD).any())
            continue
        if c.variant == "clamped":
            (band, firm), = LT.band_counts(s, y, kw)
            assert firm > 0, "the clamped case clamps nothing"
            continue
        assert c.scale in LT.LADDER
        if scheme in LT.LADDER_SCHEMES:
            s1, _ = LT.inputs(c.variant, c.B, c.S, 1.0)
            rungs = [f for f in LT.LADDER if f > c.scale]
            assert all(band > 0 for band, _ in LT.band_counts(s1, y, kw, rungs)), "an earlier rung already had an empty band"
        else:
            assert c.scale == LT.LADDER[0]
        if c.variant == "padded":
            real = (y != LT.PAD).sum(1)
            assert c.B < 2 or int(real[1]) == 1
            assert c.B < 3 or int(real[2]) == 0
            pm = y == LT.PAD
            assert bool((pm[:, 1:] >= pm[:, :-1]).all())                   # padding is a tail
        if c.variant == "flat_labels":
            assert bool((y[0] == y[0, 0]).all()) and bool((y[1] == 0).all())
        if c.variant == "tied_scores":
            assert c.S == 4 or bool(((s[:, 3] == s[:, 1]) | (s[:, 3] == s.max(1).values)).all())
            assert all(int((s[b] == s[b].max()).sum()) >= max(1, round(0.05 * c.S)) for b in range(c.B))
    assert n > 100


def test_ladder_scaling_is_exact():
    """Every rung is a power of two: the scores of two rungs differ by exactly that factor, so ranks and ties do not move."""
    for f in LT.LADDER:
        assert math.log2(f) == int(math.log2(f))
    a, ya = LT.inputs("tied_scores", 2, 257, 2.0)
    b, yb = LT.inputs("tied_scores", 2, 257, 0.125)
    assert torch.equal(a, b * 16.0) and torch.equal(ya, yb)
    assert torch.equal(O.rank_desc(a), O.rank_desc(b))


def test_band_counts_sees_a_planted_pair():
    """Two documents whose w log u sits on the floor are counted as in the band; far below it as firmly clamped."""
    le = math.log(LT.EPS)
    kw = dict(weighing_scheme=None, k=None, sigma=1.0, mu=LT.MU, reduction_log="binary")
    y = torch.tensor([[1.0, 0.0]])
    on = torch.tensor([[0.0, -le]], dtype=torch.float64)                  # kept pair (0, 1): d = log eps -> log u ~ log eps
    assert LT.band_counts(on, y, kw) == [(1, 0)]
    assert LT.band_counts(torch.tensor([[0.0, 60.0]]), y, kw) == [(0, 1)]
    assert LT.band_counts(torch.tensor([[0.0, 1.0]]), y, kw) == [(0, 0)]
    kw7 = dict(kw, weighing_scheme="rankNetWeightedByGTDiffPowed_scheme")
    y7 = torch.tensor([[4.0, 0.0]])                                      # w = 16: on the floor at log u = log(eps) / 16
    d = torch.tensor([[0.0, 0.0]], dtype=torch.float64)
    d[0, 1] = math.log(math.expm1(-le / 16.0))                           # log sigmoid(-x) = log(eps) / 16  <=>  x = log(e^{-le/16} - 1)
    assert LT.band_counts(d, y7, kw7) == [(1, 0)]


def test_oracle_bundle_matches_the_closed_form():
    """The bundle's kept-pair loss and its gradient (autograd through O.lambda_pairs) equal O.lambda_loss_closed_form; the column
    sums are the matrix summed over rows; real_pairs marks the leading n_real x n_real block."""
    for scheme in O.SCHEMES:
        c = LT.make_case("padded", 3, 33, scheme, "k5-s2-natural")
        s, y, kw = LT.build(c)
        gen = torch.Generator().manual_seed(1)
        gup, gcol = torch.randn(3, 33, 33, generator=gen), torch.randn(3, 33, generator=gen)
        o = LT.oracle_bundle(s, y, kw, gup, gcol, torch.float64)
        rl, rg, n = O.lambda_loss_closed_form(s.double(), y.double(), reduction="sum", **kw)
        assert int(o["keep"].sum()) == int(n)
        assert abs(float(o["slate"].sum()) - float(rl)) <= 1e-12 * max(1.0, abs(float(rl)))
        assert float((o["g_sum"] - rg).abs().max()) <= 1e-12 * max(1.0, float(rg.abs().max()))
        assert torch.equal(o["col"], o["losses"].sum(1))
        rp = LT.real_pairs(y)
        assert bool((o["keep"] <= rp).all()) and int(rp[2].sum()) == 0 and int(rp[1].sum()) == 1


@pytest.mark.parametrize("scheme", list(O.SCHEMES))
def test_dispatch_edge_inputs_meet_the_precondition(scheme):
    """The inputs test_losses_gpu.py::test_lambda_oracle takes at LT.EDGE_SHAPES: a rung with an empty band exists for both of
    its option sets, plain and with tied scores."""
    for B, S in LT.EDGE_SHAPES:
        for k, sigma, log in ((None, 1.0, "binary"), (5, 2.0, "natural")):
            for variant in ("plain", "tied_scores"):
                s, y = LT.edge_inputs(variant, B, S, scheme, k, sigma, log)
                kw = dict(weighing_scheme=scheme, k=k, sigma=sigma, mu=LT.MU, reduction_log=log)
                assert LT.band_counts(s, y, kw)[0][0] == 0 and s.dtype == torch.float32 and s.shape == (B, S)
