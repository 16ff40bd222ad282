"""CPU self-test of tests/slate_loss_cases.py: every case tests/test_slate_loss_paths_gpu.py runs is shown here, against the fp64 / fp32
oracle alone, to take the path it declares with the 5 % margin, to have a gradient above the floor and an oracle fp32 noise under
the cap -- so the GPU file can gate at the flat 1e-5 and a case that cannot meet its precondition is found before any GPU time is
spent.  Also: path_of against hand-made slates on both sides of 8 and 69, and the ragged oracle loop against the padded rectangle in
the no-clamp and per-pair regimes."""
import pytest
import torch

import ltr_oracle as O
import ragged_cases as RC
import slate_loss_cases as SC


def test_case_lists_are_complete():
    cases = SC.approx_cases()
    assert len(set(cases)) == len(cases)
    have = {(c.regime, c.variant, c.S, c.alpha, c.eps, c.A, c.offset) for c in cases}
    for S in SC.TIER_S:
        for regime, rows in SC.REGIMES.items():
            for A, alpha, eps, offset in rows:
                want = (regime, "tail", S, alpha, eps, A, offset)
                assert (want in have) == (regime != "perpair_overflow" or S >= SC.OVERFLOW_MIN_S), want
        assert all(c.B == (3 if S <= 512 else 2) or (c.B == 5 and (S in SC.SHARED_S or c.regime == "mixed"))
                   or (c.B == 3 and c.regime == "mixed") for c in cases if c.S == S)
    for S in SC.SHARED_S:
        assert any(c.B == 5 and c.S == S and c.regime == "noclamp" for c in cases)
    for S in SC.FULL_S:
        for regime in SC.PAD_REGIMES:
            for v in SC.PAD_VARIANTS:
                assert any(c.regime == regime and c.variant == v and c.S == S for c in cases)
    assert sum(c.pad == -7.0 for c in cases) == 1
    lc = SC.list_cases()
    assert len(set(lc)) == len(lc)
    assert {(c.regime, c.sigmoid, c.S) for c in lc} == {(r, g, S) for r in SC.LIST_REGIMES for g in (False, True) for S in SC.TIER_S}
    assert 1 in SC.TIER_S


def test_path_of_on_both_sides_of_each_threshold():
    y = torch.tensor([2.0, 0.0, 1.0, 3.0])
    for T, below, above in ((SC.T_NOCLAMP, "noclamp", "fast"), (SC.T_FAST, "fast", "perpair")):
        for alpha in (1.0, 0.7, 3.0):
            for sign in (1.0, -1.0):
                lo = torch.tensor([0.0, sign * T * 0.95 / alpha, 0.3, -0.2])
                hi = torch.tensor([0.0, sign * T * 1.05 / alpha, 0.3, -0.2])
                assert SC.path_of(lo, y, alpha, 1e-10, -1.0) == below
                assert SC.path_of(hi, y, alpha, 1e-10, -1.0) == above
                assert SC.path_of(lo + 100.0, y, alpha, 1e-10, -1.0) == below         # a common offset does not move the path
    s = torch.tensor([0.0, 1.0, -1.0, 2.0])
    assert SC.path_of(s, y, 1.0, 1e-6, -1.0) == "fast"                                # eps above 1e-7 disables the no-clamp path
    assert SC.path_of(s, torch.tensor([2.0, 0.5, 1.0, 3.0]), 1.0, 1e-10, -1.0) == "fast"
    assert SC.path_of(s, torch.tensor([2.0, 16.0, 1.0, 3.0]), 1.0, 1e-10, -1.0) == "fast"
    assert SC.path_of(s, torch.tensor([2.0, 15.0, -2.0, 3.0]), 1.0, 1e-10, -1.0) == "noclamp"
    assert SC.path_of(s, torch.tensor([2.0, 16.0, 1.0, 3.0]), 1.0, 1e-10, 16.0) == "noclamp"   # the grade-16 document is padding
    # document 0 padded: its score is still the reference point
    assert SC.path_of(torch.tensor([1e4, 1.0, -1.0, 2.0]), torch.tensor([-1.0, 0.0, 1.0, 3.0]), 1.0, 1e-10, -1.0) == "perpair"
    assert SC.path_of(torch.tensor([float("-inf"), 1.0, -1.0, 2.0]), torch.tensor([-1.0, 0.0, 1.0, 3.0]), 1.0, 1e-10, -1.0) == "perpair"
    assert SC.path_of(torch.tensor([9.0, 1.0, -1.0, 2.0]), torch.tensor([-1.0, 0.0, 1.0, 3.0]), 1.0, 1e-10, -1.0) == "fast"
    assert SC.path_of(torch.tensor([0.0, float("nan"), -1.0, 2.0]), y, 1.0, 1e-10, -1.0) == "perpair"
    assert SC.path_of(s, torch.full((4,), -1.0), 1.0, 1e-10, -1.0) == "noclamp"       # all padding: nothing disqualifies


def _check_noise(c, what):
    ref = SC.reference(c)
    top = float(ref.grad.abs().max())
    nl, ng = SC.relerr(ref.loss32, ref.loss), SC.relerr(ref.grad32, ref.grad, SC.FLOOR if SC.uses_floor(c) else 0.0)
    assert bool(torch.isfinite(ref.loss).all()) and bool(torch.isfinite(ref.grad).all()), what
    print(f"{what}: oracle fp32 noise loss {nl:.2e} gradient {ng:.2e} max|grad| {top:.2e}")
    # over the cap exactly where RELAXED says so: a listed case that no longer needs the relaxed bar fails too
    assert (max(nl, ng) > SC.NOISE_CAP) == (what in SC.RELAXED), (what, nl, ng, top)
    assert nl <= SC.NOISE_CAP, (what, "loss noise", nl)
    assert top >= SC.GRAD_MIN or c.S == 1 or SC.uses_floor(c), (what, top)
    if c.S == 1:
        assert top == 0.0, what
    return top


@pytest.mark.parametrize("regime", list(SC.REGIMES))
def test_every_approx_case_meets_its_preconditions(regime):
    n = 0
    for c in SC.approx_cases():
        if c.regime != regime:
            continue
        n += 1
        what = SC.case_id(c)
        s, y, paths = SC.approx_inputs(c)
        assert s.dtype == torch.float32 and y.dtype == torch.float32 and s.shape == y.shape == (c.B, c.S), what
        front = c.variant in ("front", "front_inf")
        for b in range(c.B):
            real = y[b] != c.pad
            assert SC.path_of(s[b], y[b], c.alpha, c.eps, c.pad) == paths[b], (what, b)
            x = SC.kernel_x(s[b], y[b], c.alpha, c.pad)
            if front:
                assert not bool(real[0]) and int(real.sum()) >= 2 and paths[b] == "perpair", (what, b)
                assert bool((x.abs() >= SC.T_FAST * (1 + SC.MARGIN)).all()), (what, b)
                pad_scores = s[b][~real][: int((~real).sum())]
                assert bool((pad_scores[:1] == (SC.FAR if c.variant == "front" else float("-inf"))).all()), (what, b)
                continue
            assert bool(torch.isfinite(s[b]).all()), (what, b)
            A = float(x.abs().max()) if x.numel() else 0.0
            for T in (SC.T_NOCLAMP, SC.T_FAST):
                assert abs(A - T) >= SC.MARGIN * T, (what, b, A)
            if int(real.sum()) >= 2 and not (regime == "tied_pairs" and int(real.sum()) == 2):      # (two tied documents: A = 0)
                want = SC.declared_A(c, b)
                assert abs(A - want) <= 0.01 * want + 1e-6, (what, b, A, want)     # the declared spread is what the kernel sees
        # what each regime / variant promises
        if regime == "noclamp_grade15":
            assert all(int((y[b] == 15.0).sum()) == 1 for b in range(c.B) if bool((y[b] != c.pad).any())), what
        if regime == "grade16":
            assert all(int((y[b] == 16.0).sum()) == 1 for b in range(c.B) if bool((y[b] != c.pad).any())), what
        if regime == "fast_clamped":
            d = c.alpha * (s.double()[:, :, None] - s.double()[:, None, :])
            pair = ((y != c.pad)[:, :, None] & (y != c.pad)[:, None, :])
            n_clamped = int(((torch.sigmoid(-d) < c.eps) & pair).sum())
            assert n_clamped > 0 or c.S <= 3, (what, "no pair is clamped")
        if regime == "tied_all":
            assert bool((s == s[:, :1]).all()), what
        if regime == "tied_pairs" and c.S >= 2:
            assert bool((s[:, 0:c.S - c.S % 2:2] == s[:, 1:c.S:2]).all()), what
        if regime == "mixed":
            assert set(paths) >= ({"noclamp", "fast", "perpair"} if c.S > 1 else {"noclamp"}), (what, paths)
            assert c.B < 5 or not bool((y[4] != c.pad).any()), what
        if c.variant == "interleaved":
            assert bool((y[:, 2::3] == c.pad).all()) and bool((y[:, 0::3] != c.pad).all()), what
        if c.variant == "one_real":
            assert int((y[1] != c.pad).sum()) == 1, what
        if c.variant == "all_padded":
            assert int((y[c.B - 1] != c.pad).sum()) == 0, what
        if c.variant == "all_zero_labels":
            assert bool((y[0] == 0.0).all()), what
        if c.variant == "negative_labels":
            assert bool((y == -2.0).any()), what
        if c.variant == "pad7":
            assert bool((y == -1.0).any()) and bool((y == -7.0).any()), what
        # gradient floor and oracle noise
        _check_noise(c, what)
    assert n >= len(SC.TIER_S) - 10


@pytest.mark.parametrize("regime", list(SC.LIST_REGIMES))
def test_every_listnet_case_meets_its_preconditions(regime):
    for c in SC.list_cases():
        if c.regime != regime:
            continue
        what = SC.case_id(c)
        yt, yp = SC.list_inputs(c)
        assert yt.dtype == torch.float32 and yp.dtype == torch.float32 and yt.shape == yp.shape == (c.B, c.S), what
        q = torch.softmax(yp, dim=1)
        assert float(q.min()) >= 1e-30, (what, float(q.min()))                    # no log q underflows in fp32
        spread, offset = SC.LIST_REGIMES[regime]
        if c.S > 1:
            got = (yp.max(1).values - yp.min(1).values).double()
            assert bool(((got - spread).abs() <= 1e-3 * max(spread, 1.0) + 4e-3 * (abs(offset) > 1e3)).all()), (what, got)
        if regime == "labels30":
            assert float(yt.max()) > 20.0 or c.S < 8, what
        if regime == "neg_labels":
            assert bool((yt == -1.0).any()) or c.S < 8
            assert bool((yt == -3.0).any()) or c.S < 8
        _check_noise(c, what)
        if c.S == 1:
            assert float(SC.reference(c).loss.abs().max()) in (0.0, 0.5), what


@pytest.mark.parametrize("regime", ["perpair", "noclamp"])
def test_ragged_oracle_loop_equals_the_padded_rectangle(regime):
    lengths = list(RC.ISSUE_LENGTHS)
    s, y, info = SC.ragged_batch(lengths, rotation=(regime,))
    assert all(p == (regime if S > 1 else "noclamp") for (r, p), S in zip(info, lengths))
    bounds = RC.bounds_of(lengths)
    loop = RC.oracle_ragged("approxNDCG", s, y, bounds)
    sp, yp = RC.pad_rectangle(s, bounds, 0.0), RC.pad_rectangle(y, bounds, -1.0)
    l, g, per = O.approx_ndcg_closed_form(sp.double(), yp.double())
    assert abs(float(l) - float(loop["loss"])) <= 1e-12 * abs(float(l))
    assert float((per - loop["per_query"]).abs().max()) <= 1e-12
    gr = RC.unpad(g, bounds)
    assert float((gr - loop["grad"]).abs().max()) <= 1e-12 * max(float(gr.abs().max()), 1e-30)
    for q, (a, b) in enumerate(zip(bounds[:-1], bounds[1:])):                      # padded positions carry no gradient
        assert not bool(g[q, b - a:].any())


def test_ragged_rotation_batches_meet_the_preconditions():
    """The ragged batches of the GPU file (one query per tier length, regimes in rotation) are gated per query at the flat bar:
    every query's oracle noise is under the cap and its gradient above the minimum (or it is a saturated small slate, or S = 1)."""
    lengths = RC.tier_lengths()
    bounds, Q = RC.bounds_of(lengths), len(lengths)
    for shift in SC.RAGGED_SHIFTS:
        s, y, info = SC.ragged_batch(lengths, shift=shift)
        assert {p for _, p in info} == {"noclamp", "fast", "perpair"}
        r64 = RC.oracle_ragged("approxNDCG", s, y, bounds)
        r32 = RC.oracle_ragged("approxNDCG", s, y, bounds, dtype=torch.float32)
        for q, (a, b) in enumerate(zip(bounds[:-1], bounds[1:])):
            c = SC.ragged_case(info[q][0], b - a)
            assert SC.case_id(c) not in SC.RELAXED
            assert SC.path_of(s[a:b], y[a:b], c.alpha, c.eps, c.pad) == info[q][1], (shift, q)
            fl = SC.FLOOR if SC.uses_floor(c) else 0.0
            top = float(r64["grad"][a:b].abs().max()) * Q
            assert SC.relerr(r32["per_query"][q:q + 1], r64["per_query"][q:q + 1]) <= SC.NOISE_CAP, (shift, q, c)
            assert SC.relerr(r32["grad"][a:b] * Q, r64["grad"][a:b] * Q, fl) <= SC.NOISE_CAP, (shift, q, c)
            assert top >= SC.GRAD_MIN or c.S == 1 or fl, (shift, q, c, top)
    for sig in (False, True):
        yt, yp, cs = SC.list_ragged_batch(lengths, sig)
        assert {c.regime for c in cs} == set(SC.LIST_REGIMES)
        r64 = RC.oracle_ragged("listnet", yp, yt, bounds, apply_sigmoid=sig)
        r32 = RC.oracle_ragged("listnet", yp, yt, bounds, dtype=torch.float32, apply_sigmoid=sig)
        for q, (a, b) in enumerate(zip(bounds[:-1], bounds[1:])):
            assert SC.case_id(cs[q]) not in SC.RELAXED
            assert SC.relerr(r32["per_query"][q:q + 1], r64["per_query"][q:q + 1]) <= SC.NOISE_CAP, (sig, q, cs[q])
            assert SC.relerr(r32["grad"][a:b], r64["grad"][a:b]) <= SC.NOISE_CAP, (sig, q, cs[q])
            assert float(r64["grad"][a:b].abs().max()) >= SC.GRAD_MIN or cs[q].S == 1, (sig, q, cs[q])
