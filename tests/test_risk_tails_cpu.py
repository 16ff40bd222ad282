"""CPU self-test of tests/risk_tail_cases.py and of the tail oracle (oracle/ltr_risk_oracle.py: risk_tail, t_risk_pair_tail): the
new oracle functions are anchored to the six loss oracles the golden fixtures pin, and every precondition the GPU file
(tests/test_risk_tails_gpu.py) relies on is checked here as a condition, before any GPU time is spent; plus the argument checks of the
C ABI that need no launch."""
import math

import numpy as np
import pytest
import torch

import ltr_risk_oracle as RO
import risk_tail_cases as C
from conftest import golden, golden_cases, relerr

T = torch.from_numpy


# ------------------------------------------------------------------------------------------------- the oracle's anchor
def _through_the_tail(case, yp, yt, yb):
    """A golden loss case evaluated as (unflipped matrix) -> risk_tail / t_risk_pair_tail."""
    fn, lt, alpha = case["fn"], case["listnet_transformation"], case["alpha"]
    pt, pp, pb = RO._softmaxes(yp, yt, yb)
    scheme = case.get("weighing_scheme", "ndcgLoss2PP_scheme")
    if fn.startswith("tRisk"):
        if "Lambda" in fn:
            m = RO._t_cols(RO.pair_colsum(pt, pt, scheme), RO.pair_colsum(pp, pt, scheme), RO.pair_colsum(pb, pt, scheme), lt, flip=False)
        else:
            m = RO._t_cols(pt * pt, pt * pp, pt * pb, lt, flip=False)
        return RO.t_risk_pair_tail(m.t(), alpha, lt == 1, 1)
    geo, rs, ideal = fn.startswith("geo"), case["return_strategy"], case["add_ideal_ranking_to_mat"]
    if "Lambda" in fn:
        m, flip = RO.lambda_matrix(pt, pp, pb, lt, ideal, scheme, geo, flip=False), lt == 1
    else:
        m, flip = RO.listnet_matrix(pt, pp, pb, lt, ideal, flip=False), lt in (1, 3)
    return RO.risk_tail(m, alpha, geo, rs, flip, 1, zquirk=fn == "zRiskListnetLoss")


@pytest.mark.parametrize("case", [c for c in golden_cases("risk") if c["kind"] == "loss"], ids=lambda c: c["id"])
def test_tail_oracle_is_the_six_losses(case):
    """risk_tail / t_risk_pair_tail on the unflipped matrix == the loss oracle (pinned to the reference by tests/golden/risk.npz), value
    and gradient, 1e-12 relative in fp64."""
    from test_oracle_golden_r2 import oracle_risk_loss
    g = golden("risk")
    yp, yt = T(g.arr(case, "y_pred")).double(), T(g.arr(case, "y_true")).double()
    yb = T(g.arr(case, "y_base")).double() if g.has(case, "y_base") else None
    a = yp.clone().requires_grad_(True)
    want = oracle_risk_loss(case, a, yt, yb)
    want.sum().backward()
    b = yp.clone().requires_grad_(True)
    got = _through_the_tail(case, b, yt, yb)
    got.sum().backward()
    assert got.shape == want.shape == (1,)
    assert relerr(got.detach().numpy(), want.detach().numpy()) <= 1e-12
    assert relerr(b.grad.numpy(), a.grad.numpy()) <= 1e-12


def test_negative_factor_and_quirk_follow_the_loss_oracles():
    """`negative` = -1 through the tail == through the loss oracles, incl. zRiskListnetLoss's precedence (f R1 - R0)."""
    gen = torch.Generator().manual_seed(3)
    yp, yt, yb = (torch.randn(6, 8, generator=gen).double(), torch.randint(0, 5, (6, 8), generator=gen).double(),
                  torch.randn(6, 8, 3, generator=gen).double())
    pt, pp, pb = RO._softmaxes(yp, yt, yb)
    for rs in (1, 2, 3):
        m = RO.listnet_matrix(pt, pp, pb, 1, 2, flip=False)
        for geo, fn in ((True, RO.geo_risk_listnet), (False, RO.z_risk_listnet)):
            want = fn(yp, yt, yb, alpha=5, lt=1, rs=rs, negative=-1, add_ideal=2)
            got = RO.risk_tail(m, 5, geo, rs, True, -1, zquirk=not geo)
            assert relerr(got.numpy(), want.numpy()) <= 1e-12, (rs, geo)
    m = RO._t_cols(pt * pt, pt * pp, pt * pb[:, :, 0], 1, flip=False)
    assert relerr(RO.t_risk_pair_tail(m.t(), 5, True, -1).numpy(), RO.t_risk_listnet(yp, yt, yb[:, :, 0], negative=-1).numpy()) <= 1e-12


def test_max_gradient_is_split_evenly_among_ties():
    x = torch.tensor([[1.0, 3.0], [3.0, 2.0]], dtype=torch.float64, requires_grad=True)
    x.max().backward()
    assert torch.equal(x.grad, torch.tensor([[0.0, 0.5], [0.5, 0.0]], dtype=torch.float64))


# ------------------------------------------------------------------------------------------------- the case tables
def test_case_tables_are_complete():
    shapes = C.tail_shapes()
    assert len(set(shapes)) == len(shapes)
    for Q in (2, 3, 63, 64, 65, 1023, 1024, 1025, 2047, 2049, 4097):
        for n in (2, 3, 9):
            for v in C.VARIANTS:
                assert (Q, n, v) in shapes
        for v in C.T_VARIANTS:
            assert (Q, v) in C.t_shapes()
    assert any(Q == 1 for Q, _, _ in shapes) and any(n == 65 for _, n, _ in shapes) and any(n == 1 for _, n, _ in shapes)
    opts = C.options()
    assert len(set(opts)) == len(opts) == (3 + 4) * 2 * 3 * 2
    assert {o.alpha for o in opts} == {0.0, 1.0, 5.0} and {o.factor for o in opts} == {1.0, -1.0}
    assert all(o.zquirk <= (not o.geo and o.strategy == 2) for o in opts) and any(o.zquirk for o in opts)
    assert len(C.t_options()) == 12
    assert set(C.MATRIX_S) == {1, 2, 3, 63, 65, 255, 256, 257, 511, 513, 1023, 1025, 2047, 2048}


@pytest.mark.parametrize("variant", C.VARIANTS)
def test_every_tail_case_meets_its_preconditions(variant):
    """fp32 inputs; the planted maximum occurs exactly as often as intended, in the rows and columns the variant promises; the fp64
    oracle is finite in value and gradient for every option set (except the named 0 / 0 cases, NaN there); strategies 2 / 3 keep
    |R1 - R0| >= 1e-3 max(|R0|, |R1|); model_worse sits in its window; the ladders took their FIRST passing rung."""
    n_cases = 0
    for Q, n, v in C.tail_shapes():
        if v != variant:
            continue
        n_cases += 1
        m = C.matrix(v, Q, n)
        assert m.dtype == torch.float32 and m.shape == (Q, n) and bool(torch.isfinite(m).all())
        pos = C.tie_positions(v, Q, n)
        if pos:
            assert len(set(pos)) == len(pos)
            assert int((m == m.max()).sum()) == len(pos) and all(float(m[r, c]) == float(m.max()) for r, c in pos)
            assert float(m.max()) == float(np.float32(C.TIE))
            rows, cols = {r for r, _ in pos}, {c for _, c in pos}
            assert {0, Q - 1} <= rows and {0, n - 1} <= cols
            if v == "max_ties2":
                assert len(pos) == 2
            else:
                assert Q // 2 in rows and (n // 2 in cols or Q == 2)      # (Q = 2: row Q / 2 is the last row)
                assert len(pos) >= 2 and (Q < 6 or abs(len(pos) - Q / 3.0) <= 2.0)
                if Q > 1024:
                    assert any(r >= 1024 for r in rows) and any(r < 1024 for r in rows)      # both sweeps own tied entries
        elif not C.absolute(v, Q, n):
            assert int((m == m.max()).sum()) == 1
        if v == "equal_rows":
            assert bool((m == m[0]).all())
            assert int(m[0].argmax()) == (n // 2 if n >= 3 else n - 1)
        bias, scale = C.recipe(v, Q, n)
        if not C.absolute(v, Q, n):
            assert C.gaps_ok(m)
            for earlier in C.BIAS_LADDER[:C.BIAS_LADDER.index(bias)]:
                assert not C.gaps_ok(C._variant(v, Q, n, earlier, scale))
        if v == "model_worse":
            assert C.WORSE_WINDOW[0] < C.worse_v(m) < C.WORSE_WINDOW[1] < -2.49
        for o in C.options():
            x = m.double().requires_grad_(True)
            val, r0, r1 = RO.risk_tail_parts(x, o.alpha, o.geo, o.strategy, o.flip, o.factor, o.zquirk)
            g, = torch.autograd.grad(val.sum(), x)
            if C.expect_nan(v, n, o):
                assert bool(torch.isnan(val).all()), (Q, n, v, o)
                continue
            assert bool(torch.isfinite(val).all()) and bool(torch.isfinite(g).all()), (Q, n, v, o)
            if o.strategy > 1 and not C.absolute(v, Q, n):
                r0, r1 = float(r0.detach()), float(r1.detach())
                assert abs(r1 - r0) >= C.GAP * max(abs(r0), abs(r1)), (Q, n, v, o)
                av, ag = C.rounding_allowance(o, r0, r1, float(val.detach()))
                assert 0.0 <= ag <= 2.0 ** -23 / C.GAP and av >= 0.0 and math.isfinite(av)     # an ulp is at most 2^-23 relative
    assert n_cases >= 33 or variant == "plain"


def test_every_trisk_case_is_finite_in_the_oracle():
    for Q, v in C.t_shapes():
        m = C.matrix(v, Q, 2)
        for o in C.t_options():
            x = m.double().requires_grad_(True)
            val = RO.t_risk_pair_tail(x, o.alpha, o.flip, o.factor)
            g, = torch.autograd.grad(val.sum(), x)
            assert bool(torch.isfinite(val).all()) and bool(torch.isfinite(g).all()) and float(val.abs()) > 0.0, (Q, v, o)
    one = torch.tensor([[0.3, 0.5]], dtype=torch.float64)
    assert bool(torch.isnan(RO.t_risk_pair_tail(one, 5.0, False, 1.0)).all())              # std of one sample


def test_rounding_allowance_formula():
    u = C.ulp32(0.4)
    assert u == 2.0 ** -25                                           # 0.4 lies in [2^-2, 2^-1): 23 fraction bits below 2^-2
    o2, o3 = C.Opt(True, 2, False, False, 5.0, 1.0), C.Opt(True, 3, False, False, 5.0, -1.0)
    assert C.rounding_allowance(C.Opt(True, 1, False, False, 5.0, 1.0), 0.4, 0.39, 0.4) == (0.0, 0.0)
    assert C.rounding_allowance(o2, 0.4, 0.39, -0.01) == (u / 0.01, 0.0)
    av, ag = C.rounding_allowance(o3, 0.4, 0.39, -1e-4)
    assert av == 2.0 * ag and abs(ag - u / 0.01) <= 1e-12 * ag


# ------------------------------------------------------------------------------------------------- blocks
@pytest.mark.parametrize("Q", C.BLOCK_Q)
def test_packer_round_trips_and_layouts_cover_the_patterns(Q):
    m = C.matrix("plain", Q, 3)
    names = set()
    for lay in C.layouts(Q):
        names.add(lay.name)
        assert sum(lay.counts) == Q and len(lay.counts) == lay.n_blocks <= 1024 and max(lay.counts) <= lay.block_rows
        for pad in (float("nan"), 7.0):
            b = C.pack(m, lay, pad)
            assert b.shape == (lay.n_blocks, 1 + lay.block_rows * 3)
            assert torch.equal(C.unpack(b, 3), m)
            mask = C.padding_mask(lay, 3)
            assert torch.equal(b[:, 0], torch.tensor(lay.counts, dtype=torch.float32))
            rest = mask.clone()
            rest[:, 0] = False
            assert bool(torch.isnan(b[rest]).all()) if math.isnan(pad) else bool((b[rest] == pad).all())
            assert int((~mask).sum()) == Q * 3
    assert {"one_full", "two_ragged_last", "three_empty_first", "eight_empty_middle_and_tail"} <= names
    lays = {lay.name: lay for lay in C.layouts(Q)}
    assert lays["three_empty_first"].counts[0] == 0
    e = lays["eight_empty_middle_and_tail"].counts
    assert e[2] == 0 and e[6] == 0 and e[7] == 0 and e[1] > 0 and e[3] > 0
    assert ("eight_full" in names) == (Q % 8 == 0)
    assert ("limit_1024_blocks" in names) == (Q <= 2048)
    if Q <= 2048:
        c = lays["limit_1024_blocks"].counts
        assert len(c) == 1024 and lays["limit_1024_blocks"].block_rows == 2 and {0, 1, 2} >= set(c)
    if Q > 1024:
        assert lays["boundary_at_row_1024"].counts[0] == 1024
        s = lays["block_straddles_row_1024"].counts
        assert s[0] < 1024 < s[0] + s[1]
    else:
        assert "boundary_at_row_1024" not in names


def test_block_layouts_reach_every_pattern_somewhere():
    names = {lay.name for Q in C.BLOCK_Q for lay in C.layouts(Q)}
    assert names == {"one_full", "two_ragged_last", "three_empty_first", "eight_empty_middle_and_tail", "eight_full", "limit_1024_blocks",
                     "boundary_at_row_1024", "block_straddles_row_1024"}
    full = [lay for lay in C.layouts(2047) if lay.name == "limit_1024_blocks"][0]
    assert sum(1 for c in full.counts if c == 2) == 1023 and sum(1 for c in full.counts if c == 1) == 1
    mixed = [lay for lay in C.layouts(1025) if lay.name == "limit_1024_blocks"][0]
    assert 0 in mixed.counts and 1 in mixed.counts and 2 in mixed.counts


# ------------------------------------------------------------------------------------------------- matrix oracle
def test_matrix_oracle_is_the_loss_oracles_matrix():
    """matrix_oracle (what the GPU file compares ltr_risk_matrix_fwd with) == RO.listnet_matrix / RO._t_cols on the same soft-maxed
    inputs, and its jac == autograd of the model column."""
    ref, x0, rest = C.matrix_inputs(33, 0, 3)
    pt, pp, pb = RO._softmaxes(x0.double(), ref.double(), rest.double())
    for lt in (1, 2, 3):
        for ideal in (False, True):
            mat, jac = C.matrix_oracle(ref, x0, rest, 0, lt, ideal, torch.float64)
            want = RO.listnet_matrix(pt, pp, pb, lt, 2 if ideal else 1, flip=False)
            assert mat.shape == (C.MATRIX_B, 4 + int(ideal)) and relerr(mat.numpy(), want.numpy()) <= 1e-12
            assert jac.shape == x0.shape and bool(torch.isfinite(jac).all())
        mat2, _ = C.matrix_oracle(ref, x0, rest[:, :, :1], 2, lt, False, torch.float64)
        want2 = RO._t_cols(pt * pt, pt * pp, pt * pb[:, :, 0], lt, flip=False).t()
        assert relerr(mat2.numpy(), want2.numpy()) <= 1e-12
    r1, x1, rest1 = C.matrix_inputs(33, 1, 3)
    m1, j1 = C.matrix_oracle(r1, x1, rest1, 1, 1, True, torch.float64)
    assert float(m1[:, -1].abs().max()) == 0.0 and relerr(j1.numpy(), (2.0 * (x1.double() - r1.double())).numpy()) <= 1e-12
    m2, _ = C.matrix_oracle(r1, x1, rest1, 1, 2, True, torch.float64)
    assert relerr(m2[:, -1].numpy(), np.ones(C.MATRIX_B)) <= 1e-12
    for S in C.MATRIX_S:                                              # a slate and a baseline of one keep their dimensions
        for mode in (0, 1, 2):
            ref, x0, rest = C.matrix_inputs(S, mode, 1)
            mat, jac = C.matrix_oracle(ref, x0, rest, mode, 2, True, torch.float32)
            assert mat.shape == (C.MATRIX_B, 3) and jac.shape == (C.MATRIX_B, S) and mat.dtype == torch.float32


# ------------------------------------------------------------------------------------------------- C ABI, no launch
def test_abi_rejections_without_a_launch():
    """Argument checks that run before any device work (pointers are never dereferenced on the host)."""
    import ctypes
    from ltr_mi355x import _lib
    from ltr_mi355x.build import build
    build(force=False, verbose=False)
    h = _lib.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    SHAPE, PARAM = -2, -3
    ok = dict(n_blocks=2, block_rows=4, n=3, kind=1, strategy=1)

    def risk_blocks(**kw):
        a = dict(ok, **kw)
        return h.ltr_risk_tail_blocks_fwd_bwd(p, a["n_blocks"], a["block_rows"], a["n"], 5.0, a["kind"], a["strategy"], 1, 1.0, 0, p, p, None)

    def trisk_blocks(n_blocks=2, block_rows=4):
        return h.ltr_trisk_tail_blocks_fwd_bwd(p, n_blocks, block_rows, 5.0, 1, 1.0, p, p, None)

    for nb in (0, 1025):
        assert risk_blocks(n_blocks=nb) == SHAPE and trisk_blocks(n_blocks=nb) == SHAPE
    assert risk_blocks(block_rows=-1) == SHAPE and trisk_blocks(block_rows=-1) == SHAPE
    for strategy in (0, 4):
        assert risk_blocks(strategy=strategy) == PARAM
        assert h.ltr_risk_tail_fwd_bwd(p, 4, 3, 5.0, 1, strategy, 1, 1.0, 0, p, p, None) == PARAM
    assert risk_blocks(kind=2) == PARAM
    assert h.ltr_risk_tail_fwd_bwd(p, 4, 3, 5.0, 2, 1, 1, 1.0, 0, p, p, None) == PARAM
