"""CPU checks of tests/eval_edge_cases.py and of the oracles the GPU file (tests/test_eval_edges_gpu.py) compares against.

  * ranks: the sort-based form of ltr_metrics_oracle.ranks_desc equals the counting form exactly, both tie rules, on every small
    shape of the case module (heavy-tie rows, +0.0 / -0.0 included) -- the counting form is what the reference fixtures pin;
  * NDCG inputs are fp32-representable, and every row kind holds what its name says;
  * the ordinal oracle equals plain torch in fp64 -- torch.nn.functional.binary_cross_entropy(reduction="none"), the mask and the
    divide of losses/ordinal.py, differentiated by autograd -- on EVERY ordinal case: clamps, pad in {-1, 0, 1}, 0 / 0.  That pin,
    not the kernel, is what says which targets `pad` masks and what the clamp constants are;
  * the derived bound of the fp32 reduction is what the issue states, and the gather cases reach the loops they are named for.
No case is skipped or filtered anywhere in this file.
"""
import math

import numpy as np
import pytest
import torch

import eval_edge_cases as C
import ltr_metrics_oracle as MO
import ltr_oracle as O

COUNTING_UP_TO = 1025            # the [Q, S, S] cube of the counting form: 8 MB a query here


# ------------------------------------------------------------------------------------------------- ranks
@pytest.mark.parametrize("Q,S,name,kinds", [c for c in C.ndcg_dense_cases() if c[1] <= COUNTING_UP_TO], ids=lambda v: str(v))
def test_sorting_ranks_equal_counting_ranks(Q, S, name, kinds):
    y, s = C.ndcg_batch(Q, S, kinds)
    for v in (y, s):
        for stable in (True, False):
            a, b = MO.ranks_desc_counting(v, stable), MO.ranks_desc_sorting(v, stable)
            assert a.shape == b.shape == (Q, S) and np.array_equal(a, b), (name, stable)
            assert np.array_equal(np.sort(b, axis=1), np.broadcast_to(np.arange(S), (Q, S))), (name, stable)
            assert np.array_equal(MO.ranks_desc(v, stable), a)


def test_sorting_ranks_on_the_ragged_batch_and_tiny_rows():
    y, s, bounds = C.ragged_batch()
    for q in range(bounds.size - 1):
        for v in (y[bounds[q]:bounds[q + 1]][None], s[bounds[q]:bounds[q + 1]][None]):
            for stable in (True, False):
                assert np.array_equal(MO.ranks_desc_counting(v, stable), MO.ranks_desc_sorting(v, stable))
    z = np.array([[0.0, -0.0, 0.0, -0.0]])
    assert MO.ranks_desc_sorting(z, True).tolist() == [[0, 1, 2, 3]] and MO.ranks_desc_sorting(z, False).tolist() == [[3, 2, 1, 0]]


def test_ranks_dispatch_takes_the_sorting_form_for_long_rows():
    """Above SORT_ABOVE the cube is never built: S = 16384 (2 GB of booleans a query as a cube) returns at once."""
    y, s = C.ndcg_batch(1, C.NDCG_S_LIMIT, ("quant4",))
    assert C.NDCG_S_LIMIT > MO.SORT_ABOVE
    r = MO.ranks_desc(s, False)
    assert np.array_equal(np.sort(r, axis=1)[0], np.arange(C.NDCG_S_LIMIT))
    top = np.flatnonzero(s[0] == max(C.QUANT_LEVELS))
    assert r[0, top[-1]] == 0 and r[0, top[0]] == top.size - 1            # reverse ties: the highest index of the top run first


# ------------------------------------------------------------------------------------------------- NDCG inputs
@pytest.mark.parametrize("Q,S,name,kinds", C.ndcg_dense_cases(), ids=lambda v: str(v))
def test_ndcg_inputs_are_fp32_representable_and_as_named(Q, S, name, kinds):
    y, s = C.ndcg_batch(Q, S, kinds)
    assert y.shape == s.shape == (Q, S) and y.dtype == np.float64 and s.dtype == np.float32
    assert np.array_equal(y.astype(np.float32).astype(np.float64), y)
    assert np.array_equal(s.astype(np.float64).astype(np.float32), s) and bool(np.isfinite(s).all())
    for q, kind in enumerate(kinds):
        yy, ss = y[q], s[q]
        if kind in ("normal5", "quant4", "all_equal", "signed_zero"):
            assert set(np.unique(yy)) <= {0.0, 1.0, 2.0, 3.0, 4.0} and np.unique(yy).size == 5
        if kind == "normal5":
            assert np.unique(ss).size >= S - S // 1000          # random fp32 normals: a stray equal pair at 16384 at most
        if kind in ("quant4", "relevant_last"):
            assert np.unique(ss).size == 4 and np.bincount(np.searchsorted(np.unique(ss), ss)).max() >= S // 4
        if kind == "all_equal":
            assert np.unique(ss).size == 1
        if kind == "signed_zero":
            z = ss == 0.0
            assert bool((np.signbit(ss) & z).any()) and bool((~np.signbit(ss) & z).any())
        if kind == "no_relevant":
            assert not yy.any()
        if kind == "relevant_last":
            assert yy[S - 1] > 0 and not yy[: S - 1].any() and int((ss == ss[S - 1]).sum()) > 1
        if kind == "fractional":
            assert yy.min() >= 0.0 and yy.max() < 4.0 and bool((yy != np.floor(yy)).any())
        if kind == "negative":
            assert yy.max() <= 0.0 and yy.min() < 0.0


def test_every_row_kind_appears_at_every_shape_and_no_shape_is_missing():
    cases = C.ndcg_dense_cases()
    assert {(Q, S) for Q, S, _, _ in cases} == set(C.NDCG_SHAPES)
    for Q, S in C.NDCG_SHAPES:
        assert {k for q, s, _, kinds in cases if s == S for k in kinds} == set(C.ROW_KINDS)
        opts = C.ndcg_options(S)
        assert {o.k for o in opts} == {1, S - 1, S, S + 7, None}
        for field, both in (("gains", {"linear", "exponential"}), ("no_relevant", {True, False}), ("reverse_ties", {True, False}),
                            ("want", {"ndcg", "dcg"})):
            assert {getattr(o, field) for o in opts} == both
        assert len(opts) == (80 if S <= C.FULL_PRODUCT_UP_TO else 5)
    blocks = {S: min(max(1 << (S - 1).bit_length(), 64), 1024) for _, S in C.NDCG_SHAPES}
    assert blocks[63] == blocks[64] == 64 and blocks[65] == 128 and blocks[1023] == blocks[1024] == blocks[1025] == 1024
    assert 8 * 8192 == 64 * 1024 < 8 * 8193


def test_negative_ideal_dcg_divides_like_the_reference():
    """utils/metrics.py:72-74 returns dcg / idcg for every idcg but 0, a negative one included: the oracle does the same."""
    y = np.array([[-1.0, -2.0, 0.0, -3.0]])
    s = np.array([[0.3, 0.1, -0.2, 0.9]], dtype=np.float32)
    order = [3, 0, 1, 2]
    d = sum(y[0, j] / math.log2(i + 2) for i, j in enumerate(order))
    ideal = sum(v / math.log2(i + 2) for i, v in enumerate(sorted(y[0], reverse=True)))
    assert ideal < 0
    assert abs(MO.ndcg_per_query(y, s, k=4, gains="linear")[0] - d / ideal) < 1e-15
    assert MO.ndcg_per_query(y, s, k=1, gains="linear", no_relevant=True)[0] == 1.0      # ideal DCG@1 = 0 / log2(2)
    assert MO.ndcg_per_query(y, s, k=1, gains="linear", no_relevant=False)[0] == 0.0


def test_ragged_batch_sits_on_the_tier_edges():
    y, s, bounds = C.ragged_batch()
    assert np.diff(bounds).tolist() == [L for L in C.RAGGED_LENGTHS for _ in range(2)]
    assert np.array_equal(y.astype(np.float32).astype(np.float64), y) and s.dtype == np.float32
    for q in range(1, bounds.size - 1, 2):                                # the second query of each length is heavy-tie
        assert np.unique(s[bounds[q]:bounds[q + 1]]).size <= 4


# ------------------------------------------------------------------------------------------------- ordinal
def torch_ordinal(p, y, n, pad):
    """losses/ordinal.py in plain torch, fp64, differentiated by autograd.  The targets carry the DEFAULT indicator -1; the mask
    compares them with `pad`.  ATen's BCE is affine in the target, l(p, t) = t l(p, 1) + (1 - t) l(p, 0), and current torch refuses
    targets outside [0, 1], so the two halves are taken from binary_cross_entropy and combined: identical for t in {0, 1}, and what
    the formula gives for the -1 targets that pad = 0 / 1 leave unmasked."""
    F = torch.nn.functional
    x = p.double().clone().requires_grad_(True)
    ks = torch.arange(1, n + 1, dtype=torch.float64)
    rep = y.double().unsqueeze(2).repeat(1, 1, n)
    t = (rep >= ks).double()
    t[rep == -1] = -1.0                                                   # ordinal.py:39: with_ordinals(y, n), default indicator
    mask = t == pad                                                       # :41
    l1 = F.binary_cross_entropy(x, torch.ones_like(x), reduction="none")
    l0 = F.binary_cross_entropy(x, torch.zeros_like(x), reduction="none")
    ls = t * l1 + (1.0 - t) * l0
    ls = torch.where(mask, torch.zeros_like(ls), ls)                      # :45
    valid = ((~mask).sum(dim=2).float() > 0.0).sum()                      # :49
    loss = ls.sum(dim=2).sum() / valid                                    # :47, :51
    g, = torch.autograd.grad(loss, x)
    return loss.detach(), g


@pytest.mark.parametrize("c", C.ORDINAL_CASES, ids=lambda c: c.name)
def test_ordinal_oracle_equals_torch_fp64_bce_with_autograd(c):
    p, y, clamp = C.ordinal_inputs(c)
    assert p.dtype == torch.float32 and y.dtype == (torch.float64 if c.y64 else torch.float32)
    loss, g = O.ordinal_closed_form(p.double(), y, c.n, c.pad)
    assert loss.dtype == torch.float64 and g.dtype == torch.float64 and g.shape == p.shape
    rl, rg = torch_ordinal(p, y, c.n, c.pad)
    if C.ordinal_expect_nan(c):
        assert bool(torch.isnan(loss)) and bool(torch.isnan(rl))
        assert not bool(g.any()) and not bool(rg.any())                   # masked entries are zeroed before the division
        return
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(g).all())
    assert abs(float(loss) - float(rl)) <= 1e-13 * abs(float(rl))
    # element-wise: ATen holds its 1e-12 as an fp32 constant (4e-9 away from the double), so a clamped denominator agrees to 4e-9
    assert bool(((g - rg).abs() <= 1e-8 * rg.abs()).all())
    plain = ~clamp
    assert bool(((g - rg).abs()[plain] <= 1e-13 * rg.abs()[plain]).all())
    # the same case through the fp32 flavour of the oracle stays within the project's bar of the fp64 one
    l32, _ = O.ordinal_closed_form(p, y.float(), c.n, c.pad)
    assert l32.dtype == torch.float32 and abs(float(l32) - float(loss)) <= 1e-5 * abs(float(loss))


def test_ordinal_cases_reach_their_edges():
    docs = {c.B * c.S for c in C.ORDINAL_CASES}
    assert {1, 255, 256, 257, C.ORD_STRIDE * C.ORD_BLOCK, C.ORD_STRIDE * C.ORD_BLOCK + 1, 1088 * C.ORD_BLOCK} <= docs
    assert {c.n for c in C.ORDINAL_CASES} >= {1, 2, 5, 64} and {c.pad for c in C.ORDINAL_CASES} == {-1, 0, 1}
    assert any(c.go == 3.0 for c in C.ORDINAL_CASES) and any(c.y64 for c in C.ORDINAL_CASES)
    for c in C.ORDINAL_CASES:
        p, y, clamp = C.ordinal_inputs(c)
        if c.labels == "mixed" and c.B * c.S >= c.n + 4:
            assert set(C.ordinal_label_values(c.n)) == set(y.view(-1).tolist())
        if c.clamp:
            assert int(clamp.sum()) == len(C.CLAMP_P)
            got = p.view(-1, c.n)[clamp.view(-1)]
            assert got[:, 0].double().tolist() == list(C.CLAMP_P) and bool((got == got[:, :1]).all())
            assert bool((y.view(-1)[clamp.view(-1)] == 1.0).all()) and c.n >= 2        # targets (1, 0, ..): both per document
        else:
            assert not bool(clamp.any())
    assert 0.0 < C.SUBNORMAL < C.SMALLEST_NORMAL and float(np.float32(C.NEAR_ONE)) == C.NEAR_ONE < 1.0
    # the clamps bite: log p < -100 only at p = 0; (1 - p) p < 1e-12 at 0, 1, the smallest normal and the subnormal
    assert [v * (1.0 - v) < 1e-12 for v in C.CLAMP_P] == [True, True, True, True, False]


def test_leaving_out_the_second_stride_moves_the_reference_past_the_bar():
    """What the GPU file's second-stride cases can catch.  reduce_pairs_kernel without its second stride sums the partials of the
    first 1024 x 256 documents only.  At 1024 x 256 + 1 documents that is one document out of 262145: loss and gradient move by less
    than the 1e-5 bar, so there only the raw sums of the C ABI tell (the valid-document count is an integer, exact in fp32, and is
    off by one).  At 1088 x 256 documents the second stride holds 5.9 % of them: the count, the raw sum and the gradient (which
    divides by the count) all move by about 6 %, far past the bar."""
    first = C.ORD_STRIDE * C.ORD_BLOCK
    cases = [c for c in C.ORDINAL_CASES if C.ordinal_second_stride(c)]
    assert [c.B * c.S for c in cases] == [first + 1, 1088 * C.ORD_BLOCK, first + 1]
    for c in cases:
        p, y, _ = C.ordinal_inputs(c)
        total, count = C.ordinal_sums(O, p, y, c.n, c.pad)
        t1, c1 = C.ordinal_sums(O, p, y, c.n, c.pad, docs=first)
        assert 0 < c1 < count and count - c1 >= 1, c.name                           # the count alone always tells
        if "6pct" in c.name:
            assert (count - c1) / count > 0.05 and abs(total - t1) / total > 0.05, c.name
            assert count / c1 - 1.0 > 0.05                                          # every gradient entry, through the divisor


def test_pad_masks_targets_not_documents():
    """pad = 0 masks every 0 target and pad = 1 every 1 target, while a padded document (label -1) keeps its -1 targets in the loss:
    the reference builds the targets with the default indicator and compares them with `pad`."""
    p = torch.tensor([[[0.3, 0.6], [0.2, 0.9], [0.5, 0.5]]], dtype=torch.float64)
    y = torch.tensor([[1.0, -1.0, 0.0]])
    bce = lambda q, t: -(t * math.log(q) + (1 - t) * math.log(1 - q))
    want = {-1: (bce(.3, 1) + bce(.6, 0) + bce(.5, 0) + bce(.5, 0)) / 2,
            0: (bce(.3, 1) + bce(.2, -1) + bce(.9, -1)) / 2,
            1: (bce(.6, 0) + bce(.2, -1) + bce(.9, -1) + bce(.5, 0) + bce(.5, 0)) / 3}
    for pad, w in want.items():
        assert abs(float(O.ordinal_closed_form(p, y, 2, pad)[0]) - w) < 1e-14
        assert abs(float(torch_ordinal(p, y, 2, pad)[0]) - w) < 1e-14


# ------------------------------------------------------------------------------------------------- reduce_sum
def test_reduce_bound_and_inputs():
    assert C.REDUCE_N == (0, 1, 63, 64, 65, 1023, 1024, 1025, 100003)
    for n in C.REDUCE_N:
        x = C.reduce_input(n)
        assert x.dtype == np.float32 and x.size == max(n, 1)
        if n >= 63:
            assert bool((x < 0).any()) and bool((x > 0).any()) and 1e-3 <= np.abs(x).min() and np.abs(x).max() <= 1e3
        for scale in C.REDUCE_SCALES:
            sabs = float(np.abs(x[:n].astype(np.float64)).sum()) * float(np.float32(scale))
            assert math.isclose(C.reduce_bound(x, n, scale), (math.ceil(n / 1024) + 22 + 1) * 2.0 ** -24 * sabs, rel_tol=1e-14, abs_tol=0.0)
            assert abs(C.reduce_reference(x, n, scale) - float(x[:n].astype(np.float64).sum()) * float(np.float32(scale))) <= 1e-9 * max(sabs, 1e-30)
    assert C.reduce_reference(C.reduce_input(0), 0, 1.0) == 0.0 and C.reduce_bound(C.reduce_input(0), 0, 1.0) == 0.0


# ------------------------------------------------------------------------------------------------- gather
def test_gather_cases_reach_the_loops_they_name():
    by = {c.name: c for c in C.GATHER_CASES}
    assert len(by) == len(C.GATHER_CASES)
    for c in C.GATHER_CASES:
        assert C.gather_kernel_of(c) == c.kernel, c.name
        assert 4 * c.rows * c.row_floats < C.GATHER_MAX_BYTES, c.name
        again = "second-stride" in c.name or "above-the-workgroup-cap" in c.name
        assert (C.gather_strides(c) >= 2) if again else (C.gather_strides(c) == 1), c.name
    assert {c.row_floats for c in C.GATHER_CASES if c.rows == 300} == {2044, 2048, 4092, 4096, 4100, 8192}


def test_gather_indices_and_expected_rows():
    c = C.GatherCase("tiny", 50, 8, False, "narrow")
    src = torch.arange(400.0).view(50, 8)
    sets = C.gather_indices(c)
    perm, none = sets["perm"]
    assert sorted(perm.tolist()) == list(range(50)) and not bool(none.any())
    assert torch.equal(sets["sub"][0], perm[:16])
    mixed, bad = sets["mixed"]
    assert bool((mixed < 0).any()) and int(bad.sum()) == 7 and set(mixed[bad].tolist()) == {50, -51, 55}
    good = ~bad
    assert torch.equal(torch.where(mixed[good] < 0, mixed[good] + 50, mixed[good]), perm[good])
    exp = C.gather_expected(src, mixed, bad)
    assert torch.equal(exp[good], src[perm[good]]) and not bool(exp[bad].any())
