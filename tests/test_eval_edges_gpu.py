"""NDCG@k, the ordinal loss, ltr_reduce_sum_f32 and the gather kernels at the edges of their launch geometry.

Cases and inputs come from tests/eval_edge_cases.py (checked on the CPU by test_eval_edges_cpu.py, which also pins the two oracles:
sort-based ranks == counting ranks, ordinal closed form == torch fp64 BCE with autograd).  Every comparison is against a
high-precision reference of the same operation on the same fp32 inputs, or is bit equality between two forms declared equal:

  NDCG@k      oracle/ltr_metrics_oracle.py in fp64; bar 1e-12 on max|delta| / max|ref| (the sums are fp64 on both sides), the mean too
  ordinal     oracle/ltr_oracle.ordinal_closed_form in fp64 on the widened fp32 probabilities; bar 1e-5
  reduce_sum  math.fsum; the derived bound eval_edge_cases.reduce_bound; a repeated call is bit-equal
  gather      torch.equal with src[idx] on every row

What each parametrize id reaches:
  S63 / S64 / S65          block clamp at 64: one partial wave, the first strided row, nw = 1 / 2 in the cross-wave sum
  S1023 / S1024 / S1025    block clamp at 1024 (nw = 16), a second row per thread from 1025; S2048 / S2049 the third
  S8192 / S8193            64 KiB of dynamic LDS exactly / the hipFuncSetAttribute opt-in; S16384 the limit; 16385 raises
  quant4, all_equal, signed_zero, relevant_last   long tie runs under both tie rules; +0.0 == -0.0
  no_relevant, negative    ideal DCG 0 (the no_relevant value) and below 0 (plain division, as utils/metrics.py does)
  fractional               non-integer labels under both gains
  k1, k(S-1), kS, k(S+7), kNone, and want = dcg: eval_edge_cases.ndcg_options, the full product up to S = 1025
  docs255 / 256 / 257      kOrdBlock; docs262144 / 262145: reduce_pairs_kernel's second stride; n1 .. n64; pad0 / pad1; clamp;
                           upstream3; fp64-labels; all-padded (0 / 0)
  reduce n0 .. n100003     empty wave slots (n < 1024 leaves lanes idle, n <= 64 leaves 15 slots at 0), ceil(n / 1024) terms a thread
  gather *-second-stride, *-above-the-workgroup-cap, the 300-row piece edges
  docs278528-...-6pct      64 partials (5.9 % of the documents) in the second stride; test_ordinal_raw_sums_through_the_c_abi holds the
                           valid-document count exact, so one dropped partial fails at 262145 documents too
The ordinal wrapper does not admit B = 0 or S = 0 (an empty tensor has no data pointer: LTR_ERR_NULL): test_ordinal_rejects_an_empty_batch.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

import eval_edge_cases as C
import ltr_metrics_oracle as MO
import ltr_oracle as O
from conftest import ledger_record, relerr

pytestmark = pytest.mark.gpu
TOL_METRIC, TOL_LOSS = 1e-12, 1e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    import ltr_mi355x
    ltr_mi355x.lib()           # fail loudly if the HIP library is missing
    return torch.device("cuda:0")


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


# ------------------------------------------------------------------------------------------------- NDCG@k, dense
@pytest.mark.parametrize("Q,S,name,kinds", C.ndcg_dense_cases(), ids=[f"Q{c[0]}-S{c[1]}-{c[2]}" for c in C.ndcg_dense_cases()])
def test_ndcg_dense_against_the_oracle(Q, S, name, kinds, dev):
    """ltr_mi355x.metrics.ndcg_at_k on a mixed batch, every option set of eval_edge_cases.ndcg_options(S), per query and the mean."""
    from ltr_mi355x.metrics import ndcg_at_k
    y, s = C.ndcg_batch(Q, S, kinds)
    yd, sd = torch.from_numpy(y.copy()).to(dev), torch.from_numpy(s.copy()).to(dev)
    refs, worst = {}, 0.0
    for o in C.ndcg_options(S):
        what = f"S{S}-{name}-{C.ndcg_opt_id(o)}"
        got = ndcg_at_k(yd, sd, k=o.k, no_relevant=o.no_relevant, gains=o.gains, reverse_ties=o.reverse_ties, want=o.want)
        assert got.dtype == torch.float64 and got.device.type == "cuda" and got.shape == (Q,), what
        got = got.cpu().numpy()
        key = o if o.want == "ndcg" else o._replace(no_relevant=True)          # DCG does not depend on no_relevant
        if key not in refs:
            refs[key] = C.ndcg_reference(MO, y, s, key)
        ref = refs[key]
        assert bool(np.isfinite(ref).all()) and bool(np.isfinite(got).all()), what
        err = relerr(got, ref)
        worst = max(worst, err)
        assert err < TOL_METRIC, (what, err, got, ref)
        # the mean a run reports is numpy's mean of these per-query values (no device code computes it): implied by the line above
        assert abs(got.mean() - ref.mean()) < TOL_METRIC * max(float(np.abs(ref).max()), 1e-30), what
        if o.want == "ndcg":
            for q, kind in enumerate(kinds):
                if kind == "no_relevant":
                    assert got[q] == (1.0 if o.no_relevant else 0.0), what
    ledger_record(f"ndcg_dense [S{S}]", worst, tol=TOL_METRIC, note=name)
    print(f"S{S} {name}: {len(C.ndcg_options(S))} option sets, worst rel_err {worst:.3e}")


def test_ndcg_above_the_limit_raises(dev):
    from ltr_mi355x._lib import LtrError
    from ltr_mi355x.metrics import ndcg_at_k
    S = C.NDCG_S_LIMIT + 1
    y, s = torch.zeros(1, S, device=dev), torch.zeros(1, S, device=dev)
    with pytest.raises(LtrError, match="ltr_ndcg_at_k"):
        ndcg_at_k(y, s, k=5)


# ------------------------------------------------------------------------------------------------- NDCG@k, ragged
@pytest.mark.parametrize("reverse_ties", [False, True], ids=["fwd", "rev"])
@pytest.mark.parametrize("k", C.RAGGED_KS, ids=lambda k: f"k{k}")
def test_ndcg_ragged_on_the_tier_edges(k, reverse_ties, dev):
    """One batch of lengths 1, 2, 63 .. 2048, two queries each (the second heavy-tie): each query against the dense oracle applied to
    that query alone, both gains, NDCG and DCG."""
    from ltr_mi355x import ragged
    y, s, bounds = C.ragged_batch()
    sl = ragged.RaggedSlates(bounds, device=dev)
    yd, sd = torch.from_numpy(y.copy()).to(dev), torch.from_numpy(s.copy()).to(dev)
    worst = 0.0
    for gains in ("linear", "exponential"):
        for want in ("ndcg", "dcg"):
            got = ragged.ndcg_at_k(yd, sd, sl, k=k, no_relevant=False, gains=gains, reverse_ties=reverse_ties, want=want).cpu().numpy()
            ref = np.empty(bounds.size - 1)
            for q in range(bounds.size - 1):
                a, b = int(bounds[q]), int(bounds[q + 1])
                o = C.NdcgOpt(k, gains, False, reverse_ties, want)
                ref[q] = C.ndcg_reference(MO, y[a:b][None], s[a:b][None], o)[0]
            assert bool(np.isfinite(got).all()) and got.shape == ref.shape
            for q in range(ref.size):                                     # per query: a long query's DCG must not hide a short one's
                assert abs(got[q] - ref[q]) <= TOL_METRIC * max(abs(ref[q]), 1e-30), (q, int(np.diff(bounds)[q]), gains, want, got[q], ref[q])
            worst = max(worst, float(np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1e-30))))
    ledger_record("ndcg_ragged (per query)", worst, tol=TOL_METRIC, note=f"k{k}-{'rev' if reverse_ties else 'fwd'}")


@pytest.mark.parametrize("S", C.RAGGED_EQUAL_S, ids=lambda S: f"S{S}")
def test_ndcg_ragged_equals_dense_bit_for_bit(S, dev):
    from ltr_mi355x import metrics, ragged
    y, s = C.ragged_equal_batch(S)
    Q = C.RAGGED_EQUAL_Q
    yd, sd = torch.from_numpy(y.copy()).to(dev), torch.from_numpy(s.copy()).to(dev)
    sl = ragged.RaggedSlates(np.arange(Q + 1, dtype=np.int64) * S, device=dev)
    for k in (1, 10, None):
        for rev in (False, True):
            for want in ("ndcg", "dcg"):
                a = ragged.ndcg_at_k(yd.view(-1), sd.view(-1), sl, k=k, gains="exponential", reverse_ties=rev, want=want)
                b = metrics.ndcg_at_k(yd, sd, k=k, gains="exponential", reverse_ties=rev, want=want)
                assert torch.equal(a, b), (S, k, rev, want)


# ------------------------------------------------------------------------------------------------- ordinal
@pytest.mark.parametrize("c", C.ORDINAL_CASES, ids=lambda c: c.name)
def test_ordinal_against_the_fp64_oracle(c, dev):
    """losses.ordinal.ordinalLoss, loss and gradient (through backward, upstream gradient c.go).  Ordinary documents: max|delta| /
    max|ref| < 1e-5 over them.  Clamp documents (p in {0, 1, smallest normal, a subnormal, 1 - 2^-24}, gradients up to 1e12) would
    hide every ordinary element in that ratio: they are compared element by element, |delta| <= 1e-5 |ref|.  No valid document: the
    loss is NaN on both sides and the gradient 0 on both sides."""
    from losses.ordinal import ordinalLoss
    p, y, clamp = C.ordinal_inputs(c)
    pd = p.to(dev).requires_grad_(True)
    loss = ordinalLoss(pd, y.to(dev), c.n, c.pad)
    (c.go * loss).backward()
    got_l, got_g = float(loss.detach().cpu()), pd.grad.cpu().double()
    rl, rg = O.ordinal_closed_form(p.double(), y, c.n, c.pad)
    rg = rg * c.go
    if C.ordinal_expect_nan(c):
        assert math.isnan(float(rl)) and math.isnan(got_l), (got_l, float(rl))
        assert torch.equal(torch.isnan(got_g), torch.isnan(rg)) and torch.equal(got_g, rg)
        return
    assert math.isfinite(float(rl)) and bool(torch.isfinite(rg).all()) and math.isfinite(got_l) and bool(torch.isfinite(got_g).all())
    e_loss = abs(got_l - float(rl)) / abs(float(rl))
    plain = ~clamp
    e_grad = relerr(got_g[plain].numpy(), rg[plain].numpy())
    ledger_record("ordinal.loss", e_loss, tol=TOL_LOSS, note=c.name)
    ledger_record("ordinal.dpred (ordinary documents)", e_grad, tol=TOL_LOSS, note=c.name)
    print(f"{c.name}: loss rel_err {e_loss:.3e}, ordinary dpred rel_err {e_grad:.3e}")
    assert e_loss < TOL_LOSS, (c.name, got_l, float(rl))
    assert e_grad < TOL_LOSS, c.name
    if c.clamp:
        g, r = got_g[clamp], rg[clamp]
        assert g.shape == (len(C.CLAMP_P), c.n)
        rel = ((g - r).abs() / r.abs().clamp(min=1e-300)).where(r != 0, (g - r).abs())
        ledger_record("ordinal.dpred (clamp documents, element-wise)", float(rel.max()), tol=TOL_LOSS, note=c.name)
        print(f"{c.name}: clamp documents element-wise rel_err {float(rel.max()):.3e}, largest |gradient| {float(r.abs().max()):.3e}")
        assert bool(((g - r).abs() <= TOL_LOSS * r.abs()).all()), (c.name, g, r)


@pytest.mark.parametrize("c", C.ORDINAL_CASES, ids=lambda c: c.name)
def test_ordinal_raw_sums_through_the_c_abi(c, dev):
    """ltr_ordinal_fwd_bwd's own outputs, before any division: sums[1], the number of valid documents, is an integer below 2^24 and so
    exact in fp32 -- it equals the oracle's count bit for bit, which a reduce_pairs_kernel that skipped or misread ONE partial of its
    second stride cannot do; sums[0] against the fp64 sum of the unmasked terms at 1e-5.  The block partials add up to both."""
    from ltr_mi355x._lib import check, lib
    from ltr_mi355x.functional import _stream
    p, y, _ = C.ordinal_inputs(c)
    n_docs = c.B * c.S
    pd, yd = p.to(dev), y.float().to(dev)
    nb = int(lib().ltr_ordinal_num_blocks(n_docs))
    assert nb == -(-n_docs // C.ORD_BLOCK)
    partials = torch.full((2 * nb,), float("nan"), dtype=torch.float32, device=dev)
    sums = torch.full((2,), float("nan"), dtype=torch.float32, device=dev)
    check(lib().ltr_ordinal_fwd_bwd(_p(pd), _p(yd), n_docs, c.n, float(c.pad), _p(partials), _p(sums), None, _stream()), "ltr_ordinal_fwd_bwd")
    total, count = C.ordinal_sums(O, p, y, c.n, c.pad)
    got = sums.cpu().double()
    assert float(got[1]) == float(count), (c.name, float(got[1]), count)
    part = partials.cpu().double().view(nb, 2)
    assert float(part[:, 1].sum()) == float(count), c.name
    if count:
        err = abs(float(got[0]) - total) / abs(total)
        ledger_record("ordinal.sums[0]", err, tol=TOL_LOSS, note=c.name)
        print(f"{c.name}: sums[0] rel_err {err:.3e}, count {count}")
        assert err < TOL_LOSS, (c.name, float(got[0]), total)
        assert abs(float(part[:, 0].sum()) - total) / abs(total) < TOL_LOSS, c.name
    else:
        assert float(got[0]) == 0.0


def test_ordinal_rejects_an_empty_batch(dev):
    """B = 0 or S = 0: an empty tensor has no data pointer, the launcher answers LTR_ERR_NULL and the wrapper raises (the reference
    would return 0 / 0)."""
    from losses.ordinal import ordinalLoss
    from ltr_mi355x._lib import LtrError
    for B, S in ((0, 5), (3, 0)):
        with pytest.raises(LtrError, match="ltr_ordinal_fwd_bwd"):
            ordinalLoss(torch.zeros(B, S, 2, device=dev), torch.zeros(B, S, device=dev), 2)


# ------------------------------------------------------------------------------------------------- reduce_sum
@pytest.mark.parametrize("scale", C.REDUCE_SCALES, ids=["scale1", "scale1over7"])
@pytest.mark.parametrize("n", C.REDUCE_N, ids=lambda n: f"n{n}")
def test_reduce_sum_within_its_derived_bound(n, scale, dev):
    """ltr_reduce_sum_f32 through the C ABI against math.fsum.  reduce_sum_kernel (csrc/ltr_losses.hip) adds ceil(n / 1024) terms a
    thread (`for (i = threadIdx.x; i < n; i += 1024) a += in[i]`), then 6 shuffle levels (`wave_allsum`), then 16 wave slots
    (`for (i = 0; i < 16; ++i) x += red[i]`), then scales (`x * scale`): |err| <= (ceil(n / 1024) + 22 + 1) 2^-24 sum|x| |scale|
    (eval_edge_cases.reduce_bound).  Two calls on one input give the same bits."""
    from ltr_mi355x._lib import check, lib
    from ltr_mi355x.functional import _stream
    x = C.reduce_input(n)
    xd = torch.from_numpy(x).to(dev)
    outs = []
    for _ in range(2):
        out = torch.full((1,), float("nan"), dtype=torch.float32, device=dev)
        check(lib().ltr_reduce_sum_f32(_p(xd), n, float(scale), _p(out), _stream()), "ltr_reduce_sum_f32")
        outs.append(out)
    assert torch.equal(outs[0], outs[1])
    got, ref, bound = float(outs[0]), C.reduce_reference(x, n, scale), C.reduce_bound(x, n, scale)
    err = abs(got - ref)
    print(f"n{n} scale {scale:g}: got {got!r} ref {ref!r} |err| {err:.3e} bound {bound:.3e}")
    sabs = float(np.abs(x[:n].astype(np.float64)).sum()) * abs(float(np.float32(scale)))
    ledger_record("reduce_sum (|err| / sum|x scale|)", err / sabs if sabs else 0.0, tol=bound / sabs if sabs else 0.0, note=f"n{n}-scale{scale:g}")
    if n == 0:
        assert got == 0.0
    assert err <= bound, (n, scale, got, ref, err, bound)


# ------------------------------------------------------------------------------------------------- gather
@pytest.mark.parametrize("c", C.GATHER_CASES, ids=lambda c: c.name)
def test_gather_every_row(c, dev):
    """gather_rows against src[idx] on EVERY row: a permutation, a third of it, and the permutation with negative indices (the same
    rows) and out-of-range ones (zero rows) spread over the whole launch."""
    from ltr_mi355x.data import gather_rows
    host = C.gather_source(c)
    if c.misaligned:
        src = torch.empty(host.numel() + 1, dtype=torch.float32, device=dev)[1:].view(c.rows, c.row_floats)
        src.copy_(host)
        assert src.data_ptr() % 16 == 4
    else:
        src = host.to(dev)
        assert src.data_ptr() % 16 == 0
    for name, (idx, bad) in C.gather_indices(c).items():
        idx_d, bad_d = idx.to(dev), bad.to(dev)
        out = torch.full((idx.numel(), c.row_floats), float("nan"), dtype=torch.float32, device=dev)
        got = gather_rows(src, idx_d, out=out)
        assert got.data_ptr() == out.data_ptr()
        assert torch.equal(got, C.gather_expected(src, idx_d, bad_d)), (c.name, name)
