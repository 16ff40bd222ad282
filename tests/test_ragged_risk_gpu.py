"""GPU: the six risk-sensitive losses on ragged batches (FusedRanker.step_ragged(..., y_base= / base_cols=), ragged.risk_loss,
QueryShardedTrainer.step_ragged) against the fp64 reference of tests/ragged_risk_cases.py.

Bars are the rectangular risk step's (tests/test_risk_fused_gpu.py): loss and every parameter gradient within max(floor, 4 x the fp32
oracle's own deviation from fp64), floor 1e-5 for the Listnet forms and 1e-4 for the Lambda forms, every use ledgered.  The 1e-3 floor
of batches whose fp32 oracle is non-finite is never taken: tests/test_ragged_risk_cpu.py checks every case used here for that, and
_bars asserts it again."""
import os
import socket
import sys
import tempfile

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import ragged_cases as RC
import ragged_risk_cases as RR
from conftest import ledger_record
from test_risk_fused_gpu import _assert_grads, _assert_loss, _floor

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    import ltr_mi355x
    ltr_mi355x.lib()
    return torch.device("cuda:0")


def _slates(lengths, dev):
    from ltr_mi355x.ragged import RaggedSlates
    return RaggedSlates(RC.bounds_of(lengths), device=dev)


def _grads(net, geom):
    if geom == "fc136":
        return {str(i): p.grad.detach().cpu().numpy() for i, p in enumerate(net._ltr_params())}
    return {k: p.grad.detach().cpu().numpy() for k, p in net.named_parameters()}


def _bars(name, rl32, rg32):
    fl = _floor(name, rl32, rg32)
    assert fl < 1e-3, "the fp32 oracle of a case of this file is non-finite (tests/test_ragged_risk_cpu.py checks every case)"
    return fl


# ---------------------------------------------------------------------------------------------------- 6. the step
@pytest.mark.parametrize("case", RR.STEP_CASES, ids=RR.step_case_id)
def test_step_ragged_vs_oracle(case, dev):
    from ltr_mi355x.scorer import FusedRanker
    name, geom, batch, train = case
    lengths, x, y, yb, keep = RR.step_data(case)
    bounds = RC.bounds_of(lengths)
    net, params = RR.make_net(geom, dev)
    kw = {}
    if train:
        net.train()
        kw = dict(keep1=keep[0].to(dev), keep2=keep[1].to(dev))
    ranker = FusedRanker(net, loss=name)
    out = float(ranker.step_ragged(x.to(dev), y.to(dev), _slates(lengths, dev), y_base=yb.to(dev), **kw))
    rl, rg = RR.step_oracle(name, geom, params, x, y, yb, bounds, dict(ranker.risk.args), keep)
    rl32, rg32 = RR.step_oracle(name, geom, params, x, y, yb, bounds, dict(ranker.risk.args), keep, dtype=torch.float32)
    print(f"[{RR.step_case_id(case)}] loss {out:.9g} fp64 {rl:.9g} fp32 {rl32:.9g}")
    _bars(name, rl32, rg32)
    _assert_loss(name, out, rl, rl32)
    _assert_grads(name, _grads(net, geom), rg, rg32)
    for p, gv in zip(ranker.params, ranker._grad_views):
        assert p.grad is gv


# ---------------------------------------------------------------------------------------------------- 7. equal lengths: same bits
def _rect_step(ranker, geom, *a, **kw):
    # The folded make_model ranker's `step` sends the Listnet forms at S in {32, 64, 128} through the one-pass tile kernel, which agrees
    # with the launch chain to 1e-5 only (tests/test_linear_risk_gpu.py::test_one_pass_agrees_with_the_chain); step_ragged takes the
    # chain, so the bitwise twin is `step` on its chain route.
    if geom == "fc136":
        kw["_one_pass"] = False
    return ranker.step(*a, **kw)


@pytest.mark.parametrize("S", [17, 128, 257, 1025])
@pytest.mark.parametrize("geom", RR.GEOMS)
@pytest.mark.parametrize("name,args", [("geoRiskLambdaLoss", {}), ("zRiskListnetLoss", dict(listnet_transformation=3, return_strategy=3)),
                                       ("tRiskLambdaLoss", {}), ("tRiskListnetLoss", dict(listnet_transformation=2)),
                                       ("zRiskLambdaLoss", dict(listnet_transformation=2, add_ideal_ranking_to_mat=2)),
                                       ("geoRiskListnetLoss", dict(add_ideal_ranking_to_mat=2))],
                         ids=lambda v: v if isinstance(v, str) else "-".join(f"{k[:6]}{a}" for k, a in v.items()))
def test_equal_lengths_are_the_rectangular_step_bits(name, args, geom, S, dev):
    from ltr_mi355x.scorer import FusedRanker
    Q = 5
    x, _, y, yb = RR.data(name, [S] * Q, 900 + S, F=136)
    X, Y, YB = x.to(dev), y.to(dev), yb.to(dev)
    sl = _slates([S] * Q, dev)
    net, _ = RR.make_net(geom, dev)
    ranker = FusedRanker(net, loss=name, risk_args=args)
    _rect_step(ranker, geom, X.view(Q, S, 136), Y.view(Q, S), y_base=YB.view(Q, S, -1) if YB.dim() == 2 else YB.view(Q, S))
    a = ranker.flat.clone()
    assert torch.isfinite(a).all() and float(a[:-1].abs().max()) > 0.0
    ranker.flat.zero_()
    ranker.step_ragged(X, Y, sl, y_base=YB)
    assert torch.equal(a, ranker.flat), "y_base"
    # cached columns: rectangular and ragged
    cols = ranker.baseline_columns(Y.view(Q, S), YB.view(Q, S, -1) if YB.dim() == 2 else YB.view(Q, S))
    _rect_step(ranker, geom, X.view(Q, S, 136), Y.view(Q, S), base_cols=cols)
    b = ranker.flat.clone()
    ent, ics = ranker.baseline_columns_ragged(Y, YB, sl)
    if ranker.risk.lam:
        assert torch.equal(torch.cat([ent, ics.view(Q, S)], 1), cols)
    else:
        assert ics is None and torch.equal(ent, cols)
    ranker.flat.zero_()
    ranker.step_ragged(X, Y, sl, base_cols=(ent, ics))
    assert torch.equal(b, ranker.flat), "base_cols"


# ---------------------------------------------------------------------------------------------------- 8. / 10. cached columns, permutation
MIXED = [40, 3, 129, 17, 64, 260, 2, 90, 1030, 300]


@pytest.mark.parametrize("geom", ["double136", "fc136"])
@pytest.mark.parametrize("name,args", [("geoRiskLambdaLoss", {}), ("geoRiskLambdaLoss", dict(listnet_transformation=2, add_ideal_ranking_to_mat=2)),
                                       ("zRiskLambdaLoss", dict(listnet_transformation=2, add_ideal_ranking_to_mat=2, return_strategy=2)),
                                       ("tRiskLambdaLoss", dict(listnet_transformation=3)), ("geoRiskListnetLoss", dict(add_ideal_ranking_to_mat=2)),
                                       ("zRiskListnetLoss", dict(listnet_transformation=3, return_strategy=3)), ("tRiskListnetLoss", {})],
                         ids=lambda v: v if isinstance(v, str) else "-".join(f"{k[:6]}{a}" for k, a in v.items()))
def test_base_cols_step_and_permutation_on_mixed_lengths(name, args, geom, dev):
    from ltr_mi355x import ragged
    from ltr_mi355x._lib import lib
    from ltr_mi355x.data import gather_rows
    from ltr_mi355x.scorer import FusedRanker
    x, s, y, yb = RR.data(name, MIXED, 61, F=136)
    X, Y, YB = x.to(dev), y.to(dev), yb.to(dev)
    sl = _slates(MIXED, dev)
    Q, n = sl.n_queries, sl.n_docs
    net, _ = RR.make_net(geom, dev)
    ranker = FusedRanker(net, loss=name, risk_args=args)
    l1 = float(ranker.step_ragged(X, Y, sl, y_base=YB))
    g1 = ranker.flat_grad.clone()
    ent, ics = ranker.baseline_columns_ragged(Y, YB, sl)
    assert ent.shape[0] == Q and (ics is None) == (not ranker.risk.lam)
    l2 = float(ranker.step_ragged(X, Y, sl, base_cols=(ent, ics)))
    g2 = ranker.flat_grad.clone()
    assert abs(l1 - l2) <= 1e-6 * abs(l1), (l1, l2)
    assert float((g1 - g2).abs().max()) <= 1e-6 * float(g1.abs().max())
    # the matrix the tail sees
    spec = ranker.risk
    yb2 = ragged.risk_baselines(spec, n, YB)
    nsys = 1 + spec.n_const(yb2.shape[1])
    sc = s.to(dev)
    m1, m2 = (torch.full((Q, nsys), -7.0, device=dev) for _ in range(2))
    j1, j2 = (torch.full((n,), -7.0, device=dev) for _ in range(2))
    ragged.risk_matrix(lib(), spec, sl, sc, Y, yb2, None, m1, j1)
    ragged.risk_matrix(lib(), spec, sl, sc, Y, None, ragged.risk_cached(spec, sl, (ent, ics)), m2, j2)
    assert torch.equal(m1, m2) and torch.equal(j1, j2)
    assert torch.isfinite(m1).all() and torch.isfinite(j1).all()
    # queries in another order carry their own columns: same loss within 1e-6 (the tail sums in query order: not bitwise)
    perm = np.random.default_rng(5).permutation(Q)
    sl2, idx = sl.permuted(perm)
    Xp, Yp = gather_rows(X, idx), gather_rows(Y[:, None], idx)[:, 0]
    YBp = gather_rows(YB if YB.dim() == 2 else YB[:, None], idx)
    entp = ent[torch.as_tensor(perm, device=dev)]
    icsp = None if ics is None else gather_rows(ics[:, None], idx)[:, 0]
    l3 = float(ranker.step_ragged(Xp, Yp, sl2, y_base=YBp))
    g3 = ranker.flat_grad.clone()
    l4 = float(ranker.step_ragged(Xp, Yp, sl2, base_cols=(entp, icsp)))
    g4 = ranker.flat_grad.clone()
    top = float(g1.abs().max())
    for l, g in ((l3, g3), (l4, g4)):
        assert abs(l - l1) <= 1e-6 * abs(l1), (l, l1)
        assert float((g - g1).abs().max()) <= 1e-6 * top


# ---------------------------------------------------------------------------------------------------- 9. the autograd node
@pytest.mark.parametrize("case", RR.LOSS_CASES, ids=lambda c: c[0] + "".join(f"-{k[:6]}{v}" for k, v in c[3].items()))
def test_risk_loss_vs_oracle(case, dev):
    from ltr_mi355x import ragged
    name, lengths, seed, args = case
    _, s, y, yb = RR.data(name, lengths, seed)
    bounds = RC.bounds_of(lengths)

    def ref(dtype):
        x = s.clone().requires_grad_(True)
        out = RR.ragged_risk_oracle(name, x, y, yb, bounds, dtype, **args).sum()
        out.backward()
        return float(out), {"dscores": x.grad.numpy()}

    rl, rg = ref(torch.float64)
    rl32, rg32 = ref(torch.float32)
    _bars(name, rl32, rg32)
    x = s.to(dev).requires_grad_(True)
    out = getattr(ragged, name)(x, y.to(dev), _slates(lengths, dev), yb.to(dev), **args)
    assert out.shape == (1,)
    out.sum().backward()
    _assert_loss(name, float(out), rl, rl32)
    _assert_grads(name, {"dscores": x.grad.cpu().numpy()}, rg, rg32)


@pytest.mark.parametrize("name", RR.LOSSES)
def test_risk_loss_backward_uses_forward_time_state(name, dev):
    """One autograd node whose backward reads only what its forward saved: scores, labels, baselines and the slates' device arrays
    overwritten between forward and backward leave the forward-time gradient."""
    from ltr_mi355x import ragged
    lengths = RR.LOSS_LENGTHS
    _, s, y, yb = RR.data(name, lengths, 56)
    x = s.to(dev).requires_grad_(True)
    ragged.risk_loss(name, x, y.to(dev), _slates(lengths, dev), yb.to(dev)).sum().backward()
    want = x.grad.cpu()
    assert float(want.abs().max()) > 0.0
    sl, yy, ybb = _slates(lengths, dev), y.to(dev), yb.to(dev)
    x0 = s.to(dev).requires_grad_(True)
    xx = x0 * 1.0                                   # a non-leaf the test may overwrite in place
    out = ragged.risk_loss(name, xx, yy, sl, ybb)
    assert out.grad_fn is not None and out.grad_fn.next_functions[0][0] is xx.grad_fn       # one node
    with torch.no_grad():
        xx.mul_(-3.0)
        yy.fill_(1.0)
        ybb.zero_()
        sl.offsets.zero_()
        sl.order.zero_()
    out.sum().backward()
    assert torch.equal(x0.grad.cpu(), want)


# ---------------------------------------------------------------------------------------------------- 12. untouched rows
@pytest.mark.parametrize("kernel", ["colsum", "model", "bwd"])
def test_lambda_tier_launches_leave_other_queries_untouched(kernel, dev):
    """The index list and the tier rule of the three per-tier launches: a query that is not listed, and a listed one outside the
    launch's tier (3 documents in the 17..32 tier), keep every row; the misfit's model entry is poisoned."""
    from ltr_mi355x import lib
    from ltr_mi355x.risk_step import RiskSpec
    h = lib()
    lengths = [20, 17, 3, 31, 25, 18, 32]
    bounds = RC.bounds_of(lengths)
    _, s, y, yb = RR.data("geoRiskLambdaLoss", lengths, 88)
    sl = _slates(lengths, dev)
    S_, Y, YB = s.to(dev), y.to(dev), yb.to(dev).contiguous()
    listed = [1, 2, 4, 6]
    q = torch.tensor(listed, dtype=torch.int32, device=dev)
    largs = RiskSpec("geoRiskLambdaLoss").largs
    CAN = -12345.0
    n, Q, nb = sl.n_docs, sl.n_queries, RR.NB
    st = torch.cuda.current_stream().cuda_stream
    off = sl.offsets.data_ptr()
    cs = torch.full((nb + 2, n), CAN, device=dev)
    mat = torch.full((Q, 1 + nb), CAN, device=dev)
    jac = torch.full((n,), CAN, device=dev)
    ds = torch.full((n,), CAN, device=dev)
    if kernel == "colsum":
        rc = h.ltr_lambda_colsum_sys_ragged_fwd(S_.data_ptr(), Y.data_ptr(), YB.data_ptr(), off, q.data_ptr(), len(listed), 32, n, nb, *largs,
                                                cs.data_ptr(), st)
        rows = cs.cpu()
    elif kernel == "model":
        ent, ics = torch.rand(Q, nb, device=dev), torch.rand(n, device=dev)
        rc = h.ltr_lambda_risk_model_ragged_fwd(S_.data_ptr(), Y.data_ptr(), ent.data_ptr(), nb, ics.data_ptr(), nb, off, q.data_ptr(),
                                                len(listed), 32, n, *largs, 1, mat.data_ptr(), jac.data_ptr(), st)
        rows = jac.cpu()[None]
    else:
        coef, up = torch.rand(Q, 1 + nb, device=dev), torch.rand(n, device=dev)
        rc = h.ltr_lambda_colsum_sys_ragged_bwd_coef(S_.data_ptr(), Y.data_ptr(), off, q.data_ptr(), len(listed), 32, n, *largs,
                                                     up.data_ptr(), coef.data_ptr(), 1 + nb, ds.data_ptr(), st)
        rows = ds.cpu()[None]
    assert rc == 0
    torch.cuda.synchronize()
    for i in range(Q):
        r = rows[:, bounds[i]:bounds[i + 1]]
        if i in listed and lengths[i] > 16:
            assert bool((r != CAN).all()) and bool(torch.isfinite(r).all()), i
        else:
            assert bool((r == CAN).all()), i                 # not listed, or listed outside the tier
    if kernel == "model":
        m = mat.cpu()
        for i in range(Q):
            if i == 2:
                assert bool(torch.isnan(m[i, 0])) and bool((m[i, 1:] == CAN).all())
            elif i in listed:
                assert bool(torch.isfinite(m[i]).all()) and bool((m[i] != CAN).all())
            else:
                assert bool((m[i] == CAN).all())


def test_batch_launches_honour_the_index_list_and_the_length_bound(dev):
    """ltr_risk_matrix_ragged_fwd / ltr_risk_scores_grad_ragged: one launch, any lengths up to s_max; queries that are not listed and a
    listed one longer than s_max keep their rows (the long one's model entry is poisoned)."""
    from ltr_mi355x import lib
    h = lib()
    lengths = [20, 300, 3, 31, 64]
    bounds = RC.bounds_of(lengths)
    _, s, y, yb = RR.data("geoRiskListnetLoss", lengths, 89)
    sl = _slates(lengths, dev)
    S_, Y, YB = s.to(dev), y.to(dev), yb.to(dev).contiguous()
    listed = [0, 1, 2, 4]
    q = torch.tensor(listed, dtype=torch.int32, device=dev)
    CAN = -12345.0
    n, Q, nb = sl.n_docs, sl.n_queries, RR.NB
    st = torch.cuda.current_stream().cuda_stream
    mat = torch.full((Q, 1 + nb), CAN, device=dev)
    jac = torch.full((n,), CAN, device=dev)
    ds = torch.full((n,), CAN, device=dev)
    assert h.ltr_risk_matrix_ragged_fwd(Y.data_ptr(), S_.data_ptr(), YB.data_ptr(), sl.offsets.data_ptr(), q.data_ptr(), len(listed), 64, n,
                                        nb, 0, 1, 0, 0, None, 0, mat.data_ptr(), jac.data_ptr(), st) == 0
    coef = torch.rand(Q, 1 + nb, device=dev)
    assert h.ltr_risk_scores_grad_ragged(jac.data_ptr(), coef.data_ptr(), 1 + nb, sl.offsets.data_ptr(), q.data_ptr(), len(listed), n,
                                         ds.data_ptr(), st) == 0
    torch.cuda.synchronize()
    m, j, d, c = mat.cpu(), jac.cpu(), ds.cpu(), coef.cpu()
    for i in range(Q):
        rj, rd = j[bounds[i]:bounds[i + 1]], d[bounds[i]:bounds[i + 1]]
        if i == 1:                                          # listed, 300 > s_max = 64
            assert bool(torch.isnan(m[i, 0])) and bool((m[i, 1:] == CAN).all()) and bool((rj == CAN).all())
        elif i in listed:
            assert bool(torch.isfinite(m[i]).all()) and bool((m[i] != CAN).all()) and bool((rj != CAN).all())
            assert torch.equal(rd, rj * c[i, 0])
        else:
            assert bool((m[i] == CAN).all()) and bool((rj == CAN).all()) and bool((rd == CAN).all())


def test_padded_rows_of_the_gathered_blocks_are_not_touched(dev):
    """The data-parallel tail over ragged-step rows: two blocks of 4 + 3 rows padded to 4; the padded row is neither read (a NaN
    there changes nothing) nor written, and value / gradient are the dense matrix's bits."""
    from ltr_mi355x import lib, ragged
    from ltr_mi355x import risk_step as RS
    from ltr_mi355x.risk_step import RiskSpec
    h = lib()
    lengths = [40, 3, 129, 17, 64, 260, 2]
    _, s, y, yb = RR.data("geoRiskListnetLoss", lengths, 90)
    for name in ("geoRiskListnetLoss", "tRiskListnetLoss"):
        spec = RiskSpec(name)
        sl = _slates(lengths, dev)
        ybd = ragged.risk_baselines(spec, sl.n_docs, (yb.mean(dim=1) if spec.t else yb).to(dev))
        nsys = 1 + spec.n_const(ybd.shape[1])
        mat = torch.empty(7, nsys, device=dev)
        ragged.risk_matrix(h, spec, sl, s.to(dev), y.to(dev), ybd, None, mat, torch.empty(sl.n_docs, device=dev))
        v1, d1 = torch.empty(1, device=dev), torch.empty(7, nsys, device=dev)
        RS.tail(h, spec, mat, 7, nsys, v1, d1)
        stride = 1 + 4 * nsys
        blocks = torch.full((2, stride), float("nan"), device=dev)
        blocks[0, 0], blocks[1, 0] = 4.0, 3.0
        blocks[0, 1:] = mat[:4].reshape(-1)
        blocks[1, 1:1 + 3 * nsys] = mat[4:].reshape(-1)
        CAN = -12345.0
        dblk = torch.full((2, stride), CAN, device=dev)
        v2 = torch.empty(1, device=dev)
        RS.tail_blocks(h, spec, blocks, 2, 4, nsys, v2, dblk)
        torch.cuda.synchronize()
        assert torch.equal(v1, v2) and bool(torch.isfinite(v1).all())
        assert torch.equal(dblk[0, 1:].view(4, nsys), d1[:4]) and torch.equal(dblk[1, 1:1 + 3 * nsys].view(3, nsys), d1[4:])
        assert bool((dblk[1, 1 + 3 * nsys:] == CAN).all()) and bool((dblk[:, 0] == CAN).all())


# ---------------------------------------------------------------------------------------------------- 5. (device side) / errors
def test_step_ragged_risk_errors(dev):
    from ltr_mi355x.scorer import FusedRanker
    net, _ = RR.make_net("double136", dev)
    x, _, y, yb = RR.data("geoRiskListnetLoss", [4, 9], 8, F=136)
    sl = _slates([4, 9], dev)
    X, Y, YB = x.to(dev), y.to(dev), yb.to(dev)
    r = FusedRanker(net, loss="geoRiskListnetLoss")
    with pytest.raises(NotImplementedError, match="FusedRanker.step"):
        r.step_ragged(X, Y, sl)
    with pytest.raises(ValueError, match="exactly one"):
        r.step_ragged(X, Y, sl, y_base=YB, base_cols=r.baseline_columns_ragged(Y, YB, sl))
    with pytest.raises(ValueError, match="query 1 has 1 document"):
        r.step_ragged(X[:5], Y[:5], _slates([4, 1], dev), y_base=YB[:5])
    with pytest.raises(NotImplementedError, match="at least 2 queries"):
        r.step_ragged(X[:4], Y[:4], _slates([4], dev), y_base=YB[:4])
    with pytest.raises(ValueError, match="y_base"):
        r.step_ragged(X, Y, sl, y_base=YB[:, :1])
    with pytest.raises(TypeError, match="risk-sensitive"):
        FusedRanker(net, loss="listnet").step_ragged(X, Y, sl, y_base=YB)
    assert np.isfinite(float(r.step_ragged(X, Y, sl, y_base=YB)))


# ---------------------------------------------------------------------------------------------------- 11. two ranks
DP_LENGTHS = [40, 3, 129, 17, 64, 260, 2]


def _dp_data(name):
    x, _, y, yb = RR.data(name if name in RR.LOSSES else "geoRiskListnetLoss", DP_LENGTHS, 21, F=136)
    return x, y, yb


def _dp_ranker(name, dev):
    sys.path.insert(0, os.path.join(ROOT, "nn-with-pytorch-personalized-losses_amd"))
    from ltr_mi355x.scorer import FusedRanker
    net, _ = RR.make_net("double136", dev, seed=2021)
    if name in RR.LOSSES:
        return net, FusedRanker(net, loss=name, risk_args=dict(alpha=3.0))
    return net, FusedRanker(net, loss=name)


def _worker(rank, world, port, out_dir, name, mode):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    dev = torch.device("cuda:0")
    from ltr_mi355x.dp import QueryShardedTrainer, shard_range
    from ltr_mi355x.ragged import RaggedSlates
    net, ranker = _dp_ranker(name, dev)
    tr = QueryShardedTrainer(ranker, torch.optim.SGD(net.parameters(), lr=0.0))
    x, y, yb = _dp_data(name)
    whole = RaggedSlates(RC.bounds_of(DP_LENGTHS), device=dev)
    lo, hi = shard_range(len(DP_LENGTHS), rank, world)
    d0, d1 = whole.doc_range(lo, hi)
    sl = whole.batch(lo, hi)
    extra = dict(y_base=yb[d0:d1].to(dev)) if name in RR.LOSSES else {}
    gb = len(DP_LENGTHS) if mode == "global_batch" else None
    loss = float(tr.step_ragged(x[d0:d1].to(dev), y[d0:d1].to(dev), sl, global_batch=gb, **extra))
    torch.save({"loss": loss, "flat": ranker.flat.cpu(), "rows": hi - lo}, os.path.join(out_dir, f"rank{rank}.pt"))
    dist.destroy_process_group()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.timeout(600)
@pytest.mark.parametrize("name,mode", [("geoRiskLambdaLoss", "global_batch"), ("geoRiskLambdaLoss", "size_exchange"),
                                       ("tRiskListnetLoss", "global_batch"), ("tRiskListnetLoss", "size_exchange"),
                                       ("approxNDCG", "size_exchange")])
def test_two_ranks_unequal_shards_equal_single_process(name, mode):
    assert torch.cuda.is_available()
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(_worker, args=(2, _free_port(), d, name, mode), nprocs=2, join=True)
        r = [torch.load(os.path.join(d, f"rank{k}.pt"), weights_only=True) for k in range(2)]
    assert [x["rows"] for x in r] == [4, 3]
    dev = torch.device("cuda:0")
    net, ranker = _dp_ranker(name, dev)
    x, y, yb = _dp_data(name)
    extra = dict(y_base=yb.to(dev)) if name in RR.LOSSES else {}
    ref_loss = float(ranker.step_ragged(x.to(dev), y.to(dev), _slates(DP_LENGTHS, dev), **extra))
    ref = ranker.flat_grad.cpu()
    assert r[0]["loss"] == r[1]["loss"]                      # every rank returns the same global loss
    assert torch.equal(r[0]["flat"], r[1]["flat"])
    assert abs(r[0]["loss"] - ref_loss) <= 1e-6 * abs(ref_loss), (r[0]["loss"], ref_loss)
    top = float(ref.abs().max())
    assert top > 0.0 and float((r[0]["flat"][:-1] - ref).abs().max()) <= 1e-6 * top
