"""GPU: the ragged path (queries of unequal length, no padding) against the fp64 oracle called per query.

Every comparison is loss and d loss / d scores in max-norm (conftest.relerr) at the project bar TOL = 1e-5; parameter gradients of a
step go through assert_grads(..., ref32=...).  lambdaLoss inputs come from the clamp-band rule of tests/lambda_tier_cases.py: every
query gets the first ladder rung with an empty band, asserted before comparing; no pair is ever left out."""
import numpy as np
import pytest
import torch

import lambda_tier_cases as LT
import ltr_metrics_oracle as MO
import ltr_oracle as O
import ragged_cases as RC
from conftest import ledger_record
from conftest import relerr as _relerr
from test_scorer_gpu import _make, _oracle_step, assert_grads

pytestmark = pytest.mark.gpu
TOL = 1e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    import ltr_mi355x
    ltr_mi355x.lib()
    return torch.device("cuda:0")


def relerr(a, b, quantity):
    e = _relerr(a, b)
    print(f"{quantity}: rel err {e:.3e}")
    ledger_record(quantity, e)
    return e


def _slates(lengths, dev):
    from ltr_mi355x.ragged import RaggedSlates
    return RaggedSlates(RC.bounds_of(lengths), device=dev)


BATCHES = {"tiers": RC.tier_lengths(), "mslr_like": RC.mslr_like_lengths(48, 7, hi=700)}


def _run(fn, s, dev):
    x = s.to(dev).requires_grad_(True)
    out = fn(x)
    out.backward()
    return float(out), x.grad.cpu()


# ---------------------------------------------------------------------------------------------------- 1. / 2. losses
@pytest.mark.parametrize("batch", list(BATCHES))
def test_approxndcg_vs_per_query_oracle(batch, dev):
    from ltr_mi355x import ragged
    lengths = BATCHES[batch]
    assert batch != "tiers" or sorted(lengths) == sorted(LT.TIER_S)
    s, y = RC.random_batch(lengths, 100)
    ref = RC.oracle_ragged("approxNDCG", s, y, RC.bounds_of(lengths))
    sl = _slates(lengths, dev)
    loss, g = _run(lambda x: ragged.approx_ndcg(x, y.to(dev), sl), s, dev)
    assert relerr(loss, float(ref["loss"]), "ragged approxNDCG loss") < TOL
    assert relerr(g, ref["grad"], "ragged approxNDCG dscores") < TOL


@pytest.mark.parametrize("batch", list(BATCHES))
@pytest.mark.parametrize("apply_sigmoid", [False, True])
def test_listnet_vs_per_query_oracle(batch, apply_sigmoid, dev):
    from ltr_mi355x import ragged
    lengths = BATCHES[batch]
    s, y = RC.random_batch(lengths, 101)
    ref = RC.oracle_ragged("listnet", s, y, RC.bounds_of(lengths), apply_sigmoid=apply_sigmoid)
    sl = _slates(lengths, dev)
    loss, g = _run(lambda x: ragged.listnet(y.to(dev), x, sl, apply_sigmoid=apply_sigmoid), s, dev)
    assert relerr(loss, float(ref["loss"]), "ragged listnet loss") < TOL
    assert relerr(g, ref["grad"], "ragged listnet dscores") < TOL


@pytest.mark.parametrize("batch", list(BATCHES))
@pytest.mark.parametrize("opt", LT.REQUIRED_OPTS)
@pytest.mark.parametrize("scheme", O.SCHEMES)
def test_lambda_vs_per_query_oracle(scheme, opt, batch, dev):
    from ltr_mi355x import ragged
    lengths = BATCHES[batch]
    s, y, kw = RC.band_free_batch(lengths, scheme, opt)            # asserts the empty clamp band per query
    bounds = RC.bounds_of(lengths)
    sl = _slates(lengths, dev)
    ref = RC.oracle_ragged("lambdaLoss", s, y, bounds, **kw)       # sum form; the mean is the same sums over the total count
    n_kept = int(ref["count"].sum())
    for red in ("sum", "mean"):
        loss, g = _run(lambda x: ragged.lambda_loss(x, y.to(dev), sl, reduction=red, **kw), s, dev)
        div = 1.0 if red == "sum" else float(n_kept)
        assert n_kept > 0
        assert relerr(loss, float(ref["loss"]) / div, f"ragged lambdaLoss {red} loss") < TOL
        assert relerr(g, ref["grad"] / div, f"ragged lambdaLoss {red} dscores") < TOL


def test_lambda_mean_of_nothing_and_k0(dev):
    from ltr_mi355x import ragged
    lengths = [3, 70, 1, 300]
    sl = _slates(lengths, dev)
    s = torch.randn(sum(lengths))
    y = torch.full((sum(lengths),), 2.0)                             # uniform labels: no kept pair
    loss, g = _run(lambda x: ragged.lambda_loss(x, y.to(dev), sl, weighing_scheme="ndcgLoss2PP_scheme", reduction="mean"), s, dev)
    assert np.isnan(loss) and float(g.abs().max()) == 0.0
    loss, g = _run(lambda x: ragged.lambda_loss(x, y.to(dev), sl, weighing_scheme="ndcgLoss2PP_scheme", reduction="sum"), s, dev)
    assert loss == 0.0 and float(g.abs().max()) == 0.0
    y = torch.randint(0, 5, (sum(lengths),)).float()
    loss, g = _run(lambda x: ragged.lambda_loss(x, y.to(dev), sl, k=0), s, dev)
    assert loss == 0.0 and float(g.abs().max()) == 0.0


def test_padding_label_inside_a_ragged_query_is_masked(dev):
    from ltr_mi355x import ragged
    lengths = [9, 40, 130, 300]
    s, y = RC.random_batch(lengths, 55)
    bounds = RC.bounds_of(lengths)
    for q in range(len(lengths)):
        y[bounds[q + 1] - 2] = -1.0
    sl = _slates(lengths, dev)
    ref = RC.oracle_ragged("approxNDCG", s, y, bounds)
    loss, g = _run(lambda x: ragged.approx_ndcg(x, y.to(dev), sl), s, dev)
    assert relerr(loss, float(ref["loss"]), "ragged approxNDCG (pad inside) loss") < TOL
    assert relerr(g, ref["grad"], "ragged approxNDCG (pad inside) dscores") < TOL
    assert float(g[y == -1.0].abs().max()) == 0.0
    kw = dict(weighing_scheme="ndcgLoss2PP_scheme", k=None, sigma=1.0, mu=10.0, reduction_log="binary")
    ref = RC.oracle_ragged("lambdaLoss", s, y, bounds, **kw)
    loss, g = _run(lambda x: ragged.lambda_loss(x, y.to(dev), sl, **kw), s, dev)
    assert relerr(loss, float(ref["loss"]), "ragged lambdaLoss (pad inside) loss") < TOL
    assert relerr(g, ref["grad"], "ragged lambdaLoss (pad inside) dscores") < TOL


def test_backward_uses_forward_time_state(dev):
    """One autograd node per loss whose backward reads only what its forward saved: changing scores, labels or the slates' device
    arrays between forward and backward leaves the forward-time gradient."""
    from ltr_mi355x import ragged
    lengths = [9, 40, 130, 300]
    s, y = RC.random_batch(lengths, 56)
    calls = {"approx": lambda x, yy, sl: ragged.approx_ndcg(x, yy, sl),
             "listnet": lambda x, yy, sl: ragged.listnet(yy, x, sl),
             "lambda": lambda x, yy, sl: ragged.lambda_loss(x, yy, sl, weighing_scheme="ndcgLoss2PP_scheme", reduction="mean")}
    for name, fn in calls.items():
        _, want = _run(lambda x: fn(x, y.to(dev), _slates(lengths, dev)), s, dev)
        sl, yy = _slates(lengths, dev), y.to(dev)
        x0 = s.to(dev).requires_grad_(True)
        x = x0 * 1.0                                   # a non-leaf the test may overwrite in place
        out = fn(x, yy, sl)
        assert out.grad_fn is not None and out.grad_fn.next_functions[0][0] is x.grad_fn, name     # one node
        with torch.no_grad():
            x.mul_(-3.0)
            yy.fill_(1.0)
            sl.offsets.zero_()
            sl.order.zero_()
        out.backward()
        assert torch.equal(x0.grad.cpu(), want), name


# ---------------------------------------------------------------------------------------------------- 3. rectangular agreement
def _raw(dev, name, sl, s, y, *args, ds=True):
    """One raw ragged launch over ALL queries (queries = NULL): (slate_loss [Q], count [Q] or None, dscores)."""
    from ltr_mi355x import lib
    h = lib()
    Q, n = sl.n_queries, sl.n_docs
    slate = torch.full((Q,), -7.0, device=dev)
    cnt = torch.full((Q,), -7.0, device=dev)
    d = torch.full((n,), -7.0, device=dev) if ds else None
    st = torch.cuda.current_stream().cuda_stream
    dp = d.data_ptr() if ds else None
    if name == "approx":
        rc = h.ltr_approxndcg_ragged_fwd_bwd(s.data_ptr(), y.data_ptr(), sl.offsets.data_ptr(), None, Q, sl.max_len, *args, slate.data_ptr(),
                                             dp, st)
    elif name == "listnet":
        rc = h.ltr_listnet_ragged_fwd_bwd(y.data_ptr(), s.data_ptr(), sl.offsets.data_ptr(), None, Q, sl.max_len, *args, slate.data_ptr(),
                                          dp, st)
    else:
        rc = h.ltr_lambda_ragged_fwd_bwd(s.data_ptr(), y.data_ptr(), sl.offsets.data_ptr(), None, Q, sl.max_len, *args, slate.data_ptr(),
                                         cnt.data_ptr(), dp, st)
    assert rc == 0
    torch.cuda.synchronize()
    return slate, cnt, d


@pytest.mark.parametrize("S", [17, 128, 257, 1025])
def test_equal_lengths_are_the_rectangular_bits(S, dev):
    """All lengths equal to S: the ragged launch is the rectangular launch's slate function, group size and reduction order."""
    from ltr_mi355x import lib
    h = lib()
    Q = 5
    sl = _slates([S] * Q, dev)
    g = torch.Generator().manual_seed(700 + S)
    s = (torch.randn(Q * S, generator=g) * 2).to(dev)
    y = torch.randint(0, 5, (Q * S,), generator=g).float().to(dev)
    st = torch.cuda.current_stream().cuda_stream

    def rect(name, *args):
        slate, cnt, d = torch.empty(Q, device=dev), torch.empty(Q, device=dev), torch.empty(Q * S, device=dev)
        if name == "approx":
            rc = h.ltr_approxndcg_fwd_bwd(s.data_ptr(), y.data_ptr(), Q, S, *args, slate.data_ptr(), d.data_ptr(), st)
        elif name == "listnet":
            rc = h.ltr_listnet_fwd_bwd(y.data_ptr(), s.data_ptr(), Q, S, *args, slate.data_ptr(), d.data_ptr(), st)
        else:
            rc = h.ltr_lambda_fwd_bwd(s.data_ptr(), y.data_ptr(), Q, S, *args, slate.data_ptr(), cnt.data_ptr(), d.data_ptr(), st)
        assert rc == 0
        torch.cuda.synchronize()
        return slate, cnt, d

    cases = [("approx", (1.0, 1e-10, -1.0, 0.2)), ("listnet", (0, 1.0)), ("listnet", (1, 1.0))]
    for sid in range(8):
        cases.append(("lambda", (sid, 0, 1.0, 10.0, 1e-10, -1.0, 0, 1.0)))
    cases.append(("lambda", (4, 5, 2.0, 10.0, 1e-10, -1.0, 1, 1.0)))
    for name, args in cases:
        a, b = _raw(dev, name, sl, s, y, *args), rect(name, *args)
        assert torch.equal(a[0], b[0]), (name, args, "slate_loss")
        assert torch.equal(a[2], b[2]), (name, args, "dscores")
        if name == "lambda":
            assert torch.equal(a[1], b[1]), (name, args, "slate_count")
    # the metric too
    from ltr_mi355x import metrics, ragged
    a = ragged.ndcg_at_k(y, s, sl, k=10)
    b = metrics.ndcg_at_k(y.view(Q, S), s.view(Q, S), k=10)
    assert torch.equal(a, b)


def test_ragged_vs_rectangular_kernels_on_the_padded_rectangle(dev):
    from losses.approxNDCG import approxNDCGLoss
    from losses.lambdaL import lambdaLoss
    from losses.listnet import listnetLoss
    from ltr_mi355x import ragged
    lengths = [5, 31, 64, 100, 129, 257, 40, 3]
    bounds = RC.bounds_of(lengths)
    s, y = RC.random_batch(lengths, 77)
    sl = _slates(lengths, dev)
    sp, yp = RC.pad_rectangle(s, bounds, 0.0), RC.pad_rectangle(y, bounds, -1.0)

    def rect(fn):
        x = sp.to(dev).requires_grad_(True)
        out = fn(x)
        out.backward()
        return float(out), RC.unpad(x.grad.cpu(), bounds)

    loss, g = _run(lambda x: ragged.approx_ndcg(x, y.to(dev), sl), s, dev)
    rl, rg = rect(lambda x: approxNDCGLoss(x, yp.to(dev)))
    assert relerr(loss, rl, "ragged vs padded approxNDCG loss") < TOL and relerr(g, rg, "ragged vs padded approxNDCG dscores") < TOL
    for scheme, red in (("ndcgLoss2PP_scheme", "sum"), ("ndcgLoss1_scheme", "mean"), ("lamdbaRank_scheme", "mean")):
        loss, g = _run(lambda x: ragged.lambda_loss(x, y.to(dev), sl, weighing_scheme=scheme, reduction=red), s, dev)
        rl, rg = rect(lambda x: lambdaLoss(x, yp.to(dev), weighing_scheme=scheme, reduction=red))
        assert relerr(loss, rl, "ragged vs padded lambdaLoss loss") < TOL and relerr(g, rg, "ragged vs padded lambdaLoss dscores") < TOL
    # ListNet has no padding mask: the padded rectangle is a DIFFERENT loss -- the ragged path is not padding underneath
    loss, _ = _run(lambda x: ragged.listnet(y.to(dev), x, sl), s, dev)
    rl, _ = rect(lambda x: listnetLoss(yp.to(dev), x))
    assert abs(loss - rl) > 1e-3 * abs(rl)


# ---------------------------------------------------------------------------------------------------- 4. index list and tails
@pytest.mark.parametrize("name", ["approx", "listnet", "lambda", "lambda_blocked"])
def test_index_list_leaves_other_queries_untouched(name, dev):
    from ltr_mi355x import lib
    h = lib()
    lengths = [300, 270, 310, 400, 260, 290] if name == "lambda_blocked" else [20, 17, 31, 25, 18, 32]
    bounds = RC.bounds_of(lengths)
    s, y = RC.random_batch(lengths, 88)
    sl = _slates(lengths, dev)
    s, y = s.to(dev), y.to(dev)
    listed = [1, 3, 4]
    q = torch.tensor(listed, dtype=torch.int32, device=dev)
    CAN = -12345.0
    slate, cnt, d = (torch.full((len(lengths),), CAN, device=dev), torch.full((len(lengths),), CAN, device=dev),
                     torch.full((sl.n_docs,), CAN, device=dev))
    st = torch.cuda.current_stream().cuda_stream
    s_max = max(lengths[i] for i in listed)
    if name == "approx":
        rc = h.ltr_approxndcg_ragged_fwd_bwd(s.data_ptr(), y.data_ptr(), sl.offsets.data_ptr(), q.data_ptr(), 3, s_max, 1.0, 1e-10, -1.0,
                                             1.0, slate.data_ptr(), d.data_ptr(), st)
    elif name == "listnet":
        rc = h.ltr_listnet_ragged_fwd_bwd(y.data_ptr(), s.data_ptr(), sl.offsets.data_ptr(), q.data_ptr(), 3, s_max, 0, 1.0,
                                          slate.data_ptr(), d.data_ptr(), st)
    else:
        rc = h.ltr_lambda_ragged_fwd_bwd(s.data_ptr(), y.data_ptr(), sl.offsets.data_ptr(), q.data_ptr(), 3, s_max, 4, 0, 1.0, 10.0, 1e-10,
                                         -1.0, 0, 1.0, slate.data_ptr(), cnt.data_ptr(), d.data_ptr(), st)
    assert rc == 0
    torch.cuda.synchronize()
    slate, cnt, d = slate.cpu(), cnt.cpu(), d.cpu()
    for i in range(len(lengths)):
        rows = d[bounds[i]:bounds[i + 1]]
        if i in listed:
            assert slate[i] != CAN and bool((rows != CAN).all())
            assert name in ("approx", "listnet") or cnt[i] != CAN
        else:
            # a skipped query's loss slot and EVERY row of it, the rows next to its listed neighbours included
            assert slate[i] == CAN and cnt[i] == CAN and bool((rows == CAN).all()), i
    # and the listed ones are the full launch's numbers
    full = _raw(dev, "lambda" if name.startswith("lambda") else name, sl, s, y,
                *{"approx": (1.0, 1e-10, -1.0, 1.0), "listnet": (0, 1.0)}.get(name, (4, 0, 1.0, 10.0, 1e-10, -1.0, 0, 1.0)))
    for i in listed:
        assert slate[i] == full[0].cpu()[i]
        assert torch.equal(d[bounds[i]:bounds[i + 1]], full[2].cpu()[bounds[i]:bounds[i + 1]])


def test_query_outside_the_tier_is_poisoned_not_computed(dev):
    """The offsets live on the device, so the launcher cannot check them: a listed query whose length is not in the launch's tier gets
    a NaN loss and no gradient rows (the host layer never lists one)."""
    lengths = [20, 3, 31]                    # 3 is not in the 17..32 tier
    s, y = RC.random_batch(lengths, 89)
    sl = _slates(lengths, dev)
    slate, cnt, d = _raw(dev, "lambda", sl, s.to(dev), y.to(dev), 4, 0, 1.0, 10.0, 1e-10, -1.0, 0, 1.0)
    assert bool(torch.isnan(slate[1])) and float(cnt[1]) == 0.0 and bool((d[20:23] == -7.0).all())
    assert bool(torch.isfinite(slate[[0, 2]]).all())


# ---------------------------------------------------------------------------------------------------- 5. NDCG@k
@pytest.mark.parametrize("gains", ["linear", "exponential"])
@pytest.mark.parametrize("reverse_ties", [False, True])
@pytest.mark.parametrize("no_relevant", [True, False])
def test_ndcg_ragged_vs_oracle(gains, reverse_ties, no_relevant, dev):
    from ltr_mi355x import ragged
    from utils.metrics import mNdcg
    lengths = [1, 2, 7, 64, 65, 300, 12, 1030, 5, 2048, 33]
    bounds = RC.bounds_of(lengths)
    g = torch.Generator().manual_seed(5)
    n = sum(lengths)
    s = torch.round(torch.randn(n, generator=g) * 4) / 4          # ties
    y = torch.randint(0, 5, (n,), generator=g).float()
    y[bounds[6]:bounds[7]] = 0.0                                   # a query without a relevant document
    sl = _slates(lengths, dev)
    for k in (1, 5, 10, 100):
        got = ragged.ndcg_at_k(y, s, sl, k=k, no_relevant=no_relevant, gains=gains, reverse_ties=reverse_ties).cpu().numpy()
        ref = np.array([MO.ndcg_per_query(y[a:b].numpy()[None], s[a:b].numpy()[None], k=k, no_relevant=no_relevant, gains=gains,
                                          stable=not reverse_ties)[0] for a, b in zip(bounds[:-1], bounds[1:])])
        assert got[6] == (1.0 if no_relevant else 0.0)
        assert float(np.abs(got - ref).max()) < 1e-12, (k, got, ref)
        lists_y = [y[a:b].tolist() for a, b in zip(bounds[:-1], bounds[1:])]
        lists_s = [s[a:b].tolist() for a, b in zip(bounds[:-1], bounds[1:])]
        assert mNdcg(lists_y, lists_s, k=k, no_relevant=no_relevant, gains=gains, use_numpy=reverse_ties) == got.tolist()


# ---------------------------------------------------------------------------------------------------- 6. / 7. the step
STEP_LENGTHS = [40, 3, 129, 17, 64, 260, 1, 90]
STEP_LENGTHS_2 = [5, 200, 33, 600, 12]


def _step_data(lengths, seed, F=136):
    g = torch.Generator().manual_seed(seed)
    n = sum(lengths)
    return torch.randn(n, F, generator=g), torch.randint(0, 5, (n,), generator=g).float()


def _combine(loss, red, per, counts):
    """Per-query oracle steps -> the ragged loss and gradients (the issue's table)."""
    Q = len(per)
    if loss == "approxNDCG":
        w = 1.0 / Q
    elif loss == "lambdaLoss" and red == "mean":
        w = 1.0 / sum(counts)
    else:
        w = 1.0
    total = w * sum(float(l) for l, _ in per)
    grads = {k: w * sum(np.asarray(g[k], dtype=np.float64) for _, g in per) for k in per[0][1]}
    return total, grads


def _oracle_ragged_step(kind, sd, x, y, bounds, loss, red, k1=None, k2=None, dtype=torch.float64):
    kw = dict(weighing_scheme="ndcgLoss2PP_scheme", k=None, sigma=1.0, mu=10.0, reduction="sum", reduction_log="binary")
    per, counts = [], []
    for a, b in zip(bounds[:-1], bounds[1:]):
        l, g, sc = _oracle_step(kind, sd, x[a:b][None], y[a:b][None], loss, None if k1 is None else k1[a:b][None],
                                None if k2 is None else k2[a:b][None], dtype=dtype, lambda_kw=kw)
        per.append((l, g))
        if loss == "lambdaLoss":
            _, _, keep = O.lambda_pair_parts(torch.from_numpy(np.asarray(sc)).double().reshape(1, -1), y[a:b][None].double(), 1e-10, -1,
                                             "ndcgLoss2PP_scheme", None, 10.0)
            counts.append(int(keep.sum()))
    return _combine(loss, red, per, counts)


def _net_grads(net):
    return {k: p.grad.detach().cpu().numpy() for k, p in net.named_parameters()}


@pytest.mark.parametrize("loss,red", [("approxNDCG", "sum"), ("listnet", "sum"), ("lambdaLoss", "sum"), ("lambdaLoss", "mean")])
@pytest.mark.parametrize("kind", ["double_eval", "double_train", "triple"])
def test_step_ragged_vs_per_query_oracle(kind, loss, red, dev):
    from ltr_mi355x.scorer import FusedRanker
    k = "triple" if kind == "triple" else "double"
    net, sd = _make(k, dev, 31)
    net.train(kind == "double_train")
    extra = dict(weighing_scheme="ndcgLoss2PP_scheme", reduction=red) if loss == "lambdaLoss" else {}
    ranker = FusedRanker(net, loss=loss, **extra)
    for lengths, seed in ((STEP_LENGTHS, 1), (STEP_LENGTHS_2, 2)):         # the second batch: other tiers, other sizes, nothing stale
        bounds = RC.bounds_of(lengths)
        x, y = _step_data(lengths, seed)
        n = sum(lengths)
        k1 = k2 = None
        if kind == "double_train":
            g = torch.Generator().manual_seed(50 + seed)
            k1 = (torch.rand(n, 136, generator=g) < 0.5).float()
            k2 = (torch.rand(n, 136, generator=g) < 0.5).float()
        rl, rg = _oracle_ragged_step(k, sd, x, y, bounds, loss, red, k1, k2)
        _, rg32 = _oracle_ragged_step(k, sd, x, y, bounds, loss, red, k1, k2, dtype=torch.float32)
        sl = _slates(lengths, dev)
        kw = {} if k1 is None else dict(keep1=k1.to(dev), keep2=k2.to(dev))
        out = ranker.step_ragged(x.to(dev), y.to(dev), sl, **kw)
        assert relerr(out.cpu().numpy(), rl, f"step_ragged {loss} loss") < TOL
        assert_grads(_net_grads(net), rg, ref32=rg32)
        direct_flat = ranker.flat.clone()
        ranker.step_ragged(x.to(dev), y.to(dev), sl, defer_norm=True, **kw)
        ranker.finish_norm()
        # the same sums, normalised before (direct: 1 / Q inside the loss launch) or after (deferred: one division of the flat
        # buffer) the fp32 reductions: a few roundings of 2^-24 each apart, never more than 1e-6 of the largest entry
        assert relerr(ranker.flat.cpu().numpy(), direct_flat.cpu().numpy(), "defer_norm + finish_norm vs direct") < 1e-6


@pytest.mark.parametrize("loss,red", [("approxNDCG", "sum"), ("listnet", "sum"), ("lambdaLoss", "mean")])
def test_step_ragged_fc_only_make_model(loss, red, dev):
    from test_linear_fused_cpu import oracle_step
    from test_linear_fused_gpu import SIZES, _as_dict, _model
    from ltr_mi355x.linear import LinearFusedRanker
    from ltr_mi355x.scorer import FusedRanker
    net = _model(dev)
    net.eval()
    extra = dict(weighing_scheme="ndcgLoss2PP_scheme", reduction=red) if loss == "lambdaLoss" else {}
    ranker = FusedRanker(net, loss=loss, **extra)
    assert isinstance(ranker, LinearFusedRanker)
    params = net._ltr_params()
    lkw = dict(weighing_scheme="ndcgLoss2PP_scheme", reduction="sum")
    for lengths, seed in ((STEP_LENGTHS, 3), (STEP_LENGTHS_2, 4)):
        bounds = RC.bounds_of(lengths)
        x, y = _step_data(lengths, seed)

        def loop(dtype):
            per, counts = [], []
            for a, b in zip(bounds[:-1], bounds[1:]):
                l, g = oracle_step(params, x[a:b][None], y[a:b][None], SIZES, False, loss, dtype=dtype, lambda_kw=lkw)
                per.append((l, _as_dict(g)))
                if loss == "lambdaLoss":
                    from test_linear_fused_cpu import linear_forward
                    p64 = [t.detach().cpu().double() for t in params]
                    sc = linear_forward(x[a:b][None], p64, SIZES, False)
                    _, _, keep = O.lambda_pair_parts(sc, y[a:b][None].double(), 1e-10, -1, "ndcgLoss2PP_scheme", None, 10.0)
                    counts.append(int(keep.sum()))
            return _combine(loss, red, per, counts)

        rl, rg = loop(torch.float64)
        _, rg32 = loop(torch.float32)
        out = ranker.step_ragged(x.to(dev), y.to(dev), _slates(lengths, dev))
        assert relerr(out.cpu().numpy(), rl, f"linear step_ragged {loss} loss") < TOL
        assert_grads(_as_dict([p.grad.detach().cpu().numpy() for p in params]), rg, ref32=rg32)


def test_step_ragged_dropout_stream_reproduces(dev):
    from ltr_mi355x.scorer import FusedRanker
    net, _ = _make("double", dev, 9)
    net.train()
    ranker = FusedRanker(net, loss="approxNDCG")
    x, y = _step_data(STEP_LENGTHS, 6)
    sl = _slates(STEP_LENGTHS, dev)
    a = ranker.step_ragged(x.to(dev), y.to(dev), sl, seed=1234).clone()
    fa = ranker.flat.clone()
    b = ranker.step_ragged(x.to(dev), y.to(dev), sl, seed=1234).clone()
    assert torch.equal(a, b) and torch.equal(fa, ranker.flat)
    c = ranker.step_ragged(x.to(dev), y.to(dev), sl, seed=99)
    assert not torch.equal(fa, ranker.flat) and float(c) != float(a)
    net.eval()
    d = ranker.step_ragged(x.to(dev), y.to(dev), sl)
    assert float(d) != float(a)


def test_step_ragged_edge_cases_and_risk_losses(dev):
    from ltr_mi355x.scorer import FusedRanker
    net, _ = _make("double", dev, 9)
    net.eval()
    x, y = _step_data([4, 9], 8)
    sl = _slates([4, 9], dev)
    r = FusedRanker(net, loss="lambdaLoss", k=0, reduction="mean")
    assert np.isnan(float(r.step_ragged(x.to(dev), y.to(dev), sl))) and float(r.flat_grad.abs().max()) == 0.0
    r = FusedRanker(net, loss="approxNDCG")
    empty = _slates([], dev)
    assert np.isnan(float(r.step_ragged(x[:0].to(dev), y[:0].to(dev), empty)))
    assert float(r.step_ragged(x[:0].to(dev), y[:0].to(dev), empty, world_batch=8)) == 0.0
    with pytest.raises(ValueError):
        r.step_ragged(x[:5].to(dev), y.to(dev), sl)
    for name in ("geoRiskListnetLoss", "geoRiskLambdaLoss", "zRiskListnetLoss", "zRiskLambdaLoss", "tRiskListnetLoss", "tRiskLambdaLoss"):
        rr = FusedRanker(net, loss=name)
        with pytest.raises(NotImplementedError, match="FusedRanker.step"):
            rr.step_ragged(x.to(dev), y.to(dev), sl)


@pytest.mark.parametrize("loss,red", [("approxNDCG", "sum"), ("listnet", "sum"), ("lambdaLoss", "sum"), ("lambdaLoss", "mean")])
@pytest.mark.parametrize("S", [17, 257])
@pytest.mark.parametrize("kind", ["double_train", "triple", "fc"])
def test_equal_lengths_are_the_rectangular_listwise_step_bits(kind, S, loss, red, dev):
    """Q queries of one length: `step` on [Q, S, F] and `step_ragged` on the same rows leave the same bits in `flat_ext` -- the
    listwise counterpart of test_ragged_risk_gpu.py::test_equal_lengths_are_the_rectangular_step_bits.  Neither length is a
    one-launch one, so both run the ranker's chain; the loss launches are bitwise equal at these tiers
    (test_equal_lengths_are_the_rectangular_bits), and 257 is the first length of lambdaLoss's 512 tier."""
    from ltr_mi355x.scorer import FusedRanker
    Q, F = 5, 136
    if kind == "fc":
        from test_linear_fused_gpu import _model
        net = _model(dev)
        net.eval()
    else:
        net, _ = _make("triple" if kind == "triple" else "double", dev, 31)
        net.train(kind == "double_train")
    extra = dict(weighing_scheme="ndcgLoss2PP_scheme", reduction=red) if loss == "lambdaLoss" else {}
    ranker = FusedRanker(net, loss=loss, **extra)
    x, y = _step_data([S] * Q, 700 + S, F)
    X, Y = x.to(dev), y.to(dev)
    kw = dict(seed=4321) if kind == "double_train" else {}
    ranker.step(X.view(Q, S, F), Y.view(Q, S), **kw)
    a = ranker.flat_ext.clone()
    assert torch.isfinite(a).all() and float(ranker.flat_grad.abs().max()) > 0.0
    ranker.flat_ext.zero_()
    ranker.step_ragged(X, Y, _slates([S] * Q, dev), **kw)
    assert torch.equal(a, ranker.flat_ext)
