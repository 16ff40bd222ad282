"""GPU: the fused training step of the six risk-sensitive losses (FusedRanker(net, loss="geoRiskLambdaLoss", ...), ltr_mi355x.risk_step)
against the fp64 oracle -- oracle/ltr_risk_oracle.py on the scores of oracle/ltr_oracle.py's double_layer_forward / triple_layer_forward,
under torch autograd.  Bars: max(floor, 4 x the fp32 oracle's own noise) on the loss and on every parameter gradient (assert_grads);
floor 1e-5 for the Listnet forms, 1e-4 for the Lambda forms, 1e-3 where the fp32 oracle itself is non-finite (_floor), all ledgered."""
import numpy as np
import pytest
import torch

import ltr_oracle as O
import ltr_risk_oracle as RO
from conftest import ledger_record, relerr
from test_scorer_gpu import assert_grads

pytestmark = pytest.mark.gpu
TOL = 1e-5
NB = 3
LOSSES = ["geoRiskListnetLoss", "geoRiskLambdaLoss", "zRiskListnetLoss", "zRiskLambdaLoss", "tRiskListnetLoss", "tRiskLambdaLoss"]
ORACLE = {"geoRiskListnetLoss": RO.geo_risk_listnet, "zRiskListnetLoss": RO.z_risk_listnet, "geoRiskLambdaLoss": RO.geo_risk_lambda,
          "zRiskLambdaLoss": RO.z_risk_lambda, "tRiskListnetLoss": RO.t_risk_listnet, "tRiskLambdaLoss": RO.t_risk_lambda}
KW = {"alpha": "alpha", "listnet_transformation": "lt", "return_strategy": "rs", "negative": "negative",
      "add_ideal_ranking_to_mat": "add_ideal", "weighing_scheme": "scheme"}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    import ltr_mi355x
    ltr_mi355x.lib()
    return torch.device("cuda:0")


def _net(geom, dev, seed=3):
    from architeture.doubleLayer import DoubleLayerNet
    from architeture.tripleLayer import TripleLayerNet
    torch.manual_seed(seed)
    F = {"double136": 136, "double64": 64, "double40": 40, "triple136": 136, "triple64": 64}[geom]
    net = (DoubleLayerNet if geom.startswith("double") else TripleLayerNet)(F)
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    return net.to(dev).eval(), sd, F


def _data(name, B, S, F, seed, pad=True):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, S, F, generator=g)
    y = torch.randint(0, 5, (B, S), generator=g).float()
    if pad:
        y[-1, -4:] = -1.0                             # one slate with padded documents
    yb = torch.randn(B, S, NB, generator=g) * 2.0
    if name.startswith("tRisk"):
        yb = yb.mean(dim=2)                            # the reference driver's tRisk baseline (main_batch_execution.py)
    return x, y, yb


def _oracle(name, geom, sd, x, y, yb, args, keep=None, dtype=torch.float64, device="cpu"):
    p = {k: v.to(device=device, dtype=dtype).requires_grad_(True) for k, v in sd.items()}
    xx = x.to(device=device, dtype=dtype)
    if geom.startswith("double"):
        k1, k2 = (None, None) if keep is None else (keep[0].to(device=device, dtype=dtype), keep[1].to(device=device, dtype=dtype))
        s = O.double_layer_forward(xx, p, k1, k2)
    else:
        s = O.triple_layer_forward(xx, p)
    kw = {KW[k]: v for k, v in args.items()}
    loss = ORACLE[name](s.squeeze(-1), y.to(device=device, dtype=dtype), yb.to(device=device, dtype=dtype), **kw)
    loss.sum().backward()
    return float(loss.detach().sum()), {k: v.grad.detach().cpu().numpy() for k, v in p.items()}


def _check(name, geom, B, S, dev, args=None, train=False, seed=0):
    from ltr_mi355x.scorer import FusedRanker
    net, sd, F = _net(geom, dev)
    x, y, yb = _data(name, B, S, F, seed=100 * S + B + seed)
    args = dict(args or {})
    keep = None
    kw = {}
    if train:
        g = torch.Generator().manual_seed(7 + S)
        keep = ((torch.rand(B, S, F, generator=g) < 0.5).float(), (torch.rand(B, S, F, generator=g) < 0.5).float())
        net.train()
        kw = dict(keep1=keep[0].to(dev), keep2=keep[1].to(dev))
    ranker = FusedRanker(net, loss=name, risk_args=args)
    out = float(ranker.step(x.to(dev), y.to(dev), y_base=yb.to(dev), **kw))
    ref_args = dict(ranker.risk.args)
    rl, rg = _oracle(name, geom, sd, x, y, yb, ref_args, keep)
    rl32, rg32 = _oracle(name, geom, sd, x, y, yb, ref_args, keep, dtype=torch.float32)
    _assert_loss(name, out, rl, rl32)
    _assert_grads(name, {k: p.grad.detach().cpu().numpy() for k, p in net.named_parameters()}, rg, rg32)
    return ranker, out


def _floor(name, rl32, rg32=None):
    """Bar floor.  1e-5 for the Listnet forms.  The Lambda forms' matrix entries are fp32 sums of S pair terms in predicted-rank order
    (torch sums them in its own order), then squared differences against the ideal column and the flip's subtraction from the matrix
    maximum: 1e-4, between the module path's own tail bars for the value (5e-5) and the gradient (2e-4) (tests/test_risk_gpu.py).  Where the fp32 oracle itself comes out non-finite the
    case is ill-conditioned in fp32 and there is no noise to scale: 1e-3, the module path's bar for such batches."""
    finite = np.isfinite(rl32) and (rg32 is None or all(np.isfinite(v).all() for v in rg32.values()))
    if not finite:
        return 1e-3
    return 1e-4 if "Lambda" in name else TOL


def _assert_grads(name, got, rg, rg32):
    fl = _floor(name, 0.0, rg32)
    assert_grads(got, rg, tol=fl, ref32=rg32 if fl < 1e-3 else None)


def _assert_loss(name, out, rl, rl32):
    """The loss against the fp64 oracle at max(1e-5, 4 x the fp32 oracle's own deviation): a Lambda-type risk value is a difference
    of fp32 pair-term column sums (and the flip subtracts from the matrix maximum), so the reference's fp32 arithmetic itself moves it
    by more than 1e-5 on some batches -- the bar and that noise go to the ledger."""
    e = abs(out - rl) / max(abs(rl), 1e-30)
    noise = abs(rl32 - rl) / max(abs(rl), 1e-30)
    bar = _floor(name, rl32)
    ledger_record(f"risk fused step loss ({name})", e, noise, tol=bar)
    assert e <= max(bar, 4.0 * noise), (out, rl, rl32)


@pytest.mark.parametrize("S", [32, 128])
@pytest.mark.parametrize("geom", ["double136", "double64", "triple136"])
@pytest.mark.parametrize("name", LOSSES)
def test_risk_fused_step_vs_oracle(name, geom, S, dev):
    _check(name, geom, 5, S, dev)


@pytest.mark.parametrize("name", LOSSES)
def test_risk_fused_step_td2003_slates(name, dev):
    """TD2003's shape: 64 features, 1 000 documents per query."""
    _check(name, "double64", 3, 1000, dev)


@pytest.mark.parametrize("geom", ["double40", "triple64"])
@pytest.mark.parametrize("name", ["geoRiskLambdaLoss", "tRiskListnetLoss"])
def test_risk_fused_step_padded_widths_and_folded_64(name, geom, dev):
    _check(name, geom, 4, 48, dev)


def _option_sets(name):
    out = []
    t, lam = name.startswith("tRisk"), "Lambda" in name
    lts = (1, 2) if (lam and not t) else (1, 2, 3)
    for lt in lts:
        if t:
            out.append(dict(listnet_transformation=lt, alpha=2.0, negative=-1))
            continue
        for rs in (1, 2, 3):
            for ai in (1, 2):
                out.append(dict(listnet_transformation=lt, return_strategy=rs, add_ideal_ranking_to_mat=ai))
    if lam:
        out.append(dict(weighing_scheme="ndcgLoss1_scheme", listnet_transformation=2))
    return out


@pytest.mark.parametrize("name,args", [(n, a) for n in LOSSES for a in _option_sets(n)],
                         ids=lambda v: v if isinstance(v, str) else "-".join(f"{k[:6]}{a}" for k, a in v.items()))
def test_risk_fused_step_options(name, args, dev):
    _check(name, "double136", 6, 32, dev, args=args)


@pytest.mark.parametrize("name", LOSSES)
def test_risk_fused_step_train_mode_keep_masks(name, dev):
    _check(name, "double136", 4, 64, dev, train=True)


@pytest.mark.parametrize("name", LOSSES)
def test_risk_fused_step_seeded_dropout_matches_module_stream(name, dev):
    """Train mode without explicit masks: the step's own seeded stream; the masks it drew (ltr_dropout_keep_mask with the step's seed)
    replayed through the oracle give the same loss and gradients."""
    from ltr_mi355x.scorer import FusedRanker, dropout_keep_mask
    net, sd, F = _net("double136", dev)
    net.train()
    B, S = 4, 32
    x, y, yb = _data(name, B, S, F, seed=5)
    ranker = FusedRanker(net, loss=name)
    seed = 0x1234_5678_9ABC
    out = float(ranker.step(x.to(dev), y.to(dev), y_base=yb.to(dev), seed=seed))
    k1 = dropout_keep_mask(seed, 0, B * S, F, dev).reshape(B, S, F).float().cpu()
    k2 = dropout_keep_mask(seed, 1, B * S, F, dev).reshape(B, S, F).float().cpu()
    rl, rg = _oracle(name, "double136", sd, x, y, yb, dict(ranker.risk.args), (k1, k2))
    rl32, rg32 = _oracle(name, "double136", sd, x, y, yb, dict(ranker.risk.args), (k1, k2), dtype=torch.float32)
    _assert_loss(name, out, rl, rl32)
    _assert_grads(name, {k: p.grad.detach().cpu().numpy() for k, p in net.named_parameters()}, rg, rg32)


@pytest.mark.parametrize("S", [32, 300, 1000])
@pytest.mark.parametrize("name,args", [("geoRiskLambdaLoss", {}), ("geoRiskLambdaLoss", dict(listnet_transformation=2, add_ideal_ranking_to_mat=2)),
                                       ("zRiskLambdaLoss", dict(listnet_transformation=2, add_ideal_ranking_to_mat=2, return_strategy=2)),
                                       ("tRiskLambdaLoss", dict(listnet_transformation=3)), ("geoRiskListnetLoss", dict(add_ideal_ranking_to_mat=2)),
                                       ("zRiskListnetLoss", dict(listnet_transformation=3, return_strategy=3)), ("tRiskListnetLoss", {})])
def test_base_cols_step_equals_y_base_step(name, args, S, dev):
    """The cached baseline columns: the matrix the tail sees is bitwise the uncached one; loss and gradients within 1e-6."""
    from ltr_mi355x import risk_step as RS
    from ltr_mi355x._lib import lib
    from ltr_mi355x.scorer import FusedRanker
    net, sd, F = _net("double64", dev)
    B = 4
    x, y, yb = _data(name, B, S, F, seed=9)
    X, Y, YB = x.to(dev), y.to(dev), yb.to(dev)
    ranker = FusedRanker(net, loss=name, risk_args=args)
    l1 = float(ranker.step(X, Y, y_base=YB))
    g1 = ranker.flat_grad.clone()
    cols = ranker.baseline_columns(Y, YB)
    assert cols.shape[0] == B
    l2 = float(ranker.step(X, Y, base_cols=cols))
    g2 = ranker.flat_grad.clone()
    assert abs(l1 - l2) <= 1e-6 * abs(l1), (l1, l2)
    assert float((g1 - g2).abs().max()) <= 1e-6 * float(g1.abs().max())
    # the matrix itself
    spec = ranker.risk
    scores = torch.randn(B, S, device=dev)
    yb3 = spec.baselines(B, S, YB)
    n_c = spec.n_const(yb3.shape[2])
    m1, m2 = (torch.empty(B, 1 + n_c, device=dev) for _ in range(2))
    j1, j2 = (torch.empty(B, S, device=dev) for _ in range(2))
    RS.matrix(lib(), spec, scores, Y, yb3, None, n_c, m1, j1)
    RS.matrix(lib(), spec, scores, Y, None, cols, n_c, m2, j2)
    assert torch.equal(m1, m2)
    assert torch.equal(j1, j2)
    # rows taken out of order (a shuffled epoch) carry their own columns
    perm = torch.tensor([2, 0, 3, 1])
    l3 = float(ranker.step(X[perm], Y[perm], base_cols=cols[perm]))
    l4 = float(ranker.step(X[perm], Y[perm], y_base=YB[perm]))
    assert abs(l3 - l4) <= 1e-6 * abs(l4)


@pytest.mark.parametrize("name", ["geoRiskLambdaLoss", "tRiskListnetLoss", "zRiskListnetLoss"])
def test_fused_step_matches_the_module_path(name, dev):
    """The definition: riskLoss(net(X, None, None).squeeze(-1), y, y_base, **risk_args); loss.backward()."""
    from losses.riskLosses import riskLosses as RL
    from ltr_mi355x.scorer import FusedRanker
    net, sd, F = _net("double136", dev)
    x, y, yb = _data(name, 5, 128, F, seed=3)
    X, Y, YB = x.to(dev), y.to(dev), yb.to(dev)
    args = dict(return_strategy=2) if not name.startswith("tRisk") else {}
    loss = getattr(RL, name)(net(X, None, None).squeeze(-1), Y, YB, **args)
    loss.backward()
    ref = {k: p.grad.detach().clone() for k, p in net.named_parameters()}
    for p in net.parameters():
        p.grad = None
    ranker = FusedRanker(net, loss=name, risk_args=args)
    out = ranker.step(X, Y, y_base=YB)
    assert relerr(out.cpu().numpy(), loss.detach().cpu().numpy()) <= 1e-6
    for k, p in net.named_parameters():
        assert relerr(p.grad.cpu().numpy(), ref[k].cpu().numpy()) <= 1e-5, k


def test_unsupported_options_raise(dev):
    from ltr_mi355x.scorer import FusedRanker
    net, _, F = _net("double136", dev)
    with pytest.raises(NotImplementedError, match="listnet_transformation"):
        FusedRanker(net, loss="geoRiskLambdaLoss", risk_args=dict(listnet_transformation=3))
    with pytest.raises(NotImplementedError, match="return_strategy"):
        FusedRanker(net, loss="zRiskListnetLoss", risk_args=dict(return_strategy=4))
    with pytest.raises(NotImplementedError, match="negative"):
        FusedRanker(net, loss="tRiskListnetLoss", risk_args=dict(negative=torch.ones(1, device=dev)))
    ranker = FusedRanker(net, loss="geoRiskListnetLoss")
    x, y, yb = _data("geoRiskListnetLoss", 1, 32, F, seed=1)
    with pytest.raises(NotImplementedError, match="at least 2 queries"):
        ranker.step(x.to(dev), y.to(dev), y_base=yb.to(dev))
    x, y, yb = _data("geoRiskListnetLoss", 3, 1, F, seed=1, pad=False)
    with pytest.raises(NotImplementedError, match="2..2048"):
        ranker.step(x.to(dev), y.to(dev), y_base=yb.to(dev))
    x, y, yb = _data("geoRiskListnetLoss", 3, 16, F, seed=1)
    with pytest.raises(ValueError, match="2..64"):
        ranker.step(x.to(dev), y.to(dev), y_base=yb[:, :, :1].to(dev))
    with pytest.raises(ValueError, match="exactly one"):
        ranker.step(x.to(dev), y.to(dev))
