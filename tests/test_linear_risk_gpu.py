"""GPU: the risk-loss training step of FC-only make_model rankers -- FusedRanker(make_model(...), loss=<one of the six risk losses>,
risk_args=...) (ltr_mi355x/linear.py; ltr_linear_risk_rows / ltr_linear_risk_combine in csrc/ltr_linear.hip for the Listnet forms at
S in {32, 64, 128}, the chain of existing entries otherwise).

Oracle: fp64 CPU autograd through `linear_forward` (tests/test_linear_fused_cpu.py) under the functions of oracle/ltr_risk_oracle.py.
Bars: those of the DoubleLayerNet risk step (tests/test_risk_fused_gpu.py `_floor`, `_assert_loss`, `_assert_grads`): max(floor, 4 x the
fp32 oracle's own deviation), floor 1e-5 for the Listnet forms and 1e-4 for the Lambda forms, every use ledgered.  The 1e-3 floor for
batches whose fp32 oracle is itself non-finite leaves a case out, so it is capped: no Listnet-form case, at most one in eight Lambda-form
cases (test_nonfinite_floor_cap counts them over CASES with the fp32 oracle alone; the data seeds below were chosen with that check)."""
import os
import socket
import sys
import tempfile
import time

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ledger_record
from test_linear_fused_cpu import linear_forward
from test_linear_fused_gpu import _model
from test_risk_fused_gpu import KW, LOSSES, ORACLE, _assert_grads, _assert_loss, _floor, _option_sets
from test_scorer_gpu import assert_grads

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NB = 3
NETS = {"config136": dict(seed=5, F=136, sizes=[128, 256, 128], input_norm=False),        # config.json "model"
        "norm64": dict(seed=8, F=64, sizes=[32, 16], input_norm=True)}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    import ltr_mi355x
    ltr_mi355x.lib()
    return torch.device("cuda:0")


def _data(name, B, S, F, seed, spread=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, S, F, generator=g)
    if spread:
        x = x * 3.0 + 1.5                              # rows with a mean and a spread for the LayerNorm
    y = torch.randint(0, 5, (B, S), generator=g).float()
    y[-1, -4:] = -1.0                                  # one slate with padded documents in every batch
    yb = torch.randn(B, S, NB, generator=g) * 2.0
    if name.startswith("tRisk"):
        yb = yb.mean(dim=2)                            # the reference driver's tRisk baseline (main_batch_execution.py)
    return x, y, yb


def _oracle(name, params, x, y, yb, net, args, dtype=torch.float64):
    p = [t.detach().cpu().to(dtype).clone().requires_grad_(True) for t in params]
    s = linear_forward(x, p, NETS[net]["sizes"], NETS[net]["input_norm"], dtype)
    kw = {KW[k]: v for k, v in args.items()}
    loss = ORACLE[name](s, y.to(dtype), yb.to(dtype), **kw).sum()
    loss.backward()
    return float(loss.detach()), {str(i): t.grad.numpy() for i, t in enumerate(p)}


def _full_args(name, args):
    from ltr_mi355x.risk_step import RiskSpec
    return dict(RiskSpec(name, args).args)


# (loss, network, B, S, options): everything test_step_vs_fp64_oracle runs and test_nonfinite_floor_cap counts
CASES = [(n, "config136", B, S, {}) for n in LOSSES for B, S in ((5, 32), (5, 128), (5, 100), (3, 1000))]
CASES += [(n, "norm64", 6, S, {}) for n in LOSSES for S in (64, 100)]
CASES += [(n, "config136", 6, 32, a) for n in LOSSES for a in _option_sets(n)]


def _case_id(c):
    return f"{c[0]}-{c[1]}-B{c[2]}-S{c[3]}" + "".join(f"-{k[:6]}{v}" for k, v in c[4].items())


def _case_data(case):
    name, net, B, S, args = case
    return _data(name, B, S, NETS[net]["F"], seed=1000 + 100 * S + B + 7 * len(args), spread=net == "norm64")


def _grads(net):
    return {str(i): p.grad.detach().cpu().numpy() for i, p in enumerate(net._ltr_params())}


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_step_vs_fp64_oracle(case, dev):
    from ltr_mi355x.scorer import FusedRanker
    name, netk, B, S, args = case
    net = _model(dev, **NETS[netk])
    x, y, yb = _case_data(case)
    ranker = FusedRanker(net, loss=name, risk_args=dict(args))
    assert type(ranker).__name__ == "LinearFusedRanker"
    out = float(ranker.step(x.to(dev), y.to(dev), y_base=yb.to(dev)))
    full = dict(ranker.risk.args)
    params = net._ltr_params()
    rl, rg = _oracle(name, params, x, y, yb, netk, full)
    rl32, rg32 = _oracle(name, params, x, y, yb, netk, full, dtype=torch.float32)
    print(f"[{_case_id(case)}] loss {out:.9g} fp64 {rl:.9g} fp32 {rl32:.9g} floor {_floor(name, rl32, rg32):g}")
    if "Lambda" not in name:
        assert _floor(name, rl32, rg32) == 1e-5            # no Listnet-form case takes the non-finite floor
    _assert_loss(name, out, rl, rl32)
    _assert_grads(name, _grads(net), rg, rg32)
    for p, gv in zip(ranker.params, ranker._grad_views):
        assert p.grad is gv


def test_nonfinite_floor_cap():
    """The 1e-3 floor (fp32 oracle non-finite) over CASES: never for a Listnet form, at most one in eight Lambda-form cases.  The fp32
    oracle alone decides it -- no device arithmetic enters the count."""
    cpu = torch.device("cpu")
    used = {"Listnet": 0, "Lambda": 0}
    total = {"Listnet": 0, "Lambda": 0}
    for case in CASES:
        name, netk, B, S, args = case
        params = _model(cpu, **NETS[netk])._ltr_params()
        x, y, yb = _case_data(case)
        rl32, rg32 = _oracle(name, params, x, y, yb, netk, _full_args(name, args), dtype=torch.float32)
        kind = "Lambda" if "Lambda" in name else "Listnet"
        total[kind] += 1
        if _floor(name, rl32, rg32) == 1e-3:
            used[kind] += 1
            print("non-finite fp32 oracle:", _case_id(case))
    print("1e-3 floor uses", used, "of", total)
    assert used["Listnet"] == 0
    assert 8 * used["Lambda"] <= total["Lambda"], (used, total)


@pytest.mark.parametrize("S", [32, 100])
@pytest.mark.parametrize("name,args", [("geoRiskLambdaLoss", {}), ("zRiskLambdaLoss", dict(listnet_transformation=2, add_ideal_ranking_to_mat=2)),
                                       ("tRiskLambdaLoss", {}), ("geoRiskListnetLoss", dict(add_ideal_ranking_to_mat=2)),
                                       ("zRiskListnetLoss", dict(listnet_transformation=3, return_strategy=3)), ("tRiskListnetLoss", {})],
                         ids=lambda v: v if isinstance(v, str) else "-".join(f"{k[:6]}{a}" for k, a in v.items()))
def test_base_cols_step_is_bitwise_the_y_base_step(name, args, S, dev):
    from ltr_mi355x.scorer import FusedRanker
    net = _model(dev, **NETS["config136"])
    Q = 9
    x, y, yb = _data(name, Q, S, 136, seed=31 + S)
    X, Y, YB = x.to(dev), y.to(dev), yb.to(dev)
    ranker = FusedRanker(net, loss=name, risk_args=args)
    cols = ranker.baseline_columns(Y, YB)                 # once per dataset
    assert cols.shape[0] == Q
    idx = torch.tensor([7, 2, 5, 0, 8], device=dev)       # a shuffled mini-batch
    ranker.step(X[idx], Y[idx], y_base=YB[idx])
    a = ranker.flat.clone()
    ranker.step(X[idx], Y[idx], base_cols=cols[idx])
    assert torch.equal(a, ranker.flat)
    assert torch.isfinite(a).all()


@pytest.mark.parametrize("netk", ["config136", "norm64"])
@pytest.mark.parametrize("name", ["geoRiskListnetLoss", "zRiskListnetLoss", "tRiskListnetLoss"])
def test_one_pass_agrees_with_the_chain(name, netk, dev):
    """Listnet forms at S = 128: ltr_linear_risk_rows + ltr_linear_risk_combine against ltr_linear_scores -> matrix -> scores_grad ->
    ltr_linear_grad_partials, within the Listnet bar (1e-5) on the loss and every gradient."""
    from ltr_mi355x.scorer import FusedRanker
    net = _model(dev, **NETS[netk])
    x, y, yb = _data(name, 7, 128, NETS[netk]["F"], seed=77, spread=netk == "norm64")
    X, Y, YB = x.to(dev), y.to(dev), yb.to(dev)
    ranker = FusedRanker(net, loss=name)
    l1 = float(ranker.step(X, Y, y_base=YB))
    g1 = _grads(net)
    g1 = {k: v.copy() for k, v in g1.items()}
    l2 = float(ranker.step(X, Y, y_base=YB, _one_pass=False))
    g2 = _grads(net)
    e = abs(l1 - l2) / max(abs(l2), 1e-30)
    ledger_record(f"one-pass vs chain loss ({name})", e)
    assert e <= 1e-5, (l1, l2)
    assert_grads(g1, g2, tol=1e-5)
    with pytest.raises(NotImplementedError, match="one-pass"):
        FusedRanker(net, loss=name.replace("Listnet", "Lambda")).step(X, Y, y_base=YB, _one_pass=True)


@pytest.mark.parametrize("name,S", [("tRiskListnetLoss", 128), ("geoRiskListnetLoss", 32), ("zRiskListnetLoss", 100), ("geoRiskLambdaLoss", 100),
                                    ("tRiskLambdaLoss", 128)])
def test_two_identical_steps_are_bitwise_identical(name, S, dev):
    from ltr_mi355x.scorer import FusedRanker
    net = _model(dev, **NETS["config136"])
    x, y, yb = (t.to(dev) for t in _data(name, 40, S, 136, seed=1))
    r = FusedRanker(net, loss=name)
    r.step(x, y, y_base=yb)
    a = r.flat.clone()
    r.step(x, y, y_base=yb)
    assert torch.equal(a, r.flat)
    assert torch.isfinite(a).all() and float(a[:-1].abs().max()) > 0.0


def test_adam_training_tracks_fp64(dev):
    """20 Adam steps of tRiskListnetLoss through FusedRanker against the same loop on the fp64 oracle (and on the fp32 oracle, whose
    own drift sets the bar: max(1e-5, 4 x it)): a stale fold, R or coefficient would drift at once."""
    from ltr_mi355x.scorer import FusedRanker
    name, netk = "tRiskListnetLoss", "config136"
    sizes = NETS[netk]["sizes"]
    net = _model(dev, seed=12)
    r = FusedRanker(net, loss=name)
    full = dict(r.risk.args)
    kw = {KW[k]: v for k, v in full.items()}
    refs = {dt: [p.detach().cpu().to(dt).clone().requires_grad_(True) for p in net._ltr_params()] for dt in (torch.float64, torch.float32)}
    opts = {dt: torch.optim.Adam(ps, lr=1e-3, eps=1e-6) for dt, ps in refs.items()}
    opt = torch.optim.Adam(net.parameters(), lr=1e-3, eps=1e-6)
    for it in range(20):
        x, y, yb = _data(name, 16, 128, 136, seed=100 + it)
        l = float(r.step(x.to(dev), y.to(dev), y_base=yb.to(dev)))
        opt.step()
        ls = {}
        for dt, ps in refs.items():
            opts[dt].zero_grad()
            lo = ORACLE[name](linear_forward(x, ps, sizes, False, dt), y.to(dt), yb.to(dt), **kw).sum()
            lo.backward()
            opts[dt].step()
            ls[dt] = float(lo.detach())
        _assert_loss(name, l, ls[torch.float64], ls[torch.float32])
    for p, q, q32 in zip(net._ltr_params(), refs[torch.float64], refs[torch.float32]):
        if p.dim() == 2:
            top = float(q.detach().abs().max())
            d = float((p.detach().cpu().double() - q.detach()).abs().max()) / top
            noise = float((q32.detach().double() - q.detach()).abs().max()) / top
            ledger_record("Adam x20 risk weights / max|tensor|", d, noise)
            print(f"[adam] tensor {tuple(p.shape)}: fused {d:.3e}, fp32 oracle {noise:.3e}")
            assert d <= max(1e-5, 4.0 * noise)


def test_surface_and_rules(dev):
    from ltr_mi355x.scorer import FusedRanker
    net = _model(dev, seed=3, dropout=0.2)
    r = FusedRanker(net, loss="geoRiskListnetLoss", risk_args=dict(alpha=5, return_strategy=2))
    x, y, yb = (t.to(dev) for t in _data("geoRiskListnetLoss", 4, 32, 136, seed=2))
    net.train()
    with pytest.raises(NotImplementedError, match="module path"):
        r.step(x, y, y_base=yb)
    net.eval()
    with pytest.raises(ValueError, match="exactly one"):
        r.step(x, y)
    with pytest.raises(ValueError, match="exactly one"):
        r.step(x, y, y_base=yb, base_cols=r.baseline_columns(y, yb))
    with pytest.raises(NotImplementedError, match="at least 2 queries"):
        r.step(x[:1], y[:1], y_base=yb[:1])
    with pytest.raises(NotImplementedError, match="2..2048"):
        r.step(x[:, :1], y[:, :1], y_base=yb[:, :1])
    with pytest.raises(TypeError, match="y_base"):
        FusedRanker(net, loss="listnet").step(x, y, y_base=yb)
    with pytest.raises(TypeError, match="baseline_columns"):
        FusedRanker(net, loss="listnet").baseline_columns(y, yb)
    ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    r.kernel_events = ev
    r.step(x, y, y_base=yb)
    torch.cuda.synchronize()
    assert ev[0].elapsed_time(ev[1]) > 0.0
    assert torch.isfinite(r.flat).all() and r.flat_ext.numel() == r.info.n_params + 2


def test_step_matches_the_module_path(dev):
    """The definition: riskLoss(model(X, None, None).squeeze(-1), y, y_base, **risk_args); backward() -- the module path runs bf16 GEMMs,
    so the comparison is at its precision (1e-2), the fp64 oracle tests above being the exact ones."""
    from losses.riskLosses import riskLosses as RL
    from ltr_mi355x.scorer import FusedRanker
    net = _model(dev, **NETS["config136"])
    x, y, yb = (t.to(dev) for t in _data("geoRiskListnetLoss", 6, 128, 136, seed=4))
    args = dict(alpha=5, return_strategy=2)
    loss = RL.geoRiskListnetLoss(net(x, None, None).squeeze(-1), y, yb, **args)
    out = FusedRanker(net, loss="geoRiskListnetLoss", risk_args=args).step(x, y, y_base=yb)
    assert abs(float(out) - float(loss)) <= 1e-2 * abs(float(loss)), (float(out), float(loss))


# ---------------------------------------------------------------------------------------------------------- forced grids
# The default grid (2 workgroups per CU) exceeds the tile count of every batch above, so there each workgroup of ltr_linear_risk_rows
# walks one tile and each workgroup of ltr_linear_risk_combine sums one slate.  FusedRanker(grid=2 / 3) makes them loop: several tiles
# per workgroup (unequal counts at grid 3), a partial last tile, combine ranges of several slates with a short last one.
FORCED_B = {32: 37, 64: 17, 128: 11}      # 10 tiles (the last holds 1 of 4 slates), 9 tiles (1 of 2), 11 tiles


@pytest.mark.parametrize("grid", [2, 3])
@pytest.mark.parametrize("S", [32, 64, 128])
@pytest.mark.parametrize("netk", ["config136", "norm64"])
@pytest.mark.parametrize("name", ["geoRiskListnetLoss", "zRiskListnetLoss", "tRiskListnetLoss"])
def test_one_pass_forced_grid(name, netk, S, grid, dev):
    from ltr_mi355x.scorer import FusedRanker
    net = _model(dev, **NETS[netk])
    B = FORCED_B[S]
    tiles = -(-B * S // 128)
    assert tiles >= 3 * grid - 1 and (S == 128 or (B * S) % 128) and B % grid      # loops, partial last tile, short last combine range
    x, y, yb = _data(name, B, S, NETS[netk]["F"], seed=500 + S + grid, spread=netk == "norm64")
    X, Y, YB = x.to(dev), y.to(dev), yb.to(dev)
    ranker = FusedRanker(net, loss=name, grid=grid)
    assert ranker.grid == grid
    out = float(ranker.step(X, Y, y_base=YB))
    full = dict(ranker.risk.args)
    params = net._ltr_params()
    rl, rg = _oracle(name, params, x, y, yb, netk, full)
    rl32, rg32 = _oracle(name, params, x, y, yb, netk, full, dtype=torch.float32)
    assert _floor(name, rl32, rg32) == 1e-5
    _assert_loss(name, out, rl, rl32)
    _assert_grads(name, _grads(net), rg, rg32)
    out0 = float(FusedRanker(net, loss=name).step(X, Y, y_base=YB))
    assert out == out0, (out, out0)                      # mat[:, 0] does not depend on the grid: the same loss bit for bit


@pytest.mark.parametrize("name", ["geoRiskListnetLoss", "tRiskListnetLoss"])
def test_idle_workgroups_leave_no_stale_partials(name, dev):
    """A 24-tile step at grid 6 (every workgroup writes non-zero partials), then a 3-slate step on the same ranker: the three workgroups
    of ltr_linear_risk_combine with an empty range must write zeros.  Bit-identical to a fresh ranker's step."""
    from ltr_mi355x.scorer import FusedRanker
    net = _model(dev, **NETS["config136"])
    r = FusedRanker(net, loss=name, grid=6)
    bx, by, byb = (t.to(dev) for t in _data(name, 24, 128, 136, seed=5))
    r.step(bx, by, y_base=byb)
    assert float(r.partials.abs().view(6, -1).max(dim=1).values.min()) > 0.0
    x, y, yb = (t.to(dev) for t in _data(name, 3, 128, 136, seed=6))
    r.step(x, y, y_base=yb)
    a = r.flat.clone()
    fresh = FusedRanker(net, loss=name, grid=6)
    fresh.step(x, y, y_base=yb)
    assert torch.equal(a, fresh.flat)
    assert float(r.partials.view(6, -1)[3:].abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------- data parallel
DP_B, DP_S = 7, 64


def _dp_worker(rank, world, port, out_dir, name, mode):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sys.path.insert(0, os.path.join(ROOT, "nn-with-pytorch-personalized-losses_amd"))
    dev = torch.device("cuda:0")
    net = _model(dev, **NETS["config136"])
    from ltr_mi355x.dp import QueryShardedTrainer, shard_range
    from ltr_mi355x.scorer import FusedRanker
    ranker = FusedRanker(net, loss=name, risk_args=dict(alpha=3.0))
    tr = QueryShardedTrainer(ranker, torch.optim.SGD(net.parameters(), lr=0.0))
    X, y, yb = _data(name, DP_B, DP_S, 136, seed=21)
    lo, hi = shard_range(DP_B, rank, world)
    Xs, ys, ybs = X[lo:hi].to(dev), y[lo:hi].to(dev), yb[lo:hi].to(dev)
    extra = dict(base_cols=ranker.baseline_columns(ys, ybs)) if mode == "base_cols" else dict(y_base=ybs)
    loss = float(tr.step(Xs, ys, global_batch=DP_B if mode == "global_batch" else None, **extra))
    torch.save({"loss": loss, "flat": ranker.flat.cpu(), "rows": hi - lo}, os.path.join(out_dir, f"rank{rank}.pt"))
    dist.destroy_process_group()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _spawn(fn, args, nprocs, seconds):
    """Fresh child processes under a time limit of their own: past it they are killed and the test fails."""
    ctx = mp.spawn(fn, args=args, nprocs=nprocs, join=False)
    deadline = time.time() + seconds
    while not ctx.join(timeout=5):
        if time.time() > deadline:
            for p in ctx.processes:
                p.kill()
            pytest.fail(f"data-parallel workers still running after {seconds} s")


@pytest.mark.parametrize("mode", ["global_batch", "size_exchange", "base_cols"])
@pytest.mark.parametrize("name", ["tRiskListnetLoss", "geoRiskLambdaLoss"])
def test_two_ranks_ragged_equal_single_process(name, mode):
    """7 queries split 4 + 3 over two ranks on one card (gloo): the single-process loss and gradients at 1e-6 relative
    (tests/test_risk_dp_gpu.py's bar) -- tRiskListnetLoss through the one-pass kernels, geoRiskLambdaLoss through the chain."""
    assert torch.cuda.is_available()
    with tempfile.TemporaryDirectory() as d:
        _spawn(_dp_worker, (2, _free_port(), d, name, mode), 2, 300)
        r = [torch.load(os.path.join(d, f"rank{k}.pt"), weights_only=True) for k in range(2)]
    assert [x["rows"] for x in r] == [4, 3]
    dev = torch.device("cuda:0")
    from ltr_mi355x.scorer import FusedRanker
    net = _model(dev, **NETS["config136"])
    ranker = FusedRanker(net, loss=name, risk_args=dict(alpha=3.0))
    X, y, yb = _data(name, DP_B, DP_S, 136, seed=21)
    ref_loss = float(ranker.step(X.to(dev), y.to(dev), y_base=yb.to(dev)))
    ref = ranker.flat_grad.cpu()
    assert r[0]["loss"] == r[1]["loss"]                      # every rank returns the same global loss
    assert torch.equal(r[0]["flat"], r[1]["flat"])
    assert abs(r[0]["loss"] - ref_loss) <= 1e-6 * abs(ref_loss), (r[0]["loss"], ref_loss)
    top = float(ref.abs().max())
    assert top > 0.0
    assert float((r[0]["flat"][:-1] - ref).abs().max()) <= 1e-6 * top
