"""GPU: query-sharded data parallelism for the batch-coupled risk losses.  Two ranks share the one card (gloo, as tests/test_dp_gpu.py),
with ragged shards (7 queries -> 4 + 3): QueryShardedTrainer over a risk FusedRanker -- one all_gather of the matrix rows, the tail on
the whole matrix on every rank -- must give the single-process loss and gradients of the whole batch, while the sum of per-shard risks
(what summing per-rank losses and gradients computes) does not."""
import os
import socket
import sys
import tempfile

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, S, F, NB = 7, 64, 64, 3


def _data(name):
    g = torch.Generator().manual_seed(21)
    X = torch.randn(B, S, F, generator=g)
    y = torch.randint(0, 5, (B, S), generator=g).float()
    yb = torch.randn(B, S, NB, generator=g) * 2.0
    if name.startswith("tRisk"):
        yb = yb.mean(dim=2)
    return X, y, yb


def _net(dev):
    sys.path.insert(0, os.path.join(ROOT, "nn-with-pytorch-personalized-losses_amd"))
    from architeture.doubleLayer import DoubleLayerNet
    torch.manual_seed(2021)
    return DoubleLayerNet(F).to(dev).eval()


def _worker(rank, world, port, out_dir, name, mode):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    dev = torch.device("cuda:0")
    net = _net(dev)
    from ltr_mi355x.dp import QueryShardedTrainer, shard_range
    from ltr_mi355x.scorer import FusedRanker
    ranker = FusedRanker(net, loss=name, risk_args=dict(alpha=3.0))
    tr = QueryShardedTrainer(ranker, torch.optim.SGD(net.parameters(), lr=0.0))
    X, y, yb = _data(name)
    lo, hi = shard_range(B, rank, world)
    Xs, ys, ybs = X[lo:hi].to(dev), y[lo:hi].to(dev), yb[lo:hi].to(dev)
    if mode == "base_cols":
        extra = dict(base_cols=ranker.baseline_columns(ys, ybs))
    else:
        extra = dict(y_base=ybs)
    gb = B if mode == "global_batch" else None
    loss = float(tr.step(Xs, ys, global_batch=gb, **extra))
    torch.save({"loss": loss, "flat": ranker.flat.cpu(), "rows": hi - lo}, os.path.join(out_dir, f"rank{rank}.pt"))
    dist.destroy_process_group()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.timeout(600)
@pytest.mark.parametrize("mode", ["global_batch", "size_exchange", "base_cols"])
@pytest.mark.parametrize("name", ["geoRiskLambdaLoss", "tRiskListnetLoss"])
def test_two_ranks_ragged_equal_single_process(name, mode):
    assert torch.cuda.is_available()
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(_worker, args=(2, _free_port(), d, name, mode), nprocs=2, join=True)
        r = [torch.load(os.path.join(d, f"rank{k}.pt"), weights_only=True) for k in range(2)]
    assert [x["rows"] for x in r] == [4, 3]
    dev = torch.device("cuda:0")
    from ltr_mi355x.scorer import FusedRanker
    net = _net(dev)
    ranker = FusedRanker(net, loss=name, risk_args=dict(alpha=3.0))
    X, y, yb = _data(name)
    ref_loss = float(ranker.step(X.to(dev), y.to(dev), y_base=yb.to(dev)))
    ref = ranker.flat_grad.cpu()
    assert r[0]["loss"] == r[1]["loss"]                      # every rank returns the same global loss
    assert torch.equal(r[0]["flat"], r[1]["flat"])
    assert abs(r[0]["loss"] - ref_loss) <= 1e-6 * abs(ref_loss), (r[0]["loss"], ref_loss)
    top = float(ref.abs().max())
    assert float((r[0]["flat"][:-1] - ref).abs().max()) <= 1e-6 * top
    # the bug this fixes: per-shard risks added up (ModuleShardedTrainer's reduction) are not the global-batch loss / gradient
    parts, grads = [], torch.zeros_like(ref)
    for lo, hi in ((0, 4), (4, 7)):
        parts.append(float(ranker.step(X[lo:hi].to(dev), y[lo:hi].to(dev), y_base=yb[lo:hi].to(dev))))
        grads += ranker.flat_grad.cpu()
    assert abs(sum(parts) - ref_loss) > 1e-3 * abs(ref_loss)
    assert float((grads - ref).abs().max()) > 1e-3 * top
