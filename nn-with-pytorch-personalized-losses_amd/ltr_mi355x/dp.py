"""Query-sharded data parallelism: one process per GPU, one all-reduce per step.

Slates are independent, so the path shards by query with no data-path collective; the only exchange is a
single all-reduce(SUM) of ONE flat fp32 buffer [all parameter gradients | loss] (37 402 floats = 150 KB for
DoubleLayerNet) over RCCL/xGMI (`torch.distributed` backend "nccl" on ROCm).  At this size the collective is
latency-bound, so it is issued once per step, not bucketed.  Reduction rules:
approxNDCG is a MEAN over the global batch -> each rank pre-scales by 1/B_global when the caller knows it, else the
local batch size rides along in the buffer and the division follows the all-reduce; ListNet / lambdaLoss("sum") are
SUMs -> no scaling; lambdaLoss("mean") divides by the GLOBAL kept-pair count, all-reduced in the same buffer.
Works unchanged on the gloo backend (CPU tests, world_size 2).

The risk-sensitive losses (geoRisk / zRisk / tRisk, Listnet and Lambda forms) are NOT sums over queries: the flip's whole-matrix
maximum, the column sums, the total and tRisk's mean / std are batch-wide.  Through ModuleShardedTrainer each rank computes the risk
of its own shard and the gradients are added -- that is not the global-batch loss, and not its gradient.  QueryShardedTrainer with a
risk FusedRanker trains them correctly: one all_gather of the [queries, systems] matrix rows, the tail on the whole matrix on every
rank (ltr_mi355x.risk_step), then the usual one all-reduce of [grads | loss].
"""
import torch
import torch.distributed as dist


def world():
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(), dist.get_world_size()
    return 0, 1


def shard_range(n_queries, rank, world_size):
    """Contiguous query shard [lo, hi) of rank; sizes differ by at most one."""
    base, rem = divmod(n_queries, world_size)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def sync_parameters(module, src=0, group=None):
    """Every rank starts from rank `src`'s weights (one broadcast of the flattened parameters)."""
    _, ws = world()
    if ws == 1:
        return
    flat = torch.cat([p.detach().reshape(-1) for p in module.parameters()])
    dist.broadcast(flat, src=src, group=group)
    off = 0
    with torch.no_grad():
        for p in module.parameters():
            p.copy_(flat[off:off + p.numel()].view_as(p))
            off += p.numel()


class QueryShardedTrainer:
    """local_step: object with `.flat` ([grads | loss] fp32 tensor whose slices alias every param.grad) and
    `.step(X, y, world_batch=...)` (ltr_mi355x.scorer.FusedRanker on the GPU; any stand-in in tests).

    Deferred normalisation (local steps that have `.flat_ext`, `.finish_norm()` and `step(defer_norm=True)`): the rank
    leaves SUM-form contributions in [grads | loss] and appends its normaliser -- its batch size for the batch-mean loss
    (approxNDCG.py:53), its kept-pair count for lambdaLoss reduction="mean" (lambdaL.py:88-89) -- as one more float of
    the SAME buffer; after the single all-reduce every rank divides by the global normaliser on the device.  Ragged
    shards and data-dependent normalisers therefore cost no second collective and no host read."""

    def __init__(self, local_step, optimizer, group=None, always_collective=False):
        self.local = local_step
        self.opt = optimizer
        self.group = group
        self.rank, self.world_size = world()
        # always_collective: issue the all-reduce even at world_size 1 (exercises the backend on a one-GPU box)
        self.collective = self.world_size > 1 or (always_collective and dist.is_available() and dist.is_initialized())
        self.deferred = all(hasattr(local_step, a) for a in ("flat_ext", "finish_norm"))
        self.comm_events = None
        # every rank draws its OWN dropout stream: the keep bits are keyed on (seed, local document index), so
        # without a per-rank salt document i of every shard would share one mask (ltr_scorer.hip keep_word)
        if hasattr(self.local, "seed_salt"):
            self.local.seed_salt = self.rank
        # a risk-loss ranker gathers its effectiveness-matrix rows over the same group inside its step
        if hasattr(self.local, "risk_group"):
            self.local.risk_group, self.local.risk_rank, self.local.risk_world = group, self.rank, self.world_size

    def global_batch_of(self, b_local, device):
        """Sum of the ranks' local batch sizes (one 8-byte all-reduce + host read): only for local steps WITHOUT the
        deferred-normalisation protocol."""
        if self.world_size == 1:
            return b_local
        t = torch.tensor([b_local], dtype=torch.int64, device=device)
        dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.group)
        return int(t.item())

    def step(self, X, y, global_batch=None, **extras):
        """One optimizer step on this rank's slates.  Returns the GLOBAL loss (0-dim tensor, no host sync).
        global_batch: total slates over all ranks this step when the caller knows it (equal shards: bench.py) -- the
        batch-mean loss is then pre-scaled inside the launch.  Default: deferred normalisation (see the class docstring);
        every rank must make the same choice.  extras: per-batch inputs of the local step, passed through (a risk loss's
        y_base= or base_cols=, sharded like X).  A risk loss has no normaliser and is not pre-scaled in either branch; with
        global_batch its ragged-shard gather needs no host read."""
        data_dependent = getattr(self.local, "mean_kind", None) == "pairs"
        ev = self.comm_events                   # optional (start, end) torch.cuda.Event pair around the collective (bench.py)
        if self.deferred and (global_batch is None or data_dependent):
            self.local.step(X, y, defer_norm=True, **extras)
            if self.collective:
                if ev is not None:
                    ev[0].record()
                dist.all_reduce(self.local.flat_ext, op=dist.ReduceOp.SUM, group=self.group)
                if ev is not None:
                    ev[1].record()
            self.local.finish_norm()
        else:
            gb = int(global_batch) if global_batch else self.global_batch_of(int(X.shape[0]), X.device)
            self.local.step(X, y, world_batch=gb, **extras)
            if self.collective:
                if ev is not None:
                    ev[0].record()
                dist.all_reduce(self.local.flat, op=dist.ReduceOp.SUM, group=self.group)
                if ev is not None:
                    ev[1].record()
        self.opt.step()
        return self.local.flat[-1]

    def step_ragged(self, X, y, slates, global_batch=None, **extras):
        """`step` for this rank's queries of unequal length (local_step.step_ragged: X [n_docs, F], y [n_docs], slates a
        ltr_mi355x.ragged.RaggedSlates of the rank's own queries).  global_batch: the total QUERY count over all ranks.  The same
        deferred-normalisation / one-all-reduce protocol as `step`, for the three listwise losses and -- with y_base= or base_cols=,
        sharded like X -- the risk losses (their rows are gathered inside the local step)."""
        data_dependent = getattr(self.local, "mean_kind", None) == "pairs"
        ev = self.comm_events
        if self.deferred and (global_batch is None or data_dependent):
            self.local.step_ragged(X, y, slates, defer_norm=True, **extras)
            buf = self.local.flat_ext
        else:
            gb = int(global_batch) if global_batch else self.global_batch_of(int(slates.n_queries), X.device)
            self.local.step_ragged(X, y, slates, world_batch=gb, **extras)
            buf = None
        if self.collective:
            if ev is not None:
                ev[0].record()
            dist.all_reduce(self.local.flat if buf is None else buf, op=dist.ReduceOp.SUM, group=self.group)
            if ev is not None:
                ev[1].record()
        if buf is not None:
            self.local.finish_norm()
        self.opt.step()
        return self.local.flat[-1]


class ModuleShardedTrainer:
    """Query-sharded data parallelism for scorers whose backward fills `param.grad` (the `make_model` networks of
    architeture/multiLayer.py): every rank runs forward + loss + backward on its slates, then ONE all-reduce(SUM) of the
    flattened gradients (+ the loss) and the optimizer step.  `reduction`: "mean" (approxNDCG: each rank's gradient is
    weighted by B_local / B_global first) or "sum" (ListNet, lambdaLoss with reduction="sum").  Every rank gets its own
    dropout streams (module.ltr_seed is offset by the rank).

    Not for the risk-sensitive losses: a risk value is batch-coupled, so the sum of per-shard risks (and of their gradients) is not
    the global-batch loss.  Train those with QueryShardedTrainer and a risk FusedRanker (see the module docstring)."""

    def __init__(self, module, optimizer, reduction="mean", group=None):
        if reduction not in ("mean", "sum"):
            raise ValueError("reduction must be 'mean' or 'sum'")
        self.module, self.opt, self.reduction, self.group = module, optimizer, reduction, group
        self.rank, self.world_size = world()
        if hasattr(module, "ltr_seed"):
            module.ltr_seed = (int(module.ltr_seed) + 0xA24BAED4963EE407 * self.rank) & ((1 << 64) - 1)
        self.params = [p for p in module.parameters() if p.requires_grad]

    def step(self, loss_closure, b_local, global_batch=None, weight=None):
        """loss_closure() -> this rank's loss (0-dim, attached to the graph).  Returns the GLOBAL loss (0-dim).
        reduction "mean": every rank's gradient and loss are weighted by `weight` (default: its batch size b_local; a
        0-dim device tensor for data-dependent normalisers such as a kept-pair count) and the weight rides along as the
        last float of the one all-reduced buffer -- no size collective, no host read."""
        self.opt.zero_grad(set_to_none=True)
        loss = loss_closure()
        loss.backward()
        if self.world_size > 1:
            dt = torch.float64 if any(p.dtype == torch.float64 for p in self.params) else torch.float32
            flat = torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1).to(dt) for p in self.params]
                             + [loss.detach().reshape(1).to(dt)])
            if self.reduction == "mean":
                if weight is None and global_batch:
                    flat = flat * (float(b_local) / int(global_batch))
                    w = None
                else:
                    w = (weight.detach().reshape(1).to(dt) if torch.is_tensor(weight) else
                         torch.full((1,), float(b_local if weight is None else weight), dtype=dt, device=flat.device))
                    flat = torch.cat([flat * w, w])
            else:
                w = None
            dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=self.group)
            if w is not None:
                flat = flat[:-1] / flat[-1]
            off = 0
            for p in self.params:
                g = flat[off:off + p.numel()].view_as(p).to(p.dtype)
                if p.grad is None:
                    p.grad = g.clone()
                else:
                    p.grad.copy_(g)
                off += p.numel()
            loss = flat[off]
        self.opt.step()
        return loss.detach()
