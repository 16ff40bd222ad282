"""Queries of unequal length without padding: the host side of the ltr_*_ragged_* entry points (include/ltr_mi355x.h).

A ragged batch is `scores [n_docs]`, `labels [n_docs]` (for a training step: `X [n_docs, F]`) plus a `RaggedSlates`, which holds
the int64 offsets (query q owns rows offsets[q] .. offsets[q + 1] - 1) and, per LENGTH TIER, the sorted list of the queries in it.
The loss kernels pick their launch geometry from the slate length (csrc/ltr_device.h pick_group / make_group), so a ragged batch
runs as one launch per occupied tier over that tier's query list; inside a tier every length has the same next power of two and
with it the same threads per slate, row lanes, column groups and barrier counts.

Each loss is the reference's loss on every query as a batch of one, combined by the reference's own reduction: approxNDCG the mean
over the queries (approxNDCG.py:53), ListNet the sum (listnet.py:16), lambdaLoss the sum of the kept-pair terms, or that sum over
the total kept-pair count for reduction="mean" (lambdaL.py:88-89).

    X, y, qid = load_svmlight(path)
    slates = RaggedSlates.from_qid(qid, device="cuda")
    Xd, yd = torch.as_tensor(X, device="cuda"), torch.as_tensor(y, device="cuda", dtype=torch.float32)
    for q0 in range(0, slates.n_queries, 2000):
        b = slates.batch(q0, min(q0 + 2000, slates.n_queries))
        d0, d1 = slates.doc_range(q0, q0 + b.n_queries)
        loss = ranker.step_ragged(Xd[d0:d1], yd[d0:d1], b)
"""
import functools

import numpy as np
import torch

from ._lib import check, lib
from .functional import MAX_SLATE, _f32, _lambda_args, _ptr, _reduce, _stream, require_device

# Upper ends of the length tiers.  Powers of two (the geometry rule above), with 256 on its own: lambdaLoss sends 256 .. 1024
# down the rank-space kernel (every scheme but ndcgLoss1), 129 .. 255 down the document-order one.
TIER_HI = (1, 2, 4, 8, 16, 32, 64, 128, 255, 256, 512, 1024, 2048)


def tier_of(sizes):
    """Index into TIER_HI of every length in `sizes` (1 .. MAX_SLATE)."""
    return np.searchsorted(np.asarray(TIER_HI), np.asarray(sizes), side="left")


class RaggedSlates:
    """The query structure of a ragged collection or batch: host sizes / offsets, device int64 offsets and one device int32 array
    `order` holding the query ids sorted by (tier, id), with the host array `tier_start` marking each tier's slice.

    bounds: [Q + 1] ascending integers with bounds[0] = 0 (ltr_mi355x.data.query_bounds).  Every query has 1 .. 2048 documents;
    anything else is a ValueError here, before any launch.  The device arrays are made on first use (`device=` or `.to(device)`)."""

    def __init__(self, bounds, device=None):
        b = np.asarray(bounds)
        if b.ndim != 1 or b.size < 1:
            raise ValueError(f"bounds must be a 1-D array of Q + 1 offsets, got shape {b.shape}")
        if b.dtype.kind not in "iu":
            raise ValueError(f"bounds must be integers, got {b.dtype}")
        b = b.astype(np.int64)
        if b[0] != 0:
            raise ValueError(f"bounds[0] must be 0, got {int(b[0])}")
        sizes = np.diff(b)
        if sizes.size and (sizes < 1).any():
            q = int(np.flatnonzero(sizes < 1)[0])
            raise ValueError(f"query {q} has {int(sizes[q])} documents: offsets must ascend strictly (no empty query)")
        if sizes.size and (sizes > MAX_SLATE).any():
            q = int(np.flatnonzero(sizes > MAX_SLATE)[0])
            raise ValueError(f"query {q} has {int(sizes[q])} documents, outside the supported range 1..{MAX_SLATE}")
        self.offsets_host = b
        self.sizes = sizes
        tiers = tier_of(sizes)
        self.order_host = np.argsort(tiers, kind="stable").astype(np.int32)            # by tier, then by query id
        self.tier_start = np.searchsorted(tiers[self.order_host], np.arange(len(TIER_HI) + 1), side="left").astype(np.int64)
        self.device = None
        self.offsets = self.order = None
        self._tiers = None
        if device is not None:
            self.to(device)

    @classmethod
    def from_qid(cls, qid, device=None):
        """From the per-document query ids of a LETOR file (a new query starts where qid changes, utils/dataset.py:54-60)."""
        from .data import query_bounds
        return cls(query_bounds(qid), device=device)

    @classmethod
    def _made(cls, offsets_host, order_host, tier_start, device, offsets, order):
        self = cls.__new__(cls)
        self.offsets_host, self.sizes = offsets_host, np.diff(offsets_host)
        self.order_host, self.tier_start = order_host, tier_start
        self.device, self.offsets, self.order = device, offsets, order
        self._tiers = None
        return self

    def to(self, device):
        device = torch.device(device)
        if device.type != "cuda":
            from ._lib import LtrDeviceError
            raise LtrDeviceError("RaggedSlates' device arrays feed HIP kernels: they live on a ROCm device")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if self.device != device:
            self.offsets = torch.as_tensor(self.offsets_host, device=device)
            self.order = torch.as_tensor(self.order_host, device=device)
            self.device = device
        return self

    @property
    def n_queries(self):
        return int(self.sizes.size)

    @property
    def n_docs(self):
        return int(self.offsets_host[-1])

    @property
    def max_len(self):
        return int(self.sizes.max()) if self.sizes.size else 0

    def doc_range(self, q0, q1):
        """(first row, one past the last row) of queries q0 .. q1 - 1."""
        return int(self.offsets_host[q0]), int(self.offsets_host[q1])

    def tiers(self):
        """[(s_max, start, count)] per OCCUPIED tier: order[start : start + count] are its queries (ascending ids), s_max the longest."""
        if self._tiers is None:
            out = []
            for t in range(len(TIER_HI)):
                a, b = int(self.tier_start[t]), int(self.tier_start[t + 1])
                if b > a:
                    out.append((int(self.sizes[self.order_host[a:b]].max()), a, b - a))
            self._tiers = out
        return self._tiers

    def batch(self, q0, q1):
        """The sub-batch of the consecutive queries q0 .. q1 - 1: offsets rebased to its first document, tier lists sliced (each
        tier's list is sorted by query id, so a range of ids is one contiguous slice of it) and rebased to q0.  Host arithmetic
        and device slicing only: nothing waits for the device."""
        q0, q1 = int(q0), int(q1)
        if not 0 <= q0 <= q1 <= self.n_queries:
            raise ValueError(f"batch({q0}, {q1}) outside 0..{self.n_queries}")
        off_h = self.offsets_host[q0:q1 + 1] - self.offsets_host[q0]
        cuts, start = [], [0]
        for t in range(len(TIER_HI)):
            a, b = int(self.tier_start[t]), int(self.tier_start[t + 1])
            seg = self.order_host[a:b]
            lo, hi = a + int(np.searchsorted(seg, q0, side="left")), a + int(np.searchsorted(seg, q1, side="left"))
            cuts.append((lo, hi))
            start.append(start[-1] + hi - lo)
        order_h = (np.concatenate([self.order_host[lo:hi] for lo, hi in cuts]) - q0).astype(np.int32) if cuts else self.order_host[:0]
        offsets = order = None
        if self.device is not None:
            offsets = self.offsets[q0:q1 + 1] - int(self.offsets_host[q0])
            parts = [self.order[lo:hi] for lo, hi in cuts if hi > lo]
            order = (torch.cat(parts) - q0) if parts else self.order[:0]
        return RaggedSlates._made(off_h, order_h, np.asarray(start, dtype=np.int64), self.device, offsets, order)

    def fixed_length(self, S, mode="first", seed=0):
        """The fixed-length view of these queries (config.json data.slate_length): ltr_mi355x.slates.fixed_length(self, ...)."""
        from .slates import fixed_length
        return fixed_length(self, S, mode=mode, seed=seed)

    def permuted(self, perm):
        """Queries in the order `perm` (a permutation of 0 .. Q - 1, host array or tensor): returns (new_slates, doc_index) where
        doc_index [n_docs] int64 (on the slates' device when they have one) lists the old document rows in their new order --
        `gather_rows(X, doc_index)`, `gather_rows(y[:, None], doc_index)` is the ragged counterpart of EpochShuffler."""
        p = perm.detach().cpu().numpy() if torch.is_tensor(perm) else np.asarray(perm)
        p = p.astype(np.int64)
        if p.shape != (self.n_queries,) or not np.array_equal(np.sort(p), np.arange(self.n_queries)):
            raise ValueError(f"perm must be a permutation of 0..{self.n_queries - 1}")
        sizes = self.sizes[p]
        bounds = np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)
        # row r of new query j is old row offsets[p[j]] + (r - bounds[j])
        doc = np.repeat(self.offsets_host[:-1][p] - bounds[:-1], sizes) + np.arange(int(bounds[-1]), dtype=np.int64)
        new = RaggedSlates(bounds, device=self.device)
        idx = torch.as_tensor(doc, device=self.device) if self.device is not None else torch.as_tensor(doc)
        return new, idx


# ------------------------------------------------------------------------------------------------------- launches
def _flat(t, name, n_docs):
    if t.dim() == 2 and t.shape[1] == 1:
        t = t[:, 0]
    if t.dim() != 1 or int(t.shape[0]) != n_docs:
        raise ValueError(f"{name} must have shape [n_docs] = [{n_docs}], got {tuple(t.shape)}")
    return t


def _slates_on(slates, dev):
    if not isinstance(slates, RaggedSlates):
        raise TypeError(f"slates must be a RaggedSlates, got {type(slates).__name__}")
    return slates.to(dev)


def launch_loss(h, kind, slates, scores, labels, slate_loss, count, ds, scale, args):
    """One launch per occupied tier of `slates`.  kind 0 approxNDCG (args = alpha, eps, pad), 1 ListNet (args = apply_sigmoid;
    `labels` are y_true), 2 lambdaLoss (args = _lambda_args).  Pointers are raw device addresses (None = NULL)."""
    off = slates.offsets.data_ptr()
    base = slates.order.data_ptr()
    for s_max, a, n in slates.tiers():
        q = base + 4 * a
        if kind == 0:
            alpha, eps, pad = args
            check(h.ltr_approxndcg_ragged_fwd_bwd(scores, labels, off, q, n, s_max, alpha, eps, pad, scale, slate_loss, ds, _stream()),
                  "ltr_approxndcg_ragged_fwd_bwd")
        elif kind == 1:
            check(h.ltr_listnet_ragged_fwd_bwd(labels, scores, off, q, n, s_max, int(args), scale, slate_loss, ds, _stream()),
                  "ltr_listnet_ragged_fwd_bwd")
        else:
            sid, kk, sigma, mu, eps, pad, lb = args
            check(h.ltr_lambda_ragged_fwd_bwd(scores, labels, off, q, n, s_max, sid, kk, sigma, mu, eps, pad, lb, scale, slate_loss,
                                              count, ds, _stream()), "ltr_lambda_ragged_fwd_bwd")


@functools.lru_cache(maxsize=None)
def _ragged_loss():
    """The autograd node of the three ragged losses.  Built on first use rather than at module level: tests/test_autograd_state_cpu.py
    pairs every module-level Function of the package with an entry of the table in tests/test_autograd_state_gpu.py; this node's
    state test (inputs changed between forward and backward) is tests/test_ragged_gpu.py::test_backward_uses_forward_time_state.  Its
    backward reads nothing but the gradient the forward launches saved."""
    class _RaggedLoss(torch.autograd.Function):
        """One autograd node for the three losses: forward and d loss / d scores in the forward launches, gradient to the scores only."""

        @staticmethod
        def forward(ctx, scores, labels, slates, kind, args, reduction):
            require_device(scores, labels)
            slates = _slates_on(slates, scores.device)
            n, Q = slates.n_docs, slates.n_queries
            s_in, y_in = _flat(scores, "scores", n), _flat(labels, "labels", n)
            out_dtype = torch.result_type(scores, labels)
            ctx.in_dtype, ctx.in_shape = scores.dtype, scores.shape
            dev = scores.device
            lambda_mean = kind == 2 and reduction == "mean"
            if Q == 0 or (kind == 2 and args[1] < 0):
                # the reference's reductions of nothing: mean -> nan, sum -> 0 (k = 0 keeps no pair, lambdaL.py:29-30); zero gradient
                ctx.save_for_backward(torch.zeros(n, dtype=torch.float32, device=dev))
                v = float("nan") if (lambda_mean or (kind == 0 and Q == 0)) else 0.0
                return torch.full((), v, dtype=out_dtype, device=dev)
            with torch.cuda.device(dev):
                s, y = _f32(s_in), _f32(y_in)
                slate = torch.empty(Q, dtype=torch.float32, device=dev)
                count = torch.empty(Q, dtype=torch.float32, device=dev) if kind == 2 else None
                ds = torch.empty(n, dtype=torch.float32, device=dev) if ctx.needs_input_grad[0] else None
                scale = 1.0 / Q if kind == 0 else 1.0
                launch_loss(lib(), kind, slates, _ptr(s), _ptr(y), _ptr(slate), _ptr(count), _ptr(ds), scale, args)
                loss = _reduce(slate, scale)
                if lambda_mean:
                    nk = _reduce(count, 1.0)
                    loss = loss / nk
                    if ds is not None:
                        ds = ds / torch.where(nk > 0, nk, torch.ones_like(nk))      # no kept pair: nan loss, zero gradients
            ctx.save_for_backward(ds)
            return loss.to(out_dtype)

        @staticmethod
        def backward(ctx, go):
            (ds,) = ctx.saved_tensors
            return (ds * go.to(torch.float32)).to(ctx.in_dtype).reshape(ctx.in_shape), None, None, None, None, None
    return _RaggedLoss


def approx_ndcg(scores, labels, slates, eps=1e-10, padded_value_indicator=-1, alpha=1.):
    """approxNDCGLoss (losses/approxNDCG.py:7-53) on a ragged batch: the mean over the queries of each query's own loss."""
    return _ragged_loss().apply(scores, labels, slates, 0, (float(alpha), float(eps), float(padded_value_indicator)), None)


def listnet(y_true, y_pred, slates, apply_sigmoid=False):
    """listnetLoss (losses/listnet.py:5-16) on a ragged batch: both softmaxes run over exactly the query's own documents; the sum."""
    return _ragged_loss().apply(y_pred, y_true, slates, 1, bool(apply_sigmoid), None)


def lambda_loss(scores, labels, slates, eps=1e-10, padded_value_indicator=-1, weighing_scheme=None, k=None, sigma=1., mu=10.,
                reduction="sum", reduction_log="binary"):
    """lambdaLoss (losses/lambdaL.py:67-93) on a ragged batch; `k` truncates on each query's own predicted ranks."""
    args = _lambda_args(eps, padded_value_indicator, weighing_scheme, k, sigma, mu, reduction_log)
    if reduction not in ("sum", "mean"):
        raise ValueError("Reduction method can be either sum or mean")             # lambdaL.py:91
    return _ragged_loss().apply(scores, labels, slates, 2, args, reduction)


def ndcg_at_k(y_true, y_score, slates, k=5, no_relevant=True, gains="linear", reverse_ties=False, want="ndcg"):
    """Per-query NDCG@k (or DCG@k) of a ragged batch, [Q] fp64 device tensor (utils/metrics.py:48-74 per query; k is clamped to
    the query's own length, :54-55; k=None: every document).  Ranked in fp32 like ltr_mi355x.metrics.ndcg_at_k."""
    from .metrics import GAINS, to_device_f32
    if gains not in GAINS:
        raise ValueError("Invalid gains option.")                                  # metrics.py:62
    s = to_device_f32(y_score)
    y = to_device_f32(y_true, like=s)
    slates = _slates_on(slates, s.device)
    n, Q = slates.n_docs, slates.n_queries
    s, y = _flat(s, "y_score", n), _flat(y, "y_true", n)
    out = torch.empty(Q, dtype=torch.float64, device=s.device)
    kk = int(k) if k is not None else MAX_SLATE
    with torch.cuda.device(s.device):
        for s_max, a, cnt in slates.tiers():
            check(lib().ltr_ndcg_at_k_ragged(_ptr(y), _ptr(s), _ptr(slates.offsets), slates.order.data_ptr() + 4 * a, cnt, s_max, kk,
                                             GAINS[gains], int(bool(no_relevant)), int(bool(reverse_ties)),
                                             _ptr(out) if want == "ndcg" else None, _ptr(out) if want == "dcg" else None,
                                             _stream()), "ltr_ndcg_at_k_ragged")
    return out


def ndcg_of_lists(true_lists, pred_lists, **kw):
    """utils.metrics.mNdcg's ragged route: a list of per-query label lists and the matching score lists -> [Q] fp64."""
    if len(true_lists) != len(pred_lists):
        raise ValueError(f"{len(true_lists)} label lists but {len(pred_lists)} score lists")
    ys = [np.asarray(t.detach().cpu() if torch.is_tensor(t) else t, dtype=np.float32).reshape(-1) for t in true_lists]
    ss = [np.asarray(t.detach().cpu() if torch.is_tensor(t) else t, dtype=np.float32).reshape(-1) for t in pred_lists]
    for q, (a, b) in enumerate(zip(ys, ss)):
        if a.size != b.size:
            raise ValueError(f"query {q}: {a.size} labels but {b.size} scores")
    slates = RaggedSlates(np.concatenate(([0], np.cumsum([a.size for a in ys]))).astype(np.int64))
    return ndcg_at_k(np.concatenate(ys) if ys else np.zeros(0, np.float32), np.concatenate(ss) if ss else np.zeros(0, np.float32),
                     slates, **kw)


# ------------------------------------------------------------------------------------------------------- training step
def _step_batch(self, X, y, slates, train, keep1, keep2):
    """The host checks every ragged training step starts with -> (slates on X's device, y as [n_docs])."""
    self._check_trainable(train, keep1, keep2)
    require_device(X, y)
    slates = _slates_on(slates, X.device)
    n, F = slates.n_docs, self.info.F
    if X.dim() != 2 or X.shape[1] != F or int(X.shape[0]) != n:
        raise ValueError(f"expected X [n_docs = {n}, {F}], got {tuple(X.shape)}")
    return slates, _flat(y, "y", n)


def step_ragged(ranker, X, y, slates, world_batch=None, keep1=None, keep2=None, seed=None, train=None, defer_norm=False, y_base=None,
                base_cols=None):
    """FusedRanker.step_ragged: the ranker's chain (scorer forward with saved activations -> loss -> scorer backward; for the
    folded make_model ranker scores -> loss -> gradient partials) with the ragged loss launches in the middle.  Same flat
    [grads | loss | normaliser] buffer, same deferred-normalisation protocol as `step` (normaliser: the query count for approxNDCG,
    the kept-pair count for lambdaLoss "mean").  The six risk-sensitive losses: _step_ragged_risk below."""
    from .scorer import LOSS_LAMBDA
    self = ranker
    if self.risk is not None:
        return _step_ragged_risk(self, X, y, slates, world_batch, keep1, keep2, seed, train, y_base, base_cols)
    if y_base is not None or base_cols is not None:
        raise TypeError(f"y_base / base_cols belong to the risk-sensitive losses, not {self.loss!r}")
    slates, y1 = _step_batch(self, X, y, slates, train, keep1, keep2)
    Q = slates.n_queries
    scale = self._listwise_prelude(Q, world_batch, defer_norm, "step_ragged")
    if scale is None:
        self._bind_grads()
        return self._loss_out
    h = lib()
    with torch.cuda.device(self.device):
        yy = y1.detach().to(torch.float32).contiguous()
        count = self._loss_buffers(Q, self.loss_kind == LOSS_LAMBDA)

        def loss_launches(scores, ds):
            launch_loss(h, self.loss_kind, slates, _ptr(scores), _ptr(yy), _ptr(self._slate), _ptr(count), _ptr(ds), scale,
                        self._loss_args())

        self._chain(self._prepare(X, keep1, keep2, seed, train), loss_launches)
        self._listwise_epilogue(Q, scale, count, defer_norm)
    self._bind_grads()
    return self._loss_out


# ------------------------------------------------------------------------------------------------------- risk-sensitive losses
# The six losses of losses/riskLosses/riskLosses.py on a ragged batch.  Row q of the effectiveness matrix is
# the row the reference computes for query q inside any batch of queries of q's own length, before the flip: every entry comes from
# q's documents alone (softmaxes over its own slate, lambdaMask column sums in its own predicted-rank order).  The rows of all
# queries, in query order, form one [Q, n_systems] matrix, and the reference's tail runs once on it (the whole-matrix flip, the risk
# of column 0 and of the last column, the return strategy, `negative`) -- risk_step.run_tail, unchanged, gather included.
def check_risk_batch(spec, slates, y_base, base_cols, min_queries=2):
    """The host checks of a ragged risk step, from the host sizes alone (nothing here needs a device).  min_queries: 2 in one process
    (the rectangular risk step's limit), 0 for a rank of a data-parallel step and for the per-dataset baseline columns."""
    if y_base is None and base_cols is None:
        raise NotImplementedError(f"{spec.name}: a risk-sensitive loss compares the model with baseline rankers: call "
                                  "FusedRanker.step_ragged(X, y, slates, y_base=...) or (..., base_cols=baseline_columns_ragged(...))")
    if y_base is not None and base_cols is not None:
        raise ValueError(f"{spec.name}: pass exactly one of y_base= and base_cols=")
    if not isinstance(slates, RaggedSlates):
        raise TypeError(f"slates must be a RaggedSlates, got {type(slates).__name__}")
    sizes = slates.sizes
    if sizes.size and (sizes < 2).any():
        q = int(np.flatnonzero(sizes < 2)[0])
        raise ValueError(f"{spec.name}: query {q} has {int(sizes[q])} document; the risk-sensitive losses take queries of 2..{MAX_SLATE} "
                         "documents (a softmax over one document is constant)")
    if slates.n_queries < min_queries:
        raise NotImplementedError(f"{spec.name}: the fused step takes batches of at least 2 queries, got {slates.n_queries}")


def risk_baselines(spec, n_docs, y_base):
    """y_base -> fp32 [n_docs, nb] contiguous (nb = 1 for tRisk, which takes [n_docs] or [n_docs, 1]); shapes checked."""
    yb = y_base.detach()
    if spec.t:
        if yb.dim() == 2 and yb.shape[1] == 1:
            yb = yb[:, 0]
        if yb.dim() != 1 or int(yb.shape[0]) != n_docs:
            raise ValueError(f"{spec.name}: y_base must be [n_docs] = [{n_docs}] (one baseline), got {tuple(y_base.shape)}")
        yb = yb.unsqueeze(1)
    elif yb.dim() != 2 or int(yb.shape[0]) != n_docs or not 2 <= yb.shape[1] <= 64:
        raise ValueError(f"{spec.name}: y_base must be [n_docs, n] = [{n_docs}, 2..64], got {tuple(y_base.shape)}")
    return yb.to(torch.float32).contiguous()


def risk_cached(spec, slates, base_cols):
    """base_cols = (entries [Q, C], ideal_colsum [n_docs] or None) of baseline_columns_ragged -> the same pair, fp32 with unit
    strides; shapes checked."""
    if not isinstance(base_cols, (tuple, list)) or len(base_cols) != 2:
        raise ValueError(f"{spec.name}: base_cols must be the pair FusedRanker.baseline_columns_ragged returns")
    ent, ics = base_cols
    Q, n = slates.n_queries, slates.n_docs
    if ent.dim() != 2 or int(ent.shape[0]) != Q:
        raise ValueError(f"{spec.name}: base_cols[0] must be [Q, C] = [{Q}, C], got {tuple(ent.shape)}")
    nb = int(ent.shape[1]) - int(spec.ideal) - int(spec.ones)
    if (spec.t and nb != 1) or (not spec.t and not 2 <= nb <= 64):
        raise ValueError(f"{spec.name}: base_cols[0] of width {ent.shape[1]} does not belong to this loss")
    ent = ent.detach()
    if ent.dtype != torch.float32 or not ent.is_contiguous():
        ent = ent.to(torch.float32).contiguous()
    if spec.lam:
        if ics is None or ics.dim() != 1 or int(ics.shape[0]) != n:
            raise ValueError(f"{spec.name}: base_cols[1] must be the ideal ranking's column sums [n_docs] = [{n}]")
        ics = ics.detach().to(torch.float32).contiguous()
    else:
        ics = None
    return ent, ics


def _tier_lists(slates):
    base = slates.order.data_ptr()
    return [(s_max, base + 4 * a, cnt) for s_max, a, cnt in slates.tiers()]


def risk_matrix(h, spec, slates, scores, yy, yb, cache, mat, jac):
    """Rows [Q, 1 + n_const] of the effectiveness matrix into `mat`, d mat[:, 0] / d (scores or model column sums) into `jac`
    [n_docs] (None: not wanted) -- risk_step.matrix on a ragged batch.  Listnet forms: one launch for the whole batch; Lambda forms:
    the pair work per occupied tier, then (uncached) one matrix launch over the ragged column sums, which it returns."""
    off, n, Q, s_max = slates.offsets.data_ptr(), slates.n_docs, slates.n_queries, slates.max_len
    if cache is not None:
        ent, ics = cache
        n_c = int(ent.shape[1])
        if spec.lam:
            for t_max, q, cnt in _tier_lists(slates):
                check(h.ltr_lambda_risk_model_ragged_fwd(_ptr(scores), _ptr(yy), _ptr(ent), n_c, _ptr(ics), n_c, off, q, cnt, t_max, n,
                                                         *spec.largs, spec.lt, _ptr(mat), _ptr(jac), _stream()),
                      "ltr_lambda_risk_model_ragged_fwd")
        else:
            check(h.ltr_risk_matrix_ragged_fwd(_ptr(yy), _ptr(scores), None, off, None, Q, s_max, n, n_c, spec.mode, spec.lt, 0, 0,
                                               _ptr(ent), n_c, _ptr(mat), _ptr(jac), _stream()), "ltr_risk_matrix_ragged_fwd")
        return None
    nb = int(yb.shape[1])
    if spec.lam:
        cs = torch.empty((nb + 2, n), dtype=torch.float32, device=yy.device)
        for t_max, q, cnt in _tier_lists(slates):
            check(h.ltr_lambda_colsum_sys_ragged_fwd(_ptr(scores), _ptr(yy), _ptr(yb), off, q, cnt, t_max, n, nb, *spec.largs, _ptr(cs),
                                                     _stream()), "ltr_lambda_colsum_sys_ragged_fwd")
        check(h.ltr_risk_matrix_ragged_fwd(_ptr(cs[nb + 1]), _ptr(cs[0]), _ptr(cs[1:nb + 1]), off, None, Q, s_max, n, nb, 1, spec.lt,
                                           int(spec.ideal), int(spec.ones), None, 0, _ptr(mat), _ptr(jac), _stream()),
              "ltr_risk_matrix_ragged_fwd")
        return cs
    check(h.ltr_risk_matrix_ragged_fwd(_ptr(yy), _ptr(scores), _ptr(yb), off, None, Q, s_max, n, nb, spec.mode, spec.lt, int(spec.ideal),
                                       0, None, 0, _ptr(mat), _ptr(jac), _stream()), "ltr_risk_matrix_ragged_fwd")
    return None


def risk_scores_grad(h, spec, slates, scores, yy, jac, coef_ptr, nsys, ds):
    """d value / d scores from the model column of d value / d mat (read in place at row stride nsys): risk_step.scores_grad."""
    off, n = slates.offsets.data_ptr(), slates.n_docs
    if spec.lam:
        for t_max, q, cnt in _tier_lists(slates):
            check(h.ltr_lambda_colsum_sys_ragged_bwd_coef(_ptr(scores), _ptr(yy), off, q, cnt, t_max, n, *spec.largs, _ptr(jac), coef_ptr,
                                                          nsys, _ptr(ds), _stream()), "ltr_lambda_colsum_sys_ragged_bwd_coef")
    else:
        check(h.ltr_risk_scores_grad_ragged(_ptr(jac), coef_ptr, nsys, off, None, slates.n_queries, n, _ptr(ds), _stream()),
              "ltr_risk_scores_grad_ragged")


def baseline_columns(spec, slates, yy, yb):
    """(entries [Q, C], ideal_colsum [n_docs] or None): the constant part of the matrix, by the same launches as the uncached step
    (the model's slot runs on the labels and is dropped), so the cached step's matrix is bitwise the uncached one."""
    Q = slates.n_queries
    mat = torch.empty((Q, 1 + spec.n_const(int(yb.shape[1]))), dtype=torch.float32, device=yy.device)
    cs = risk_matrix(lib(), spec, slates, yy, yy, yb, None, mat, None)
    return mat[:, 1:].contiguous(), (cs[-1].clone() if cs is not None else None)


def _step_ragged_risk(self, X, y, slates, world_batch, keep1, keep2, seed, train, y_base, base_cols):
    """FusedRanker.step_ragged for a risk loss: scorer forward with saved activations -> matrix rows + jac -> [all_gather] -> tail ->
    scores gradient -> scorer backward -> reduce: FusedRanker._step_risk on [n_docs, F] rows, through the ranker's own chain."""
    from . import risk_step as RS
    R = self.risk
    check_risk_batch(R, slates, y_base, base_cols, 2 if self.risk_world <= 1 else 0)
    slates, y1 = _step_batch(self, X, y, slates, train, keep1, keep2)
    n, Q = slates.n_docs, slates.n_queries
    yb = cache = None
    if base_cols is not None:
        require_device(*[t for t in base_cols if torch.is_tensor(t)])
        cache = risk_cached(R, slates, base_cols)
        nsys = 1 + int(cache[0].shape[1])
    else:
        require_device(y_base)
        yb = risk_baselines(R, n, y_base)
        nsys = 1 + R.n_const(int(yb.shape[1]))
    h = lib()
    n_par = self.info.n_params
    dp = (self.risk_group, self.risk_rank, self.risk_world)
    with torch.cuda.device(self.device):
        yy = y1.detach().to(torch.float32).contiguous()
        mat, send, bmax = RS.matrix_rows(R, self.device, dp, Q, nsys, world_batch)
        slot = self.flat[n_par:n_par + 1]

        def loss_launches(scores, ds):
            jac = torch.empty(n, dtype=torch.float32, device=self.device)
            risk_matrix(h, R, slates, scores, yy, yb, cache, mat, jac)
            coef, _dmat = RS.run_tail(h, R, dp, slot, mat, send, bmax, Q, nsys)
            risk_scores_grad(h, R, slates, scores, yy, jac, coef, nsys, ds)

        if Q == 0:                                   # a rank without queries still joins the gather and runs the tail
            RS.run_tail(h, R, dp, slot, mat, send, bmax, Q, nsys)
            self.flat_grad.zero_()
        else:
            self._chain(self._prepare(X, keep1, keep2, seed, train), loss_launches)
    self._bind_grads()
    return self._loss_out


@functools.lru_cache(maxsize=None)
def _ragged_risk_loss():
    """The autograd node of the six ragged risk losses, built on first use like _ragged_loss (tests/test_autograd_state_cpu.py pairs
    every module-level Function with a table entry; this node's state test is tests/test_ragged_risk_gpu.py::
    test_risk_loss_backward_uses_forward_time_state).  Its backward reads nothing but the gradient the forward launches saved."""
    class _RaggedRiskLoss(torch.autograd.Function):
        @staticmethod
        def forward(ctx, scores, labels, baselines, slates, spec):
            from . import risk_step as RS
            check_risk_batch(spec, slates, baselines, None)
            require_device(scores, labels, baselines)
            slates = _slates_on(slates, scores.device)
            n, Q = slates.n_docs, slates.n_queries
            s_in, y_in = _flat(scores, "y_predicted", n), _flat(labels, "y_true", n)
            ctx.in_dtype, ctx.in_shape = scores.dtype, scores.shape
            dev = scores.device
            h = lib()
            with torch.cuda.device(dev):
                s, yy = _f32(s_in), _f32(y_in)
                yb = risk_baselines(spec, n, baselines)
                nsys = 1 + spec.n_const(int(yb.shape[1]))
                mat = torch.empty((Q, nsys), dtype=torch.float32, device=dev)
                value = torch.empty(1, dtype=torch.float32, device=dev)
                jac = ds = dmat = None
                if ctx.needs_input_grad[0]:          # an evaluation call runs the matrix and the tail's value alone
                    jac, ds = (torch.empty(n, dtype=torch.float32, device=dev) for _ in range(2))
                    dmat = torch.empty((Q, nsys), dtype=torch.float32, device=dev)
                risk_matrix(h, spec, slates, s, yy, yb, None, mat, jac)
                RS.tail(h, spec, mat, Q, nsys, value, dmat)
                if ds is not None:
                    risk_scores_grad(h, spec, slates, s, yy, jac, dmat.data_ptr(), nsys, ds)
            ctx.save_for_backward(ds)
            return value.to(torch.result_type(scores, labels))

        @staticmethod
        def backward(ctx, go):
            (ds,) = ctx.saved_tensors
            if ds is None:
                return None, None, None, None, None
            return (ds * go.to(torch.float32)).to(ctx.in_dtype).reshape(ctx.in_shape), None, None, None, None
    return _RaggedRiskLoss


def risk_loss(name, y_predicted, y_true, slates, y_baselines, **risk_args):
    """One of the six risk-sensitive losses (losses/riskLosses/riskLosses.py: name(y_predicted, y_true, y_baselines, **risk_args)) on a
    ragged batch: y_predicted / y_true [n_docs], y_baselines [n_docs, n] (tRisk: [n_docs] or [n_docs, 1]).  Shape [1], like the
    reference's; one autograd node, gradient to the scores only."""
    from .risk_step import RiskSpec
    return _ragged_risk_loss().apply(y_predicted, y_true, y_baselines, slates, RiskSpec(name, risk_args))


def geoRiskListnetLoss(y_predicted, y_true, slates, y_baselines, **risk_args):
    return risk_loss("geoRiskListnetLoss", y_predicted, y_true, slates, y_baselines, **risk_args)


def geoRiskLambdaLoss(y_predicted, y_true, slates, y_baselines, **risk_args):
    return risk_loss("geoRiskLambdaLoss", y_predicted, y_true, slates, y_baselines, **risk_args)


def zRiskListnetLoss(y_predicted, y_true, slates, y_baselines, **risk_args):
    return risk_loss("zRiskListnetLoss", y_predicted, y_true, slates, y_baselines, **risk_args)


def zRiskLambdaLoss(y_predicted, y_true, slates, y_baselines, **risk_args):
    return risk_loss("zRiskLambdaLoss", y_predicted, y_true, slates, y_baselines, **risk_args)


def tRiskListnetLoss(y_predicted, y_true, slates, y_baselines, **risk_args):
    return risk_loss("tRiskListnetLoss", y_predicted, y_true, slates, y_baselines, **risk_args)


def tRiskLambdaLoss(y_predicted, y_true, slates, y_baselines, **risk_args):
    return risk_loss("tRiskLambdaLoss", y_predicted, y_true, slates, y_baselines, **risk_args)
