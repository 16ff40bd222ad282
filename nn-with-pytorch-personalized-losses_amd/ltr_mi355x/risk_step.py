"""The fused training step of the six risk-sensitive losses (losses/riskLosses/riskLosses.py, the reference's own contribution) behind
ltr_mi355x.scorer.FusedRanker:

    ranker = FusedRanker(net, loss="geoRiskLambdaLoss", risk_args=dict(alpha=5, return_strategy=2))
    loss = ranker.step(X, y, y_base=y_base)          # == riskLoss(net(X, None, None).squeeze(-1), y, y_base, **risk_args); backward()
    cols = ranker.baseline_columns(y, y_base)         # once per dataset; shuffled with X / y
    loss = ranker.step(X, y, base_cols=cols)          # same loss and gradients, the constant systems' pair work skipped

Launch chain (every step, any slate length 2..2048): scorer forward with the hidden activations saved (ltr_mlp_forward_save) ->
the [queries, systems] effectiveness matrix and d mat[:, 0] / d (model input) (ltr_risk_matrix_fwd; Lambda forms: all systems' column
sums first, ltr_lambda_colsum_sys_fwd; with cached baseline columns: ltr_risk_matrix_cached_fwd / ltr_lambda_risk_model_fwd, the model
only) -> the tail (flip, risks, return strategy, `negative`; value and d value / d mat in one launch, the same call and flags as the
module path) -> the scores gradient from the model column of d value / d mat (ltr_risk_scores_grad; Lambda forms: the pair backward
with that coefficient, ltr_lambda_colsum_sys_bwd_coef) -> scorer backward on the saved activations -> the weight-gradient reduce.

Data parallel (ltr_mi355x.dp.QueryShardedTrainer hands the ranker its process group): a risk value is NOT a sum over queries (the flip's
whole-matrix maximum, the column sums, the total, tRisk's mean and standard deviation are batch-wide), so every rank computes its own
rows of the matrix, ONE all_gather assembles the global matrix (each rank's rows padded to the largest shard, the row count in the
block's first float), every rank runs the deterministic tail on all of it -- identical value and d mat everywhere -- and back-propagates
its own rows.  The trainer's one all-reduce of [grads | loss] then sums the weight gradients; only rank 0 writes the loss slot.
"""
import torch

from ._lib import check
from .functional import MAX_SLATE, _lambda_args, _ptr, _stream   # noqa: F401  (MAX_SLATE: read as risk_step.MAX_SLATE)

RISK_LOSSES = ("geoRiskListnetLoss", "geoRiskLambdaLoss", "zRiskListnetLoss", "zRiskLambdaLoss", "tRiskListnetLoss", "tRiskLambdaLoss")
RISK_Z, RISK_GEO = 0, 1
_GZ = dict(alpha=5, listnet_transformation=1, return_strategy=1, negative=1, add_ideal_ranking_to_mat=1)
_T = dict(alpha=5, listnet_transformation=1, negative=1)
# the reference signatures' keyword arguments and defaults (riskLosses.py:8, :63, :128, :183, :247, :294)
DEFAULTS = {"geoRiskListnetLoss": _GZ, "zRiskListnetLoss": _GZ,
            "geoRiskLambdaLoss": dict(_GZ, weighing_scheme="ndcgLoss2PP_scheme"), "zRiskLambdaLoss": dict(_GZ, weighing_scheme="ndcgLoss2PP_scheme"),
            "tRiskListnetLoss": _T, "tRiskLambdaLoss": dict(_T, weighing_scheme="ndcgLoss2PP_scheme")}


class RiskSpec:
    """The options of one risk loss, checked on the host, and the flags the module path hands its kernels for them.  The scope is
    the module path's regular-shape fast path (riskLosses.py `_regular`, `_regular_pair`, `_lambda_loss_fused`, `_tail`); an option it
    sends to its tensor-algebra fallback raises NotImplementedError."""

    def __init__(self, name, risk_args=None):
        if name not in DEFAULTS:
            raise KeyError(f"risk loss must be one of {list(RISK_LOSSES)}, got {name!r}")
        args = dict(DEFAULTS[name])
        for k, v in (risk_args or {}).items():
            if k not in args:
                raise TypeError(f"{name}() got an unexpected keyword argument {k!r}")
            args[k] = v
        self.name, self.args = name, args
        self.t = name.startswith("tRisk")
        self.lam = "Lambda" in name
        self.kind = RISK_GEO if name.startswith("geo") else RISK_Z
        self.alpha = float(args["alpha"])
        lt = args["listnet_transformation"]
        if isinstance(args["negative"], torch.Tensor) or not isinstance(args["negative"], (int, float)):
            raise NotImplementedError(f"{name}: the fused step takes a plain-number `negative`, got {type(args['negative']).__name__}")
        self.factor = float(args["negative"])
        ok_lt = (1, 2) if (self.lam and not self.t) else (1, 2, 3)
        if lt not in ok_lt:
            raise NotImplementedError(f"{name}: listnet_transformation={lt!r} is not on the fused path (takes {ok_lt})")
        self.lt = int(lt)
        self.strategy = 1
        if not self.t:
            if args["return_strategy"] not in (1, 2, 3):
                raise NotImplementedError(f"{name}: return_strategy={args['return_strategy']!r} is not on the fused path (takes 1, 2, 3)")
            self.strategy = int(args["return_strategy"])
            add_ideal = args["add_ideal_ranking_to_mat"]
        else:
            add_ideal = 1
        if self.lam:
            # the module path's lambdaMask arguments (riskLosses.py LambdaRiskLoss / lambda_colsum_systems)
            a = _lambda_args(1e-10, -1, args["weighing_scheme"], None, 1., 10., "binary")
            self.largs = (a[0], max(a[1], 0)) + a[2:]
        self.ones = (not self.t) and self.lam and self.kind == RISK_GEO and add_ideal == 2 and self.lt == 2
        self.ideal = (not self.t) and add_ideal == 2 and not self.ones          # the ideal ranking's column, computed
        self.flip = self.lt == 1 if (self.lam or self.t) else self.lt in (1, 3)
        self.zquirk = name == "zRiskListnetLoss"
        self.mode = 1 if self.lam else (2 if self.t else 0)

    def n_const(self, nb):
        """Matrix columns after the model's: baselines, ideal ranking, ones column."""
        return nb + int(self.ideal) + int(self.ones)

    def baselines(self, B, S, y_base):
        """y_base -> fp32 [B, S, nb] contiguous (nb = 1 for tRisk, which takes [B, S] or [B, S, 1]); shapes checked."""
        if y_base is None:
            raise ValueError(f"{self.name}: pass y_base= ([B, S, n] baseline scores{', or [B, S]' if self.t else ''}) or base_cols=")
        yb = y_base.detach()
        if self.t:
            if yb.dim() == 3 and yb.shape[2] == 1:
                yb = yb[:, :, 0]
            if yb.dim() != 2 or tuple(yb.shape) != (B, S):
                raise ValueError(f"{self.name}: y_base must be [B, S] = [{B}, {S}] (one baseline), got {tuple(y_base.shape)}")
            yb = yb.unsqueeze(2)
        elif yb.dim() != 3 or tuple(yb.shape[:2]) != (B, S) or not 2 <= yb.shape[2] <= 64:
            raise ValueError(f"{self.name}: y_base must be [B, S, n] = [{B}, {S}, 2..64], got {tuple(y_base.shape)}")
        return yb.to(torch.float32).contiguous()

    def cached(self, B, S, base_cols):
        """base_cols -> (fp32 [B, C] with unit column stride, number of cached matrix entries per row); shapes checked."""
        if base_cols.dim() != 2 or base_cols.shape[0] != B:
            raise ValueError(f"{self.name}: base_cols must be [B, C] = [{B}, C] (FusedRanker.baseline_columns), got {tuple(base_cols.shape)}")
        n_c = int(base_cols.shape[1]) - (S if self.lam else 0)
        nb = n_c - int(self.ideal) - int(self.ones)
        if (self.t and nb != 1) or (not self.t and not 2 <= nb <= 64):
            raise ValueError(f"{self.name}: base_cols of width {base_cols.shape[1]} do not belong to slates of {S} documents")
        bc = base_cols.detach()
        if bc.dtype != torch.float32 or bc.stride(1) != 1 or (B > 1 and bc.stride(0) < bc.shape[1]):
            bc = bc.to(torch.float32).contiguous()
        return bc, n_c


def baseline_columns(spec, yy, yb):
    """[B, C] per-query constants of the risk matrix: the baselines' (and ideal ranking's, and the ones column's) entries; for the
    Lambda forms followed by the ideal ranking's column sums [S].  Computed by the same launches as the uncached step, so the matrix the
    cached step feeds the tail is bitwise the same."""
    from ._lib import lib
    h = lib()
    B, S = yy.shape
    nb = yb.shape[2]
    n_c = spec.n_const(nb)
    dev = yy.device
    mat = torch.empty((B, 1 + n_c), dtype=torch.float32, device=dev)
    if spec.lam:
        cs = torch.empty((nb + 2, B, S), dtype=torch.float32, device=dev)
        check(h.ltr_lambda_colsum_sys_fwd(_ptr(yy), _ptr(yy), _ptr(yb), B, S, nb, *spec.largs, _ptr(cs), _stream()), "ltr_lambda_colsum_sys_fwd")
        check(h.ltr_risk_matrix_rows_fwd(_ptr(cs[nb + 1]), _ptr(cs[0]), _ptr(cs[1:nb + 1]), B, S, nb, 1, spec.lt, int(spec.ideal),
                                         int(spec.ones), _ptr(mat), None, _stream()), "ltr_risk_matrix_rows_fwd")
        return torch.cat([mat[:, 1:], cs[nb + 1]], 1)
    check(h.ltr_risk_matrix_fwd(_ptr(yy), _ptr(yy), _ptr(yb), B, S, nb, spec.mode, spec.lt, int(spec.ideal), _ptr(mat), None, _stream()),
          "ltr_risk_matrix_fwd")
    return mat[:, 1:].contiguous()


def matrix(h, spec, scores, yy, yb, cache, n_c, mat, jac):
    """Rows [B, 1 + n_c] of the effectiveness matrix into `mat` and d mat[:, 0] / d (scores or model column sums) into `jac`."""
    B, S = yy.shape
    if cache is not None:
        cs_ = int(cache.stride(0)) if B > 1 else int(cache.shape[1])
        if spec.lam:
            check(h.ltr_lambda_risk_model_fwd(_ptr(scores), _ptr(yy), _ptr(cache), cs_, n_c, B, S, *spec.largs, spec.lt, _ptr(mat), _ptr(jac),
                                              _stream()), "ltr_lambda_risk_model_fwd")
        else:
            check(h.ltr_risk_matrix_cached_fwd(_ptr(yy), _ptr(scores), _ptr(cache), cs_, B, S, n_c, spec.mode, spec.lt, _ptr(mat), _ptr(jac),
                                               _stream()), "ltr_risk_matrix_cached_fwd")
        return
    nb = yb.shape[2]
    if spec.lam:
        cs = torch.empty((nb + 2, B, S), dtype=torch.float32, device=yy.device)
        check(h.ltr_lambda_colsum_sys_fwd(_ptr(scores), _ptr(yy), _ptr(yb), B, S, nb, *spec.largs, _ptr(cs), _stream()),
              "ltr_lambda_colsum_sys_fwd")
        check(h.ltr_risk_matrix_rows_fwd(_ptr(cs[nb + 1]), _ptr(cs[0]), _ptr(cs[1:nb + 1]), B, S, nb, 1, spec.lt, int(spec.ideal),
                                         int(spec.ones), _ptr(mat), _ptr(jac), _stream()), "ltr_risk_matrix_rows_fwd")
    else:
        check(h.ltr_risk_matrix_fwd(_ptr(yy), _ptr(scores), _ptr(yb), B, S, nb, spec.mode, spec.lt, int(spec.ideal), _ptr(mat), _ptr(jac),
                                    _stream()), "ltr_risk_matrix_fwd")


def tail(h, spec, mat, Q, nsys, value, dmat):
    """The module path's tail call on a dense [Q, nsys] matrix."""
    if spec.t:
        check(h.ltr_trisk_tail_fwd_bwd(_ptr(mat), Q, spec.alpha, int(spec.flip), spec.factor, _ptr(value), _ptr(dmat), _stream()),
              "ltr_trisk_tail_fwd_bwd")
    else:
        check(h.ltr_risk_tail_fwd_bwd(_ptr(mat), Q, nsys, spec.alpha, spec.kind, spec.strategy, int(spec.flip), spec.factor, int(spec.zquirk),
                                      _ptr(value), _ptr(dmat), _stream()), "ltr_risk_tail_fwd_bwd")


def tail_blocks(h, spec, blocks, n_blocks, block_rows, nsys, value, dmat):
    """The same tail over the all-gathered, per-rank padded blocks (row counts read on the device)."""
    if spec.t:
        check(h.ltr_trisk_tail_blocks_fwd_bwd(_ptr(blocks), n_blocks, block_rows, spec.alpha, int(spec.flip), spec.factor, _ptr(value),
                                              _ptr(dmat), _stream()), "ltr_trisk_tail_blocks_fwd_bwd")
    else:
        check(h.ltr_risk_tail_blocks_fwd_bwd(_ptr(blocks), n_blocks, block_rows, nsys, spec.alpha, spec.kind, spec.strategy, int(spec.flip),
                                             spec.factor, int(spec.zquirk), _ptr(value), _ptr(dmat), _stream()), "ltr_risk_tail_blocks_fwd_bwd")


def scores_grad(h, spec, scores, yy, jac, coef_ptr, nsys, ds):
    """d value / d scores from the model column of d value / d mat (read in place at row stride nsys)."""
    B, S = yy.shape
    if spec.lam:
        check(h.ltr_lambda_colsum_sys_bwd_coef(_ptr(scores), _ptr(yy), B, S, *spec.largs, _ptr(jac), coef_ptr, nsys, _ptr(ds), _stream()),
              "ltr_lambda_colsum_sys_bwd_coef")
    else:
        check(h.ltr_risk_scores_grad(_ptr(jac), coef_ptr, nsys, B, S, _ptr(ds), _stream()), "ltr_risk_scores_grad")


def matrix_rows(spec, device, dp, B, nsys, world_batch):
    """Where a step writes its [B, nsys] matrix rows -> (mat, send, bmax).  dp = (group, rank, world).  One process: a dense matrix
    (send is None).  Data parallel (world > 1): the rows sit inside this rank's block of the gather -- padded to the largest shard `bmax`,
    behind one float holding the row count."""
    import torch.distributed as dist
    group, _, world = dp
    if world <= 1:
        return torch.empty((B, nsys), dtype=torch.float32, device=device), None, B
    if world_batch:
        bmax = -(-int(world_batch) // world)
    else:                                     # one size exchange (as QueryShardedTrainer.global_batch_of)
        t = torch.tensor([B], dtype=torch.int64, device=device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX, group=group)
        bmax = int(t.item())
    if B > bmax:
        raise ValueError(f"{spec.name}: this rank holds {B} queries, more than ceil(global batch / world) = {bmax}: shard with "
                         "ltr_mi355x.dp.shard_range")
    send = torch.empty(1 + bmax * nsys, dtype=torch.float32, device=device)
    send[:1].fill_(float(B))
    return send[1:1 + B * nsys].view(B, nsys), send, bmax


def run_tail(h, spec, dp, loss_slot, mat, send, bmax, B, nsys):
    """[ONE all_gather of the padded row blocks ->] the tail on the whole matrix, its value into `loss_slot` (rank 0 alone under data
    parallel: the all-reduced slot holds the global value once) -> (device address of d value / d mat of this rank's first row, the
    tensor it points into)."""
    import torch.distributed as dist
    dev = mat.device
    if send is None:
        dmat = torch.empty((B, nsys), dtype=torch.float32, device=dev)
        tail(h, spec, mat, B, nsys, loss_slot, dmat)
        return dmat.data_ptr(), dmat
    group, rank, world = dp
    stride = send.numel()
    recv = torch.empty((world, stride), dtype=torch.float32, device=dev)
    dist.all_gather(list(recv.unbind(0)), send, group=group)
    drecv = torch.empty_like(recv)
    value = loss_slot if rank == 0 else torch.empty(1, dtype=torch.float32, device=dev)
    tail_blocks(h, spec, recv, world, bmax, nsys, value, drecv)
    if rank != 0:
        loss_slot.fill_(0.0)
    return drecv.data_ptr() + 4 * (rank * stride + 1), drecv
