"""Fused training step for FC-only `make_model` rankers (csrc/ltr_linear.hip).

FCModel and OutputLayer hard-wire nn.Identity activations (multiLayer.py:29, :105), so an LTRModel with no transformer,
`d_output = 1` and no active dropout is one affine map of its input (LayerNorm'd when `input_norm` is set):

    s = w_eff . h_0 + b_eff,    v_L = w_o,  v_{i-1} = v_i W_i,  w_eff = v_0,  b_eff = b_o + sum_i v_i . b_i.

Per step, from the live parameters: ltr_linear_fold (fp64) -> the one-launch step for S in {32, 64, 128} (scores, listwise
loss and the document sums G_1 = sum ds, Ghat = sum ds h_0 in one pass over X), or scores + loss kernel + gradient partials
for any other slate -> ltr_linear_unfold_grads (fp64), which writes every parameter's gradient into the flat buffer.
`FusedRanker(model)` returns a `LinearFusedRanker` for such a model; the module path (`model(x, mask, indices)`) is unchanged.

The six risk-sensitive losses (`loss="geoRiskListnetLoss"`, ..., `risk_args=`; `step(..., y_base=)` or `step(..., base_cols=)`, the
surface and data-parallel protocol of ltr_mi355x.risk_step).  Entry mat[q, 0] of their matrix depends on slate q's scores only, so with
j_d = d mat[q, 0] / d s_d and c_q = d value / d mat[q, 0] (the tail's output)

    [Ghat | G_1] = sum_q c_q R_q,      R_q = [ sum_d j_d h_0,d | sum_d j_d ]      (F + 1 floats per slate, known before the tail)

Listnet forms with S in {32, 64, 128}: fold -> ltr_linear_risk_rows (X read ONCE: scores, mat[:, 0], the cached constant columns, R)
-> [all_gather] -> tail -> ltr_linear_risk_combine -> unfold.  Every other case (Lambda forms, other slates, F > 256): fold ->
ltr_linear_scores -> risk_step.matrix -> [all_gather] -> tail -> risk_step.scores_grad -> ltr_linear_grad_partials -> unfold.
"""
import ctypes

import torch

from ._lib import check, lib
from .functional import _ptr, _stream, require_device
from .scorer import LOSS_APPROXNDCG, LOSS_LAMBDA, LOSS_LISTNET, LOSS_RISK, FusedRanker, cu_count

MAX_LAYERS = 16
MAX_FEATURES = 1024


class _Info:
    """What FusedRanker's shared methods read (`n_params`) plus the network's shape."""

    def __init__(self, n_features, sizes, input_norm, n_params):
        self.F = int(n_features)
        self.sizes = list(sizes)
        self.input_norm = bool(input_norm)
        self.n_params = int(n_params)


def linear_shape(model):
    """(n_features, fc sizes, input_norm, FC dropout module or None) of an FC-only LTRModel; NotImplementedError for what does
    not fold (a transformer encoder, d_output > 1)."""
    import torch.nn as nn
    if isinstance(model.encoder, nn.Module):
        raise NotImplementedError("the fused step folds FC-only make_model networks: a transformer encoder is not linear; train it "
                                  "through the module path (model(x, mask, indices) + the loss + backward())")
    out = model.output_layer
    if int(out.d_output) != 1:
        raise NotImplementedError(f"the fused step scores with d_output = 1 (multiLayer.py:113), got d_output = {out.d_output}; "
                                  "train it through the module path")
    fc = model.input_layer if hasattr(model.input_layer, "layers") else None
    if fc is None:
        F = int(out.w_1.in_features)
        return F, [], False, None
    lins = list(fc.layers)
    F = int(lins[0].in_features) if lins else int(out.w_1.in_features)
    return F, [int(l.out_features) for l in lins], isinstance(fc.input_norm, nn.LayerNorm), fc.dropout


class LinearFusedRanker(FusedRanker):
    """FusedRanker for an FC-only make_model LTRModel (see the module docstring).  Same interface and buffers as for
    DoubleLayerNet: `flat` = [grads | loss] aliased by every `p.grad`, `flat_ext` with the normaliser slot, `world_batch`,
    `defer_norm` / `finish_norm`, `kernel_events`."""

    def __init__(self, module, loss="approxNDCG", alpha=1.0, eps=1e-10, padded_value_indicator=-1, apply_sigmoid=False, grid=None,
                 weighing_scheme=None, k=None, sigma=1.0, mu=10.0, reduction="sum", reduction_log="binary", risk_args=None):
        if loss not in self.LOSSES:
            raise KeyError(f"fused loss must be one of {sorted(self.LOSSES)}, got {loss!r}")
        self.risk = None
        if self.LOSSES[loss] == LOSS_RISK:
            from .risk_step import RiskSpec
            self.risk = RiskSpec(loss, risk_args)          # option errors first: they need no device
            # data parallel: ltr_mi355x.dp.QueryShardedTrainer sets (group, rank, world) -- the risk step all-gathers its matrix rows
            self.risk_group = None
            self.risk_rank, self.risk_world = 0, 1
        elif risk_args is not None:
            raise TypeError(f"risk_args belongs to the risk-sensitive losses, not {loss!r}")
        F, sizes, ln, self._dropout = linear_shape(module)
        if len(sizes) > MAX_LAYERS:
            raise ValueError(f"at most {MAX_LAYERS} FC layers fold, got {len(sizes)}")
        if F > MAX_FEATURES:
            raise ValueError(f"at most {MAX_FEATURES} input features, got {F}")
        self.module = module
        self.loss = loss
        self.loss_kind = self.LOSSES[loss]
        self.alpha, self.eps, self.pad = float(alpha), float(eps), float(padded_value_indicator)
        self.apply_sigmoid = bool(apply_sigmoid)
        self.lambda_args = (4, 0, 1.0, 10.0, 1e-10, -1.0, 0)
        if self.loss_kind == LOSS_LAMBDA:
            from .functional import _lambda_args
            if reduction not in ("sum", "mean"):
                raise ValueError("Reduction method can be either sum or mean")
            self.lambda_args = _lambda_args(eps, padded_value_indicator, weighing_scheme, k, sigma, mu, reduction_log)
        self.reduction = reduction
        self.params = module._ltr_params()
        require_device(*self.params)
        self.info = _Info(F, sizes, ln, sum(p.numel() for p in self.params))
        dev = self.params[0].device
        self.device = dev
        h = lib()
        self.grid = int(grid) if grid else int(h.ltr_linear_grid(cu_count(dev)))
        self.flat_ext = torch.zeros(self.info.n_params + 2, dtype=torch.float32, device=dev)
        self.flat = self.flat_ext[:self.info.n_params + 1]
        self.flat_grad = self.flat[:self.info.n_params]
        self._norm = self.flat_ext[self.info.n_params + 1:]
        self._grad_views = []
        off = 0
        for p in self.params:
            self._grad_views.append(self.flat_grad[off:off + p.numel()].view_as(p))
            off += p.numel()
        self._bind_grads()
        self._sizes = (ctypes.c_int * max(1, len(sizes)))(*sizes)
        nws = int(h.ltr_linear_ws_doubles(len(sizes), F, self._sizes))
        check(-2 if nws < 0 else 0, "ltr_linear_ws_doubles")
        self.ws = torch.empty(nws, dtype=torch.float64, device=dev)         # fold -> unfold of ONE step; rewritten every step
        self.weff = torch.empty(F + 2, dtype=torch.float32, device=dev)
        self.partials = torch.empty(self.grid * (F + 1), dtype=torch.float32, device=dev)
        self._loss_out = self.flat[self.info.n_params]
        self._slate = None
        self._bufs = None              # scores / ds / stats of the multi-launch path (grown on demand)
        self._rows = None              # R [B][F + 1] of the one-pass risk step (grown on demand)
        self._jac = None               # d mat[:, 0] / d scores of the risk chain (grown on demand)
        self._calls = 0
        self.seed_salt = 0
        self.kernel_events = None

    def _param_ptrs(self):
        """Device pointers of the live parameters (fp32, contiguous), in _ltr_params() order -- read every step."""
        ps = []
        for p in self.params:
            t = p.detach()
            if t.dtype != torch.float32 or not t.is_contiguous():
                t = t.to(torch.float32).contiguous()
            ps.append(t)
        return ps, (ctypes.c_void_p * len(ps))(*[t.data_ptr() for t in ps])

    def _check_trainable(self, train, keep1, keep2):
        if keep1 is not None or keep2 is not None:
            raise NotImplementedError("keep1 / keep2 are DoubleLayerNet's dropout masks; an FC-only make_model network has none")
        train = self.module.training if train is None else bool(train)
        if train and self._dropout is not None and float(self._dropout.p) > 0:
            raise NotImplementedError(
                f"FC dropout p = {self._dropout.p} in training mode: the fused step folds the FC stack into one vector, which only "
                "exists without per-document dropout masks.  Train this network through the module path "
                "(model(x, mask, indices) + the loss + backward()), or call model.eval() / step(train=False) for p-free steps")

    def step(self, X, y, world_batch=None, keep1=None, keep2=None, seed=None, train=None, defer_norm=False, y_base=None, base_cols=None,
             _one_pass=None):
        """FusedRanker.step for the folded network (seed is accepted and unused: nothing here is random).  Risk losses: y_base or
        base_cols as in FusedRanker.step; `_one_pass=False` sends a Listnet form through the multi-launch chain (tests, benchmarks)."""
        info = self.info
        self._check_trainable(train, keep1, keep2)
        require_device(X, y)
        F = info.F
        if X.dim() != 3 or X.shape[2] != F or tuple(y.shape[:2]) != tuple(X.shape[:2]):
            raise ValueError(f"expected X [B,S,{F}] and y [B,S], got {tuple(X.shape)} / {tuple(y.shape)}")
        B, S = int(X.shape[0]), int(X.shape[1])
        if S < 1 or S > 2048:
            raise ValueError(f"slate_length {S} outside the supported range 1..2048")
        if self.risk is not None:
            return self._step_risk(X, y, B, S, self._risk_inputs(B, S, y_base, base_cols), world_batch, _one_pass)
        if y_base is not None or base_cols is not None:
            raise TypeError(f"y_base / base_cols belong to the risk-sensitive losses, not {self.loss!r}")
        lambda_mean = self.loss_kind == LOSS_LAMBDA and self.reduction == "mean"
        if lambda_mean and not defer_norm and world_batch not in (None, B):
            raise ValueError('lambdaLoss reduction="mean" divides by the GLOBAL kept-pair count, which no rank knows before '
                             "the all-reduce: under data parallel call step(defer_norm=True) (QueryShardedTrainer does)")
        if B == 0:
            self.flat_ext.zero_()
            if self.loss_kind == LOSS_APPROXNDCG and not world_batch and not defer_norm:
                self.flat[info.n_params] = float("nan")
            self._bind_grads()
            return self._loss_out
        if self.loss_kind == LOSS_LAMBDA and self.lambda_args[1] < 0:
            self.flat_ext.zero_()
            if lambda_mean and not defer_norm:
                self.flat[info.n_params] = float("nan")
            self._bind_grads()
            return self._loss_out
        gb = int(world_batch) if world_batch else B
        scale = 1.0 / gb if (self.loss_kind == LOSS_APPROXNDCG and not defer_norm) else 1.0
        if defer_norm and self.loss_kind == LOSS_APPROXNDCG:
            self._norm.fill_(float(B))
        self._calls += 1
        h = lib()
        L, ln = len(info.sizes), int(info.input_norm)
        with torch.cuda.device(self.device):
            x2 = self._docs(X)
            yy = y.detach().reshape(B, S).to(torch.float32).contiguous()
            if self._slate is None or self._slate.numel() < B:
                self._slate = torch.empty(B, dtype=torch.float32, device=self.device)
            count = torch.empty(B, dtype=torch.float32, device=self.device) if self.loss_kind == LOSS_LAMBDA else None
            ps, ptrs = self._param_ptrs()
            check(h.ltr_linear_fold(L, F, self._sizes, ln, ptrs, _ptr(self.ws), _ptr(self.weff), _stream()), "ltr_linear_fold")
            sid, kk, sigma, mu, leps, pad, lb = self.lambda_args
            if self.kernel_events is not None:
                self.kernel_events[0].record()
            if h.ltr_linear_fused_supported(F, S):
                check(h.ltr_linear_fused_step(self.loss_kind, _ptr(x2), _ptr(yy), B, S, F, _ptr(self.weff), ln, self.alpha, self.eps,
                                              self.pad, int(self.apply_sigmoid), sid, kk, sigma, mu, leps, lb, scale, _ptr(self._slate),
                                              _ptr(count), _ptr(self.partials), self.grid, _stream()), "ltr_linear_fused_step")
            else:
                self._three_launches(h, x2, yy, B, S, scale, count)
            if self.kernel_events is not None:
                self.kernel_events[1].record()
            check(h.ltr_linear_unfold_grads(L, F, self._sizes, ln, ptrs, _ptr(self.partials), self.grid, _ptr(self.ws),
                                            _ptr(self.flat_grad), _stream()), "ltr_linear_unfold_grads")
            del ps
            check(h.ltr_reduce_sum_f32(_ptr(self._slate), B, scale, self.flat.data_ptr() + 4 * info.n_params, _stream()),
                  "ltr_reduce_sum_f32")
            if lambda_mean:
                torch.sum(count, dim=0, keepdim=True, out=self._norm)
                if not defer_norm:
                    self._divide_by_norm()
        self._bind_grads()
        return self._loss_out

    def _docs(self, X):
        """X [B, S, F] -> fp32 [B S, F], contiguous and 16-byte aligned."""
        x2 = X.detach().reshape(-1, self.info.F)
        if x2.dtype != torch.float32:
            raise TypeError(f"the fused step takes fp32 features, got {x2.dtype}")
        if not x2.is_contiguous() or x2.data_ptr() % 16:
            x2 = x2.contiguous() if not x2.is_contiguous() else x2.clone()
        return x2

    def _step_risk(self, X, y, B, S, risk_in, world_batch, one_pass=None):
        """The risk step of the folded network (module docstring): one pass over X for the Listnet forms where the one-launch tile kernel
        takes (F, S), the multi-launch chain otherwise.  The gather, the tail and the loss slot are risk_step's, as for DoubleLayerNet."""
        from . import risk_step as RS
        info, R = self.info, self.risk
        F, L, ln = info.F, len(info.sizes), int(info.input_norm)
        yb, cache, n_c = risk_in
        nsys = 1 + n_c
        n = B * S
        h = lib()
        self._calls += 1
        fused_ok = (not R.lam) and bool(h.ltr_linear_fused_supported(F, S))
        if one_pass and not fused_ok:
            raise NotImplementedError(f"{R.name}: the one-pass kernel takes the Listnet forms at S in (32, 64, 128), F % 4 == 0, F <= 256")
        one_pass = fused_ok if one_pass is None else bool(one_pass)
        with torch.cuda.device(self.device):
            x2 = self._docs(X)
            yy = y.detach().reshape(B, S).to(torch.float32).contiguous()
            if cache is None and not R.lam and B > 0:
                # Listnet forms: the baselines' columns are O(S) work per system, so y_base= is base_cols= of this batch and one code
                # path feeds both kernels.  (The Lambda forms' constant columns are S^2 pair sweeps, n_base + 1 of them: with y_base
                # they run once inside risk_step.matrix's uncached launch, whose matrix is bitwise the cached one.)
                cache, yb = RS.baseline_columns(R, yy, yb), None
            dp = (self.risk_group, self.risk_rank, self.risk_world)
            mat, send, bmax = RS.matrix_rows(R, self.device, dp, B, nsys, world_batch)
            ps, ptrs = self._param_ptrs()
            if B > 0:
                check(h.ltr_linear_fold(L, F, self._sizes, ln, ptrs, _ptr(self.ws), _ptr(self.weff), _stream()), "ltr_linear_fold")
                if self.kernel_events is not None:
                    self.kernel_events[0].record()
                if one_pass:
                    if self._rows is None or self._rows.numel() < B * (F + 1):
                        self._rows = torch.empty(B * (F + 1), dtype=torch.float32, device=self.device)
                    cs_ = int(cache.stride(0)) if B > 1 else int(cache.shape[1])
                    check(h.ltr_linear_risk_rows(_ptr(x2), _ptr(yy), B, S, F, _ptr(self.weff), ln, R.mode, R.lt, _ptr(cache), cs_, n_c,
                                                 _ptr(mat), nsys, _ptr(self._rows), self.grid, _stream()), "ltr_linear_risk_rows")
                else:
                    if self._bufs is None or self._bufs[0].numel() < n:
                        self._bufs = [torch.empty(n, dtype=torch.float32, device=self.device),
                                      torch.empty(n, dtype=torch.float32, device=self.device),
                                      torch.empty(2 * n, dtype=torch.float32, device=self.device)]
                    if self._jac is None or self._jac.numel() < n:
                        self._jac = torch.empty(n, dtype=torch.float32, device=self.device)
                    scores, ds, stats = self._bufs
                    jac = self._jac
                    check(h.ltr_linear_scores(_ptr(x2), n, F, _ptr(self.weff), ln, _ptr(scores), _ptr(stats), _stream()),
                          "ltr_linear_scores")
                    RS.matrix(h, R, scores[:n].view(B, S), yy, yb, cache, n_c, mat, jac)
            coef, _dmat = RS.run_tail(h, R, dp, self.flat[info.n_params:info.n_params + 1], mat, send, bmax, B, nsys)
            if B == 0:
                self.flat_grad.zero_()
                self._bind_grads()
                return self._loss_out
            if one_pass:
                check(h.ltr_linear_risk_combine(_ptr(self._rows), coef, nsys, B, F, _ptr(self.partials), self.grid, _stream()),
                      "ltr_linear_risk_combine")
            else:
                RS.scores_grad(h, R, scores, yy, jac, coef, nsys, ds)
                check(h.ltr_linear_grad_partials(_ptr(x2), n, F, _ptr(ds), _ptr(stats), ln, _ptr(self.partials), self.grid, _stream()),
                      "ltr_linear_grad_partials")
            if self.kernel_events is not None:
                self.kernel_events[1].record()
            check(h.ltr_linear_unfold_grads(L, F, self._sizes, ln, ptrs, _ptr(self.partials), self.grid, _ptr(self.ws),
                                            _ptr(self.flat_grad), _stream()), "ltr_linear_unfold_grads")
            del ps
        self._bind_grads()
        return self._loss_out

    def _three_launches(self, h, x2, yy, B, S, scale, count):
        """Any slate length: scores (GEMV, LayerNorm statistics) -> the standalone loss kernel -> gradient partials (X re-read,
        weighted by d loss / d s)."""
        n = B * S
        F, ln = self.info.F, int(self.info.input_norm)
        if self._bufs is None or self._bufs[0].numel() < n:
            self._bufs = [torch.empty(n, dtype=torch.float32, device=self.device),
                          torch.empty(n, dtype=torch.float32, device=self.device),
                          torch.empty(2 * n, dtype=torch.float32, device=self.device)]
        scores, ds, stats = self._bufs
        check(h.ltr_linear_scores(_ptr(x2), n, F, _ptr(self.weff), ln, _ptr(scores), _ptr(stats), _stream()), "ltr_linear_scores")
        if self.loss_kind == LOSS_APPROXNDCG:
            check(h.ltr_approxndcg_fwd_bwd(_ptr(scores), _ptr(yy), B, S, self.alpha, self.eps, self.pad, scale, _ptr(self._slate),
                                           _ptr(ds), _stream()), "ltr_approxndcg_fwd_bwd")
        elif self.loss_kind == LOSS_LISTNET:
            check(h.ltr_listnet_fwd_bwd(_ptr(yy), _ptr(scores), B, S, int(self.apply_sigmoid), scale, _ptr(self._slate), _ptr(ds),
                                        _stream()), "ltr_listnet_fwd_bwd")
        else:
            sid, kk, sigma, mu, eps, pad, lb = self.lambda_args
            check(h.ltr_lambda_fwd_bwd(_ptr(scores), _ptr(yy), B, S, sid, kk, sigma, mu, eps, pad, lb, scale, _ptr(self._slate),
                                       _ptr(count), _ptr(ds), _stream()), "ltr_lambda_fwd_bwd")
        check(h.ltr_linear_grad_partials(_ptr(x2), n, F, _ptr(ds), _ptr(stats), ln, _ptr(self.partials), self.grid, _stream()),
              "ltr_linear_grad_partials")

