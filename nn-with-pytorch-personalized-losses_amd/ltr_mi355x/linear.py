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
from types import SimpleNamespace

import torch

from ._lib import check, lib
from .functional import _ptr, _stream, require_device
from .scorer import LOSS_LAMBDA, FusedRanker, cu_count

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
        self._init_risk(loss, risk_args)
        F, sizes, ln, self._dropout = linear_shape(module)
        if len(sizes) > MAX_LAYERS:
            raise ValueError(f"at most {MAX_LAYERS} FC layers fold, got {len(sizes)}")
        if F > MAX_FEATURES:
            raise ValueError(f"at most {MAX_FEATURES} input features, got {F}")
        self.module = module
        self._init_loss(loss, alpha, eps, padded_value_indicator, apply_sigmoid, weighing_scheme, k, sigma, mu, reduction, reduction_log)
        self.params = module._ltr_params()
        require_device(*self.params)
        self.info = _Info(F, sizes, ln, sum(p.numel() for p in self.params))
        dev = self.device = self.params[0].device
        h = lib()
        self.grid = int(grid) if grid else int(h.ltr_linear_grid(cu_count(dev)))
        self._init_flat()
        self._sizes = (ctypes.c_int * max(1, len(sizes)))(*sizes)
        nws = int(h.ltr_linear_ws_doubles(len(sizes), F, self._sizes))
        check(-2 if nws < 0 else 0, "ltr_linear_ws_doubles")
        self.ws = torch.empty(nws, dtype=torch.float64, device=dev)         # fold -> unfold of ONE step; rewritten every step
        self.weff = torch.empty(F + 2, dtype=torch.float32, device=dev)
        self.partials = torch.empty(self.grid * (F + 1), dtype=torch.float32, device=dev)
        self._bufs = None              # scores / ds / stats of the chain (grown on demand)
        self._rows = None              # R [B][F + 1] of the one-pass risk step (grown on demand)

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
        base_cols as in FusedRanker.step; `_one_pass=False` sends a Listnet form through the chain (tests, benchmarks)."""
        self._check_trainable(train, keep1, keep2)
        B, S = self._batch_shape(X, y)
        if self.risk is not None:
            risk_in = self._risk_inputs(B, S, y_base, base_cols)
            with torch.cuda.device(self.device):
                self._step_risk(X, y.detach().reshape(B, S).to(torch.float32).contiguous(), risk_in, world_batch, one_pass=_one_pass)
            self._bind_grads()
            return self._loss_out
        if y_base is not None or base_cols is not None:
            raise TypeError(f"y_base / base_cols belong to the risk-sensitive losses, not {self.loss!r}")
        scale = self._listwise_prelude(B, world_batch, defer_norm, "step")
        if scale is None:
            self._bind_grads()
            return self._loss_out
        h = lib()
        F, ln = self.info.F, int(self.info.input_norm)
        with torch.cuda.device(self.device):
            yy = y.detach().reshape(B, S).to(torch.float32).contiguous()
            r = self._prepare(X)
            count = self._loss_buffers(B, self.loss_kind == LOSS_LAMBDA)
            if h.ltr_linear_fused_supported(F, S):
                sid, kk, sigma, mu, leps, pad, lb = self.lambda_args

                def one_launch():
                    check(h.ltr_linear_fused_step(self.loss_kind, _ptr(r.x2), _ptr(yy), B, S, F, _ptr(self.weff), ln, self.alpha, self.eps,
                                                  self.pad, int(self.apply_sigmoid), sid, kk, sigma, mu, leps, lb, scale, _ptr(self._slate),
                                                  _ptr(count), _ptr(self.partials), self.grid, _stream()), "ltr_linear_fused_step")
                self._folded(r, one_launch)
            else:
                self._chain(r, self._dense_loss(yy, scale, count))
            self._listwise_epilogue(B, scale, count, defer_norm)
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

    def _prepare(self, X, keep1=None, keep2=None, seed=None, train=None):
        """FusedRanker._prepare for the folded network: X as [n_docs, F] rows and the live parameters' pointers (nothing here is random;
        `_calls` counts the executed steps)."""
        self._calls += 1
        x2 = self._docs(X)
        ps, ptrs = self._param_ptrs()
        return SimpleNamespace(x2=x2, n=int(x2.shape[0]), ps=ps, ptrs=ptrs)

    def _folded(self, rows, launches):
        """ltr_linear_fold (w_eff, b_eff from the live parameters) -> launches(), which leave [Ghat | G_1] partials in `partials` ->
        ltr_linear_unfold_grads into `flat_grad`.  `kernel_events` bracket everything between the two."""
        h, info = lib(), self.info
        F, L, ln = info.F, len(info.sizes), int(info.input_norm)
        check(h.ltr_linear_fold(L, F, self._sizes, ln, rows.ptrs, _ptr(self.ws), _ptr(self.weff), _stream()), "ltr_linear_fold")
        if self.kernel_events is not None:
            self.kernel_events[0].record()
        launches()
        if self.kernel_events is not None:
            self.kernel_events[1].record()
        check(h.ltr_linear_unfold_grads(L, F, self._sizes, ln, rows.ptrs, _ptr(self.partials), self.grid, _ptr(self.ws),
                                        _ptr(self.flat_grad), _stream()), "ltr_linear_unfold_grads")

    def _chain(self, rows, loss_launches):
        """Any slate length, every loss: fold -> scores (GEMV, LayerNorm statistics) -> loss_launches(scores, ds), which fill
        d loss / d scores -> gradient partials (X re-read, weighted by d loss / d s) -> unfold."""
        h, n = lib(), rows.n
        F, ln = self.info.F, int(self.info.input_norm)

        def launches():
            if self._bufs is None or self._bufs[0].numel() < n:
                self._bufs = [torch.empty(n, dtype=torch.float32, device=self.device),
                              torch.empty(n, dtype=torch.float32, device=self.device),
                              torch.empty(2 * n, dtype=torch.float32, device=self.device)]
            scores, ds, stats = self._bufs
            check(h.ltr_linear_scores(_ptr(rows.x2), n, F, _ptr(self.weff), ln, _ptr(scores), _ptr(stats), _stream()), "ltr_linear_scores")
            loss_launches(scores, ds)
            check(h.ltr_linear_grad_partials(_ptr(rows.x2), n, F, _ptr(ds), _ptr(stats), ln, _ptr(self.partials), self.grid, _stream()),
                  "ltr_linear_grad_partials")
        self._folded(rows, launches)

    def _step_risk(self, X, yy, risk_in, world_batch, keep1=None, keep2=None, seed=None, train=None, one_pass=None):
        """The risk step of the folded network (module docstring): one pass over X for the Listnet forms where the one-launch tile kernel
        takes (F, S), FusedRanker._step_risk's chain otherwise.  The gather, the tail and the loss slot are risk_step's either way."""
        from . import risk_step as RS
        h, R = lib(), self.risk
        F, ln = self.info.F, int(self.info.input_norm)
        B, S = yy.shape
        yb, cache, n_c = risk_in
        fused_ok = (not R.lam) and bool(h.ltr_linear_fused_supported(F, S))
        if one_pass and not fused_ok:
            raise NotImplementedError(f"{R.name}: the one-pass kernel takes the Listnet forms at S in (32, 64, 128), F % 4 == 0, F <= 256")
        one_pass = fused_ok if one_pass is None else bool(one_pass)
        if cache is None and not R.lam and B > 0:
            # Listnet forms: the baselines' columns are O(S) work per system, so y_base= is base_cols= of this batch and one code
            # path feeds both kernels.  (The Lambda forms' constant columns are S^2 pair sweeps, n_base + 1 of them: with y_base
            # they run once inside risk_step.matrix's uncached launch, whose matrix is bitwise the cached one.)
            cache, yb = RS.baseline_columns(R, yy, yb), None
        if not one_pass or B == 0:
            return super()._step_risk(X, yy, (yb, cache, n_c), world_batch)
        nsys = 1 + n_c
        dp = (self.risk_group, self.risk_rank, self.risk_world)
        rows = self._prepare(X)
        mat, send, bmax = RS.matrix_rows(R, self.device, dp, B, nsys, world_batch)
        if self._rows is None or self._rows.numel() < B * (F + 1):
            self._rows = torch.empty(B * (F + 1), dtype=torch.float32, device=self.device)

        def one_pass_launches():
            cs_ = int(cache.stride(0)) if B > 1 else int(cache.shape[1])
            check(h.ltr_linear_risk_rows(_ptr(rows.x2), _ptr(yy), B, S, F, _ptr(self.weff), ln, R.mode, R.lt, _ptr(cache), cs_, n_c,
                                         _ptr(mat), nsys, _ptr(self._rows), self.grid, _stream()), "ltr_linear_risk_rows")
            coef, _dmat = RS.run_tail(h, R, dp, self.flat[self.info.n_params:self.info.n_params + 1], mat, send, bmax, B, nsys)
            check(h.ltr_linear_risk_combine(_ptr(self._rows), coef, nsys, B, F, _ptr(self.partials), self.grid, _stream()),
                  "ltr_linear_risk_combine")
        self._folded(rows, one_pass_launches)
