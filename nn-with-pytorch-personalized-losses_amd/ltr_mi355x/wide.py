"""Fused training step for FC scorers with 137 .. 1024 input features (csrc/ltr_wide.hip).

DoubleLayerNet(n) and TripleLayerNet(n) accept any n (doubleLayer.py:55-60, tripleLayer.py:6-10); the slate pipeline behind
`FusedRanker` holds a 128-document tile of at most 136 features in LDS.  The public LETOR collections beyond the reference's two are
wider (Istella 220, Yahoo LTRC 700), and `WideFusedRanker` gives such a network everything `FusedRanker` offers -- the three
listwise and six risk-sensitive losses, `step` and `step_ragged`, the flat [grads | loss | normaliser] buffer, deferred
normalisation and `QueryShardedTrainer` -- on a chain of launches around the exact-fp32 GEMM `ltr_gemm_f32`:

    ltr_wide_forward_save (fc1, fc2 with their ReLU + dropout epilogues, scores; the post-activation layers stay in HBM)
    -> the loss launches (d loss / d scores)
    -> ltr_wide_backward_saved (dz2, dW2, db2, dz1, dW1, db1, dw3, db3 straight into the flat gradient)

DoubleLayerNet runs as it is (LTR_WIDE_RELU3).  TripleLayerNet always runs folded: ltr_triple_fold(copies = 1) makes the F -> 32
sigmoid layer l2 . l1 (LTR_WIDE_SIGMOID2), ltr_triple_unfold_grads turns its gradient into the six tensors'.  There is no
one-launch path: every slate length 1 .. 2048 takes the chain.  Between X and the flat gradient a step runs library entries of this
project only; torch allocates the buffers.

    ranker = WideFusedRanker(DoubleLayerNet(220).cuda(), loss="approxNDCG")
    loss = ranker.step(X, y)          # X [B, S, 220] fp32 device, y [B, S]; fills p.grad for every parameter
"""
import ctypes
from types import SimpleNamespace

import torch

from ._lib import check, lib
from .functional import _ptr, _stream, require_device
from .scorer import _MASK64, FusedRanker, _mask, _params_f32, cu_count, drop_code, next_seed, triple_fold, triple_unfold

WIDE_RELU3, WIDE_SIGMOID2 = 0, 1
MIN_FEATURES, MAX_FEATURES = 137, 1024


ACT_NONE, ACT_RELU, ACT_SIGMOID = 0, 1, 2
GATE_NONE, GATE_RELU, GATE_SIGMOID = 0, 1, 2


class GemmDesc(ctypes.Structure):
    """ltr_gemm_f32_desc of include/ltr_mi355x.h."""
    _fields_ = [("A", ctypes.c_void_p), ("B", ctypes.c_void_p),
                ("M", ctypes.c_int64), ("N", ctypes.c_int64), ("K", ctypes.c_int64),
                ("lda", ctypes.c_int64), ("ldb", ctypes.c_int64), ("ldc", ctypes.c_int64),
                ("a_kmajor", ctypes.c_int32), ("b_kmajor", ctypes.c_int32), ("splits", ctypes.c_int32), ("act", ctypes.c_int32),
                ("C", ctypes.c_void_p), ("bias", ctypes.c_void_p), ("gate", ctypes.c_void_p), ("ldg", ctypes.c_int64),
                ("gate_kind", ctypes.c_int32), ("gate_scale", ctypes.c_float),
                ("dropout", ctypes.c_int32), ("drop_layer", ctypes.c_int32),
                ("seed", ctypes.c_uint64), ("keep", ctypes.c_void_p)]


def gemm_f32(A, B, C, M, N, K, lda, ldb, ldc, a_kmajor=False, b_kmajor=False, splits=1, bias=None, act=ACT_NONE, gate=None, ldg=0,
             gate_kind=GATE_NONE, gate_scale=1.0, dropout=0, drop_layer=0, seed=0, keep=None):
    """C[m][n] = sum_k A(m, k) B(n, k) with the scorers' epilogues: ltr_gemm_f32 on fp32 device tensors (any shape; the extents and
    leading dimensions say how they are read).  splits > 1: C holds the raw partials [splits][M][ldc]."""
    tensors = [t for t in (A, B, C, bias, gate, keep) if t is not None]
    require_device(*tensors)
    d = GemmDesc(A=_ptr(A), B=_ptr(B), M=M, N=N, K=K, lda=lda, ldb=ldb, ldc=ldc, a_kmajor=int(a_kmajor), b_kmajor=int(b_kmajor),
                 splits=splits, act=act, C=_ptr(C), bias=_ptr(bias), gate=_ptr(gate), ldg=ldg, gate_kind=gate_kind,
                 gate_scale=gate_scale, dropout=dropout, drop_layer=drop_layer, seed=int(seed) & _MASK64, keep=_ptr(keep))
    with torch.cuda.device(C.device):
        check(lib().ltr_gemm_f32(ctypes.byref(d), _stream()), "ltr_gemm_f32")
    return C


class _Info:
    """What FusedRanker's shared methods read (`F`, `n_params`) plus the widths of the network the chain runs."""

    def __init__(self, F, H1, H2, n_params):
        self.F, self.H1, self.H2, self.n_params = int(F), int(H1), int(H2), int(n_params)


class WideFusedRanker(FusedRanker):
    """FusedRanker for a DoubleLayerNet / TripleLayerNet of 137 .. 1024 input features (see the module docstring).  Same interface
    and buffers: `flat` = [grads | loss] aliased by every `p.grad`, `flat_ext` with the normaliser slot, `world_batch`,
    `defer_norm` / `finish_norm`, `kernel_events`, `seed_salt`."""

    def __init__(self, module, loss="approxNDCG", alpha=1.0, eps=1e-10, padded_value_indicator=-1, apply_sigmoid=False, grid=None,
                 weighing_scheme=None, k=None, sigma=1.0, mu=10.0, reduction="sum", reduction_log="binary", risk_args=None):
        self._init_risk(loss, risk_args)
        if hasattr(module, "fc1") and hasattr(module, "fc3"):
            kind, F = WIDE_RELU3, int(module.fc1.in_features)
            H1, H2 = int(module.fc1.out_features), int(module.fc2.out_features)
        elif hasattr(module, "l1") and hasattr(module, "l3"):
            kind, F = WIDE_SIGMOID2, int(module.l1.in_features)
            H1 = H2 = int(module.l2.out_features)             # the folded layer l2 . l1
        else:
            raise TypeError(f"WideFusedRanker takes a DoubleLayerNet or a TripleLayerNet, got {type(module).__name__}")
        if F < MIN_FEATURES:
            raise ValueError(f"{F} input features: networks of up to 136 features train through FusedRanker (the slate pipeline); "
                             f"WideFusedRanker takes {MIN_FEATURES} .. {MAX_FEATURES}")
        if F > MAX_FEATURES:
            raise ValueError(f"at most {MAX_FEATURES} input features, got {F}")
        self.module, self.kind = module, kind
        self._init_loss(loss, alpha, eps, padded_value_indicator, apply_sigmoid, weighing_scheme, k, sigma, mu, reduction, reduction_log)
        self.params = module._ltr_params()
        require_device(*self.params)
        self.info = _Info(F, H1, H2, sum(p.numel() for p in self.params))
        dev = self.device = self.params[0].device
        self.grid = int(grid) if grid else 2 * cu_count(dev)      # workgroups a launch of the chain should fill
        self._init_flat()
        self.fold_w = self.fold_flat = None
        if kind == WIDE_SIGMOID2:
            self.fold_w = [torch.empty(sh, dtype=torch.float32, device=dev) for sh in ((H1, F), (H1,), (1, H1))]
            self.fold_flat = torch.empty(H1 * F + 2 * H1 + 1, dtype=torch.float32, device=dev)
        self._acts = self._ws = None       # saved layers / backward workspace of the chain (grown on demand)

    def _check_trainable(self, train, keep1, keep2):
        if self.kind == WIDE_SIGMOID2 and (keep1 is not None or keep2 is not None):
            raise NotImplementedError("keep1 / keep2 are DoubleLayerNet's dropout masks; TripleLayerNet has no dropout")

    def _docs(self, X):
        """X [..., F] -> fp32 [n_docs, F], contiguous and 16-byte aligned."""
        F = self.info.F
        if X.dim() < 2 or X.shape[-1] != F:
            raise ValueError(f"expected [..., {F}] features, got {tuple(X.shape)}")
        if X.dtype != torch.float32:
            raise TypeError(f"the fused step takes fp32 features, got {X.dtype}")
        x2 = X.detach().reshape(-1, F)
        if not x2.is_contiguous():
            x2 = x2.contiguous()
        if x2.data_ptr() % 16:
            x2 = x2.clone()
        return x2

    def _prepare(self, X, keep1=None, keep2=None, seed=None, train=None, one_launch=False):
        """FusedRanker._prepare for the wide chain: the dropout code and seed (a default seed comes from `_calls`; every call here
        advances it), X as [n_docs, F] rows, the explicit masks, and the live parameters' pointers -- for a TripleLayerNet those of
        the folded network, made here from the six tensors."""
        info = self.info
        train = self.module.training if train is None else train
        dropout = 0
        if self.kind == WIDE_RELU3:
            dropout = drop_code(bool(train), float(self.module.dropout.p))
        if seed is None:
            seed = next_seed(self._calls) ^ ((self.seed_salt * 0xA24BAED4963EE407) & _MASK64)
        self._calls += 1
        x2 = self._docs(X)
        n = int(x2.shape[0])
        k1, k2 = _mask(keep1, n, info.H1), _mask(keep2, n, info.H2)
        pf = _params_f32(self.params)                       # W1, b1, W2, b2, w3, b3
        ps = pf if self.kind == WIDE_RELU3 else triple_fold(pf, 1, self.fold_w) + [pf[5]]
        ptrs = (ctypes.c_void_p * len(ps))(*[t.data_ptr() for t in ps])
        return SimpleNamespace(x2=x2, n=n, dropout=int(dropout), seed=int(seed) & _MASK64, k1=k1, k2=k2, pf=pf, ps=ps, ptrs=ptrs)

    def _chain(self, rows, loss_launches):
        """Any slate length, every loss: forward launches (scores and the saved post-activation layers) -> loss_launches(scores, ds),
        which fill d loss / d scores -> backward launches, which read the saved layers and write the flat gradient (through the
        unfold for a TripleLayerNet).  `kernel_events` bracket the backward."""
        h, r, dev, info = lib(), rows, self.device, self.info
        dims = (self.kind, info.F, info.H1, info.H2)
        scores = torch.empty(r.n, dtype=torch.float32, device=dev)
        ds = torch.empty(r.n, dtype=torch.float32, device=dev)
        n_acts = int(h.ltr_wide_acts_floats(*dims, r.n))
        n_ws = int(h.ltr_wide_ws_floats(*dims, r.n, self.grid))
        check(min(n_acts, n_ws, 0), "ltr_wide_ws_floats")
        if self._acts is None or self._acts.numel() < n_acts:
            self._acts = torch.empty(n_acts, dtype=torch.float32, device=dev)
        if self._ws is None or self._ws.numel() < n_ws:
            self._ws = torch.empty(n_ws, dtype=torch.float32, device=dev)
        check(h.ltr_wide_forward_save(*dims, _ptr(r.x2), r.n, r.ptrs, r.dropout, r.seed, _ptr(r.k1), _ptr(r.k2), _ptr(scores),
                                      _ptr(self._acts), _stream()), "ltr_wide_forward_save")
        loss_launches(scores, ds)
        if self.kernel_events is not None:
            self.kernel_events[0].record()
        out = self.flat_grad if self.kind == WIDE_RELU3 else self.fold_flat
        check(h.ltr_wide_backward_saved(*dims, _ptr(r.x2), r.n, r.ptrs, r.dropout, _ptr(self._acts), _ptr(ds), _ptr(self._ws), self.grid,
                                        _ptr(out), _stream()), "ltr_wide_backward_saved")
        if self.kernel_events is not None:
            self.kernel_events[1].record()
        if self.kind == WIDE_SIGMOID2:
            triple_unfold(self.fold_flat, 1, r.pf, self.flat_grad)

    def step(self, X, y, world_batch=None, keep1=None, keep2=None, seed=None, train=None, defer_norm=False, y_base=None, base_cols=None):
        """FusedRanker.step on the chain (no one-launch path at these widths): same arguments, buffers and return value."""
        self._check_trainable(train, keep1, keep2)
        B, S = self._batch_shape(X, y)
        if self.risk is not None:
            risk_in = self._risk_inputs(B, S, y_base, base_cols)
            with torch.cuda.device(self.device):
                self._step_risk(X, y.detach().reshape(B, S).to(torch.float32).contiguous(), risk_in, world_batch, keep1, keep2, seed, train)
            self._bind_grads()
            return self._loss_out
        if y_base is not None or base_cols is not None:
            raise TypeError(f"y_base / base_cols belong to the risk-sensitive losses, not {self.loss!r}")
        scale = self._listwise_prelude(B, world_batch, defer_norm, "step")
        if scale is None:
            self._bind_grads()
            return self._loss_out
        from .scorer import LOSS_LAMBDA
        with torch.cuda.device(self.device):
            yy = y.detach().reshape(B, S).to(torch.float32).contiguous()
            r = self._prepare(X, keep1, keep2, seed, train)
            count = self._loss_buffers(B, self.loss_kind == LOSS_LAMBDA)
            self._chain(r, self._dense_loss(yy, scale, count))
            self._listwise_epilogue(B, scale, count, defer_norm)
        self._bind_grads()
        return self._loss_out
