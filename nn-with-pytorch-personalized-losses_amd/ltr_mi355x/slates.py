"""Fixed-length slates from a ragged collection, and back: the host side of the ltr_slates_* entry points (include/ltr_mi355x.h).

The reference's config carries `data.slate_length` (config.json: 100), the allRank rule: every query becomes one slate of S documents, a
longer query randomly sub-sampled anew each epoch, a shorter one padded with label -1.  Here that step runs on the device: a
RaggedSlates plus (S, mode, seed) gives the padded `[B, S, F]` batch, its labels, its padding mask (1 = padded, what
blocks.slate_mask takes) and the row map `rows [B, S]` (document row of every slot, -1 in padding) -- ltr_slates_build, one launch.
The row map also takes any per-document tensor to slates (`gather`) and any per-slot tensor back to document order (`scatter`), both
differentiable, so a dense model trains under the ragged losses, which ignore nothing and pad nothing:

    slates = RaggedSlates.from_qid(qid, device="cuda")
    X3, y2, fixed = to_slates(Xd, yd, slates, S=100, mode="sample", seed=epoch)
    scores = model(X3, fixed.mask, None)                          # [B, S]
    loss = ragged.listnet(yd, from_slates(scores, fixed), slates)  # documents a sampled query left out score 0 (FixedSlates)
    loss.backward()
"""
import functools

import numpy as np
import torch

from ._lib import check, lib
from .functional import MAX_SLATE, _ptr, _stream, require_device
from .ragged import _slates_on

MODES = {"first": 0, "sample": 1}                     # LTR_SLATES_FIRST / LTR_SLATES_SAMPLE


def _mode_seed(S, mode, seed):
    S = int(S)
    if not 1 <= S <= MAX_SLATE:
        raise ValueError(f"slate length {S} outside the supported range 1..{MAX_SLATE}")
    if mode not in MODES:
        raise ValueError(f"mode must be one of {sorted(MODES)}, got {mode!r}")
    return S, MODES[mode], int(seed) & 0xFFFFFFFFFFFFFFFF


def _rows_of(t, name, lead, rows=None):
    """fp32 device tensor whose leading shape is `lead` (on the row map's device) -> (contiguous detached view, trailing shape, floats
    per row)."""
    require_device(*([t] if rows is None else [t, rows]))
    if t.dtype != torch.float32:
        raise TypeError(f"{name} must be fp32, got {t.dtype}")
    if tuple(t.shape[:len(lead)]) != tuple(lead):
        raise ValueError(f"{name} must have the leading shape {list(lead)}, got {tuple(t.shape)}")
    tail = tuple(t.shape[len(lead):])
    return t.detach().contiguous(), tail, int(np.prod(tail, dtype=np.int64)) if tail else 1


def _gather(t, rows, n_docs, fill):
    src, tail, row = _rows_of(t, "gather's tensor", (n_docs,), rows)
    out = torch.empty(tuple(rows.shape) + tail, dtype=torch.float32, device=src.device)
    if out.numel():
        with torch.cuda.device(src.device):
            check(lib().ltr_slates_gather_f32(_ptr(src), n_docs, _ptr(rows), rows.numel(), row, float(fill), _ptr(out), _stream()),
                  "ltr_slates_gather_f32")
    return out


def _scatter(t, rows, n_docs, out=None):
    src, tail, row = _rows_of(t, "scatter's tensor", tuple(rows.shape), rows)
    if out is None:
        out = torch.zeros((n_docs,) + tail, dtype=torch.float32, device=src.device)
    elif (not out.is_cuda or out.device != src.device or out.dtype != torch.float32 or tuple(out.shape) != (n_docs,) + tail
          or not out.is_contiguous()):
        raise ValueError(f"out must be a contiguous fp32 tensor of shape {[n_docs] + list(tail)} on {src.device}")
    if src.numel():
        with torch.cuda.device(src.device):
            check(lib().ltr_slates_scatter_f32(_ptr(src), _ptr(rows), rows.numel(), row, n_docs, _ptr(out), _stream()),
                  "ltr_slates_scatter_f32")
    return out


@functools.lru_cache(maxsize=None)
def _row_map_functions():
    """(gather, scatter) autograd nodes.  Built on first use rather than at module level, like ragged._ragged_loss:
    tests/test_autograd_state_cpu.py pairs every module-level Function of the package with an entry of the table in
    tests/test_autograd_state_gpu.py; these nodes' state test is tests/test_slate_build_gpu.py::test_backward_uses_forward_time_rows.
    The backward of one is the other (a scatter into zeros / a gather with fill 0) over a private copy of the forward-time rows --
    nothing else is saved, and the FixedSlates may be overwritten or dropped in between."""
    class _Gather(torch.autograd.Function):
        @staticmethod
        def forward(ctx, t, rows, n_docs, fill):
            ctx.n_docs = n_docs
            if ctx.needs_input_grad[0]:
                ctx.save_for_backward(rows.clone())
            return _gather(t, rows, n_docs, fill)

        @staticmethod
        def backward(ctx, go):
            (rows,) = ctx.saved_tensors
            return _scatter(go.to(torch.float32), rows, ctx.n_docs), None, None, None

    class _Scatter(torch.autograd.Function):
        @staticmethod
        def forward(ctx, t, rows, n_docs):
            ctx.n_docs = n_docs
            if ctx.needs_input_grad[0]:
                ctx.save_for_backward(rows.clone())
            return _scatter(t, rows, n_docs)

        @staticmethod
        def backward(ctx, go):
            (rows,) = ctx.saved_tensors
            return _gather(go.to(torch.float32), rows, ctx.n_docs, 0.0), None, None

    return _Gather, _Scatter


class FixedSlates:
    """The fixed-length view of a RaggedSlates: `rows [B, S]` int64 (document row of every slot, -1 = padding) and `mask [B, S]` uint8
    (1 = padding) on the device; `S`, `n_docs`, and from the host sizes alone `kept = min(sizes, S)` and `truncated` (some query is
    longer than S: its other documents sit in no slot, so `scatter` gives them 0 and no gradient reaches them)."""

    def __init__(self, slates, S, rows, mask):
        self.S, self.n_docs = int(S), slates.n_docs
        self.kept = np.minimum(slates.sizes, self.S)
        self.truncated = bool((slates.sizes > self.S).any())
        self.rows, self.mask = rows, mask

    @property
    def n_queries(self):
        return int(self.kept.size)

    def gather(self, t, fill=0.0):
        """t [n_docs, ...] fp32 -> [B, S, ...]: slot (b, s) holds t[rows[b, s]], a padding slot `fill`.  Differentiable in t."""
        return _row_map_functions()[0].apply(t, self.rows, self.n_docs, float(fill))

    def scatter(self, t, out=None):
        """t [B, S, ...] fp32 -> [n_docs, ...]: document rows[b, s] receives t[b, s]; padding slots go nowhere.  A document no slot
        names is 0 in the returned tensor.  With `out=` (contiguous, fp32) the named rows are overwritten in place, the others left
        alone, and `out` is returned as it is, outside autograd; without it the result is differentiable in t."""
        if out is not None:
            return _scatter(t, self.rows, self.n_docs, out)
        return _row_map_functions()[1].apply(t, self.rows, self.n_docs)


def fixed_length(slates, S, mode="first", seed=0):
    """The row map of `slates` at slate length S, one ltr_slates_select launch: mode "first" keeps each query's first S documents,
    "sample" a seeded sample of S of a longer query in document order (another seed, another sample: pass the epoch)."""
    S, mode_id, seed = _mode_seed(S, mode, seed)
    if slates.device is None:
        from ._lib import LtrDeviceError
        raise LtrDeviceError("fixed_length runs on the device: give the RaggedSlates one (device= or .to(device))")
    B = slates.n_queries
    rows = torch.empty((B, S), dtype=torch.int64, device=slates.device)
    mask = torch.empty((B, S), dtype=torch.uint8, device=slates.device)
    if B:
        with torch.cuda.device(slates.device):
            check(lib().ltr_slates_select(_ptr(slates.offsets), None, B, S, mode_id, seed, _ptr(rows), _ptr(mask), _stream()),
                  "ltr_slates_select")
    return FixedSlates(slates, S, rows, mask)


def to_slates(X, y, slates, S, mode="first", seed=0, pad=-1.0, y_base=None, base_fill=0.0):
    """The padded batch of a ragged one in one ltr_slates_build launch: X [n_docs, F], y [n_docs] fp32 on the device ->
    (X3 [B, S, F] with zero rows in padding, y2 [B, S] with `pad` there, FixedSlates); with y_base [n_docs, n] also its
    [B, S, n] gather (`base_fill` in padding; one more launch).  No gradient flows to X, as everywhere in the package."""
    S, mode_id, seed = _mode_seed(S, mode, seed)
    require_device(X, y)
    slates = _slates_on(slates, X.device)
    n, B = slates.n_docs, slates.n_queries
    if X.dim() != 2:
        raise ValueError(f"X must be [n_docs, F], got {tuple(X.shape)}")
    Xc, _, F = _rows_of(X, "X", (n,))
    if y.dim() == 2 and y.shape[1] == 1:
        y = y[:, 0]
    yc, tail, _ = _rows_of(y, "y", (n,))
    if tail or F < 1:
        raise ValueError(f"expected X [n_docs, F >= 1] and y [n_docs], got {tuple(X.shape)} and {tuple(y.shape)}")
    dev = Xc.device
    X3 = torch.empty((B, S, F), dtype=torch.float32, device=dev)
    y2 = torch.empty((B, S), dtype=torch.float32, device=dev)
    rows = torch.empty((B, S), dtype=torch.int64, device=dev)
    mask = torch.empty((B, S), dtype=torch.uint8, device=dev)
    if B:
        with torch.cuda.device(dev):
            check(lib().ltr_slates_build(_ptr(Xc), _ptr(yc), _ptr(slates.offsets), None, B, S, F, mode_id, seed, float(pad), _ptr(X3),
                                         _ptr(y2), _ptr(mask), _ptr(rows), _stream()), "ltr_slates_build")
    fixed = FixedSlates(slates, S, rows, mask)
    if y_base is None:
        return X3, y2, fixed
    return X3, y2, fixed, fixed.gather(y_base.detach(), fill=base_fill)


def from_slates(scores, fixed):
    """Per-slot scores [B, S] (or [B, S, ...]) back in document order [n_docs, ...]: `fixed.scatter(scores)`, differentiable."""
    return fixed.scatter(scores)
