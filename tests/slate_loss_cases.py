"""Case builders shared by tests/test_slate_loss_paths_cpu.py and tests/test_slate_loss_paths_gpu.py (a plain module, no fixtures).

approx_ndcg_slate (csrc/ltr_slate_losses.h) decides PER SLATE, behind one barrier, between three code paths.  With
x_k = alpha s_k - alpha s_0 formed in fp32 from document 0's score (also when document 0 is padding) and A = max |x_k| over the real
documents:
    noclamp : eps <= 1e-7, A <= 8, every clamped label max(y, 0) an integer <= 15   (four pairs per reciprocal, histogram ideal DCG)
    fast    : A <= 69                                                               (one exponential per document, eps clamp)
    perpair : anything wider, or NaN                                                (one exponential per pair)
`path_of` restates that rule on the host; every case here DECLARES its spread A and from it the path each slate is meant to take
(third result of `approx_inputs`), and the CPU test holds the two together.  Scores are (z - z_ref) / max|z - z_ref| * A / alpha + offset with seeded
z = randn, z_ref the first real document and the maximum over the real documents, so A is met exactly by one document.  The declared
spreads (0, 2, 7.5, 20, 60, 150, 3000) are all at least 5 % away from 8 and from 69.

Preconditions, asserted over every case by the CPU test:
  * each slate takes its intended path, with the 5 % margin on A;
  * the fp64 oracle's max|gradient| is >= 1e-6 at grad_scale = 1 and the oracle's own fp32-vs-fp64 deviation is <= 2.5e-6 on the loss
    and on the gradient: such a case is gated at the flat 1e-5 of BASELINE.md;
  * saturated small slates (S <= 16 with A >= 20): the exact gradient is 0 or below 1e-7, so the gradient alone is gated as
    max|delta| / max(max|ref|, 1e-4) <= 1e-5 (FLOOR); the loss as everywhere.  No other case uses a floor;
  * at S <= 3 the regimes declared with A = 7.5 use A = 2: at S = 2 and A = 7.5 the gradient is a difference of two pair terms that
    cancels down to 5e-5 while each carries fp32 rounding of 1e-4 of it;
  * `perpair_overflow` (A = 3000) runs from S = 129 on: below, its exact gradient is about 1e-7 and fp32 noise is 1e-4 of that;
  * the cases named in RELAXED miss the noise cap (measured by the CPU test, which also fails if one of them stops needing it) and are
    gated at the standing relaxed bar max(1e-5, 4 x the oracle's fp32 noise of that quantity): two-document slates at A = 20 under
    the floor, S = 16 with clamped pairs, front padding at S = 17 / A = 150, A = 3000 at S = 257 and the wide apply_sigmoid ListNet
    at S = 2 -- short slates whose gradient is a handful of nearly saturated terms;
  * a slate whose exact gradient is identically 0 (one real document, all padding, all-zero labels, S = 1) must come back exactly 0;
  * ListNet: the fp32 softmax(y_pred) has every q >= 1e-30, so no log q underflows (the reference goes to inf there in fp32).

No pair is left out of any comparison.  The eps-clamp band needs no input search here (it did for lambdaLoss, lambda_tier_cases.py): a
pair that takes different sides of the clamp in fp32 and fp64 has a sigmoid within rounding of eps, and it enters the gradient as
t = c (1 - c) [c >= eps] g_k <= eps g_k -- ten orders of magnitude below the gated maximum at eps = 1e-10, six at eps = 1e-6.
"""
import functools
from collections import namedtuple

import numpy as np
import torch

import lambda_tier_cases as LT
import ltr_oracle as O

TIER_S, FULL_S, SHARED_S = LT.TIER_S, LT.FULL_S, LT.RAGGED_S
T_NOCLAMP, T_FAST, MARGIN = 8.0, 69.0, 0.05
EPS, PAD = 1e-10, -1.0
FLOOR = 1e-4                         # saturated small slates only (see the docstring)
NOISE_CAP, GRAD_MIN = 2.5e-6, 1e-6
FAR = 1e4                            # a padded document's score in the `front` variant

ApproxCase = namedtuple("ApproxCase", "regime variant B S alpha eps pad A offset")
ListCase = namedtuple("ListCase", "regime sigmoid B S")

# regime -> [(A, alpha, eps, offset)]
REGIMES = {
    "noclamp": [(7.5, 1.0, EPS, 0.0), (7.5, 3.0, EPS, 0.0)],
    "noclamp_grade15": [(7.5, 1.0, EPS, 0.0)],
    "grade16": [(7.5, 1.0, EPS, 0.0)],
    "fractional": [(7.5, 1.0, EPS, 0.0)],
    "eps1e-6": [(7.5, 1.0, 1e-6, 0.0)],
    "fast": [(20.0, 1.0, EPS, 0.0)],
    "fast_clamped": [(60.0, 0.7, EPS, 0.0), (60.0, 0.7, 1e-6, 0.0)],
    "perpair": [(150.0, 1.0, EPS, 0.0)],
    "perpair_overflow": [(3000.0, 1.0, EPS, 0.0)],
    "offset": [(7.5, 3.0, EPS, -5000.0), (7.5, 3.0, EPS, 1000.0), (20.0, 0.7, EPS, -5000.0), (20.0, 0.7, EPS, 1000.0)],
    "tied_all": [(0.0, 1.0, EPS, 0.0)],
    "tied_pairs": [(7.5, 1.0, EPS, 0.0)],
    "mixed": [(None, 1.0, EPS, 0.0)],
}
MIXED_CYCLE = (("noclamp", 7.5), ("fast", 20.0), ("perpair", 150.0), ("fractional", 7.5), ("all_padded", 0.0))
PAD_VARIANTS = ("none", "front", "front_inf", "interleaved", "one_real", "all_padded", "all_zero_labels", "negative_labels")
PAD_REGIMES = ("noclamp", "fast", "perpair")
OVERFLOW_MIN_S = 129
# one launch has one alpha and one eps: the regimes a ragged batch rotates through share alpha = 1, eps = 1e-10
RAGGED_ROTATION = ("noclamp", "fast", "perpair", "fractional", "noclamp_grade15", "tied_pairs", "grade16")


def batch_of(S):
    return LT.batch_of(S)


def spread_of(A, S):
    """The declared spread at slate length S: 2 instead of 7.5 at S <= 3 (cancelling gradient, see the docstring)."""
    return 2.0 if (A == 7.5 and S <= 3) else A


def case_id(c):
    if isinstance(c, ListCase):
        return f"listnet-{c.regime}-sig{int(c.sigmoid)}-B{c.B}-S{c.S}"
    A = "mix" if c.A is None else f"{c.A:g}"
    return f"{c.regime}-{c.variant}-B{c.B}-S{c.S}-a{c.alpha:g}-A{A}-e{c.eps:g}-o{c.offset:g}-p{c.pad:g}"


RELAXED = frozenset((
    "fast-tail-B3-S2-a1-A20-e1e-10-o0-p-1",
    "fast-tail-B3-S3-a1-A20-e1e-10-o0-p-1",
    "offset-tail-B3-S3-a0.7-A20-e1e-10-o-5000-p-1",
    "offset-tail-B3-S3-a0.7-A20-e1e-10-o1000-p-1",
    "fast_clamped-tail-B3-S16-a0.7-A60-e1e-10-o0-p-1",
    "fast_clamped-tail-B3-S16-a0.7-A60-e1e-06-o0-p-1",
    "perpair-front-B3-S17-a1-A150-e1e-10-o0-p-1",
    "perpair-front_inf-B3-S17-a1-A150-e1e-10-o0-p-1",
    "perpair_overflow-tail-B3-S257-a1-A3000-e1e-10-o0-p-1",
    "listnet-wide-sig1-B3-S2",
    "listnet-offset-3e4-sig1-B3-S2",
))
TOL = 1e-5


def bar_of(c, noise):
    """The bar of one quantity of a case: the flat 1e-5, or max(1e-5, 4 x noise) for the cases in RELAXED."""
    return max(TOL, 4.0 * noise) if case_id(c) in RELAXED else TOL


def uses_floor(c):
    if isinstance(c, ListCase):
        return False
    if c.regime == "mixed":
        return c.S <= 16
    return c.S <= 16 and c.A is not None and c.A >= 20.0


# ------------------------------------------------------------------------------------------------- the kernel's path rule
def kernel_x(s, y, alpha, pad):
    """x_k = alpha s_k - alpha s_0 in fp32 for the real documents of ONE slate (document 0's score whether it is real or not)."""
    a = torch.tensor(alpha, dtype=torch.float32)
    s = s.to(torch.float32)
    with np.errstate(all="ignore"):
        x = a * s - a * s[0]
    return x[y != pad]


def path_of(s, y, alpha, eps, pad):
    """'noclamp' / 'fast' / 'perpair' for one slate ([S] fp32 scores and labels), from the kernel's own thresholds."""
    x = kernel_x(s, y, alpha, pad)
    if not bool((x.abs() <= T_FAST).all()):                     # NaN compares false: the per-pair path
        return "perpair"
    yc = y[y != pad].clamp(min=0.0)
    ints = bool(((yc <= 15.0) & (yc == yc.floor())).all())
    if eps <= 1e-7 and ints and bool((x.abs() <= T_NOCLAMP).all()):
        return "noclamp"
    return "fast"


def declared_path(A, eps, integer_grades):
    if A > T_FAST:
        return "perpair"
    if A > T_NOCLAMP or eps > 1e-7 or not integer_grades:
        return "fast"
    return "noclamp"


# ------------------------------------------------------------------------------------------------- approxNDCG inputs
def _slate_scores(z, real, A, alpha, offset):
    """[S] fp32: spread A / alpha around the first real document, the maximum taken over the real documents."""
    idx = torch.nonzero(real).flatten()
    ref = int(idx[0]) if len(idx) else 0
    d = z.double() - z[ref].double()
    m = float(d[real].abs().max()) if len(idx) else 0.0
    s = d / m * (A / alpha) if m > 0.0 else torch.zeros_like(d)
    return (s + offset).to(torch.float32)


def _slate_plan(c, b):
    """(regime name, declared A) of slate b."""
    if c.regime == "mixed":
        name, A = MIXED_CYCLE[b % len(MIXED_CYCLE)]
        return name, spread_of(A, c.S)
    return c.regime, spread_of(c.A, c.S)


@functools.lru_cache(maxsize=None)
def approx_inputs(c):
    """(scores [B,S], labels [B,S], intended path per slate) of a case; fp32, a function of the case alone (seed 1000 + S)."""
    B, S, pad = c.B, c.S, float(c.pad)
    gen = torch.Generator().manual_seed(1000 + S)
    z = torch.randn(B, S, generator=gen)
    y = torch.randint(0, 5, (B, S), generator=gen).float()
    frac = 0.25 * torch.rand(B, S, generator=gen)
    tails = [int(torch.randint(0, S, (1,), generator=gen)) for _ in range(B)]            # 0 .. S-1 padded documents
    fronts = [1 + int(torch.randint(0, max(1, (S - 1) // 2), (1,), generator=gen)) for _ in range(B)]
    picks = torch.rand(B, S, generator=gen)
    neg = torch.rand(B, S, generator=gen) < 0.2
    v = c.variant
    if v == "pad7":
        y[neg] = -1.0                                              # real documents under pad = -7: gain 0
    if v == "negative_labels":
        y[neg] = -2.0
    s = torch.empty(B, S)
    paths = []
    for b in range(B):
        name, A = _slate_plan(c, b)
        if name == "fractional":
            y[b] = y[b] + frac[b]
        if name == "tied_pairs":
            z[b] = z[b, torch.arange(S) // 2]
        # padding
        if name == "all_padded" or (v == "all_padded" and b == B - 1):
            y[b] = pad
        elif v == "one_real" and b == min(1, B - 1):
            y[b, 1:] = pad
        elif v in ("front", "front_inf"):
            y[b, :min(fronts[b], S - 2)] = pad
        elif v == "interleaved":
            y[b, 2::3] = pad
        elif v == "all_zero_labels" and b == 0:
            y[b] = 0.0
        elif v != "none" and tails[b]:
            y[b, S - tails[b]:] = pad
        real = y[b] != pad
        n_real = int(real.sum())
        if name in ("noclamp_grade15", "grade16") and n_real:
            k = int(torch.argmax(torch.where(real, picks[b], torch.full_like(picks[b], -1.0))))
            y[b, k] = 15.0 if name == "noclamp_grade15" else 16.0
        s[b] = _slate_scores(z[b], real, A, c.alpha, c.offset)
        front = v in ("front", "front_inf") and not bool(real[0])
        if front:
            s[b, ~real] = FAR if v == "front" else float("-inf")
        # the path this slate is meant to take
        ints = name not in ("grade16", "fractional") or n_real == 0
        if front:
            paths.append("perpair")          # sref comes from the padded document 0: every real |x| is far beyond 69
        elif n_real == 0 or (n_real == 1 and bool(real[0])):
            paths.append(declared_path(0.0, c.eps, ints))
        else:
            paths.append(declared_path(A, c.eps, ints))
    return s, y, tuple(paths)


def declared_A(c, b):
    return _slate_plan(c, b)[1]


@functools.lru_cache(maxsize=None)
def approx_cases():
    out = []
    for S in TIER_S:
        Bs = (batch_of(S),) + ((5,) if S in SHARED_S else ())
        for regime, rows in REGIMES.items():
            if regime == "perpair_overflow" and S < OVERFLOW_MIN_S:
                continue
            for A, alpha, eps, offset in rows:
                for B in Bs:
                    if regime == "mixed":
                        B = 5 if S <= 512 else 3
                    out.append(ApproxCase(regime, "tail", B, S, alpha, eps, PAD, A, offset))
        if S in FULL_S:
            for regime in PAD_REGIMES:
                A, alpha, eps, offset = REGIMES[regime][0]
                for v in PAD_VARIANTS:
                    out.append(ApproxCase(regime, v, batch_of(S), S, alpha, eps, PAD, A, offset))
    out.append(ApproxCase("noclamp", "pad7", 3, 257, 1.0, EPS, -7.0, 7.5, 0.0))
    return tuple(dict.fromkeys(out))


# ------------------------------------------------------------------------------------------------- ListNet inputs
LIST_REGIMES = {        # regime -> (spread of y_pred = max - min, offset)
    "plain": (4.0, 0.0), "wide": (60.0, 0.0), "offset+1e4": (8.0, 1e4), "offset-3e4": (60.0, -3e4), "labels30": (4.0, 0.0),
    "neg_labels": (4.0, 0.0), "all_equal": (0.0, 0.5),
}


@functools.lru_cache(maxsize=None)
def list_inputs(c):
    """(y_true [B,S], y_pred [B,S]) fp32, seed 2000 + S."""
    B, S = c.B, c.S
    gen = torch.Generator().manual_seed(2000 + S)
    z = torch.randn(B, S, generator=gen).double()
    y = torch.randint(0, 5, (B, S), generator=gen).float()
    y30 = torch.randint(0, 31, (B, S), generator=gen).float()
    r = torch.rand(B, S, generator=gen)
    spread, offset = LIST_REGIMES[c.regime]
    lo, hi = z.min(1, keepdim=True).values, z.max(1, keepdim=True).values
    w = (hi - lo).clamp(min=1e-300)
    s = ((z - lo) / w * spread + offset).to(torch.float32) if S > 1 and spread > 0 else torch.full((B, S), float(offset))
    if c.regime == "labels30":
        y = y30
    if c.regime == "neg_labels":
        y = torch.where(r < 0.2, torch.full_like(y, -1.0), torch.where(r > 0.85, torch.full_like(y, -3.0), y))
    return y, s


@functools.lru_cache(maxsize=None)
def list_cases():
    out = []
    for S in TIER_S:
        for regime in LIST_REGIMES:
            for sig in (False, True):
                for B in (batch_of(S),) + ((5,) if S in SHARED_S else ()):
                    out.append(ListCase(regime, sig, B, S))
    return tuple(out)


# ------------------------------------------------------------------------------------------------- the oracle side
def approx_oracle(s, y, c, dtype):
    """(per-slate loss [B], d sum_b loss_b / d scores [B,S]) in `dtype` on the fp32 inputs: what the C ABI returns at grad_scale 1."""
    B = s.shape[0]
    with np.errstate(all="ignore"):
        _, g, per = O.approx_ndcg_closed_form(s.to(dtype), y.to(dtype), eps=c.eps, pad=c.pad, alpha=c.alpha)
    return per, g * B


def list_oracle(yt, yp, sigmoid, dtype):
    per, gs = [], []
    for b in range(yt.shape[0]):
        l, g = O.listnet_closed_form(yt[b:b + 1].to(dtype), yp[b:b + 1].to(dtype), apply_sigmoid=sigmoid)
        per.append(l.reshape(()))
        gs.append(g[0])
    return torch.stack(per), torch.stack(gs)


Ref = namedtuple("Ref", "loss grad loss32 grad32")


@functools.lru_cache(maxsize=None)
def reference(c):
    """fp64 and fp32 oracle results of a case, computed once and shared by every test of the session (treat as read-only)."""
    if isinstance(c, ListCase):
        yt, yp = list_inputs(c)
        l, g = list_oracle(yt, yp, c.sigmoid, torch.float64)
        l32, g32 = list_oracle(yt, yp, c.sigmoid, torch.float32)
    else:
        s, y, _ = approx_inputs(c)
        l, g = approx_oracle(s, y, c, torch.float64)
        l32, g32 = approx_oracle(s, y, c, torch.float32)
    return Ref(l, g, l32.double(), g32.double())


def relerr(a, b, floor=0.0):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max()) / max(float(np.abs(b).max()), floor, 1e-30)


def regime_of(S):
    return LT.regime(S)


# ------------------------------------------------------------------------------------------------- ragged batches
RAGGED_SHIFTS, LIST_RAGGED_SHIFT = (1, 2, 3, 4, 5, 6), 1   # rotations whose every query meets the preconditions (held by the CPU test)


def ragged_case(regime, S):
    A, alpha, eps, offset = REGIMES[regime][0]
    return ApproxCase(regime, "none", 1, int(S), alpha, eps, PAD, A, offset)


def list_ragged_batch(lengths, sigmoid, shift=LIST_RAGGED_SHIFT):
    """(y_true [n_docs], y_pred [n_docs], [ListCase] per query): query q in ListNet regime (q + shift) mod 7."""
    regimes = list(LIST_REGIMES)
    yts, yps, cs = [], [], []
    for q, S in enumerate(lengths):
        c = ListCase(regimes[(q + shift) % len(regimes)], bool(sigmoid), 1, int(S))
        yt, yp = list_inputs(c)
        yts.append(yt[0])
        yps.append(yp[0])
        cs.append(c)
    return torch.cat(yts), torch.cat(yps), cs


def ragged_batch(lengths, rotation=RAGGED_ROTATION, shift=0):
    """One query per length, query q in regime rotation[(q + shift) % len] (perpair_overflow never: alpha = 1, eps = 1e-10 throughout).
    Returns (scores [n_docs], labels [n_docs], [(regime, path)] per query)."""
    ss, ys, info = [], [], []
    for q, S in enumerate(lengths):
        regime = rotation[(q + shift) % len(rotation)]
        s, y, paths = approx_inputs(ragged_case(regime, S))
        ss.append(s[0])
        ys.append(y[0])
        info.append((regime, paths[0]))
    return torch.cat(ss), torch.cat(ys), info
