"""Case builders shared by tests/test_lambda_tiers_cpu.py and tests/test_lambda_tiers_gpu.py (a plain module, no fixtures).

The LambdaLoss kernels change their launch geometry with the slate length S (`pick_group` / `slate_geom` in csrc/ltr_device.h):
S <= 16, 17..32, 33..64, 65..128, 129..256, 257..512 (two column groups at 1024 threads), 513..1024 (one) and 1025..2048 (fewer row
lanes than documents, LDS past 64 KiB).  TIER_S sits on both sides of every edge.  Everything here runs on the CPU against the fp64
oracle alone: the inputs, the clamp-band precondition and the score-scale ladder.

Clamp band.  A pair term is max(w log max(u, eps), log eps): continuous across both clamps, its gradient is not, so a kept pair
within rounding of a clamp may take different branches in fp32 and fp64.  No pair is ever left out of a comparison; instead the
inputs are chosen so that the fp64 oracle shows NO kept pair with |w log u - log eps| < 1e-4 |log eps| (or the same for log u alone).
fp32 rounding moves w log u by about 1e-6 relative, so the band leaves two orders of margin.  The band count grows with the number
of pairs for the two label-difference schemes (w up to 4 and 16), so a seed search cannot empty it at S = 2048; a smaller score scale
can: the builder takes the first rung of LADDER (times randn) whose band count is 0 and raises if none has.  All rungs are powers of
two, so scores, ranks and ties are the same numbers at every rung up to the factor.
"""
import functools
import math
from collections import namedtuple

import torch

import ltr_oracle as O

TIER_S = [1, 2, 3, 16, 17, 31, 33, 64, 65, 127, 129, 255, 256, 257, 511, 513, 1023, 1024, 1025, 1500, 2047, 2048]
FULL_S = (17, 129, 256, 257, 1024, 1025, 2048)        # where every variant and option set runs
RAGGED_S = (17, 31)                                    # B = 5: a 256-thread workgroup shared by slates has a ragged last one
CLAMPED_S = (64, 1025)
LADDER = (2.0, 1.0, 0.5, 0.25, 0.125, 0.0625)
LADDER_SCHEMES = ("rankNetWeightedByGTDiff_scheme", "rankNetWeightedByGTDiffPowed_scheme")
OPTS = {                                               # (k, sigma, reduction_log); k "S+3" = beyond the slate
    "kNone-s1-binary": (None, 1.0, "binary"),
    "k5-s2-natural": (5, 2.0, "natural"),
    "k1-s1-binary": (1, 1.0, "binary"),
    "kS+3-s1-binary": ("S+3", 1.0, "binary"),
}
REQUIRED_OPTS = ("kNone-s1-binary", "k5-s2-natural")
EXTRA_OPTS = ("k1-s1-binary", "kS+3-s1-binary")
VARIANTS = ("plain", "padded", "flat_labels", "tied_scores", "softmaxed")
EPS, PAD, MU = 1e-10, -1, 10.0

Case = namedtuple("Case", "variant B S scheme opt scale")


def batch_of(S):
    return 3 if S <= 512 else 2


def regime(S):
    for hi, name in ((16, "1..16"), (32, "17..32"), (64, "33..64"), (128, "65..128"), (256, "129..256"), (512, "257..512"),
                     (1024, "513..1024")):
        if S <= hi:
            return name
    return "1025..2048"


def options(case):
    k, sigma, log = OPTS[case.opt]
    return dict(weighing_scheme=case.scheme, k=case.S + 3 if k == "S+3" else k, sigma=sigma, mu=MU, reduction_log=log)


def case_id(c):
    sc = "none" if c.scale is None else f"{c.scale:g}"
    return f"{c.variant}-B{c.B}-S{c.S}-{c.scheme}-{c.opt}-x{sc}"


# ------------------------------------------------------------------------------------------------- inputs
def inputs(variant, B, S, scale, seed=None):
    """(scores, labels) fp32 on the CPU, a function of (B, S, seed) and the score scale.  Both are fp32 numbers before the kernel
    or the oracle sees them, so the two sides rank the same values; equal scores are ranked by index on both sides."""
    gen = torch.Generator().manual_seed(300 + S if seed is None else seed)
    z = torch.randn(B, S, generator=gen)
    y = torch.randint(0, 5, (B, S), generator=gen).float()
    if variant == "softmaxed":           # what the risk losses feed in: tiny score gaps, five distinct label values, never == pad
        return torch.softmax(z, dim=1), torch.softmax(y, dim=1)
    s = z * float(scale)
    if variant in ("plain", "clamped"):
        return s, y
    if variant == "padded":
        for b in range(B):
            c = int(torch.randint(0, S, (1,), generator=gen))       # padded tail of 0 .. S-1 documents
            if c:
                y[b, S - c:] = -1.0
        if B >= 2:
            y[1, 1:] = -1.0                                          # a single real document
        if B >= 3:
            y[2, :] = -1.0                                           # all padding
        return s, y
    if variant == "flat_labels":
        y[0, :] = 2.0                                                # no kept pair except under ndcgLoss1
        if B >= 2:
            y[1, :] = 0.0                                            # ideal DCG clamps to eps
        return s, y
    if variant == "tied_scores":
        assert S >= 4
        s[:, 3] = s[:, 1]
        s[:, S - 1] = s[:, 1]
        n = max(1, int(round(0.05 * S)))
        for b in range(B):
            idx = torch.randperm(S, generator=gen)[:n]
            s[b, idx] = s[b].max()
        return s, y
    raise KeyError(variant)


# ------------------------------------------------------------------------------------------------- clamp band
def band_counts(s, y, kw, scales=(1.0,)):
    """Per score factor in `scales` (applied to `s`): (kept pairs in the clamp band, kept pairs firmly clamped), fp64 oracle only."""
    w, d, keep = O.lambda_pair_parts(s.double(), y.double(), EPS, PAD, kw["weighing_scheme"], kw["k"], kw["mu"])
    w = w.expand_as(d)[keep]
    d = d[keep]
    le = math.log(EPS)
    out = []
    for f in scales:
        lu = torch.nn.functional.logsigmoid(kw["sigma"] * f * d)
        near = lambda t: (t - le).abs() < 1e-4 * abs(le)
        band = near(lu) | near(w * lu)
        firm = ((lu < le) | (w * lu < le)) & ~band
        out.append((int(band.sum()), int(firm.sum())))
    return out


@functools.lru_cache(maxsize=None)
def ladder_scale(variant, B, S, scheme, opt):
    """First rung of LADDER with an empty clamp band for this case; raises if there is none."""
    c = Case(variant, B, S, scheme, opt, 1.0)
    s, y = inputs(variant, B, S, 1.0)
    counts = band_counts(s, y, options(c), LADDER)
    for f, (band, _) in zip(LADDER, counts):
        if band == 0:
            return f
    raise AssertionError(f"no rung of the score-scale ladder empties the clamp band for {case_id(c)}: {counts}")


def make_case(variant, B, S, scheme, opt):
    if variant == "softmaxed":
        scale = None
    elif variant == "clamped":
        scale = 30.0
    elif scheme in LADDER_SCHEMES:
        scale = ladder_scale(variant, B, S, scheme, opt)
    else:
        scale = LADDER[0]        # by the issue's table these schemes have an empty band at 2; check_precondition holds them to it
    return Case(variant, B, S, scheme, opt, scale)


def build(case):
    """(scores, labels, options) of a case, after asserting its precondition: no kept pair in the clamp band (fp64 oracle)."""
    s, y = inputs(case.variant, case.B, case.S, case.scale)
    kw = options(case)
    if case.variant != "clamped":
        (band, firm), = band_counts(s, y, kw)
        assert band == 0, f"{case_id(case)}: {band} kept pairs in the clamp band ({firm} firmly clamped)"
    return s, y, kw


@functools.lru_cache(maxsize=None)
def tier_cases():
    """Required: every scheme x every S x plain / padded x the first two option sets (B = 5 too at S = 17, 31); the other variants
    (first option set) and the other option sets (plain) at FULL_S for every scheme; one deliberately clamped case per scheme at
    S = 64 and 1025 (forward quantities only)."""
    out = []
    for scheme in O.SCHEMES:
        for S in TIER_S:
            for B in (batch_of(S),) + ((5,) if S in RAGGED_S else ()):
                for variant in ("plain", "padded"):
                    for opt in REQUIRED_OPTS:
                        out.append(make_case(variant, B, S, scheme, opt))
            if S in FULL_S:
                for variant in ("flat_labels", "tied_scores", "softmaxed"):
                    out.append(make_case(variant, batch_of(S), S, scheme, REQUIRED_OPTS[0]))
                for opt in EXTRA_OPTS:
                    out.append(make_case("plain", batch_of(S), S, scheme, opt))
        for S in CLAMPED_S:
            out.append(make_case("clamped", batch_of(S), S, scheme, REQUIRED_OPTS[0]))
    return tuple(out)


# ------------------------------------------------------------------------------------------------- lambdaLoss dispatch edges
EDGE_SHAPES = [(2, 255), (2, 256), (2, 257), (2, 1023), (2, 1024), (2, 1025), (2, 2047), (1, 2048)]


def edge_inputs(variant, B, S, scheme, k, sigma, log):
    """Inputs for the lambdaLoss dispatch-edge shapes (lambda_blocked_kernel takes 256 <= S <= 1024 except under ndcgLoss1): from
    the ladder, because at these sizes the two label-difference schemes have kept pairs in the clamp band with scores 2 randn."""
    kw = dict(weighing_scheme=scheme, k=k, sigma=sigma, mu=MU, reduction_log=log)
    s1, y = inputs(variant, B, S, 1.0)
    scales = LADDER if scheme in LADDER_SCHEMES else LADDER[:1]
    for f, (band, _) in zip(scales, band_counts(s1, y, kw, scales)):
        if band == 0:
            return inputs(variant, B, S, f)
    raise AssertionError(f"no score scale empties the clamp band: {variant} B{B} S{S} {scheme} k={k} sigma={sigma}")


# ------------------------------------------------------------------------------------------------- the oracle side of a case
def oracle_bundle(s, y, kw, gup, gcol, dtype, grads=True):
    """The oracle's pair matrix, keep mask, column sums and kept-pair loss in `dtype`, with the gradients of sum(losses * gup),
    sum(colsum * gcol) and -sum(losses[keep]) w.r.t. the scores (autograd through O.lambda_pairs)."""
    x = s.detach().clone().to(dtype).requires_grad_(True)      # a copy: .to() of the same dtype would alias the caller's tensor
    yy = y.to(dtype)
    losses, keep = O.lambda_pairs(x, yy, EPS, PAD, **kw)
    col = losses.sum(dim=1)
    slate = -(losses * keep.to(dtype)).sum(dim=(1, 2))
    out = dict(losses=losses.detach(), keep=keep, col=col.detach(), slate=slate.detach())
    if grads:
        out["g_full"], = torch.autograd.grad((losses * gup.to(dtype)).sum(), x, retain_graph=True)
        out["g_col"], = torch.autograd.grad((col * gcol.to(dtype)).sum(), x, retain_graph=True)
        out["g_sum"], = torch.autograd.grad(slate.sum(), x)
    return out


def real_pairs(y):
    """[B,S,S] bool in predicted-rank order: both documents of the pair are real (padded documents rank last)."""
    n = (y != PAD).sum(dim=1)
    r = torch.arange(y.shape[1])[None, :] < n[:, None]
    return r[:, :, None] & r[:, None, :]
