"""Helpers shared by tests/test_ragged_cpu.py and tests/test_ragged_gpu.py (a plain module, no fixtures): length lists, the
per-query fp64 oracle loop that defines a ragged loss, the -1-padded rectangle of a ragged batch, and the clamp-band-free lambdaLoss
inputs of a ragged batch.

The reference of every ragged loss is the committed oracle (oracle/ltr_oracle.py) called on each query as a batch of one and
combined by the reference's own reduction: approxNDCG mean over queries, ListNet sum, lambdaLoss sum of kept-pair terms or that sum
over the total kept-pair count ("mean").
"""
import functools

import numpy as np
import torch

import lambda_tier_cases as LT
import ltr_oracle as O

EPS, PAD = 1e-10, -1
ISSUE_LENGTHS = (1, 2, 3, 17, 33, 64, 65, 129, 257, 40, 5, 200)          # the CPU equivalence check


def tier_lengths(seed=11):
    """Every value of lambda_tier_cases.TIER_S once, in a seeded shuffled order."""
    rng = np.random.default_rng(seed)
    return [int(s) for s in rng.permutation(np.asarray(LT.TIER_S))]


def mslr_like_lengths(n, seed, mean=120.0, hi=1251):
    """A long-tailed synthetic length list (log-normal, clipped to 1 .. hi): the SHAPE of a web-search collection's documents per
    query, not a histogram of any real one."""
    rng = np.random.default_rng(seed)
    sigma = 0.9
    v = rng.lognormal(np.log(mean) - 0.5 * sigma * sigma, sigma, size=n)
    return [int(x) for x in np.clip(np.rint(v), 1, hi)]


def bounds_of(lengths):
    return np.concatenate(([0], np.cumsum(lengths))).astype(np.int64)


def random_batch(lengths, seed, scale=2.0):
    """(scores, labels) [n_docs] fp32: randn * scale, integer grades 0 .. 4."""
    g = torch.Generator().manual_seed(seed)
    n = int(sum(lengths))
    return torch.randn(n, generator=g) * scale, torch.randint(0, 5, (n,), generator=g).float()


def pad_rectangle(v, bounds, fill):
    """[n_docs] -> [Q, longest] with `fill` behind each query's documents."""
    sizes = np.diff(bounds)
    out = torch.full((len(sizes), int(sizes.max())), float(fill), dtype=v.dtype)
    for q, (a, b) in enumerate(zip(bounds[:-1], bounds[1:])):
        out[q, :b - a] = v[a:b]
    return out


def unpad(rect, bounds):
    return torch.cat([rect[q, :b - a] for q, (a, b) in enumerate(zip(bounds[:-1], bounds[1:]))])


def oracle_ragged(loss, s, y, bounds, dtype=torch.float64, **kw):
    """The per-query oracle loop.  Returns dict(loss, grad [n_docs], per_query [Q] (approxNDCG / ListNet: the query's loss;
    lambdaLoss: its kept-pair sum), count [Q] (lambdaLoss: kept pairs)).  kw: the oracle function's keywords."""
    x = s.detach().clone().to(dtype).requires_grad_(True)
    yy = y.to(dtype)
    per, cnt = [], []
    red = kw.pop("reduction", "sum")
    for a, b in zip(bounds[:-1], bounds[1:]):
        sq, yq = x[a:b][None, :], yy[a:b][None, :]
        if loss == "approxNDCG":
            per.append(O.approx_ndcg(sq, yq, **kw))
        elif loss == "listnet":
            per.append(O.listnet(yq, sq, **kw))
        else:
            losses, keep = O.lambda_pairs(sq, yq, EPS, PAD, **kw)
            per.append(-(losses * keep.to(dtype)).sum())
            cnt.append(int(keep.sum()))
    per_t = torch.stack([p.reshape(()) for p in per])
    if loss == "approxNDCG":
        total = per_t.mean()
    elif loss == "lambdaLoss" and red == "mean":
        total = per_t.sum() / sum(cnt) if sum(cnt) else per_t.sum() * float("nan")
    else:
        total = per_t.sum()
    grad, = torch.autograd.grad(total, x, allow_unused=True)
    if grad is None or not sum(cnt or [1]):
        grad = torch.zeros_like(x)
    return dict(loss=total.detach(), grad=grad.detach(), per_query=per_t.detach(), count=np.asarray(cnt, dtype=np.int64))


def lambda_kw(scheme, opt):
    k, sigma, log = LT.OPTS[opt]
    assert k != "S+3"
    return dict(weighing_scheme=scheme, k=k, sigma=sigma, mu=LT.MU, reduction_log=log)


@functools.lru_cache(maxsize=None)
def band_free_query(S, scheme, opt):
    """(scores, labels) [S] of one query: lambda_tier_cases.inputs("plain", 1, S, rung, seed=9000 + S) at the first LADDER rung whose
    clamp band holds no kept pair for this query (fp64 oracle); raises if no rung has."""
    kw = lambda_kw(scheme, opt)
    bkw = dict(weighing_scheme=scheme, k=kw["k"], sigma=kw["sigma"], mu=kw["mu"])
    s1, y = LT.inputs("plain", 1, S, 1.0, seed=9000 + S)
    counts = LT.band_counts(s1, y, bkw, LT.LADDER)
    for f, (band, _) in zip(LT.LADDER, counts):
        if band == 0:
            s, y = LT.inputs("plain", 1, S, f, seed=9000 + S)
            return s[0], y[0], f
    raise AssertionError(f"no rung of the ladder empties the clamp band: S={S} {scheme} {opt}: {counts}")


def band_free_batch(lengths, scheme, opt):
    """A ragged batch of band-free queries; asserts the band is empty for every query before returning."""
    kw = lambda_kw(scheme, opt)
    bkw = dict(weighing_scheme=scheme, k=kw["k"], sigma=kw["sigma"], mu=kw["mu"])
    ss, ys = [], []
    for S in lengths:
        s, y, _ = band_free_query(int(S), scheme, opt)
        (band, _firm), = LT.band_counts(s[None, :], y[None, :], bkw)
        assert band == 0, (S, scheme, opt, band)
        ss.append(s)
        ys.append(y)
    return torch.cat(ss), torch.cat(ys), kw
