"""Helpers shared by tests/test_ragged_risk_cpu.py and tests/test_ragged_risk_gpu.py (a plain module, no fixtures): the fp64 reference
of the six risk-sensitive losses on a ragged batch, and the cases both files use.

Definition (the issue's): row q of the effectiveness matrix is the row the reference computes for query q inside any batch of queries
of q's own length, BEFORE the flip; the rows of all queries, in query order, form one [Q, n_systems] matrix, and the reference's tail
runs once on it.  The committed oracle's matrix functions (oracle/ltr_risk_oracle.py listnet_matrix / lambda_matrix / _t_cols) flip
with a per-call maximum, so they cannot be concatenated across length groups: `ragged_risk_rows` restates their column formulas
un-flipped, per query, from the oracle's own building blocks (torch.softmax over the query's documents, pair_colsum, _cos), and
`ragged_risk_oracle` runs the oracle's own geo_risk / z_risk / t_risk_tail and strategies on the assembled matrix.  Each query is a
batch of ONE, so the oracle's torch.squeeze (which would drop the batch axis) is not applied: the softmax keeps shape [1, S].
tests/test_ragged_risk_cpu.py anchors the restatement to the committed functions on equal lengths (1e-12)."""
import numpy as np
import torch

import ltr_risk_oracle as RO
import ragged_cases as RC

LOSSES = ["geoRiskListnetLoss", "geoRiskLambdaLoss", "zRiskListnetLoss", "zRiskLambdaLoss", "tRiskListnetLoss", "tRiskLambdaLoss"]
NB = 3
_DEFAULTS = dict(alpha=5, listnet_transformation=1, return_strategy=1, negative=1, add_ideal_ranking_to_mat=1,
                 weighing_scheme="ndcgLoss2PP_scheme")


def option_sets(name):
    """tests/test_risk_fused_gpu.py::_option_sets (every option the rectangular fused step accepts), restated here because that module
    is GPU-marked and imports the device suite."""
    out = []
    t, lam = name.startswith("tRisk"), "Lambda" in name
    lts = (1, 2) if (lam and not t) else (1, 2, 3)
    for lt in lts:
        if t:
            out.append(dict(listnet_transformation=lt, alpha=2.0, negative=-1))
            continue
        for rs in (1, 2, 3):
            for ai in (1, 2):
                out.append(dict(listnet_transformation=lt, return_strategy=rs, add_ideal_ranking_to_mat=ai))
    if lam:
        out.append(dict(weighing_scheme="ndcgLoss1_scheme", listnet_transformation=2))
    return out


def _args(name, args):
    a = dict(_DEFAULTS)
    for k, v in args.items():
        if k not in a:
            raise TypeError(f"{name}: unexpected keyword {k!r}")
        a[k] = v
    return a


def _query_row(name, sq, yq, ybq, a):
    """One query as a batch of one: sq, yq [1, S], ybq [1, S, nb] -> its un-flipped matrix row [n_systems]."""
    t, lam = name.startswith("tRisk"), "Lambda" in name
    lt, ai, scheme = a["listnet_transformation"], a["add_ideal_ranking_to_mat"], a["weighing_scheme"]
    pt, pp, pb = torch.softmax(yq, dim=1), torch.softmax(sq, dim=1), torch.softmax(ybq, dim=1)
    base = [pb[:, :, j] for j in range(pb.shape[2])]
    if t:
        # t_risk_listnet / t_risk_lambda + _t_cols, un-flipped: (model, baseline)
        if lam:
            qt, cols_in = RO.pair_colsum(pt, pt, scheme), [RO.pair_colsum(pp, pt, scheme), RO.pair_colsum(base[0], pt, scheme)]
        else:
            qt, cols_in = pt * pt, [pt * pp, pt * base[0]]
        if lt == 1:
            cols = [((c - qt) ** 2).sum(dim=1) for c in cols_in]
        elif lt == 2:
            cols = [RO._cos(qt, c) for c in cols_in]
        else:
            cols = [(c.sum(dim=1) - qt.sum(dim=1)) ** 2 for c in cols_in]
    elif lam:
        # lambda_matrix, un-flipped
        tt = RO.pair_colsum(pt, pt, scheme)
        systems = [RO.pair_colsum(p, pt, scheme) for p in [pp] + base]
        if lt == 1:
            cols = [((c - tt) ** 2).sum(dim=1) for c in systems]
            if ai == 2:
                cols.append(torch.zeros_like(cols[0]))
        else:
            cols = [RO._cos(tt, c) for c in systems]
            if ai == 2:
                cols.append(torch.ones(1, dtype=torch.float) if name.startswith("geo") else RO._cos(tt, tt))
    else:
        # listnet_matrix, un-flipped
        systems = [pp] + base + ([pt] if ai == 2 else [])
        if lt == 1:
            cols = [((pt * p - pt * pt) ** 2).sum(dim=1) for p in systems]
        elif lt == 2:
            cols = [RO._cos(pt, p) for p in systems]
        else:
            ref = (pt * pt).sum(dim=1)
            cols = [((pt * p).sum(dim=1) - ref) ** 2 for p in systems]
    return torch.cat([c.to(sq.dtype).reshape(1) for c in cols])


def ragged_risk_rows(name, s, y, yb, bounds, dtype=torch.float64, **args):
    """The un-flipped [Q, n_systems] matrix.  s, y [n_docs]; yb [n_docs, nb] (tRisk: [n_docs] or [n_docs, 1]).  `s` may carry a graph."""
    a = _args(name, args)
    s, y, yb = s.to(dtype), y.to(dtype), yb.to(dtype)
    if yb.dim() == 1:
        yb = yb[:, None]
    rows = [_query_row(name, s[lo:hi][None], y[lo:hi][None], yb[lo:hi][None], a) for lo, hi in zip(bounds[:-1], bounds[1:])]
    return torch.stack(rows)


def ragged_risk_tail(name, mat, **args):
    """The reference's tail on the assembled matrix: flip, risk(s), strategy, `negative` (the zRiskListnetLoss precedence included)."""
    a = _args(name, args)
    t, lam = name.startswith("tRisk"), "Lambda" in name
    lt, rs, neg, alpha = a["listnet_transformation"], a["return_strategy"], a["negative"], a["alpha"]
    if lt == 1 or (lt == 3 and not lam and not t):
        mat = mat.max() - mat
    if t:
        return (neg * RO.t_risk_tail(mat[:, 0], mat[:, 1], alpha)).reshape(1)
    if name == "zRiskListnetLoss" and rs == 2:
        return (neg * RO.z_risk(mat, alpha, -1) - RO.z_risk(mat, alpha)).reshape(1)
    fn = RO.geo_risk if name.startswith("geo") else RO.z_risk
    return (neg * RO._strategy(fn, mat, alpha, rs)).reshape(1)


def ragged_risk_oracle(name, s, y, yb, bounds, dtype=torch.float64, **args):
    """The loss [1] (in `s`'s graph); args: the reference's keywords (alpha, listnet_transformation, return_strategy, negative,
    add_ideal_ranking_to_mat, weighing_scheme)."""
    return ragged_risk_tail(name, ragged_risk_rows(name, s, y, yb, bounds, dtype, **args), **args)


# ------------------------------------------------------------------------------------------------------------ cases
def lengths_of(batch):
    """The two length lists of the GPU step test: every tier's lengths but 1, and a long-tailed batch clipped to >= 2."""
    if batch == "tiers":
        return [n for n in RC.tier_lengths() if n >= 2]
    return [max(2, n) for n in RC.mslr_like_lengths(64, 7)]


def data(name, lengths, seed, F=None):
    """(x [n_docs, F] or None, s [n_docs] random scores, y, yb) -- integer grades 0 .. 4, baselines randn * 2 (tRisk: their mean, the
    reference driver's tRisk baseline, main_batch_execution.py)."""
    g = torch.Generator().manual_seed(seed)
    n = int(sum(lengths))
    x = torch.randn(n, F, generator=g) if F else None
    s = torch.randn(n, generator=g) * 2.0
    y = torch.randint(0, 5, (n,), generator=g).float()
    yb = torch.randn(n, NB, generator=g) * 2.0
    if name.startswith("tRisk"):
        yb = yb.mean(dim=1)
    return x, s, y, yb


LOSS_LENGTHS = [40, 3, 129, 17, 64, 260, 2, 90]                      # the autograd-node cases: eight tiers in one batch
# (loss, lengths, seed, options) of every ragged.risk_loss comparison of the GPU file.  Seed of option set i: the first of the ladder
# 300 + i + 1000 k, k = 0, 1, ..., whose fp32 AND fp64 oracle come out finite -- the oracle alone decides (some draws put the flipped
# matrix's zero, the old maximum, where a risk divides by the expected effectiveness: 0 / 0 in the reference itself); k = 0 everywhere
# but for the three below, and tests/test_ragged_risk_cpu.py::test_loss_cases_have_a_finite_fp32_oracle re-checks every case.
_SEED_RUNG = {("geoRiskLambdaLoss", 3): 3, ("geoRiskLambdaLoss", 8): 1, ("zRiskLambdaLoss", 8): 1}
LOSS_CASES = [(n, LOSS_LENGTHS, 300 + i + 1000 * _SEED_RUNG.get((n, i), 0), a) for n in LOSSES for i, a in enumerate(option_sets(n))]


def relgrad(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


# ------------------------------------------------------------------------------------------------------------ the training step
GEOMS = ("double136", "triple136", "fc136")          # DoubleLayerNet(136), TripleLayerNet(136), make_model FC 136-128-256-128-1
FC_SIZES = [128, 256, 128]
# (loss, network, batch, train): everything test_step_ragged_vs_oracle runs; train = exported keep masks (DoubleLayerNet's dropout)
STEP_CASES = [(n, g, b, False) for n in LOSSES for g in GEOMS for b in ("tiers", "mslr_like")]
STEP_CASES += [(n, "double136", "mslr_like", True) for n in LOSSES]


def step_case_id(c):
    return f"{c[0]}-{c[1]}-{c[2]}" + ("-train" if c[3] else "")


def make_net(geom, device, seed=3):
    """(module on `device`, its parameters for the oracle: a state_dict copy, or the _ltr_params() list for the FC network)."""
    torch.manual_seed(seed)
    if geom == "fc136":
        from architeture.multiLayer import make_model
        net = make_model(dict(sizes=list(FC_SIZES), input_norm=False, activation=None, dropout=0.0), False,
                         dict(output_activation="Sigmoid", d_output=1), 136)
        return net.to(device).eval(), [p.detach().cpu().clone() for p in net._ltr_params()]
    from architeture.doubleLayer import DoubleLayerNet
    from architeture.tripleLayer import TripleLayerNet
    net = (DoubleLayerNet if geom.startswith("double") else TripleLayerNet)(136)
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    return net.to(device).eval(), sd


def step_data(case):
    name, geom, batch, train = case
    lengths = lengths_of(batch)
    seed = 500 + 7 * LOSSES.index(name) + 3 * GEOMS.index(geom) + (1 if batch == "tiers" else 0)
    x, _, y, yb = data(name, lengths, seed, F=136)
    keep = None
    if train:
        g = torch.Generator().manual_seed(seed + 1)
        n = x.shape[0]
        keep = ((torch.rand(n, 136, generator=g) < 0.5).float(), (torch.rand(n, 136, generator=g) < 0.5).float())
    return lengths, x, y, yb, keep


def step_oracle(name, geom, params, x, y, yb, bounds, args, keep=None, dtype=torch.float64):
    """Loss and every parameter gradient of net -> ragged risk loss by CPU autograd in `dtype` -> (float, {key: array})."""
    import ltr_oracle as O
    xx = x.to(dtype)
    if geom == "fc136":
        from test_linear_fused_cpu import linear_forward
        p = [t.detach().cpu().to(dtype).clone().requires_grad_(True) for t in params]
        s = linear_forward(xx, p, FC_SIZES, False, dtype)
        named = {str(i): t for i, t in enumerate(p)}
    else:
        named = {k: v.to(dtype).clone().requires_grad_(True) for k, v in params.items()}
        if geom.startswith("double"):
            k1, k2 = (None, None) if keep is None else (keep[0].to(dtype), keep[1].to(dtype))
            s = O.double_layer_forward(xx, named, k1, k2).squeeze(-1)
        else:
            s = O.triple_layer_forward(xx, named).squeeze(-1)
    loss = ragged_risk_oracle(name, s, y, yb, bounds, dtype, **args).sum()
    loss.backward()
    return float(loss.detach()), {k: v.grad.detach().numpy() for k, v in named.items()}
