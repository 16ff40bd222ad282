"""CPU: the six risk-sensitive losses on ragged batches -- the reference restatement (tests/ragged_risk_cases.py) anchored to the
committed rectangular oracle, its row independence, the conditioning of every case the GPU file uses, the new C-ABI entries and the
host contract of FusedRanker.step_ragged's risk route (the checks that precede device use)."""
import ctypes

import numpy as np
import pytest
import torch

import ltr_risk_oracle as RO
import ragged_cases as RC
import ragged_risk_cases as RR

ORACLE = {"geoRiskListnetLoss": RO.geo_risk_listnet, "zRiskListnetLoss": RO.z_risk_listnet, "geoRiskLambdaLoss": RO.geo_risk_lambda,
          "zRiskLambdaLoss": RO.z_risk_lambda, "tRiskListnetLoss": RO.t_risk_listnet, "tRiskLambdaLoss": RO.t_risk_lambda}
KW = {"alpha": "alpha", "listnet_transformation": "lt", "return_strategy": "rs", "negative": "negative",
      "add_ideal_ranking_to_mat": "add_ideal", "weighing_scheme": "scheme"}
NEW_ENTRIES = ("ltr_risk_matrix_ragged_fwd", "ltr_risk_scores_grad_ragged", "ltr_lambda_colsum_sys_ragged_fwd",
               "ltr_lambda_risk_model_ragged_fwd", "ltr_lambda_colsum_sys_ragged_bwd_coef")


def _rel(a, b):
    """max|a - b| / max|b| over the finite entries; the non-finite ones (a two-document query under a cosine of constant column sums
    is 0 / 0 in the committed oracle too) must be the same values at the same places."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    bad = ~np.isfinite(b)
    assert np.array_equal(a[bad], b[bad], equal_nan=True) and np.isfinite(a[~bad]).all()
    if bad.all():
        return 0.0
    return float(np.abs(a[~bad] - b[~bad]).max() / max(np.abs(b[~bad]).max(), 1e-300))


# ------------------------------------------------------------------------------------- 1. equal lengths: the committed oracle
@pytest.mark.parametrize("S", [2, 17, 128])
@pytest.mark.parametrize("name", RR.LOSSES)
def test_equal_lengths_are_the_rectangular_oracle(name, S):
    Q = 5
    for i, args in enumerate(RR.option_sets(name)):
        _, s, y, yb = RR.data(name, [S] * Q, 40 + i)
        bounds = RC.bounds_of([S] * Q)
        a = s.double().requires_grad_(True)
        la = RR.ragged_risk_oracle(name, a, y, yb, bounds, **args)
        la.sum().backward()
        b = s.double().requires_grad_(True)
        ybr = yb.double().view(Q, S) if name.startswith("tRisk") else yb.double().view(Q, S, RR.NB)
        lb = ORACLE[name](b.view(Q, S), y.double().view(Q, S), ybr, **{KW[k]: v for k, v in args.items()})
        lb.sum().backward()
        assert la.shape == lb.shape == (1,)
        assert _rel(la.detach(), lb.detach()) <= 1e-12, (name, S, args, float(la), float(lb))
        assert _rel(a.grad, b.grad) <= 1e-12, (name, S, args)


# ------------------------------------------------------------------------------------- 2. row independence
@pytest.mark.parametrize("name", RR.LOSSES)
def test_rows_do_not_depend_on_the_other_queries(name):
    lengths = [9, 2, 40, 17, 130]
    bounds = RC.bounds_of(lengths)
    for args in (RR.option_sets(name)[0], RR.option_sets(name)[-1]):
        _, s, y, yb = RR.data(name, lengths, 77)
        mat = RR.ragged_risk_rows(name, s, y, yb, bounds, **args)
        for q, (lo, hi) in enumerate(zip(bounds[:-1], bounds[1:])):
            two = RR.ragged_risk_rows(name, torch.cat([s[lo:hi]] * 2), torch.cat([y[lo:hi]] * 2), torch.cat([yb[lo:hi]] * 2),
                                      RC.bounds_of([lengths[q]] * 2), **args)
            assert torch.equal(two[0], two[1]) and torch.equal(mat[q], two[0]), (name, q)


# ------------------------------------------------------------------------------------- 3. every GPU case is well conditioned in fp32
def _finite(loss, grads):
    return bool(np.isfinite(loss)) and all(np.isfinite(v).all() for v in grads.values())


def test_loss_cases_have_a_finite_fp32_oracle():
    assert {c[0] for c in RR.LOSS_CASES} == set(RR.LOSSES)
    for name, lengths, seed, args in RR.LOSS_CASES:
        i = RR.option_sets(name).index(args)
        for dtype in (torch.float32, torch.float64):
            _, s, y, yb = RR.data(name, lengths, seed)
            x = s.clone().requires_grad_(True)
            out = RR.ragged_risk_oracle(name, x, y, yb, RC.bounds_of(lengths), dtype, **args).sum()
            out.backward()
            assert _finite(float(out.detach()), {"s": x.grad.numpy()}), (
                f"the {dtype} oracle of ({name!r}, option set {i}) = {args} is non-finite at seed {seed}: move the entry "
                f"({name!r}, {i}) of ragged_risk_cases._SEED_RUNG to the next rung whose oracle is finite")
    # the table holds nothing but rungs above the first, each the FIRST finite one of its ladder
    for (name, i), k in RR._SEED_RUNG.items():
        assert k >= 1 and name in RR.LOSSES and 0 <= i < len(RR.option_sets(name)), (name, i, k)
        args = RR.option_sets(name)[i]
        for lower in range(k):
            fin = []
            for dtype in (torch.float32, torch.float64):
                _, s, y, yb = RR.data(name, RR.LOSS_LENGTHS, 300 + i + 1000 * lower)
                x = s.clone().requires_grad_(True)
                out = RR.ragged_risk_oracle(name, x, y, yb, RC.bounds_of(RR.LOSS_LENGTHS), dtype, **args).sum()
                out.backward()
                fin.append(_finite(float(out.detach()), {"s": x.grad.numpy()}))
            assert not all(fin), f"_SEED_RUNG[({name!r}, {i})] = {k}, but rung {lower} is already finite: lower the entry"


@pytest.mark.parametrize("case", RR.STEP_CASES, ids=RR.step_case_id)
def test_step_cases_have_a_finite_fp32_oracle(case):
    name, geom, batch, train = case
    lengths, x, y, yb, keep = RR.step_data(case)
    assert min(lengths) >= 2 and (batch != "tiers" or max(lengths) == 2048)
    _, params = RR.make_net(geom, "cpu")
    loss, grads = RR.step_oracle(name, geom, params, x, y, yb, RC.bounds_of(lengths), {}, keep, dtype=torch.float32)
    assert _finite(loss, grads), case


# ------------------------------------------------------------------------------------- 4. ABI
def test_new_entries_exported_and_bound():
    from ltr_mi355x import _lib
    from ltr_mi355x.build import build
    build(force=False, verbose=False)
    raw = ctypes.CDLL(_lib.library_path())
    for name in NEW_ENTRIES:
        assert hasattr(raw, name), name
        assert name in _lib._PROTOTYPES, name
    h = _lib.lib()
    # argument checks run before any device work
    assert h.ltr_risk_matrix_ragged_fwd(None, None, None, None, None, 2, 8, 16, 3, 0, 1, 0, 0, None, 0, None, None, None) == -1
    assert h.ltr_risk_scores_grad_ragged(None, None, 1, None, None, 2, 16, None, None) == -1
    assert h.ltr_lambda_colsum_sys_ragged_fwd(None, None, None, None, None, 2, 8, 16, 3, 4, 0, 1.0, 10.0, 1e-10, -1.0, 0, None, None) == -1
    assert h.ltr_lambda_risk_model_ragged_fwd(None, None, None, 4, None, 4, None, None, 2, 8, 16, 4, 0, 1.0, 10.0, 1e-10, -1.0, 0, 1, None,
                                              None, None) == -1
    assert h.ltr_lambda_colsum_sys_ragged_bwd_coef(None, None, None, None, 2, 8, 16, 4, 0, 1.0, 10.0, 1e-10, -1.0, 0, None, None, 4, None,
                                                   None) == -1


# ------------------------------------------------------------------------------------- 5. host contract
def test_host_checks_precede_device_use():
    from ltr_mi355x import ragged
    from ltr_mi355x.ragged import RaggedSlates
    from ltr_mi355x.risk_step import RiskSpec
    ok = RaggedSlates(RC.bounds_of([4, 9, 2]))
    yb = torch.zeros(15, 3)
    for name in RR.LOSSES:
        spec = RiskSpec(name)
        with pytest.raises(NotImplementedError, match="FusedRanker.step"):
            ragged.check_risk_batch(spec, ok, None, None)
        with pytest.raises(ValueError, match="exactly one"):
            ragged.check_risk_batch(spec, ok, yb, (yb, None))
        with pytest.raises(ValueError, match="query 1 has 1 document"):
            ragged.check_risk_batch(spec, RaggedSlates(RC.bounds_of([4, 1, 9, 1])), yb, None)
        with pytest.raises(NotImplementedError, match="at least 2 queries"):
            ragged.check_risk_batch(spec, RaggedSlates(RC.bounds_of([4])), yb, None)
        ragged.check_risk_batch(spec, RaggedSlates(RC.bounds_of([4])), yb, None, min_queries=0)       # a rank of a data-parallel step
        ragged.check_risk_batch(spec, ok, yb, None)
    g, t = RiskSpec("geoRiskListnetLoss"), RiskSpec("tRiskLambdaLoss")
    assert ragged.risk_baselines(g, 15, yb).shape == (15, 3)
    assert ragged.risk_baselines(t, 15, yb[:, 0]).shape == ragged.risk_baselines(t, 15, yb[:, :1]).shape == (15, 1)
    for spec, bad in ((g, yb[:, :1]), (g, yb[:, 0]), (g, yb[:14]), (t, yb), (t, yb[:14, 0])):
        with pytest.raises(ValueError, match="y_base"):
            ragged.risk_baselines(spec, 15, bad)
    lam = RiskSpec("geoRiskLambdaLoss")
    ent, ics = ragged.risk_cached(lam, ok, (torch.zeros(3, 3), torch.zeros(15)))
    assert ent.shape == (3, 3) and ics.shape == (15,)
    for bad in ((torch.zeros(3, 3), None), (torch.zeros(3, 3), torch.zeros(14)), (torch.zeros(2, 3), torch.zeros(15)),
                (torch.zeros(3, 1), torch.zeros(15)), torch.zeros(3, 3)):
        with pytest.raises(ValueError, match="base_cols"):
            ragged.risk_cached(lam, ok, bad)
    assert ragged.risk_cached(g, ok, (torch.zeros(3, 3), None))[1] is None


def test_risk_wrappers_mirror_the_reference_names():
    import inspect
    from ltr_mi355x import ragged
    for name in RR.LOSSES:
        assert list(inspect.signature(getattr(ragged, name)).parameters)[:4] == ["y_predicted", "y_true", "slates", "y_baselines"]
    with pytest.raises(KeyError):
        ragged.risk_loss("geoRiskWhatever", torch.zeros(4), torch.zeros(4), None, torch.zeros(4, 3))
    with pytest.raises(NotImplementedError, match="return_strategy"):
        ragged.risk_loss("zRiskListnetLoss", torch.zeros(4), torch.zeros(4), None, torch.zeros(4, 3), return_strategy=4)


def test_trainer_step_ragged_protocol():
    from ltr_mi355x.dp import QueryShardedTrainer
    from ltr_mi355x.ragged import RaggedSlates

    class Local:
        def __init__(self):
            self.flat = torch.zeros(3)
            self.flat_ext = torch.zeros(4)
            self.calls, self.finished = [], 0

        def step_ragged(self, X, y, slates, **kw):
            self.calls.append(kw)

        def finish_norm(self):
            self.finished += 1
            return self.flat[-1]

    loc = Local()
    tr = QueryShardedTrainer(loc, torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=0.1), group=None)
    sl = RaggedSlates(RC.bounds_of([2, 3]))
    yb = torch.zeros(5, 3)
    tr.step_ragged(torch.zeros(5, 4), torch.zeros(5), sl, y_base=yb)
    tr.step_ragged(torch.zeros(5, 4), torch.zeros(5), sl, global_batch=7, base_cols=(yb, None))
    tr.step_ragged(torch.zeros(5, 4), torch.zeros(5), sl)
    assert loc.calls[0]["y_base"] is yb and loc.calls[0]["defer_norm"] is True
    assert loc.calls[1]["world_batch"] == 7 and "base_cols" in loc.calls[1] and "defer_norm" not in loc.calls[1]
    assert loc.calls[2] == dict(defer_norm=True) and loc.finished == 2
