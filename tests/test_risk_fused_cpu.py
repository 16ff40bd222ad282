"""CPU: the host contract of the fused risk-loss step (ltr_mi355x.risk_step, FusedRanker's risk losses) -- names, options, required
baselines and their shapes, CPU tensors refused, new C-ABI symbols exported -- without a GPU."""
import ctypes

import pytest
import torch

LOSSES = ["geoRiskListnetLoss", "geoRiskLambdaLoss", "zRiskListnetLoss", "zRiskLambdaLoss", "tRiskListnetLoss", "tRiskLambdaLoss"]


def test_fused_ranker_lists_the_six_risk_losses():
    from ltr_mi355x.scorer import LOSS_RISK, FusedRanker
    for name in LOSSES:
        assert FusedRanker.LOSSES[name] == LOSS_RISK
    for name in ("approxNDCG", "listnet", "lambdaLoss"):
        assert FusedRanker.LOSSES[name] != LOSS_RISK


def test_reference_defaults_and_flags():
    from ltr_mi355x.risk_step import RISK_GEO, RISK_Z, RiskSpec
    s = RiskSpec("geoRiskLambdaLoss")
    assert s.args == dict(alpha=5, listnet_transformation=1, return_strategy=1, negative=1, add_ideal_ranking_to_mat=1,
                          weighing_scheme="ndcgLoss2PP_scheme")
    assert (s.kind, s.lam, s.t, s.mode, s.flip, s.zquirk, s.ideal, s.ones) == (RISK_GEO, True, False, 1, True, False, False, False)
    s = RiskSpec("geoRiskLambdaLoss", dict(listnet_transformation=2, add_ideal_ranking_to_mat=2))
    assert s.ones and not s.ideal and not s.flip and s.n_const(3) == 4
    s = RiskSpec("zRiskLambdaLoss", dict(listnet_transformation=2, add_ideal_ranking_to_mat=2))
    assert s.ideal and not s.ones and s.kind == RISK_Z and s.n_const(3) == 4
    s = RiskSpec("zRiskListnetLoss", dict(listnet_transformation=3))
    assert s.zquirk and s.flip and s.mode == 0
    s = RiskSpec("tRiskListnetLoss")
    assert s.args == dict(alpha=5, listnet_transformation=1, negative=1) and s.mode == 2 and s.n_const(1) == 1
    s = RiskSpec("tRiskLambdaLoss", dict(listnet_transformation=3, negative=-2))
    assert s.mode == 1 and not s.flip and s.factor == -2.0


def test_options_outside_the_fused_path_raise():
    from ltr_mi355x.risk_step import RiskSpec
    with pytest.raises(NotImplementedError, match="listnet_transformation"):
        RiskSpec("zRiskLambdaLoss", dict(listnet_transformation=3))
    with pytest.raises(NotImplementedError, match="listnet_transformation"):
        RiskSpec("geoRiskListnetLoss", dict(listnet_transformation=4))
    with pytest.raises(NotImplementedError, match="return_strategy"):
        RiskSpec("geoRiskListnetLoss", dict(return_strategy=0))
    with pytest.raises(NotImplementedError, match="negative"):
        RiskSpec("geoRiskListnetLoss", dict(negative=torch.ones(1)))
    with pytest.raises(TypeError, match="return_strategy"):
        RiskSpec("tRiskListnetLoss", dict(return_strategy=2))           # not a keyword of the reference's tRisk losses
    with pytest.raises(TypeError):
        RiskSpec("geoRiskListnetLoss", dict(normalization=True))          # the driver's keyword, not the function's
    with pytest.raises(KeyError):
        RiskSpec("geoRiskWhatever")
    with pytest.raises(KeyError):
        RiskSpec("geoRiskLambdaLoss", dict(weighing_scheme="no_such_scheme"))


def test_baseline_shapes_per_loss():
    from ltr_mi355x.risk_step import RiskSpec
    B, S = 4, 10
    g = RiskSpec("geoRiskListnetLoss")
    assert g.baselines(B, S, torch.zeros(B, S, 3)).shape == (B, S, 3)
    for bad in (torch.zeros(B, S), torch.zeros(B, S, 1), torch.zeros(B, S, 65), torch.zeros(B, S + 1, 3)):
        with pytest.raises(ValueError):
            g.baselines(B, S, bad)
    with pytest.raises(ValueError, match="y_base"):
        g.baselines(B, S, None)
    t = RiskSpec("tRiskLambdaLoss")
    assert t.baselines(B, S, torch.zeros(B, S)).shape == (B, S, 1)
    assert t.baselines(B, S, torch.zeros(B, S, 1)).shape == (B, S, 1)
    with pytest.raises(ValueError):
        t.baselines(B, S, torch.zeros(B, S, 3))
    # cached columns: the Lambda forms carry the ideal column sums [S] after the constant matrix entries
    lam = RiskSpec("geoRiskLambdaLoss")
    bc, n_c = lam.cached(B, S, torch.zeros(B, 3 + S))
    assert n_c == 3 and bc.shape == (B, 3 + S)
    with pytest.raises(ValueError):
        lam.cached(B, S, torch.zeros(B, 1 + S))
    assert g.cached(B, S, torch.zeros(B, 3))[1] == 3
    assert RiskSpec("tRiskListnetLoss").cached(B, S, torch.zeros(B, 1))[1] == 1
    with pytest.raises(ValueError):
        RiskSpec("tRiskListnetLoss").cached(B, S, torch.zeros(B, 2))


def test_cpu_tensors_are_refused():
    from ltr_mi355x import LtrDeviceError
    from architeture.doubleLayer import DoubleLayerNet
    from ltr_mi355x.scorer import FusedRanker
    with pytest.raises(LtrDeviceError):
        FusedRanker(DoubleLayerNet(64), loss="geoRiskLambdaLoss")
    with pytest.raises(KeyError):
        FusedRanker(DoubleLayerNet(64), loss="geoRiskLambda")
    with pytest.raises(NotImplementedError):
        FusedRanker(DoubleLayerNet(64), loss="geoRiskLambdaLoss", risk_args=dict(listnet_transformation=3))


def test_trainer_passes_extras_and_hands_the_group():
    from ltr_mi355x.dp import QueryShardedTrainer

    class Local:
        def __init__(self):
            self.flat = torch.zeros(3)
            self.flat_ext = torch.zeros(4)
            self.risk_group, self.risk_rank, self.risk_world = "unset", -1, -1
            self.calls = []

        def step(self, X, y, **kw):
            self.calls.append(kw)

        def finish_norm(self):
            return self.flat[-1]

    loc = Local()
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=0.1)
    tr = QueryShardedTrainer(loc, opt, group=None)
    assert (loc.risk_group, loc.risk_rank, loc.risk_world) == (None, 0, 1)
    yb = torch.zeros(2, 3, 2)
    tr.step(torch.zeros(2, 3, 4), torch.zeros(2, 3), y_base=yb)
    tr.step(torch.zeros(2, 3, 4), torch.zeros(2, 3), global_batch=2, base_cols=yb[:, 0])
    assert loc.calls[0]["y_base"] is yb and loc.calls[0]["defer_norm"] is True
    assert loc.calls[1]["world_batch"] == 2 and "base_cols" in loc.calls[1]


def test_new_symbols_exported_and_bound(root):
    from ltr_mi355x import _lib
    from ltr_mi355x.build import build
    build(force=False, verbose=False)
    raw = ctypes.CDLL(_lib.library_path())
    for name in ("ltr_lambda_colsum_sys_bwd_coef", "ltr_lambda_risk_model_fwd", "ltr_risk_matrix_rows_fwd", "ltr_risk_matrix_cached_fwd",
                 "ltr_risk_scores_grad", "ltr_risk_tail_blocks_fwd_bwd", "ltr_trisk_tail_blocks_fwd_bwd"):
        assert hasattr(raw, name), name
        assert name in _lib._PROTOTYPES, name
    h = _lib.lib()
    # argument checks run before any device work
    assert h.ltr_risk_tail_blocks_fwd_bwd(None, 2, 4, 3, 5.0, 1, 1, 1, 1.0, 0, None, None, None) == -1
    assert h.ltr_trisk_tail_blocks_fwd_bwd(None, 2, 4, 5.0, 1, 1.0, None, None, None) == -1
    assert h.ltr_risk_scores_grad(None, None, 1, 2, 2, None, None) == -1
