"""CPU: the host contract of the risk-loss step of FC-only make_model rankers (ltr_mi355x.linear.LinearFusedRanker with one of the six
risk-sensitive losses): option errors surface before any device check, and the two new C-ABI entries are declared, exported and bound."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOSSES = ["geoRiskListnetLoss", "geoRiskLambdaLoss", "zRiskListnetLoss", "zRiskLambdaLoss", "tRiskListnetLoss", "tRiskLambdaLoss"]


def _cpu_model(F=136, sizes=(128, 256, 128)):
    from architeture.multiLayer import make_model
    return make_model(dict(sizes=list(sizes), input_norm=False, activation=None, dropout=0.0), False,
                      dict(output_activation="Sigmoid", d_output=1), F)


def test_option_errors_surface_without_a_device():
    from ltr_mi355x.scorer import FusedRanker
    net = _cpu_model()
    with pytest.raises(NotImplementedError, match="return_strategy"):
        FusedRanker(net, loss="geoRiskListnetLoss", risk_args=dict(return_strategy=0))
    with pytest.raises(NotImplementedError, match="listnet_transformation"):
        FusedRanker(net, loss="zRiskLambdaLoss", risk_args=dict(listnet_transformation=3))
    with pytest.raises(TypeError, match="normalization"):
        FusedRanker(net, loss="geoRiskListnetLoss", risk_args=dict(normalization=True))
    with pytest.raises(TypeError, match="return_strategy"):
        FusedRanker(net, loss="tRiskLambdaLoss", risk_args=dict(return_strategy=2))


@pytest.mark.parametrize("name", LOSSES)
def test_valid_options_on_a_cpu_model_reach_the_device_check(name):
    from ltr_mi355x import LtrDeviceError
    from ltr_mi355x.scorer import FusedRanker
    args = dict(alpha=5) if name.startswith("tRisk") else dict(alpha=5, return_strategy=2)
    with pytest.raises(LtrDeviceError):
        FusedRanker(_cpu_model(), loss=name, risk_args=args)
    with pytest.raises(LtrDeviceError):
        FusedRanker(_cpu_model(), loss=name)


def test_risk_args_belong_to_the_risk_losses():
    from ltr_mi355x.scorer import FusedRanker
    for loss in ("listnet", "approxNDCG", "lambdaLoss"):
        with pytest.raises(TypeError, match="risk_args"):
            FusedRanker(_cpu_model(), loss=loss, risk_args=dict(alpha=5))


def test_step_takes_y_base_and_base_cols():
    import inspect
    from ltr_mi355x.linear import LinearFusedRanker
    sig = inspect.signature(LinearFusedRanker.step).parameters
    assert "y_base" in sig and "base_cols" in sig
    assert "risk_args" in inspect.signature(LinearFusedRanker.__init__).parameters


def test_new_entries_declared_exported_and_bound():
    with open(os.path.join(ROOT, "include", "ltr_mi355x.h")) as f:
        header = f.read()
    from ltr_mi355x import _lib
    from ltr_mi355x._scorer_protos import PROTOTYPES
    from ltr_mi355x.build import build
    build(force=False, verbose=False)
    raw = ctypes.CDLL(_lib.library_path())
    for name in ("ltr_linear_risk_rows", "ltr_linear_risk_combine"):
        assert re.search(r"\bint\s+" + name + r"\(", header), name
        assert hasattr(raw, name), name
        assert name in PROTOTYPES, name
    for ref in ("riskLosses.py:8-49", ":128-169", ":247-276", "main_batch_execution.py:93-94"):
        assert ref in header, ref


def test_new_entries_reject_bad_arguments_before_any_launch():
    from ltr_mi355x import _lib
    h = _lib.lib()
    buf = (ctypes.c_float * 64)()                       # 16-byte alignment is checked after the shapes
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert h.ltr_linear_risk_rows(None, None, 2, 32, 136, None, 0, 0, 1, None, 0, 0, None, 1, None, 8, None) == -1
    for B, S, F in ((0, 32, 136), (2, 100, 136), (2, 32, 260), (2, 32, 134), (2, 16, 64)):
        assert h.ltr_linear_risk_rows(p, p, B, S, F, p, 0, 0, 1, p, 3, 3, p, 4, p, 8, None) == -2, (B, S, F)
    assert h.ltr_linear_risk_rows(p, p, 2, 32, 136, p, 0, 0, 1, p, 3, 3, p, 3, p, 8, None) == -2      # n_systems < 1 + n_cached
    assert h.ltr_linear_risk_combine(None, None, 1, 2, 136, None, 8, None) == -1
    assert h.ltr_linear_risk_combine(p, p, 4, 0, 136, p, 8, None) == -2
    assert h.ltr_linear_risk_combine(p, p, 4, 2, 2000, p, 8, None) == -2
    assert h.ltr_linear_risk_combine(p, p, 4, 2, 136, p, 0, None) == -3
