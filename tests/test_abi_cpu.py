"""CPU: the C-ABI library builds, loads and exports every symbol include/*.h declares (no compute calls),
and the host layer refuses CPU tensors instead of falling back."""
import ctypes
import glob
import os
import re

import pytest
import torch


def _declared(root):
    names = set()
    for h in glob.glob(os.path.join(root, "include", "*.h")):
        src = re.sub(r"/\*.*?\*/", "", open(h).read(), flags=re.S)
        names |= set(re.findall(r"\b(ltr_[a-z0-9_]+)\s*\(", src))
    return sorted(names)


@pytest.fixture(scope="module")
def handle():
    from ltr_mi355x.build import build
    build(force=False, verbose=False)
    import ltr_mi355x
    return ltr_mi355x.lib()


def test_exports_every_declared_symbol(handle, root):
    import ctypes
    from ltr_mi355x import library_path
    raw = ctypes.CDLL(library_path())
    names = _declared(root)
    assert len(names) >= 10
    missing = [n for n in names if not hasattr(raw, n)]
    assert not missing, missing
    assert handle.ltr_abi_version() == 1
    assert handle.ltr_error_string(0) == b"ok"
    assert b"NULL" in handle.ltr_error_string(-1)


def test_bound_prototypes_cover_header(handle, root):
    from ltr_mi355x import _lib, _scorer_protos
    bound = set(_lib._PROTOTYPES) | set(_scorer_protos.PROTOTYPES)
    assert set(_declared(root)) == bound


def test_argument_rejection_without_gpu(handle):
    # launchers validate before touching the device: NULL pointers / bad shapes come back as LTR_ERR_*
    assert handle.ltr_approxndcg_fwd_bwd(None, None, 1, 8, 1.0, 1e-10, -1.0, 1.0, None, None, None) == -1
    assert handle.ltr_reduce_sum_f32(None, 4, 1.0, None, None) == -1
    assert handle.ltr_ordinal_num_blocks(1000) == 4


# Every launcher of csrc/ltr_losses.hip with a call that passes its argument checks: (name, value) in the C order, the stream (NULL)
# left off.  _PTR is a pointer that is valid to pass and never dereferenced -- every row below is answered before any launch.
_PTR = object()
_LAMBDA = [("scheme", 0), ("k", 0), ("sigma", 1.0), ("mu", 10.0), ("eps", 1e-10), ("pad", -1.0), ("log_base", 0)]
_RECT = [("B", 2), ("S", 8)]
_TIER = [("offsets", _PTR), ("queries", _PTR), ("n_queries", 2), ("s_max", 8)]
_SIGNATURES = {
    "ltr_reduce_sum_f32": [("in", _PTR), ("n", 4), ("scale", 1.0), ("out", _PTR)],
    "ltr_approxndcg_fwd_bwd": [("scores", _PTR), ("labels", _PTR)] + _RECT + [
        ("alpha", 1.0), ("eps", 1e-10), ("pad", -1.0), ("grad_scale", 1.0), ("slate_loss", _PTR), ("dscores", _PTR)],
    "ltr_listnet_fwd_bwd": [("y_true", _PTR), ("y_pred", _PTR)] + _RECT + [
        ("apply_sigmoid", 0), ("grad_scale", 1.0), ("slate_loss", _PTR), ("dscores", _PTR)],
    "ltr_lambda_fwd_bwd": [("scores", _PTR), ("labels", _PTR)] + _RECT + _LAMBDA + [
        ("grad_scale", 1.0), ("slate_loss", _PTR), ("slate_count", _PTR), ("dscores", _PTR)],
    "ltr_lambda_pairs_fwd": [("scores", _PTR), ("labels", _PTR)] + _RECT + _LAMBDA + [
        ("losses", _PTR), ("keep", _PTR), ("rank", _PTR)],
    "ltr_lambda_pairs_bwd": [("scores", _PTR), ("labels", _PTR)] + _RECT + _LAMBDA + [("grad_losses", _PTR), ("dscores", _PTR)],
    "ltr_lambda_colsum_fwd": [("scores", _PTR), ("labels", _PTR)] + _RECT + _LAMBDA + [("colsum", _PTR)],
    "ltr_lambda_colsum_bwd": [("scores", _PTR), ("labels", _PTR)] + _RECT + _LAMBDA + [("grad_colsum", _PTR), ("dscores", _PTR)],
    "ltr_lambda_colsum_sys_fwd": [("y_pred", _PTR), ("y_true", _PTR), ("y_base", _PTR)] + _RECT + [("n_base", 1)] + _LAMBDA + [
        ("colsum", _PTR)],
    "ltr_lambda_colsum_sys_bwd": [("y_pred", _PTR), ("y_true", _PTR)] + _RECT + _LAMBDA + [("grad_colsum", _PTR), ("dy_pred", _PTR)],
    "ltr_lambda_risk_model_fwd": [("y_pred", _PTR), ("y_true", _PTR), ("cache", _PTR), ("cache_stride", 16), ("n_cached", 1)]
    + _RECT + _LAMBDA + [("lt", 1), ("mat", _PTR), ("jac", _PTR)],
    "ltr_lambda_colsum_sys_bwd_coef": [("y_pred", _PTR), ("y_true", _PTR)] + _RECT + _LAMBDA + [
        ("jac", _PTR), ("coef", _PTR), ("coef_stride", 1), ("dy_pred", _PTR)],
    "ltr_approxndcg_ragged_fwd_bwd": [("scores", _PTR), ("labels", _PTR)] + _TIER + [
        ("alpha", 1.0), ("eps", 1e-10), ("pad", -1.0), ("grad_scale", 1.0), ("slate_loss", _PTR), ("dscores", _PTR)],
    "ltr_listnet_ragged_fwd_bwd": [("y_true", _PTR), ("y_pred", _PTR)] + _TIER + [
        ("apply_sigmoid", 0), ("grad_scale", 1.0), ("slate_loss", _PTR), ("dscores", _PTR)],
    "ltr_lambda_ragged_fwd_bwd": [("scores", _PTR), ("labels", _PTR)] + _TIER + _LAMBDA + [
        ("grad_scale", 1.0), ("slate_loss", _PTR), ("slate_count", _PTR), ("dscores", _PTR)],
    "ltr_lambda_colsum_sys_ragged_fwd": [("y_pred", _PTR), ("y_true", _PTR), ("y_base", _PTR)] + _TIER + [
        ("n_docs", 16), ("n_base", 1)] + _LAMBDA + [("colsum", _PTR)],
    "ltr_lambda_risk_model_ragged_fwd": [("y_pred", _PTR), ("y_true", _PTR), ("cache", _PTR), ("cache_stride", 1),
                                         ("ideal_colsum", _PTR), ("n_cached", 1)] + _TIER + [("n_docs", 16)] + _LAMBDA + [
        ("lt", 1), ("mat", _PTR), ("jac", _PTR)],
    "ltr_lambda_colsum_sys_ragged_bwd_coef": [("y_pred", _PTR), ("y_true", _PTR)] + _TIER + [("n_docs", 16)] + _LAMBDA + [
        ("jac", _PTR), ("coef", _PTR), ("coef_stride", 1), ("dy_pred", _PTR)],
    "ltr_ordinal_fwd_bwd": [("y_pred", _PTR), ("y_true", _PTR), ("n_docs", 8), ("n", 4), ("pad", -1.0),
                            ("block_partials", _PTR), ("sums", _PTR), ("dpred", _PTR)],
}
_SCRATCH = (ctypes.c_char * 64)()


def _call(handle, name, changed):
    sig = _SIGNATURES[name]
    assert set(changed) <= {n for n, _ in sig}, (name, changed)
    args = [changed.get(n, v) for n, v in sig]
    return getattr(handle, name)(*[ctypes.addressof(_SCRATCH) if a is _PTR else a for a in args], None)


# (arguments changed from the valid call, returned code): -1 LTR_ERR_NULL, -2 LTR_ERR_SHAPE, -3 LTR_ERR_PARAM, 0 the zero-size call.
# Per launcher: every required pointer NULL in turn; the batch size -1; the slate length 0 and 2049; the zero-size call; the scalar
# rules that apply to it; then rows that break two rules at once, which pin the order the checks run in.  The codes are those of the
# library before the launchers were rewritten onto one launch layer, recorded as literals.
_CONTRACT = {
    "ltr_reduce_sum_f32": [
        ({"in": None}, -1), ({"out": None}, -1), ({"n": -1}, -2), ({"n": -1, "in": None}, -1),
    ],
    "ltr_approxndcg_fwd_bwd": [
        ({"scores": None}, -1), ({"labels": None}, -1), ({"slate_loss": None}, -1), ({"B": -1}, -2), ({"S": 0}, -2), ({"S": 2049}, -2),
        ({"B": 0}, 0), ({"scores": None, "S": 0}, -1), ({"slate_loss": None, "B": -1}, -1), ({"S": 0, "B": 0}, -2),
    ],
    "ltr_listnet_fwd_bwd": [
        ({"y_true": None}, -1), ({"y_pred": None}, -1), ({"slate_loss": None}, -1), ({"B": -1}, -2), ({"S": 0}, -2), ({"S": 2049}, -2),
        ({"B": 0}, 0), ({"y_true": None, "S": 0}, -1), ({"slate_loss": None, "B": -1}, -1), ({"S": 0, "B": 0}, -2),
    ],
    "ltr_lambda_fwd_bwd": [
        ({"scores": None}, -1), ({"labels": None}, -1), ({"slate_loss": None}, -1), ({"slate_count": None}, -1), ({"B": -1}, -2),
        ({"S": 0}, -2), ({"S": 2049}, -2), ({"B": 0}, 0), ({"scheme": -1}, -3), ({"scheme": 8}, -3), ({"log_base": 2}, -3),
        ({"eps": 0.0}, -3), ({"scores": None, "S": 0}, -1), ({"slate_count": None, "B": -1}, -2), ({"S": 0, "B": 0}, -2),
        ({"S": 2049, "scheme": 8}, -2), ({"slate_count": None, "scheme": 8}, -1), ({"scheme": 8, "B": 0}, -3),
        ({"log_base": 2, "eps": 0.0}, -3), ({"slate_count": None, "eps": 0.0}, -1),
    ],
    "ltr_lambda_pairs_fwd": [
        ({"scores": None}, -1), ({"labels": None}, -1), ({"losses": None}, -1), ({"B": -1}, -2), ({"S": 0}, -2), ({"S": 2049}, -2),
        ({"B": 0}, 0), ({"scheme": -1}, -3), ({"scheme": 8}, -3), ({"log_base": 2}, -3), ({"eps": 0.0}, -3),
        ({"scores": None, "S": 0}, -1), ({"losses": None, "B": -1}, -1), ({"S": 0, "B": 0}, -2), ({"S": 2049, "scheme": 8}, -2),
        ({"losses": None, "scheme": 8}, -1), ({"scheme": 8, "B": 0}, -3), ({"log_base": 2, "eps": 0.0}, -3),
    ],
    "ltr_lambda_pairs_bwd": [
        ({"scores": None}, -1), ({"labels": None}, -1), ({"grad_losses": None}, -1), ({"dscores": None}, -1), ({"B": -1}, -2),
        ({"S": 0}, -2), ({"S": 2049}, -2), ({"B": 0}, 0), ({"scheme": -1}, -3), ({"scheme": 8}, -3), ({"log_base": 2}, -3),
        ({"eps": 0.0}, -3), ({"scores": None, "S": 0}, -1), ({"dscores": None, "B": -1}, -1), ({"S": 0, "B": 0}, -2),
        ({"S": 2049, "scheme": 8}, -2), ({"dscores": None, "scheme": 8}, -1), ({"scheme": 8, "B": 0}, -3),
        ({"log_base": 2, "eps": 0.0}, -3),
    ],
    "ltr_lambda_colsum_fwd": [
        ({"scores": None}, -1), ({"labels": None}, -1), ({"colsum": None}, -1), ({"B": -1}, -2), ({"S": 0}, -2), ({"S": 2049}, -2),
        ({"B": 0}, 0), ({"scheme": -1}, -3), ({"scheme": 8}, -3), ({"log_base": 2}, -3), ({"eps": 0.0}, -3),
        ({"scores": None, "S": 0}, -1), ({"colsum": None, "B": -1}, -1), ({"S": 0, "B": 0}, -2), ({"S": 2049, "scheme": 8}, -2),
        ({"colsum": None, "scheme": 8}, -1), ({"scheme": 8, "B": 0}, -3), ({"log_base": 2, "eps": 0.0}, -3),
    ],
    "ltr_lambda_colsum_bwd": [
        ({"scores": None}, -1), ({"labels": None}, -1), ({"grad_colsum": None}, -1), ({"dscores": None}, -1), ({"B": -1}, -2),
        ({"S": 0}, -2), ({"S": 2049}, -2), ({"B": 0}, 0), ({"scheme": -1}, -3), ({"scheme": 8}, -3), ({"log_base": 2}, -3),
        ({"eps": 0.0}, -3), ({"scores": None, "S": 0}, -1), ({"dscores": None, "B": -1}, -1), ({"S": 0, "B": 0}, -2),
        ({"S": 2049, "scheme": 8}, -2), ({"dscores": None, "scheme": 8}, -1), ({"scheme": 8, "B": 0}, -3),
        ({"log_base": 2, "eps": 0.0}, -3),
    ],
    "ltr_lambda_colsum_sys_fwd": [
        ({"y_pred": None}, -1), ({"y_true": None}, -1), ({"colsum": None}, -1), ({"B": -1}, -2), ({"S": 0}, -2), ({"S": 2049}, -2),
        ({"B": 0}, 0), ({"scheme": -1}, -3), ({"scheme": 8}, -3), ({"log_base": 2}, -3), ({"eps": 0.0}, -3), ({"n_base": -1}, -2),
        ({"n_base": 4097}, -2), ({"y_base": None}, -1), ({"n_base": 0, "y_base": None, "B": 0}, 0), ({"y_pred": None, "S": 0}, -1),
        ({"colsum": None, "B": -1}, -1), ({"S": 0, "B": 0}, -2), ({"S": 2049, "scheme": 8}, -2), ({"colsum": None, "scheme": 8}, -1),
        ({"scheme": 8, "B": 0}, -3), ({"log_base": 2, "eps": 0.0}, -3), ({"n_base": 4097, "y_base": None}, -1),
        ({"n_base": -1, "eps": 0.0}, -2), ({"y_base": None, "S": 0}, -2),
    ],
    "ltr_lambda_colsum_sys_bwd": [
        ({"y_pred": None}, -1), ({"y_true": None}, -1), ({"grad_colsum": None}, -1), ({"dy_pred": None}, -1), ({"B": -1}, -2),
        ({"S": 0}, -2), ({"S": 2049}, -2), ({"B": 0}, 0), ({"scheme": -1}, -3), ({"scheme": 8}, -3), ({"log_base": 2}, -3),
        ({"eps": 0.0}, -3), ({"y_pred": None, "S": 0}, -1), ({"dy_pred": None, "B": -1}, -1), ({"S": 0, "B": 0}, -2),
        ({"S": 2049, "scheme": 8}, -2), ({"dy_pred": None, "scheme": 8}, -1), ({"scheme": 8, "B": 0}, -3),
        ({"log_base": 2, "eps": 0.0}, -3),
    ],
    "ltr_lambda_risk_model_fwd": [
        ({"y_pred": None}, -1), ({"y_true": None}, -1), ({"cache": None}, -1), ({"mat": None}, -1), ({"jac": None}, -1),
        ({"B": -1}, -2), ({"S": 0}, -2), ({"S": 2049}, -2), ({"B": 0}, 0), ({"scheme": -1}, -3), ({"scheme": 8}, -3),
        ({"log_base": 2}, -3), ({"eps": 0.0}, -3), ({"lt": 0}, -3), ({"lt": 4}, -3), ({"n_cached": -1}, -2), ({"n_cached": 66}, -2),
        ({"S": 1}, -2), ({"cache_stride": 0}, -2), ({"y_pred": None, "S": 0}, -1), ({"jac": None, "B": -1}, -2), ({"S": 0, "B": 0}, -2),
        ({"S": 2049, "scheme": 8}, -2), ({"jac": None, "scheme": 8}, -1), ({"scheme": 8, "B": 0}, -3),
        ({"log_base": 2, "eps": 0.0}, -3), ({"lt": 0, "scheme": -1}, -3), ({"lt": 4, "n_cached": 66}, -2), ({"lt": 0, "jac": None}, -1),
    ],
    "ltr_lambda_colsum_sys_bwd_coef": [
        ({"y_pred": None}, -1), ({"y_true": None}, -1), ({"jac": None}, -1), ({"coef": None}, -1), ({"dy_pred": None}, -1),
        ({"B": -1}, -2), ({"S": 0}, -2), ({"S": 2049}, -2), ({"B": 0}, 0), ({"scheme": -1}, -3), ({"scheme": 8}, -3),
        ({"log_base": 2}, -3), ({"eps": 0.0}, -3), ({"coef_stride": 0}, -2), ({"y_pred": None, "S": 0}, -1),
        ({"dy_pred": None, "B": -1}, -1), ({"S": 0, "B": 0}, -2), ({"S": 2049, "scheme": 8}, -2), ({"dy_pred": None, "scheme": 8}, -1),
        ({"scheme": 8, "B": 0}, -3), ({"log_base": 2, "eps": 0.0}, -3), ({"coef_stride": 0, "coef": None}, -1),
        ({"coef_stride": 0, "log_base": 2}, -2),
    ],
    "ltr_approxndcg_ragged_fwd_bwd": [
        ({"scores": None}, -1), ({"labels": None}, -1), ({"offsets": None}, -1), ({"slate_loss": None}, -1), ({"n_queries": -1}, -2),
        ({"s_max": 0}, -2), ({"s_max": 2049}, -2), ({"n_queries": 0}, 0), ({"scores": None, "s_max": 0}, -1),
        ({"slate_loss": None, "n_queries": -1}, -1), ({"s_max": 0, "n_queries": 0}, -2),
    ],
    "ltr_listnet_ragged_fwd_bwd": [
        ({"y_true": None}, -1), ({"y_pred": None}, -1), ({"offsets": None}, -1), ({"slate_loss": None}, -1), ({"n_queries": -1}, -2),
        ({"s_max": 0}, -2), ({"s_max": 2049}, -2), ({"n_queries": 0}, 0), ({"y_true": None, "s_max": 0}, -1),
        ({"slate_loss": None, "n_queries": -1}, -1), ({"s_max": 0, "n_queries": 0}, -2),
    ],
    "ltr_lambda_ragged_fwd_bwd": [
        ({"scores": None}, -1), ({"labels": None}, -1), ({"offsets": None}, -1), ({"slate_loss": None}, -1),
        ({"slate_count": None}, -1), ({"n_queries": -1}, -2), ({"s_max": 0}, -2), ({"s_max": 2049}, -2), ({"n_queries": 0}, 0),
        ({"scheme": -1}, -3), ({"scheme": 8}, -3), ({"log_base": 2}, -3), ({"eps": 0.0}, -3), ({"scores": None, "s_max": 0}, -1),
        ({"slate_count": None, "n_queries": -1}, -2), ({"s_max": 0, "n_queries": 0}, -2), ({"s_max": 2049, "scheme": 8}, -2),
        ({"slate_count": None, "scheme": 8}, -1), ({"scheme": 8, "n_queries": 0}, -3), ({"log_base": 2, "eps": 0.0}, -3),
        ({"slate_count": None, "eps": 0.0}, -1),
    ],
    "ltr_lambda_colsum_sys_ragged_fwd": [
        ({"y_pred": None}, -1), ({"y_true": None}, -1), ({"offsets": None}, -1), ({"colsum": None}, -1), ({"n_queries": -1}, -2),
        ({"s_max": 0}, -2), ({"s_max": 2049}, -2), ({"n_queries": 0}, 0), ({"scheme": -1}, -3), ({"scheme": 8}, -3),
        ({"log_base": 2}, -3), ({"eps": 0.0}, -3), ({"n_base": -1}, -2), ({"n_base": 4097}, -2), ({"y_base": None}, -1),
        ({"n_base": 0, "y_base": None, "n_queries": 0}, 0), ({"n_docs": -1}, -2), ({"y_pred": None, "s_max": 0}, -1),
        ({"colsum": None, "n_queries": -1}, -1), ({"s_max": 0, "n_queries": 0}, -2), ({"s_max": 2049, "scheme": 8}, -2),
        ({"colsum": None, "scheme": 8}, -1), ({"scheme": 8, "n_queries": 0}, -3), ({"log_base": 2, "eps": 0.0}, -3),
        ({"n_base": 4097, "y_base": None}, -1), ({"n_base": -1, "eps": 0.0}, -2), ({"y_base": None, "s_max": 0}, -2),
        ({"y_base": None, "n_docs": -1}, -1),
    ],
    "ltr_lambda_risk_model_ragged_fwd": [
        ({"y_pred": None}, -1), ({"y_true": None}, -1), ({"cache": None}, -1), ({"ideal_colsum": None}, -1), ({"offsets": None}, -1),
        ({"mat": None}, -1), ({"jac": None}, -1), ({"n_queries": -1}, -2), ({"s_max": 0}, -2), ({"s_max": 2049}, -2),
        ({"n_queries": 0}, 0), ({"scheme": -1}, -3), ({"scheme": 8}, -3), ({"log_base": 2}, -3), ({"eps": 0.0}, -3), ({"lt": 0}, -3),
        ({"lt": 4}, -3), ({"n_cached": -1}, -2), ({"n_cached": 66}, -2), ({"s_max": 1}, -2), ({"cache_stride": 0}, -2),
        ({"n_docs": -1}, -2), ({"y_pred": None, "s_max": 0}, -1), ({"jac": None, "n_queries": -1}, -2),
        ({"s_max": 0, "n_queries": 0}, -2), ({"s_max": 2049, "scheme": 8}, -2), ({"jac": None, "scheme": 8}, -1),
        ({"scheme": 8, "n_queries": 0}, -3), ({"log_base": 2, "eps": 0.0}, -3), ({"lt": 0, "scheme": -1}, -3),
        ({"lt": 4, "n_cached": 66}, -2), ({"lt": 0, "jac": None}, -1),
    ],
    "ltr_lambda_colsum_sys_ragged_bwd_coef": [
        ({"y_pred": None}, -1), ({"y_true": None}, -1), ({"offsets": None}, -1), ({"jac": None}, -1), ({"coef": None}, -1),
        ({"dy_pred": None}, -1), ({"n_queries": -1}, -2), ({"s_max": 0}, -2), ({"s_max": 2049}, -2), ({"n_queries": 0}, 0),
        ({"scheme": -1}, -3), ({"scheme": 8}, -3), ({"log_base": 2}, -3), ({"eps": 0.0}, -3), ({"coef_stride": 0}, -2),
        ({"n_docs": -1}, -2), ({"y_pred": None, "s_max": 0}, -1), ({"dy_pred": None, "n_queries": -1}, -1),
        ({"s_max": 0, "n_queries": 0}, -2), ({"s_max": 2049, "scheme": 8}, -2), ({"dy_pred": None, "scheme": 8}, -1),
        ({"scheme": 8, "n_queries": 0}, -3), ({"log_base": 2, "eps": 0.0}, -3), ({"coef_stride": 0, "coef": None}, -1),
        ({"coef_stride": 0, "log_base": 2}, -2),
    ],
    "ltr_ordinal_fwd_bwd": [
        ({"y_pred": None}, -1), ({"y_true": None}, -1), ({"block_partials": None}, -1), ({"sums": None}, -1), ({"n_docs": -1}, -2),
        ({"n": 0}, -2), ({"n": 65}, -2), ({"n": 0, "sums": None}, -1), ({"n_docs": -1, "n": 65}, -2),
    ],
}


@pytest.mark.parametrize("name", sorted(_CONTRACT))
def test_loss_launchers_answer_before_any_launch(handle, name):
    assert set(_CONTRACT) == set(_SIGNATURES)
    for changed, code in _CONTRACT[name]:
        assert _call(handle, name, changed) == code, (name, changed)


def test_cpu_tensors_are_refused():
    from ltr_mi355x import LtrDeviceError
    from losses.approxNDCG import approxNDCGLoss
    from losses.listnet import listnetLoss
    from losses.lambdaL import lambdaLoss
    from losses.ordinal import ordinalLoss
    s, y = torch.randn(2, 8), torch.randint(0, 5, (2, 8)).float()
    for call in (lambda: approxNDCGLoss(s, y), lambda: listnetLoss(y, s), lambda: lambdaLoss(s, y),
                 lambda: ordinalLoss(torch.rand(2, 8, 4), y, 4)):
        with pytest.raises(LtrDeviceError):
            call()


def test_host_argument_contract():
    from ltr_mi355x.functional import SCHEME_IDS, _lambda_args, slate_2d
    with pytest.raises(ValueError, match="Reduction logarithm base can be either natural or binary"):
        _lambda_args(1e-10, -1, None, None, 1.0, 10.0, "decimal")
    with pytest.raises(KeyError):
        _lambda_args(1e-10, -1, "nope_scheme", None, 1.0, 10.0, "binary")
    assert _lambda_args(1e-10, -1, "lamdbaRank_scheme", 7, 1.0, 10.0, "natural")[:2] == (3, 7)
    assert len(SCHEME_IDS) == 8
    assert slate_2d(torch.zeros(3, 5, 1), "x").shape == (3, 5)
    with pytest.raises(ValueError):
        slate_2d(torch.zeros(3), "x")


def test_scorer_modules_construct_on_cpu():
    """state_dict keys/shapes of SURVEY 3.3 for the compiled input sizes; other sizes refuse loudly."""
    from architeture.doubleLayer import DoubleLayerNet
    from architeture.tripleLayer import TripleLayerNet
    for F in (136, 64):
        d, t = DoubleLayerNet(F), TripleLayerNet(F)
        assert {k: tuple(v.shape) for k, v in d.state_dict().items()} == {
            "fc1.weight": (F, F), "fc1.bias": (F,), "fc2.weight": (F, F), "fc2.bias": (F,), "fc3.weight": (1, F), "fc3.bias": (1,)}
        assert {k: tuple(v.shape) for k, v in t.state_dict().items()} == {
            "l1.weight": (64, F), "l1.bias": (64,), "l2.weight": (32, 64), "l2.bias": (32,), "l3.weight": (1, 32), "l3.bias": (1,)}
        assert isinstance(d.dropout, torch.nn.Dropout) and d.dropout.p == 0.5
    d = DoubleLayerNet(100)                       # any input size up to 136 runs zero-padded on a compiled geometry
    assert tuple(d.fc2.weight.shape) == (100, 100) and tuple(TripleLayerNet(46).l1.weight.shape) == (64, 46)
    w = DoubleLayerNet(220)                       # wider than the fused kernels' tile: library-GEMM path (scorer.wide_forward), still device-only
    assert tuple(w.fc1.weight.shape) == (220, 220) and tuple(TripleLayerNet(300).l1.weight.shape) == (64, 300)
    from ltr_mi355x import LtrDeviceError
    with pytest.raises(LtrDeviceError):
        TripleLayerNet(136)(torch.zeros(2, 4, 136), None, None)
    with pytest.raises(LtrDeviceError):
        w(torch.zeros(2, 4, 220), None, None)     # no CPU path for the wide networks either


def test_module_surface_matches_reference():
    """Names/signatures of SURVEY.md section 8(b)."""
    import inspect
    import losses
    from losses import approxNDCG, lambdaL, listnet, ordinal
    assert hasattr(losses, "approxNDCG") and hasattr(losses, "lambdaL")
    sig = inspect.signature
    assert list(sig(approxNDCG.approxNDCGLoss).parameters) == ["y_pred", "y_true", "eps", "padded_value_indicator", "alpha"]
    assert list(sig(listnet.listnetLoss).parameters) == ["y_true", "y_predicted", "apply_sigmoid"]
    assert list(sig(lambdaL.lambdaLoss).parameters) == ["y_pred", "y_true", "eps", "padded_value_indicator",
                                                         "weighing_scheme", "k", "sigma", "mu", "reduction", "reduction_log"]
    assert list(sig(lambdaL.lambdaMask).parameters)[-1] == "return_losses"
    for n in ("ndcgLoss1_scheme", "ndcgLoss2_scheme", "lamdbaRank_scheme", "ndcgLoss2PP_scheme", "rankNet_scheme",
              "rankNetWeightedByGTDiff_scheme", "rankNetWeightedByGTDiffPowed_scheme"):
        assert callable(getattr(lambdaL, n))
    assert ordinal.PADDED_Y_VALUE == -1
    assert list(sig(ordinal.ordinalLoss).parameters) == ["y_pred", "y_true", "n", "padded_value_indicator"]
    y = torch.tensor([[0., 2., -1.]])
    assert ordinal.with_ordinals(y, 2).tolist() == [[[0., 0.], [1., 1.], [-1., -1.]]]
