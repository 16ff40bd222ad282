"""Prototypes of the scorer / fused-step entry points (include/ltr_mi355x.h, second half)."""
from ctypes import c_float, c_int, c_int64, c_uint64, c_void_p

P = c_void_p
PROTOTYPES = {
    "ltr_net_info": (c_int, [c_int, P]),
    "ltr_fused_grid": (c_int, [c_int, c_int]),
    "ltr_mlp_pack": (c_int, [c_int, P, P, P, P, P, P, P, P]),
    "ltr_mlp_pack_sub": (c_int, [c_int, c_int, c_int, c_int, P, P, P, P, P, P, P, P]),
    "ltr_mlp_reduce_grads_sub": (c_int, [c_int, c_int, c_int, c_int, P, c_int, P, P]),
    "ltr_dropout_keep_mask": (c_int, [c_uint64, c_int, c_int64, c_int, P, P]),
    "ltr_dropout_keep_mask_p": (c_int, [c_uint64, c_int, c_int64, c_int, c_float, P, P]),
    "ltr_mlp_forward": (c_int, [c_int, P, c_int64, P, c_int, c_uint64, P, P, P, c_int, P]),
    "ltr_mlp_backward": (c_int, [c_int, P, c_int64, P, c_int, c_uint64, P, P, P, P, c_int, P]),
    "ltr_mlp_reduce_grads": (c_int, [c_int, P, c_int, P, P]),
    "ltr_mlp_acts_floats": (c_int64, [c_int, c_int64]),
    "ltr_mlp_forward_save": (c_int, [c_int, P, c_int64, P, c_int, c_uint64, P, P, P, P, c_int, P]),
    "ltr_mlp_backward_saved": (c_int, [c_int, P, c_int64, P, c_int, P, P, P, c_int, P]),
    "ltr_fused_step": (c_int, [c_int, c_int, P, P, c_int, c_int, P, c_int, c_uint64, P, P, c_float, c_float, c_float,
                               c_int, c_float, P, P, c_int, P]),
    "ltr_triple_fold": (c_int, [P, P, P, P, P, c_int, c_int, P, P, P, P]),
    "ltr_triple_unfold_grads": (c_int, [P, c_int, c_int, P, P, P, P, P]),
    "ltr_debug_set_stamps": (c_int, [P, c_int]),
    "ltr_fused_step_lambda": (c_int, [c_int, P, P, c_int, c_int, P, c_int, c_uint64, P, P, c_int, c_int, c_float, c_float,
                                      c_float, c_float, c_int, c_float, P, P, P, c_int, P]),
    # FC-only make_model rankers (csrc/ltr_linear.hip)
    "ltr_linear_ws_doubles": (c_int64, [c_int, c_int, P]),
    "ltr_linear_fold": (c_int, [c_int, c_int, P, c_int, P, P, P, P]),
    "ltr_linear_unfold_grads": (c_int, [c_int, c_int, P, c_int, P, P, c_int, P, P, P]),
    "ltr_linear_scores": (c_int, [P, c_int64, c_int, P, c_int, P, P, P]),
    "ltr_linear_grad_partials": (c_int, [P, c_int64, c_int, P, P, c_int, P, c_int, P]),
    "ltr_linear_fused_supported": (c_int, [c_int, c_int]),
    "ltr_linear_fused_step": (c_int, [c_int, P, P, c_int, c_int, c_int, P, c_int, c_float, c_float, c_float, c_int, c_int, c_int,
                                      c_float, c_float, c_float, c_int, c_float, P, P, P, c_int, P]),
    "ltr_linear_risk_rows": (c_int, [P, P, c_int, c_int, c_int, P, c_int, c_int, c_int, P, c_int, c_int, P, c_int, P, c_int, P]),
    "ltr_linear_risk_combine": (c_int, [P, P, c_int, c_int, c_int, P, c_int, P]),
    "ltr_linear_grid": (c_int, [c_int]),
    # FC scorers with 137 .. 1024 input features (csrc/ltr_wide.hip)
    "ltr_gemm_f32": (c_int, [P, P]),
    "ltr_colsum_f32": (c_int, [P, c_int64, c_int, c_int64, P, P, c_int, P]),
    "ltr_wide_acts_floats": (c_int64, [c_int, c_int, c_int, c_int, c_int64]),
    "ltr_wide_ws_floats": (c_int64, [c_int, c_int, c_int, c_int, c_int64, c_int]),
    "ltr_wide_forward_save": (c_int, [c_int, c_int, c_int, c_int, P, c_int64, P, c_int, c_uint64, P, P, P, P, P]),
    "ltr_wide_backward_saved": (c_int, [c_int, c_int, c_int, c_int, P, c_int64, P, c_int, P, P, P, c_int, P, P]),
}


def bind(h):
    for name, (res, args) in PROTOTYPES.items():
        try:
            fn = getattr(h, name)
        except AttributeError as e:
            from ._lib import LtrBuildError
            raise LtrBuildError(f"library does not export {name}: stale build?") from e
        fn.restype = res
        fn.argtypes = args
