"""ctypes binding of include/gnf_hip.h (libgnf_hip.so).

PyTorch is used only as the owner of device memory and streams: every entry point
receives raw `data_ptr()`s, element strides and torch's current HIP stream.  There is
NO CPU fallback: a missing library or a non-HIP tensor raises."""
import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libgnf_hip.so")

c_f = ctypes.c_void_p            # device float*
c_i64 = ctypes.c_int64
c_int = ctypes.c_int
c_float = ctypes.c_float
c_double = ctypes.c_double
c_u64 = ctypes.c_uint64
c_stream = ctypes.c_void_p

MONO_MAX_LAYERS = 8
MADE_MAX_HIDDEN = 8       # GNF_MADE_MAX_HIDDEN
MADE_NORM_NONE, MADE_NORM_AFFINE = 0, 1
MADE_NORM_SPLINE = 2      # GNF_MADE_NORM_SPLINE: gnf_made_prefix_spline / gnf_made_prefix_ctx_spline only
SPLINE_MIN_BINS, SPLINE_MAX_BINS = 2, 32
SPLINE_FWD, SPLINE_BWD, SPLINE_INV = 0, 1, 2      # `which` of gnf_spline_route
STRADE_CHUNK_VARS = 8     # GNF_STRADE_CHUNK_VARS: variables per output product of gnf_strade_levels
DAG_PLAN_KC = 32          # GNF_DAG_PLAN_KC
DAG_ELEM_F32, DAG_ELEM_U8 = 0, 1      # GNF_DAG_ELEM_*
ABI_VERSION = 11          # GNF_ABI_VERSION of include/gnf_hip.h this binding was written against


class MonoNet(ctypes.Structure):
    """gnf_mono_net (include/gnf_hip.h)."""
    _fields_ = [("nl", c_int), ("dims", c_int * (MONO_MAX_LAYERS + 1)),
                ("W", ctypes.c_void_p * MONO_MAX_LAYERS), ("b", ctypes.c_void_p * MONO_MAX_LAYERS)]


class MadeNet(ctypes.Structure):
    """gnf_made_net (include/gnf_hip.h)."""
    _fields_ = [("nh", c_int), ("d", c_int), ("out", c_int), ("max_new", c_int), ("width", c_int * MADE_MAX_HIDDEN),
                ("W", ctypes.c_void_p * (MADE_MAX_HIDDEN + 1)), ("b", ctypes.c_void_p * (MADE_MAX_HIDDEN + 1)),
                ("order", ctypes.c_void_p * MADE_MAX_HIDDEN), ("off", ctypes.c_void_p * MADE_MAX_HIDDEN),
                ("var_of_step", ctypes.c_void_p)]


class StradeNet(ctypes.Structure):
    """gnf_strade_net (include/gnf_hip.h): a gnf_made_net whose tables are read by level, the masks, the level offsets."""
    _fields_ = [("made", MadeNet), ("mask", ctypes.c_void_p * (MADE_MAX_HIDDEN + 1)), ("var_off", ctypes.c_void_p),
                ("nlev", c_int), ("widest", c_int)]


# name -> (restype, argtypes); must list every symbol include/gnf_hip.h declares
SIGNATURES = {
    "gnf_abi_version": (c_int, []),
    "gnf_affine_fwd": (c_int, [c_f, c_f, c_i64, c_i64, c_i64, c_f, c_f, c_f, c_f, c_int, c_i64, c_i64, c_stream]),
    "gnf_affine_bwd": (c_int, [c_f, c_f, c_i64, c_i64, c_i64, c_f, c_f, c_f, c_f, c_f, c_f, c_i64, c_i64, c_i64, c_i64,
                               c_i64, c_stream]),
    "gnf_affine_inv": (c_int, [c_f, c_f, c_i64, c_i64, c_i64, c_f, c_i64, c_i64, c_stream]),
    "gnf_spline_fwd": (c_int, [c_f, c_f, c_i64, c_i64, c_i64, c_i64, c_int, c_double, c_f, c_f, c_f, c_f, c_i64, c_i64,
                               c_stream]),
    "gnf_spline_bwd": (c_int, [c_f, c_f, c_i64, c_i64, c_i64, c_i64, c_int, c_double, c_f, c_f, c_f, c_f, c_f, c_f, c_i64,
                               c_i64, c_i64, c_i64, c_i64, c_stream]),
    "gnf_spline_inv": (c_int, [c_f, c_f, c_i64, c_i64, c_i64, c_i64, c_int, c_double, c_f, ctypes.c_void_p, c_i64, c_i64,
                               c_i64, c_stream]),
    "gnf_spline_route": (c_int, [c_int, ctypes.c_void_p, c_i64, c_i64, c_i64, c_i64, c_int, c_i64, c_i64, ctypes.c_void_p,
                                 c_i64, c_i64, c_i64, c_int, ctypes.c_char_p, c_int]),
    "gnf_logsum_rows_fwd": (c_int, [c_f, c_f, c_i64, c_i64, c_stream]),
    "gnf_logsum_rows_bwd": (c_int, [c_f, c_f, c_f, c_i64, c_i64, c_stream]),
    "gnf_normal_logdensity_fwd": (c_int, [c_f, c_f, c_i64, c_i64, c_stream]),
    "gnf_normal_logdensity_bwd": (c_int, [c_f, c_f, c_f, c_i64, c_i64, c_stream]),
    "gnf_nll_reduce_fwd": (c_int, [c_f, c_f, c_f, c_f, c_i64, c_i64, c_stream]),
    "gnf_nll_reduce_bwd": (c_int, [c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_i64, c_i64, c_stream]),
    # (pin: uint8 [R, d], regime: int32 [B] or NULL -- device pointers of any dtype, ops passes them through rawptr)
    "gnf_nll_do_fwd": (c_int, [c_f, c_f, ctypes.c_void_p, ctypes.c_void_p, c_i64, c_f, c_f, c_i64, c_i64, c_stream]),
    "gnf_nll_do_bwd": (c_int, [c_f, c_f, ctypes.c_void_p, ctypes.c_void_p, c_i64, c_f, c_f, c_f, c_f, c_f, c_i64, c_i64,
                               c_stream]),
    "gnf_affine_do_fwd": (c_int, [c_f, c_f, c_i64, c_i64, c_i64, ctypes.c_void_p, ctypes.c_void_p, c_i64, c_f, c_f, c_f, c_f,
                                  c_i64, c_i64, c_stream]),
    "gnf_affine_do_bwd": (c_int, [c_f, c_f, c_i64, c_i64, c_i64, ctypes.c_void_p, ctypes.c_void_p, c_i64, c_f, c_f, c_f, c_f,
                                  c_f, c_f, c_i64, c_i64, c_i64, c_i64, c_i64, c_stream]),
    "gnf_nll_mean_fwd": (c_int, [c_f, c_f, c_f, c_f, c_i64, c_stream]),
    "gnf_nll_mean_bwd": (c_int, [c_f, c_f, c_f, c_i64, c_stream]),
    "gnf_nll_loss_max_elems": (c_i64, []),
    "gnf_nll_loss_fwd": (c_int, [c_f, c_f, c_f, c_f, c_i64, c_i64, c_stream]),
    "gnf_nll_loss_bwd": (c_int, [c_f, c_f, c_f, c_f, c_i64, c_i64, c_stream]),
    "gnf_colsum_ws_bytes": (c_i64, [c_i64, c_i64]),
    "gnf_colsum": (c_int, [c_f, c_i64, c_f, c_i64, c_i64, c_f, c_stream]),
    "gnf_linear_ws_bytes": (c_i64, [c_i64, c_i64, c_i64]),
    "gnf_linear_fwd": (c_int, [c_f, c_f, c_f, c_f, c_f, c_f, c_int, c_int, c_f, c_i64, c_i64, c_i64, c_f, c_i64, c_stream]),
    "gnf_linear_bwd_x": (c_int, [c_f, c_f, c_f, c_f, c_f, c_int, c_f, c_f, c_i64, c_i64, c_i64, c_f, c_i64, c_stream]),
    "gnf_linear_bwd_w": (c_int, [c_f, c_f, c_f, c_f, c_f, c_int, c_f, c_f, c_i64, c_i64, c_i64, c_f, c_i64, c_stream]),
    "gnf_linear_bwd": (c_int, [c_f, c_f, c_f, c_f, c_f, c_f, c_int, c_f, c_f, c_f, c_f, c_f, c_i64, c_i64, c_i64, c_f, c_i64,
                               c_stream]),
    "gnf_linear_gxsum_fused": (c_int, [c_i64, c_i64, c_i64, c_int]),
    "gnf_gemm_last_kernel": (ctypes.c_char_p, []),
    "gnf_gemm_ws_bytes": (c_i64, [c_i64, c_i64, c_i64]),
    "gnf_gemm_f32_ws_bytes": (c_i64, [c_i64, c_i64, c_i64]),
    "gnf_gemm": (c_int, [c_f, c_i64, c_i64, c_f, c_f, c_i64, c_i64, c_f, c_i64, c_i64, c_f, c_f, c_i64, c_i64, c_f,
                         c_i64, c_i64, c_int, c_i64, c_i64, c_i64, c_f, c_i64, c_stream]),
    "gnf_gemm_split_ws_bytes": (c_i64, [c_i64, c_i64, c_i64]),
    "gnf_gemm_split_last_kernel": (ctypes.c_char_p, []),
    "gnf_gemm_split_enabled": (c_int, []),
    "gnf_gemm_split_bf16": (c_int, [c_f, c_i64, c_i64, c_f, c_i64, c_i64, c_f, c_i64, c_i64, c_f, c_int, c_i64, c_i64, c_i64,
                                    c_int, c_int, c_i64, ctypes.c_void_p, c_i64, c_stream]),
    "gnf_dag_gate_fwd_ws_bytes": (c_i64, [c_i64]),
    "gnf_dag_gate_fwd": (c_int, [c_f, c_f, c_f, c_i64, c_int, c_int, c_float, c_float, c_f, c_f, c_u64, c_u64, c_int,
                                 c_f, c_i64, c_i64, c_stream]),
    "gnf_dag_gate_bwd_ws_bytes": (c_i64, [c_i64, c_i64]),
    "gnf_dag_gate_bwd": (c_int, [c_f, c_f, c_f, c_i64, c_int, c_int, c_float, c_float, c_f, c_f, c_u64, c_u64, c_f, c_f,
                                 c_f, c_f, c_i64, c_i64, c_stream]),
    "gnf_dag_gate_plan_bytes": (c_i64, [c_i64]),
    "gnf_dag_gate_fwd_plan": (c_int, [c_f, c_f, c_f, c_i64, c_int, c_int, c_float, c_float, c_f, c_f, c_u64, c_u64, c_int,
                                      c_f, ctypes.c_void_p, c_i64, c_i64, c_i64, c_stream]),
    "gnf_dag_gate_bwd_cols_ws_bytes": (c_i64, [c_i64, c_i64]),
    "gnf_dag_gate_bwd_cols": (c_int, [c_f, c_f, c_f, ctypes.c_void_p, c_int, c_int, c_float, c_f, c_f, c_u64, c_u64, c_f,
                                      c_f, c_int, c_f, c_i64, c_i64, c_stream]),
    "gnf_monotonic_pack_floats": (c_i64, [ctypes.POINTER(MonoNet)]),
    "gnf_monotonic_pack": (c_int, [ctypes.POINTER(MonoNet), c_f, c_stream]),
    "gnf_monotonic_fwd": (c_int, [c_f, ctypes.POINTER(MonoNet), c_f, c_f, c_i64, c_i64, c_i64, c_f, c_f, c_int, c_f,
                                  c_f, c_i64, c_i64, c_stream]),
    "gnf_monotonic_fwd_f32": (c_int, [c_f, ctypes.POINTER(MonoNet), c_f, c_f, c_i64, c_i64, c_i64, c_f, c_f, c_int, c_f,
                                      c_f, c_i64, c_i64, c_stream]),
    "gnf_monotonic_fwd_kernel": (ctypes.c_char_p, []),
    "gnf_monotonic_inv": (c_int, [c_f, ctypes.POINTER(MonoNet), c_f, c_f, c_i64, c_i64, c_i64, c_f, c_f, c_int, c_f,
                                  c_i64, c_i64, c_stream]),
    "gnf_monotonic_inv_scatter": (c_int, [c_f, ctypes.POINTER(MonoNet), c_f, c_f, c_i64, c_i64, c_i64, c_f, c_f, c_int, c_f,
                                          ctypes.c_void_p, c_i64, c_i64, c_i64, c_stream]),
    "gnf_monotonic_inv_route": (c_int, [ctypes.POINTER(MonoNet), c_int, c_i64, c_i64, ctypes.c_char_p, c_int]),
    "gnf_monotonic_inv_kernel": (ctypes.c_char_p, []),
    "gnf_monotonic_bwd_ws_bytes": (c_i64, [ctypes.POINTER(MonoNet), c_int, c_i64, c_i64]),
    "gnf_monotonic_bwd": (c_int, [c_f, ctypes.POINTER(MonoNet), c_f, c_f, c_i64, c_i64, c_i64, c_f, c_f, c_int, c_f,
                                  c_f, c_f, c_f, c_i64, c_i64, c_i64, ctypes.POINTER(ctypes.c_void_p),
                                  ctypes.POINTER(ctypes.c_void_p), ctypes.c_void_p, c_i64, c_i64, c_i64, c_stream]),
    "gnf_monotonic_bwd_f32": (c_int, [c_f, ctypes.POINTER(MonoNet), c_f, c_f, c_i64, c_i64, c_i64, c_f, c_f, c_int, c_f,
                                      c_f, c_f, c_f, c_i64, c_i64, c_i64, ctypes.POINTER(ctypes.c_void_p),
                                      ctypes.POINTER(ctypes.c_void_p), ctypes.c_void_p, c_i64, c_i64, c_i64, c_stream]),
    "gnf_monotonic_bwd_kernel": (ctypes.c_char_p, []),
    "gnf_made_prefix_pack_floats": (c_i64, [ctypes.POINTER(MadeNet)]),
    "gnf_made_prefix_pack": (c_int, [ctypes.POINTER(MadeNet), c_f, c_stream]),
    "gnf_made_prefix_ws_bytes": (c_i64, [ctypes.POINTER(MadeNet), c_i64]),
    "gnf_made_prefix": (c_int, [ctypes.POINTER(MadeNet), c_f, c_f, c_f, c_f, c_int, c_int, c_int, c_i64, ctypes.c_void_p,
                                c_i64, c_stream]),
    "gnf_made_prefix_ctx_pack_floats": (c_i64, [ctypes.POINTER(MadeNet), c_int]),
    "gnf_made_prefix_ctx_pack": (c_int, [ctypes.POINTER(MadeNet), c_int, c_f, c_stream]),
    "gnf_made_prefix_ctx_ws_bytes": (c_i64, [ctypes.POINTER(MadeNet), c_int, c_i64]),
    "gnf_made_prefix_ctx": (c_int, [ctypes.POINTER(MadeNet), c_int, c_f, c_f, c_f, c_f, c_f, c_int, c_int, c_int, c_i64,
                                    ctypes.c_void_p, c_i64, c_stream]),
    "gnf_made_prefix_spline": (c_int, [ctypes.POINTER(MadeNet), c_f, c_f, c_f, c_f, c_int, c_int, c_int, c_int, c_double,
                                       c_i64, ctypes.c_void_p, c_i64, c_stream]),
    "gnf_made_prefix_ctx_spline": (c_int, [ctypes.POINTER(MadeNet), c_int, c_f, c_f, c_f, c_f, c_f, c_int, c_int, c_int,
                                           c_int, c_double, c_i64, ctypes.c_void_p, c_i64, c_stream]),
    "gnf_made_prefix_do": (c_int, [ctypes.POINTER(MadeNet), c_int, c_f, c_f, c_f, c_f, c_f, c_int, c_int, c_int, c_int,
                                   c_double, ctypes.c_void_p, c_i64, ctypes.c_void_p, c_i64, c_stream]),
    "gnf_strade_pack_floats": (c_i64, [ctypes.POINTER(StradeNet), c_int]),
    "gnf_strade_pack": (c_int, [ctypes.POINTER(StradeNet), c_int, c_f, c_stream]),
    "gnf_strade_levels": (c_int, [ctypes.POINTER(StradeNet), c_int, c_f, c_f, c_f, c_f, c_int, c_int, c_double,
                                  ctypes.c_void_p, c_i64, c_stream]),
    "gnf_made_adjoint_pack_floats": (c_i64, [ctypes.POINTER(MadeNet), c_int]),
    "gnf_made_adjoint_pack": (c_int, [ctypes.POINTER(MadeNet), c_int, c_f, c_stream]),
    "gnf_made_adjoint_ws_bytes": (c_i64, [ctypes.POINTER(MadeNet), c_int, c_i64]),
    "gnf_made_adjoint": (c_int, [ctypes.POINTER(MadeNet), c_int, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_i64, c_int,
                                 ctypes.c_void_p, c_i64, c_stream]),
    "gnf_made_adjoint_do": (c_int, [ctypes.POINTER(MadeNet), c_int, c_f, c_f, c_f, c_f, c_f, c_f, c_f, ctypes.c_void_p, c_f,
                                    c_i64, c_int, ctypes.c_void_p, c_i64, c_stream]),
    "gnf_strade_adjoint_pack_floats": (c_i64, [ctypes.POINTER(StradeNet), c_int]),
    "gnf_strade_adjoint_pack": (c_int, [ctypes.POINTER(StradeNet), c_int, c_f, c_stream]),
    "gnf_strade_adjoint_workspace_bytes": (c_i64, [ctypes.POINTER(StradeNet), c_int, c_i64]),
    "gnf_strade_adjoint": (c_int, [ctypes.POINTER(StradeNet), c_int, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_i64, c_int,
                                   ctypes.c_void_p, c_i64, c_stream]),
    "gnf_strade_adjoint_do": (c_int, [ctypes.POINTER(StradeNet), c_int, c_f, c_f, c_f, c_f, c_f, c_f, c_f, ctypes.c_void_p,
                                      c_f, c_i64, c_int, ctypes.c_void_p, c_i64, c_stream]),
    "gnf_dag_loss_prep": (c_int, [c_f, c_f, c_float, c_f, c_i64, c_stream]),
    "gnf_dag_loss_value": (c_int, [c_f, c_f, c_f, c_f, c_float, c_f, c_f, c_f, c_f, c_int, c_f, c_f, c_i64, c_stream]),
    "gnf_dag_loss_bwd": (c_int, [c_f, c_f, c_f, c_f, c_f, c_i64, c_stream]),
    "gnf_mnistcnn_conv_fwd": (c_int, [c_f, c_f, c_f, c_f, c_f, c_f, ctypes.c_void_p, c_i64, c_int, c_stream]),
    "gnf_mnistcnn_conv_bwd_ws_bytes": (c_i64, [c_i64]),
    "gnf_mnistcnn_conv_bwd": (c_int, [c_f, c_f, c_f, c_f, c_f, ctypes.c_void_p, c_f, c_f, c_f, c_f, c_f,
                                      ctypes.c_void_p, c_i64, c_i64, c_stream]),
    "gnf_mnistcnn_conv_bwd_cols": (c_int, [c_f, c_f, c_f, c_f, c_f, ctypes.c_void_p, c_f, ctypes.c_void_p, c_i64, c_f,
                                           c_f, c_f, c_f, c_f, ctypes.c_void_p, c_i64, c_i64, c_stream]),
    "gnf_mnistcnn_conv_a1_bytes": (c_i64, [c_i64]),
    "gnf_mnistcnn_conv_fwd_save": (c_int, [c_f, c_f, c_f, c_f, c_f, c_f, ctypes.c_void_p, c_f, c_i64, c_int, c_stream]),
    "gnf_mnistcnn_conv_bwd_a1": (c_int, [c_f, c_f, c_f, c_f, c_f, c_f, ctypes.c_void_p, c_f, c_f, c_f, c_f, c_f,
                                         ctypes.c_void_p, c_i64, c_i64, c_stream]),
    "gnf_mnistcnn_conv_bwd_cols_a1": (c_int, [c_f, c_f, c_f, c_f, c_f, c_f, ctypes.c_void_p, c_f, ctypes.c_void_p, c_i64,
                                              c_f, c_f, c_f, c_f, c_f, ctypes.c_void_p, c_i64, c_i64, c_stream]),
    "gnf_lenet_conv_supported": (c_int, [c_int, c_int, c_int, c_int]),
    "gnf_lenet_conv_feat": (c_i64, [c_int, c_int, c_int, c_int]),
    "gnf_lenet_conv_fwd": (c_int, [c_f, c_i64, c_int, c_int, c_int, c_int, c_f, c_f, c_f, c_f, c_f, ctypes.c_void_p, c_i64,
                                   c_stream]),
    "gnf_lenet_conv_bwd_ws_bytes": (c_i64, [c_int, c_int, c_int, c_int, c_i64]),
    "gnf_lenet_conv_bwd": (c_int, [c_f, c_i64, c_int, c_int, c_int, c_int, c_f, c_f, c_f, c_f, ctypes.c_void_p, c_f, c_f,
                                   c_i64, c_f, c_f, c_f, c_f, ctypes.c_void_p, c_i64, c_i64, c_stream]),
    "gnf_lenet_gated_fwd": (c_int, [c_f, c_f, c_f, c_int, c_int, c_int, c_int, c_int, c_int, c_float, c_float, c_f, c_f, c_u64,
                                    c_u64, c_f, c_f, c_f, c_f, c_f, ctypes.c_void_p, c_i64, c_stream]),
    "gnf_lenet_gated_bwd_ws_bytes": (c_i64, [c_int, c_int, c_int, c_int, c_i64]),
    "gnf_lenet_gated_bwd": (c_int, [c_f, c_f, c_int, c_int, c_int, c_int, c_int, c_int, c_float, c_f, c_f, c_u64, c_u64, c_f,
                                    c_f, c_f, c_f, ctypes.c_void_p, c_f, c_f, c_int, c_f, c_f, c_f, c_f, ctypes.c_void_p,
                                    c_i64, c_i64, c_stream]),
    "gnf_lenet_rows_fwd": (c_int, [c_f, c_f, c_i64, ctypes.c_void_p, c_i64, c_int, c_int, c_int, c_int, c_f, c_f, c_f, c_f, c_f,
                                   c_int, c_i64, c_stream]),
    "gnf_lenet_rows_fwd_arg": (c_int, [c_f, c_f, c_i64, ctypes.c_void_p, c_i64, c_int, c_int, c_int, c_int, c_f, c_f, c_f, c_f,
                                       c_f, ctypes.c_void_p, c_int, c_i64, c_stream]),
    "gnf_lenet_rows_bwd_ws_bytes": (c_i64, [c_int, c_int, c_int, c_int, c_i64, c_i64, c_int]),
    "gnf_lenet_rows_bwd": (c_int, [c_f, c_f, c_i64, ctypes.c_void_p, c_i64, c_int, c_int, c_int, c_int, c_f, c_f, c_f, c_f,
                                   ctypes.c_void_p, c_f, c_int, c_f, c_f, c_f, c_f, c_f, ctypes.c_void_p, c_i64, c_i64,
                                   c_stream]),
    "gnf_dagmlp_supported": (c_int, [c_i64, c_i64]),
    "gnf_dagmlp_gated_fwd": (c_int, [c_f, c_f, c_f, c_int, c_int, c_float, c_float, c_f, c_f, c_u64, c_u64, c_f, c_i64, c_f,
                                     c_int, c_int, c_f, c_i64, c_i64, c_i64, c_stream]),
    "gnf_dagmlp_gated_bwd_ws_bytes": (c_i64, [c_i64, c_i64, c_i64]),
    "gnf_dagmlp_gated_bwd": (c_int, [c_f, c_f, c_int, c_int, c_float, c_f, c_f, c_u64, c_u64, c_f, c_i64, c_int, c_f, c_f,
                                     c_f, c_int, c_f, c_i64, c_f, ctypes.c_void_p, c_i64, c_i64, c_i64, c_i64, c_stream]),
    "gnf_dagmlp_rows_fwd": (c_int, [c_f, c_f, c_i64, ctypes.c_void_p, c_i64, c_f, c_i64, c_f, c_int, c_int, c_f, c_int,
                                    c_i64, c_i64, c_i64, c_stream]),
    "gnf_mnistcnn_sparse_ws_bytes": (c_i64, [c_i64, c_i64]),
    "gnf_mnistcnn_sparse_fwd": (c_int, [c_f, c_i64, c_f, ctypes.c_void_p, c_i64, ctypes.c_void_p, c_i64, c_f, c_f, c_f,
                                        c_f, c_f, c_f, c_i64, c_f, c_f, ctypes.c_void_p, ctypes.c_void_p, c_i64,
                                        c_stream]),
    "gnf_mnistcnn_sparse_fwd_train": (c_int, [c_f, c_i64, c_f, ctypes.c_void_p, c_i64, ctypes.c_void_p, c_i64, c_f, c_f, c_f,
                                              c_f, c_f, c_f, c_i64, c_f, c_f, ctypes.c_void_p, ctypes.c_void_p, c_i64,
                                              c_stream]),
    "gnf_mnistcnn_sparse_prep_bytes": (c_i64, [c_i64]),
    "gnf_mnistcnn_sparse_prepare": (c_int, [c_f, c_f, c_f, c_f, c_f, c_i64, ctypes.c_void_p, c_i64, c_stream]),
    "gnf_mnistcnn_sparse_fwd_prepared": (c_int, [c_f, c_i64, c_f, ctypes.c_void_p, c_i64, ctypes.c_void_p, c_i64, c_f, c_f,
                                                 c_f, c_f, c_i64, ctypes.c_void_p, c_f, ctypes.c_void_p, c_i64, c_stream]),
    "gnf_mnistcnn_sparse_fwd_prepared_fc2": (c_int, [c_f, c_i64, c_f, ctypes.c_void_p, c_i64, ctypes.c_void_p, c_i64, c_f, c_f,
                                                     c_f, c_f, c_i64, ctypes.c_void_p, c_f, c_f, c_i64, c_f, ctypes.c_void_p,
                                                     c_i64, c_stream]),
    "gnf_mnistcnn_sparse_bwd_ws_bytes": (c_i64, [c_i64, c_i64, c_i64]),
    "gnf_mnistcnn_sparse_bwd": (c_int, [c_f, c_i64, c_f, ctypes.c_void_p, c_i64, ctypes.c_void_p, c_i64,
                                        ctypes.c_void_p, c_i64, ctypes.c_void_p, c_f, c_f, c_f,
                                        c_f, c_f, c_i64, c_f, ctypes.c_void_p, c_f, c_f, c_f, c_f, c_f, c_f, c_f,
                                        ctypes.c_void_p, c_i64, c_stream]),
    "gnf_mnistcnn_sparse_bwd_tables": (c_int, [c_f, c_i64, c_f, ctypes.c_void_p, c_i64, ctypes.c_void_p, c_i64,
                                               ctypes.c_void_p, c_i64, ctypes.c_void_p, c_f, c_f, c_f,
                                               c_f, c_f, c_i64, ctypes.c_void_p, c_f, ctypes.c_void_p, c_f, c_f, c_f, c_f, c_f, c_f, c_f,
                                               ctypes.c_void_p, c_i64, c_stream]),
    "gnf_adam_step": (c_int, [c_f, c_f, c_f, c_f, c_i64, c_double, c_double, c_double, c_double, c_double, c_double, c_int,
                              c_stream]),
    "gnf_adam_step_dev": (c_int, [c_f, c_f, c_f, c_f, c_i64, c_double, c_double, c_double, c_double, c_double, c_double,
                                  ctypes.c_void_p, c_int, c_stream]),
    "gnf_image_prep": (c_int, [ctypes.c_void_p, c_i64, ctypes.c_void_p, c_int, ctypes.c_void_p, c_int, c_int, c_int, c_f, c_u64,
                               c_u64, c_float, c_f, c_f, c_i64, c_stream]),
    "gnf_toy_sample": (c_int, [ctypes.c_void_p, c_int, ctypes.c_void_p, c_f, c_u64, c_u64, c_f, c_i64, c_i64, c_stream]),
    "gnf_shuffle_keys": (c_int, [c_u64, c_u64, c_i64, ctypes.c_void_p, c_stream]),
    "gnf_tab_batch": (c_int, [c_f, c_i64, c_i64, c_i64, ctypes.c_void_p, c_i64, c_i64, c_i64, ctypes.c_void_p, c_f, c_i64,
                              c_stream]),
    "gnf_dag_levels_supported": (c_int, [c_i64]),
    "gnf_dag_levels_ws_bytes": (c_i64, [c_i64, c_i64]),
    "gnf_dag_levels": (c_int, [ctypes.c_void_p, c_int, c_i64, c_i64, c_f, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                               c_i64, c_i64, c_i64, c_stream]),
    "gnf_group_bias_fwd": (c_int, [c_f, c_f, c_f, c_int, c_i64, c_i64, c_i64, c_stream]),
    "gnf_group_bias_bwd": (c_int, [c_f, c_f, c_f, c_f, c_i64, c_i64, c_i64, c_stream]),
    "gnf_probe_mfma_f32": (c_i64, [c_f, c_int, c_int, c_stream]),
    "gnf_probe_copy": (c_int, [c_f, c_f, c_i64, c_stream]),
    "gnf_probe_empty": (c_int, [c_i64, c_int, c_stream]),
}

_lib = None


class GnfError(RuntimeError):
    pass


def load():
    """dlopen libgnf_hip.so (after `import torch`, so that the HIP runtime torch already
    loaded -- same SONAME libamdhip64.so.7 -- is the one the kernels launch on)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("libgnf_hip.so is not built: run `python __graft_entry__.py build` "
                              "(hipcc --offload-arch=gfx950).  There is no CPU fallback. [%s]" % LIB_PATH)
        lib = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)       # AttributeError if the symbol is missing
            fn.restype = res
            fn.argtypes = args
        if lib.gnf_abi_version() != ABI_VERSION:
            raise ImportError("libgnf_hip.so ABI version mismatch")
        _lib = lib
    return _lib


_ERR = {-1: "GNF_EINVAL (bad argument)", -2: "GNF_ESHAPE (unsupported shape)", -3: "GNF_EWS (workspace too small)"}


def check(rc, what):
    if rc != 0:
        raise GnfError("%s failed: %s" % (what, _ERR.get(rc, "hipError_t %d" % rc)))


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    """device pointer of a fp32 HIP tensor (None -> NULL)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise GnfError("gnf_hip kernels run on the MI355X only: got a %s tensor (no CPU fallback)" % t.device)
    if t.dtype != torch.float32:
        raise GnfError("gnf_hip kernels are fp32: got %s" % t.dtype)
    return ctypes.c_void_p(t.data_ptr())


def rawptr(t):
    """device pointer of a HIP tensor of any dtype (byte buffers)."""
    if not t.is_cuda:
        raise GnfError("gnf_hip kernels run on the MI355X only: got a %s tensor (no CPU fallback)" % t.device)
    return ctypes.c_void_p(t.data_ptr())


_prof = None        # name -> [(start_event, end_event), ...] while profiling is enabled


def profile_enable(names):
    """Record HIP events (on torch's current stream = the stream the kernels are launched
    on) around every call of the named entry points; bench.py derives roofline numbers."""
    global _prof
    _prof = {n: [] for n in names}


def profile_collect():
    """-> {name: mean milliseconds per call}; disables profiling.  Synchronises."""
    global _prof
    out = {}
    if _prof:
        torch.cuda.synchronize()
        for n, evs in _prof.items():
            if evs:
                out[n] = sum(a.elapsed_time(b) for a, b in evs) / len(evs)
    _prof = None
    return out


def call(name, *args, profile_as=None):
    """profile_as: the entry point this call stands in for -- its events are filed under that name, so that a profile
    keyed by the original names (bench.py --full) still sees the work."""
    fn = getattr(load(), name)
    pname = profile_as or name
    if _prof is not None and pname in _prof:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        rc = fn(*args)
        b.record()
        _prof[pname].append((a, b))
        check(rc, name)
    else:
        check(fn(*args), name)
