"""ctypes binding of libdsmil_hip.so (include/dsmil_hip.h).  Thin: it passes ``data_ptr()``s,
sizes and the current HIP stream, and turns negative status codes into RuntimeError.

There is deliberately NO fallback: if the shared object is missing or lacks a symbol the import
of the HIP path fails loudly (``NativeLibraryError``)."""
import ctypes
import os

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
# DSMIL_NATIVE_LIB: file name of an alternative in-tree build next to this module (profiling /
# experiment builds made by build.py --variant, e.g. libdsmil_hip_expt.so); default = the product build
LIB_PATH = os.path.join(PKG_DIR, os.path.basename(os.environ.get("DSMIL_NATIVE_LIB", "libdsmil_hip.so")))

c_f32p = ctypes.c_void_p
c_i64p = ctypes.c_void_p


class NativeLibraryError(RuntimeError):
    pass


class AggParams(ctypes.Structure):
    """struct dsmil_agg_params (include/dsmil_hip.h)."""
    _fields_ = [("fc_w", ctypes.c_void_p), ("fc_b", ctypes.c_void_p),
                ("q0_w", ctypes.c_void_p), ("q0_b", ctypes.c_void_p),
                ("q2_w", ctypes.c_void_p), ("q2_b", ctypes.c_void_p),
                ("fcc_w", ctypes.c_void_p), ("fcc_b", ctypes.c_void_p),
                ("K", ctypes.c_int32), ("Kv", ctypes.c_int32),
                ("C", ctypes.c_int32), ("nonlinear", ctypes.c_int32)]


class AggOpts(ctypes.Structure):
    """struct dsmil_agg_opts (include/dsmil_hip.h)."""
    _fields_ = [("packed_split", ctypes.c_void_p), ("row_map", ctypes.c_void_p), ("packed_f2", ctypes.c_void_p)]


class AggCall(ctypes.Structure):
    """struct dsmil_agg_call (include/dsmil_hip.h): a forward call as the library's route function sees it."""
    _fields_ = [("total_rows", ctypes.c_int64), ("max_rows", ctypes.c_int64)] + [(n, ctypes.c_int32) for n in (
        "n_bags", "K", "Kv", "C", "nonlinear", "bf16", "aligned", "classes_given", "vals_separate", "row_map", "packed_split",
        "packed_f2", "phase", "skip_pred", "prologue_job", "several_streams", "cus")]


class AggRoute(ctypes.Structure):
    """struct dsmil_agg_route (include/dsmil_hip.h): the kernels dsmil_agg_forward_route answers for a call."""
    _fields_ = [(n, ctypes.c_int32) for n in (
        "nw", "r0", "logits", "logits_vec", "logits_cp", "prologue", "rowmax", "qmax", "qmax_vec", "qmax_threads", "ragged",
        "ragged_attend", "tile_attend", "tile_logits", "image", "attend", "attend_nw", "attend_vec", "attend_np", "attend_xe",
        "attend_tu", "finish", "finish_rows", "pred")]


# enum values of include/dsmil_hip.h, by position
LOGITS = ("none", "given", "stream", "pipe", "argmax")
QMAX = ("launch", "inline", "shard1", "shard2")
IMAGE = ("none", "f2_caller", "f2_cut", "split_caller", "split_cut", "bf16")
ATTEND = ("none", "f3", "f2", "bf16_res", "bf16_dma", "bf16_ring", "split", "hs", "f32")
FINISH = ("none", "lean", "vec4", "scalar")


def forward_route(**call):
    """dsmil_agg_forward_route for a call given as dsmil_agg_call fields (missing ones are 0; ``aligned`` defaults to 7: every
    operand 16-byte aligned).  Touches no device when ``cus`` is given."""
    c = AggCall(**dict({"aligned": 7}, **call))
    r = AggRoute()
    check(lib().dsmil_agg_forward_route(ctypes.byref(c), ctypes.byref(r)), "dsmil_agg_forward_route")
    return r


class AggGrads(ctypes.Structure):
    """struct dsmil_agg_grads (include/dsmil_hip.h)."""
    _fields_ = [(n, ctypes.c_void_p) for n in
                ("fc_w", "fc_b", "q0_w", "q0_b", "q2_w", "q2_b", "fcc_w", "fcc_b")]


class AggBwdLayout(ctypes.Structure):
    """struct dsmil_agg_bwd_layout (include/dsmil_hip.h): where a backward call leaves its intermediates — FOR TESTS."""
    REGIONS = ("gB", "Dv", "qmax", "gq", "gA", "gs", "gz2", "Hb", "Qb", "gH", "gqp", "part0", "part1", "pb0", "pb1", "part", "part_b")
    _fields_ = [(n, ctypes.c_uint64) for n in REGIONS + ("total",)] + [("T32", ctypes.c_int64)] + \
        [(n, ctypes.c_int32) for n in ("S", "R", "splits", "small_rows", "tile", "qrow_vec")]


BWD_TILE = ("hs", "w1_reg", "w4_dma", "w4_reg")     # DSMIL_BWD_TILE_*, by value


def backward_layout(n_bags, N, K, Kv, C, nonlinear=1, rows_aligned16=1, q0w_aligned16=1):
    """dsmil_agg_backward_layout (FOR TESTS; host only): n_bags == 0 for the one-bag entries."""
    out = AggBwdLayout()
    check(lib().dsmil_agg_backward_layout(n_bags, N, K, Kv, C, nonlinear, rows_aligned16, q0w_aligned16, ctypes.byref(out)),
          "dsmil_agg_backward_layout")
    return out


class BceWeights(ctypes.Structure):
    """struct dsmil_bce_weights (include/dsmil_hip.h): device pointers, [C] fp32 each, either may be NULL."""
    _fields_ = [("pos_weight", ctypes.c_void_p), ("weight", ctypes.c_void_p)]


class AdamState(ctypes.Structure):
    """struct dsmil_adam_state (include/dsmil_hip.h)."""
    _fields_ = [("exp_avg", ctypes.POINTER(ctypes.c_void_p)), ("exp_avg_sq", ctypes.POINTER(ctypes.c_void_p)),
                ("step", ctypes.c_int64), ("lr", ctypes.c_double), ("beta1", ctypes.c_double), ("beta2", ctypes.c_double),
                ("eps", ctypes.c_double), ("weight_decay", ctypes.c_double)]


# symbol -> (restype, argtypes); must list every function include/dsmil_hip.h declares
SIGNATURES = {
    "dsmil_abi_version": (ctypes.c_int, []),
    "dsmil_strerror": (ctypes.c_char_p, [ctypes.c_int]),
    "dsmil_agg_mlp_form": (ctypes.c_int, []),
    "dsmil_agg_inline_query": (ctypes.c_int, [ctypes.c_int]),
    "dsmil_agg_batch_form": (ctypes.c_int, [ctypes.c_int]),
    "dsmil_agg_persistent_grid": (ctypes.c_int, [ctypes.c_int]),
    "dsmil_agg_logits_form": (ctypes.c_int, [ctypes.c_int]),
    "dsmil_device_cus": (ctypes.c_int, []),
    "dsmil_agg_packed_f2_bytes": (ctypes.c_size_t, [ctypes.c_int32]),
    "dsmil_agg_pack_f2": (ctypes.c_int, [c_f32p, c_f32p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]),
    "dsmil_agg_packed_split_bytes": (ctypes.c_size_t, [ctypes.c_int32, ctypes.c_int32]),
    "dsmil_agg_pack_split": (ctypes.c_int, [c_f32p, c_f32p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]),
    "dsmil_agg_forward_ex": (ctypes.c_int, [c_f32p, c_f32p, c_i64p, ctypes.c_int32, ctypes.c_int64,
                                            ctypes.c_int64, ctypes.POINTER(AggParams), ctypes.POINTER(AggOpts), c_f32p,
                                            c_f32p, c_f32p, c_f32p, c_f32p, c_i64p, ctypes.c_void_p,
                                            ctypes.c_size_t, ctypes.c_void_p]),
    "dsmil_agg_loss_head": (ctypes.c_int, [c_f32p, c_f32p, c_i64p, c_f32p, ctypes.c_int32, c_f32p, c_f32p, c_f32p,
                                           c_f32p, ctypes.c_void_p]),
    "dsmil_agg_loss_head_w": (ctypes.c_int, [c_f32p, c_f32p, c_i64p, c_f32p, ctypes.c_int32, c_f32p, c_f32p, c_f32p,
                                             c_f32p, ctypes.POINTER(BceWeights), ctypes.c_void_p]),
    "dsmil_agg_backward_ex": (ctypes.c_int, [c_f32p, c_f32p, ctypes.c_int64, ctypes.POINTER(AggParams), c_f32p,
                                             c_f32p, c_i64p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p,
                                             ctypes.POINTER(AggGrads), c_f32p, c_i64p, ctypes.c_void_p, ctypes.c_size_t,
                                             ctypes.c_void_p]),
    "dsmil_agg_shard_argmax": (ctypes.c_int, [c_f32p, ctypes.c_int64, ctypes.POINTER(AggParams), c_f32p, c_f32p,
                                              c_i64p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "dsmil_agg_shard_attend": (ctypes.c_int, [c_f32p, c_f32p, ctypes.c_int64, ctypes.POINTER(AggParams), c_f32p,
                                              c_f32p, c_f32p, c_f32p, ctypes.c_void_p, ctypes.c_size_t,
                                              ctypes.c_void_p]),
    "dsmil_agg_tile_rows": (ctypes.c_int, [ctypes.c_int32, ctypes.c_int64]),
    "dsmil_agg_forward_route": (ctypes.c_int, [ctypes.POINTER(AggCall), ctypes.POINTER(AggRoute)]),
    "dsmil_agg_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int32, ctypes.c_int64, ctypes.c_int32,
                                                    ctypes.c_int32, ctypes.c_int32]),
    "dsmil_agg_packed_bf16_bytes": (ctypes.c_size_t, [ctypes.c_int32]),
    "dsmil_agg_pack_bf16": (ctypes.c_int, [c_f32p, c_f32p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]),
    "dsmil_agg_forward_bf16": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, c_i64p, ctypes.c_int32,
                                              ctypes.c_int64, ctypes.c_int64, ctypes.POINTER(AggParams),
                                              ctypes.c_void_p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_i64p,
                                              ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "dsmil_profile_enable": (ctypes.c_int, [ctypes.c_int]),
    "dsmil_profile_collect": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64)]),
    "dsmil_resnet18_packed_bytes": (ctypes.c_size_t, []),
    "dsmil_resnet18_pack": (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), c_f32p, ctypes.c_void_p]),
    "dsmil_resnet18_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32]),
    "dsmil_resnet18in_forward": (ctypes.c_int, [c_f32p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                                c_f32p, c_f32p, c_f32p, c_f32p, ctypes.c_int32, c_f32p,
                                                c_f32p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "dsmil_resnet18in_forward_u8": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                                   c_f32p, c_f32p, c_f32p, c_f32p, ctypes.c_int32, c_f32p,
                                                   c_f32p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "dsmil_resnet18_norm_channels": (ctypes.c_int32, []),
    "dsmil_resnet18bn_forward": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                                ctypes.c_int32, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p,
                                                ctypes.c_int32, c_f32p, c_f32p, ctypes.c_void_p, ctypes.c_size_t,
                                                ctypes.c_void_p]),
    "dsmil_resnet_num_convs": (ctypes.c_int32, [ctypes.c_int32]),
    "dsmil_resnet_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32]),
    "dsmil_resnet_feature_dim": (ctypes.c_int32, [ctypes.c_int32]),
    "dsmil_resnet_mfma_forms": (ctypes.c_int, [ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]),
    "dsmil_resnet_norm_channels": (ctypes.c_int32, [ctypes.c_int32]),
    "dsmil_resnet_packed_bytes": (ctypes.c_size_t, [ctypes.c_int32]),
    "dsmil_resnet_packed_bytes_ex": (ctypes.c_size_t, [ctypes.c_int32, ctypes.c_int32]),
    "dsmil_resnet_pack": (ctypes.c_int, [ctypes.c_int32, ctypes.POINTER(ctypes.c_void_p), c_f32p, ctypes.c_void_p]),
    "dsmil_resnet_forward": (ctypes.c_int, [ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32,
                                            ctypes.c_int32, ctypes.c_int32, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p,
                                            c_f32p, ctypes.c_int32, c_f32p, c_f32p, ctypes.c_void_p,
                                            ctypes.c_size_t, ctypes.c_void_p]),
    "dsmil_resnet_pack_ex": (ctypes.c_int, [ctypes.c_int32, ctypes.POINTER(ctypes.c_void_p), c_f32p, ctypes.c_int32, ctypes.c_void_p]),
    "dsmil_resnet_forward_ex": (ctypes.c_int, [ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32,
                                               ctypes.c_int32, ctypes.c_int32, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p,
                                               c_f32p, ctypes.c_int32, c_f32p, c_f32p, ctypes.c_void_p,
                                               ctypes.c_size_t, ctypes.c_int32, ctypes.c_void_p]),
    # the stages of the 16-bit activation trunk alone (for tests)
    "dsmil_trunk16_positions": (ctypes.c_size_t, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32]),
    "dsmil_trunk16_layout": (ctypes.c_int, [c_f32p, ctypes.c_void_p] + [ctypes.c_int32] * 6 + [ctypes.c_void_p]),
    "dsmil_trunk16_conv_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32]),
    "dsmil_trunk16_conv": (ctypes.c_int, [ctypes.c_void_p, c_f32p, ctypes.c_void_p] + [ctypes.c_int32] * 9 +
                           [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "dsmil_trunk16_norm_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int32, ctypes.c_int32]),
    "dsmil_trunk16_norm": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int32] * 6 +
                           [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "dsmil_trunk16_pool": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, c_f32p] + [ctypes.c_int32] * 5 +
                           [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "dsmil_trunk16_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int32] * 4),
    "dsmil_trunk16_forward": (ctypes.c_int, [ctypes.c_int32, c_f32p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                             ctypes.POINTER(ctypes.c_void_p), c_f32p, ctypes.c_int32, ctypes.c_void_p,
                                             ctypes.c_size_t, ctypes.c_void_p]),
    # the stages of the fp32-class trunk alone (for tests)
    "dsmil_trunk32_conv_plan": (ctypes.c_int, [ctypes.c_int32] * 10 + [ctypes.POINTER(ctypes.c_int32)]),
    "dsmil_trunk32_conv_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int32] * 9),
    "dsmil_trunk32_conv": (ctypes.c_int, [c_f32p] * 9 + [ctypes.c_int32] * 9 + [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "dsmil_trunk32_stem_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int32] * 3),
    "dsmil_trunk32_stem": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32] + [c_f32p] * 6 + [ctypes.c_int32] * 4 +
                           [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "dsmil_trunk32_tail": (ctypes.c_int, [ctypes.c_int32] + [c_f32p] * 7 + [ctypes.c_int32] * 4 + [ctypes.c_void_p]),
    "dsmil_tile_stats": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p,
                                        ctypes.c_void_p]),
    "dsmil_jpeg_plan_bytes": (ctypes.c_size_t, [ctypes.c_int32]),
    "dsmil_jpeg_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int64]),
    "dsmil_jpeg_parse": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p]),
    "dsmil_read_files": (ctypes.c_int64, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]),
    "dsmil_csv_parse_f32": (ctypes.c_int64, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64]),
    "dsmil_csv_format_f32": (ctypes.c_int64, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int32,
                                              ctypes.c_void_p, ctypes.c_int64]),
    "dsmil_jpeg_decode": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "dsmil_fc_forward": (ctypes.c_int, [c_f32p, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32,
                                        c_f32p, c_f32p, c_f32p, ctypes.c_void_p]),
    "dsmil_agg_backward_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int32, ctypes.c_int32,
                                                             ctypes.c_int32]),
    "dsmil_agg_backward": (ctypes.c_int, [c_f32p, c_f32p, ctypes.c_int64, ctypes.POINTER(AggParams), c_f32p,
                                          c_f32p, c_i64p, c_f32p, c_f32p, c_f32p, c_f32p,
                                          ctypes.POINTER(AggGrads), c_f32p, ctypes.c_void_p, ctypes.c_size_t,
                                          ctypes.c_void_p]),
    "dsmil_agg_backward_rows_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int32, ctypes.c_int32,
                                                                  ctypes.c_int32]),
    "dsmil_agg_backward_rows": (ctypes.c_int, [c_f32p, c_f32p, ctypes.c_int64, ctypes.POINTER(AggParams), c_f32p,
                                               c_f32p, c_i64p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p,
                                               ctypes.POINTER(AggGrads), c_f32p, c_i64p, ctypes.c_void_p, ctypes.c_size_t,
                                               ctypes.c_void_p, c_f32p]),
    "dsmil_agg_backward_bags_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int32, ctypes.c_int64, ctypes.c_int32,
                                                                  ctypes.c_int32, ctypes.c_int32]),
    "dsmil_agg_backward_bags": (ctypes.c_int, [c_f32p, c_f32p, c_i64p, ctypes.c_int32, ctypes.c_int64, ctypes.c_int64,
                                               ctypes.POINTER(AggParams), c_f32p, c_f32p, c_i64p, c_f32p, c_f32p, c_f32p,
                                               c_f32p, c_f32p, ctypes.POINTER(AggGrads), c_f32p, c_i64p, ctypes.c_void_p,
                                               ctypes.c_size_t, ctypes.c_void_p, c_f32p]),
    "dsmil_agg_backward_layout": (ctypes.c_int, [ctypes.c_int32, ctypes.c_int64] + [ctypes.c_int32] * 6 + [ctypes.POINTER(AggBwdLayout)]),
    "dsmil_agg_backward_bags_bf16_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int32, ctypes.c_int64, ctypes.c_int32,
                                                                       ctypes.c_int32, ctypes.c_int32]),
    "dsmil_agg_backward_bags_bf16": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, c_i64p, ctypes.c_int32, ctypes.c_int64,
                                                    ctypes.c_int64, ctypes.POINTER(AggParams), c_f32p, c_f32p, c_i64p, c_f32p,
                                                    c_f32p, c_f32p, c_f32p, c_f32p, ctypes.POINTER(AggGrads), c_f32p,
                                                    ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "dsmil_agg_loss_head_bags": (ctypes.c_int, [c_f32p, c_i64p, c_f32p, c_i64p, c_f32p, ctypes.c_int32, ctypes.c_int32,
                                                c_f32p, c_f32p, c_f32p, c_f32p, ctypes.c_void_p]),
    "dsmil_agg_loss_head_bags_w": (ctypes.c_int, [c_f32p, c_i64p, c_f32p, c_i64p, c_f32p, ctypes.c_int32, ctypes.c_int32,
                                                  c_f32p, c_f32p, c_f32p, c_f32p, ctypes.POINTER(BceWeights), ctypes.c_void_p]),
    "dsmil_value_backward_rows": (ctypes.c_int, [c_f32p, c_f32p, c_f32p, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32,
                                                 c_f32p, ctypes.c_void_p, ctypes.c_int32, c_f32p, ctypes.c_void_p,
                                                 ctypes.c_size_t, ctypes.c_void_p]),
    "dsmil_value_packed_bytes": (ctypes.c_size_t, [ctypes.c_int32, ctypes.c_int32]),
    "dsmil_value_pack": (ctypes.c_int, [c_f32p, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]),
    "dsmil_value_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int32, ctypes.c_int32]),
    "dsmil_value_forward": (ctypes.c_int, [c_f32p, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, c_f32p, c_f32p,
                                           ctypes.c_void_p, c_i64p, c_f32p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "dsmil_value_backward": (ctypes.c_int, [c_f32p, c_f32p, c_f32p, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, c_i64p,
                                            c_f32p, c_f32p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "dsmil_value_packed_bf16_bytes": (ctypes.c_size_t, [ctypes.c_int32, ctypes.c_int32]),
    "dsmil_value_pack_bf16": (ctypes.c_int, [c_f32p, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]),
    "dsmil_value_workspace_bf16_bytes": (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int32, ctypes.c_int32]),
    "dsmil_value_forward_bf16": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, c_f32p, c_f32p,
                                                ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                                ctypes.c_void_p]),
    "dsmil_value_backward_bf16_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int32, ctypes.c_int32]),
    "dsmil_value_backward_bf16": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, c_f32p, ctypes.c_int64, ctypes.c_int32,
                                                 ctypes.c_int32, c_f32p, c_f32p, ctypes.c_void_p, ctypes.c_size_t,
                                                 ctypes.c_void_p]),
    "dsmil_agg_train_step_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32]),
    "dsmil_agg_train_step": (ctypes.c_int, [c_f32p, ctypes.c_int64, c_i64p, c_f32p, ctypes.POINTER(AggParams),
                                            ctypes.POINTER(AdamState), c_f32p, ctypes.c_void_p, ctypes.c_size_t,
                                            ctypes.c_void_p]),
    "dsmil_agg_train_step_bags_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int32, ctypes.c_int64, ctypes.c_int32,
                                                                    ctypes.c_int32, ctypes.c_int32]),
    "dsmil_agg_train_step_bags": (ctypes.c_int, [c_f32p, c_i64p, ctypes.c_int32, ctypes.c_int64, ctypes.c_int64, c_i64p,
                                                 c_f32p, ctypes.POINTER(AggParams), ctypes.POINTER(AdamState), c_f32p,
                                                 c_f32p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "dsmil_agg_train_step_bags_bf16_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int32, ctypes.c_int64, ctypes.c_int32,
                                                                         ctypes.c_int32, ctypes.c_int32]),
    "dsmil_agg_train_step_bags_bf16": (ctypes.c_int, [ctypes.c_void_p, c_i64p, ctypes.c_int32, ctypes.c_int64,
                                                      ctypes.c_int64, c_f32p, ctypes.POINTER(AggParams),
                                                      ctypes.POINTER(AdamState), c_f32p, c_f32p, ctypes.c_void_p,
                                                      ctypes.c_size_t, ctypes.c_void_p]),
    # the weighted-BCE forms: the sibling's signature + const dsmil_bce_weights* in front of the stream
    "dsmil_agg_train_step_bags_w": (ctypes.c_int, [c_f32p, c_i64p, ctypes.c_int32, ctypes.c_int64, ctypes.c_int64, c_i64p,
                                                   c_f32p, ctypes.POINTER(AggParams), ctypes.POINTER(AdamState), c_f32p,
                                                   c_f32p, ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(BceWeights),
                                                   ctypes.c_void_p]),
    "dsmil_agg_train_step_bags_bf16_w": (ctypes.c_int, [ctypes.c_void_p, c_i64p, ctypes.c_int32, ctypes.c_int64,
                                                        ctypes.c_int64, c_f32p, ctypes.POINTER(AggParams),
                                                        ctypes.POINTER(AdamState), c_f32p, c_f32p, ctypes.c_void_p,
                                                        ctypes.c_size_t, ctypes.POINTER(BceWeights), ctypes.c_void_p]),
    "dsmil_adam_step": (ctypes.c_int, [ctypes.c_int32, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p),
                                       ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p),
                                       ctypes.POINTER(ctypes.c_int64), ctypes.c_int64, ctypes.c_double, ctypes.c_double,
                                       ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_void_p]),
    # NT-Xent (SimCLR pre-training of the embedder)
    "dsmil_ntxent_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int]),
    "dsmil_ntxent_forward": (ctypes.c_int, [c_f32p, c_f32p, ctypes.c_int64, ctypes.c_int, ctypes.c_float, ctypes.c_int, c_f32p,
                                            c_f32p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "dsmil_ntxent_backward": (ctypes.c_int, [c_f32p, c_f32p, ctypes.c_int64, ctypes.c_int, ctypes.c_float, ctypes.c_int, c_f32p,
                                             c_f32p, c_f32p, c_f32p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    # SimCLR's two-view augmentation (records: struct dsmil_simclr_view, 12 x 4 bytes, passed by address)
    "dsmil_simclr_views_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "dsmil_simclr_views": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                          ctypes.c_int64, ctypes.c_int, c_f32p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                          ctypes.c_void_p]),
    "dsmil_simclr_views_host": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                               ctypes.c_int64, ctypes.c_int, c_f32p, ctypes.c_void_p, ctypes.c_void_p,
                                               ctypes.c_size_t]),
    # conv backward for embedder training (weight and data gradients)
    "dsmil_conv_bwd_plan": (ctypes.c_int, [ctypes.c_int32] * 9 + [ctypes.POINTER(ctypes.c_int32)]),
    "dsmil_conv_bwd_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int32] * 9),
    "dsmil_conv_bwd_weight": (ctypes.c_int, [c_f32p] * 5 + [ctypes.c_int32] * 8 + [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "dsmil_conv_bwd_data": (ctypes.c_int, [c_f32p] * 3 + [ctypes.c_int32] * 8 + [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    # InstanceNorm / ReLU / residual-add backward for embedder training
    "dsmil_norm_bwd_plan": (ctypes.c_int, [ctypes.c_int32] * 4 + [ctypes.POINTER(ctypes.c_int32)]),
    "dsmil_norm_bwd_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int32] * 4),
    "dsmil_norm_bwd": (ctypes.c_int, [ctypes.c_int32] + [c_f32p] * 11 + [ctypes.c_int32] * 3 +
                       [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    # the stem on the training path: a forward that keeps the raw map and the pool's winners, and its norm / ReLU / pool backward
    "dsmil_trunk32_stem_train_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int32] * 3),
    "dsmil_trunk32_stem_train": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32] + [c_f32p] * 5 + [ctypes.c_void_p] +
                                 [ctypes.c_int32] * 4 + [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "dsmil_stem_pool_bwd_plan": (ctypes.c_int, [ctypes.c_int32] * 4 + [ctypes.POINTER(ctypes.c_int32)]),
    "dsmil_stem_pool_bwd_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int32] * 4),
    "dsmil_stem_pool_bwd": (ctypes.c_int, [c_f32p] * 4 + [ctypes.c_void_p, c_f32p] + [ctypes.c_int32] * 4 +
                            [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "dsmil_agg_forward": (ctypes.c_int, [c_f32p, c_f32p, c_i64p, ctypes.c_int32, ctypes.c_int64,
                                         ctypes.c_int64, ctypes.POINTER(AggParams), c_f32p, c_f32p,
                                         c_f32p, c_f32p, c_f32p, c_i64p, ctypes.c_void_p,
                                         ctypes.c_size_t, ctypes.c_void_p]),
}

DSMIL_E_INVALID = -1        # include/dsmil_hip.h
DSMIL_E_UNSUPPORTED = -2
DSMIL_E_WORKSPACE = -3

_lib = None


def lib():
    """The loaded shared library (loads on first use)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise NativeLibraryError(
                f"{LIB_PATH} not found: build it with `python __graft_entry__.py` "
                f"(or dsmil-wsi_amd/build.py); the HIP path has no fallback")
        try:
            L = ctypes.CDLL(LIB_PATH)
        except OSError as e:  # pragma: no cover
            raise NativeLibraryError(f"cannot load {LIB_PATH}: {e}") from e
        for name, (res, args) in SIGNATURES.items():
            try:
                fn = getattr(L, name)
            except AttributeError as e:
                raise NativeLibraryError(f"{LIB_PATH} does not export {name}") from e
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(code, what):
    if code != 0:
        msg = lib().dsmil_strerror(code).decode()
        raise RuntimeError(f"{what} failed: {msg} (code {code})")
