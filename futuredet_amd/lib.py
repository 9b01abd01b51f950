"""ctypes binding of libfuturedet_hip.so (the C ABI declared in include/futuredet_hip.h).

There is no CPU fallback: loading fails loudly when the library is missing, and every op raises
when its tensors are not on a HIP device.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FD_LIB_PATH") or os.path.join(_HERE, "libfuturedet_hip.so")  # override: tuning builds only
_lib = None

c_void_p = ctypes.c_void_p
c_int = ctypes.c_int
c_i64 = ctypes.c_int64
c_size_t = ctypes.c_size_t
c_float = ctypes.c_float


class MapView(ctypes.Structure):
    """fd_map_view (include/futuredet_hip.h): element (g, ch, cell) at data[g * group_stride + ch * channel_stride + cell * cell_stride]"""
    _fields_ = [("data", ctypes.c_void_p), ("group_stride", ctypes.c_int64), ("channel_stride", ctypes.c_int64), ("cell_stride", ctypes.c_int64),
                ("dtype", ctypes.c_int)]


ABI_VERSION = 8  # include/futuredet_hip.h: fd_abi_version()


class DecodeCfg(ctypes.Structure):  # struct fd_decode_cfg
    _fields_ = [("H", c_int), ("W", c_int), ("out_size_factor", c_float), ("voxel_x", c_float), ("voxel_y", c_float),
                ("pc_x", c_float), ("pc_y", c_float), ("score_threshold", c_float), ("center_range", c_float * 6),
                ("nms_iou_threshold", c_float), ("nms_pre_max", c_int), ("nms_post_max", c_int), ("hm_channels", c_int),
                ("nms_kind", c_int), ("n_radius", c_int), ("circle_radius", c_float * 16)]


class IndexLevel(ctypes.Structure):  # struct fd_index_level
    _fields_ = [("D", ctypes.c_int32), ("H", ctypes.c_int32), ("W", ctypes.c_int32), ("ksize", ctypes.c_int32 * 3),
                ("stride", ctypes.c_int32 * 3), ("pad", ctypes.c_int32 * 3), ("words", c_void_p), ("prefix", c_void_p),
                ("coords", c_void_p), ("coords_rows", ctypes.c_int64)]


class PlanSource(ctypes.Structure):  # struct fd_plan_source
    _fields_ = [("in_words", c_void_p), ("in_prefix", c_void_p), ("out_coords", c_void_p), ("n_out_dev", c_void_p), ("ranges", c_void_p),
                ("plan", c_void_p), ("n_out", ctypes.c_int64), ("plan_stride", ctypes.c_int64), ("Din", ctypes.c_int32), ("Hin", ctypes.c_int32),
                ("Win", ctypes.c_int32), ("n_ranges", ctypes.c_int32), ("stride", ctypes.c_int32 * 3), ("pad", ctypes.c_int32 * 3)]


class ForecastBuffers(ctypes.Structure):  # struct fd_forecast_buffers
    _fields_ = [(n, c_void_p) for n in ("center", "quat", "velocity", "size", "fwd_idx", "fwd_ok", "bwd_idx", "bwd_ok", "match_idx", "cv_centers",
                                        "status", "traj_kind", "traj_src", "traj_first", "traj_group", "n_traj")]


class TargetsCfg(ctypes.Structure):  # struct fd_targets_cfg
    _fields_ = [("H", c_int), ("W", c_int), ("T", c_int), ("n_max", c_int), ("max_objs", c_int), ("n_sets", c_int), ("n_tasks", c_int),
                ("task_classes", c_int * 16), ("radius_mult", c_int), ("min_radius", c_int), ("out_size_factor", c_float), ("voxel_x", c_float),
                ("voxel_y", c_float), ("pc_x", c_float), ("pc_y", c_float), ("gaussian_overlap", ctypes.c_double)]


class OptimTable(ctypes.Structure):  # struct fd_optim_table
    _fields_ = [(n, c_void_p) for n in ("params", "numel", "offset", "flags", "step", "coef", "chunks", "partials", "norm", "grad", "exp_avg",
                                        "exp_avg_sq")] + [("total", c_i64), ("n_tensors", ctypes.c_int32), ("n_chunks", ctypes.c_int32),
                                                          ("chunk", ctypes.c_int32)]


class LossCfg(ctypes.Structure):  # struct fd_loss_cfg
    _fields_ = [(n, ctypes.c_int32) for n in ("B", "H", "W", "M", "n_tasks", "dense", "T", "D", "row_stride")] + [
        ("col", ctypes.c_int32 * 14), ("code_weights", ctypes.c_double * 14), ("code_weights_forecast", ctypes.c_double * 14),
        ("weight", ctypes.c_double)]


class LossTask(ctypes.Structure):  # struct fd_loss_task
    _fields_ = [("hm", c_void_p), ("hm_target", c_void_p), ("ind", c_void_p), ("cat", c_void_p), ("mask", c_void_p * 7), ("maps", c_void_p * 7),
                ("anno_box", c_void_p * 7), ("C", ctypes.c_int32), ("sig", c_void_p), ("d_hm", c_void_p), ("d_maps", c_void_p * 7)]


class HeadTailGroup(ctypes.Structure):  # struct fd_head_tail_group
    _fields_ = [("x", c_void_p), ("w", c_void_p), ("bias", c_void_p), ("y", c_void_p), ("x_stride", c_i64), ("cin", c_int), ("k", c_int)]


class DenseBnNhwcGroup(ctypes.Structure):  # struct fd_dense_bn_nhwc_group
    _fields_ = [("gamma", c_void_p), ("beta", c_void_p), ("running_mean", c_void_p), ("running_var", c_void_p), ("num_batches_tracked", c_void_p),
                ("c", c_int), ("eps", c_float), ("momentum", ctypes.c_double)]


class AugmentRecord(ctypes.Structure):  # struct fd_augment_record
    _fields_ = [("flip_a", ctypes.c_int32), ("flip_b", ctypes.c_int32), ("c", c_float), ("s", c_float), ("rot", c_float), ("scale", c_float),
                ("tx", ctypes.c_double), ("ty", ctypes.c_double), ("tz", ctypes.c_double)]


class GtSampleGroup(ctypes.Structure):  # struct fd_gt_sample_group
    _fields_ = [("class_id", ctypes.c_int32), ("trajectory", ctypes.c_int32), ("max_num", ctypes.c_int32), ("first", ctypes.c_int32),
                ("n", ctypes.c_int32)]


class AugmentMaskRecord(ctypes.Structure):  # struct fd_augment_mask_record
    _fields_ = [("flip_a", ctypes.c_int32), ("flip_b", ctypes.c_int32), ("m1", ctypes.c_double * 6), ("m2", ctypes.c_double * 6)]


# name -> (restype, argtypes); this table is checked against include/futuredet_hip.h by the tests
SIGNATURES = {
    "fd_abi_version": (c_int, []),
    "fd_last_error": (ctypes.c_char_p, []),
    "fd_tuning_set": (c_int, [ctypes.c_char_p, c_int]),
    "fd_voxelize_workspace_bytes": (c_size_t, [c_i64, c_i64]),
    "fd_voxelize": (c_int, [c_void_p, c_i64, c_void_p, c_int, c_void_p, c_void_p, c_int, c_i64, c_int, c_void_p, c_void_p, c_int,
                            c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "fd_index_num_cols": (c_i64, [c_int, c_int, c_int]),
    "fd_index_workspace_bytes": (c_size_t, [c_i64]),
    "fd_index_mark": (c_int, [c_void_p, c_void_p, c_i64, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "fd_index_downsample": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "fd_index_scan": (c_int, [c_void_p, c_i64, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "fd_index_coords": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "fd_index_lookup": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_i64, c_void_p, c_void_p]),
    "fd_rows_permute": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_i64, c_void_p, c_int, c_int, c_void_p]),
    "fd_rulebook": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_i64, c_void_p, c_i64, c_int, c_void_p, c_void_p,
                            c_void_p, c_void_p, c_void_p]),
    "fd_spconv_packed_weight_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "fd_spconv_pack_weight": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "fd_spconv_apply": (c_int, [c_void_p, c_i64, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_i64, c_void_p, c_int, c_int, c_i64,
                                c_void_p, c_i64, c_int, c_int, c_int, c_void_p, c_void_p]),
    "fd_spconv_num_ranges": (c_int, [c_i64, c_int, c_int, c_int]),
    "fd_spconv_wants_balanced_ranges": (c_int, [c_int, c_int, c_int]),
    "fd_spconv_ranges_workspace_bytes": (c_size_t, [c_i64]),
    "fd_spconv_ranges": (c_int, [c_void_p, c_i64, c_int, c_i64, c_void_p, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "fd_spconv_plan_stride": (c_i64, [c_i64]),
    "fd_spconv_plan_bytes": (c_size_t, [c_i64]),
    "fd_spconv_plan_wanted": (c_int, [c_int, c_int, c_int]),
    "fd_spconv_plan_build": (c_int, [c_void_p, c_i64, c_int, c_i64, c_void_p, c_void_p, c_int, c_void_p, c_i64, c_void_p]),
    "fd_spconv_apply_plan": (c_int, [c_void_p, c_i64, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_i64, c_void_p, c_int, c_int, c_i64,
                                     c_void_p, c_i64, c_int, c_int, c_int, c_void_p, c_void_p, c_i64, c_void_p]),
    "fd_spconv_index_plan_wanted": (c_int, [c_int, c_int, c_int]),
    "fd_spconv_layout_wanted": (c_int, [c_int, c_int, c_int]),
    "fd_spconv_apply_layout": (c_int, [c_void_p, c_i64, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_i64, c_void_p, c_int, c_int, c_i64,
                                       c_void_p, c_i64, c_int, c_int, c_int, c_void_p, c_void_p, c_i64, c_int, c_void_p]),
    "fd_spconv_plan_from_index": (c_int, [c_int, c_int, ctypes.POINTER(PlanSource), c_void_p]),
    "fd_spconv_ranges_from_index": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_i64, c_void_p, c_int, c_void_p, c_void_p, c_size_t,
                                            c_void_p]),
    "fd_densify": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_i64,
                           c_i64, c_i64, c_i64, c_i64, c_void_p]),
    "fd_conv2d_packed_weight_bytes": (c_size_t, [c_int, c_int, c_int]),
    "fd_conv2d_pack_weight": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p]),
    "fd_conv2d_nhwc_bf16": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int,
                                    c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "fd_conv2d_f32_packed_weight_bytes": (c_size_t, [c_int, c_int, c_int]),
    "fd_conv2d_f32_pack_weight": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p]),
    "fd_conv2d_f32_num_tiles": (c_int, []),
    "fd_conv2d_nhwc_f32": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int,
                                   c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "fd_conv2d_shuffle_nhwc_f32": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_int, c_int,
                                           c_void_p]),
    "fd_conv2d_grouped_nhwc_f32": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int,
                                           c_int, c_void_p]),
    "fd_conv2d_wino_f32_num_tiles": (c_int, []),
    "fd_conv2d_wino_f32_packed_weight_bytes": (c_size_t, [c_int, c_int]),
    "fd_conv2d_wino_f32_pack_weight": (c_int, [c_void_p, c_int, c_int, c_void_p]),
    "fd_conv2d_wino_nhwc_f32": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_int,
                                        c_void_p]),
    "fd_decode_workspace_bytes": (c_size_t, [c_int, ctypes.POINTER(DecodeCfg)]),
    "fd_centerpoint_decode": (c_int, [c_void_p, c_i64, c_void_p, c_i64, c_void_p, c_i64, c_void_p, c_i64, c_void_p, c_i64,
                                      c_int, ctypes.POINTER(DecodeCfg), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                      c_size_t, c_void_p]),
    "fd_centerpoint_decode_maps": (c_int, [ctypes.POINTER(MapView)] * 5 + [c_int, ctypes.POINTER(DecodeCfg), c_void_p, c_void_p, c_void_p, c_void_p,
                                           c_void_p, c_size_t, c_void_p]),
    "fd_centerpoint_decode_packed": (c_int, [ctypes.POINTER(MapView)] * 6 + [c_int, c_int, ctypes.POINTER(DecodeCfg), c_int, c_void_p, c_void_p, c_void_p,
                                             c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "fd_assemble_detections": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, ctypes.POINTER(MapView), c_int, c_int, c_int, c_void_p, c_void_p,
                                       c_void_p, c_void_p, c_void_p, c_void_p]),
    "fd_nms_workspace_bytes": (c_size_t, [c_int]),
    "fd_rotated_nms": (c_int, [c_void_p, c_int, c_float, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "fd_boxes_iou_bev": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p]),
    "fd_pillar_encode": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_i64, c_int, c_int, c_int, c_float, c_float, c_float,
                                 c_float, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                 c_void_p, c_int, c_void_p]),
    "fd_pillar_scatter": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_i64, c_int, c_int, c_int, c_void_p, c_int,
                                  c_i64, c_i64, c_i64, c_i64, c_int, c_void_p]),
    "fd_forecast_chains": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, ctypes.c_double, c_void_p, c_void_p,
                                   c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "fd_det_to_global_boxes": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "fd_forecast_groups": (c_int, [c_void_p, c_int, ctypes.c_double, c_void_p, c_void_p]),
    "fd_forecast_from_detections": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, ctypes.c_double, ctypes.c_double,
                                            ctypes.POINTER(ForecastBuffers), c_void_p]),
    "fd_nearest_rows": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "fd_index_pyramid": (c_int, [c_void_p, c_void_p, c_i64, c_int, c_int, ctypes.POINTER(IndexLevel), c_void_p, c_void_p, c_size_t,
                                 c_void_p]),
    "fd_index_pyramid_coords": (c_int, [c_int, c_int, ctypes.POINTER(IndexLevel), c_void_p]),
    "fd_rows_place": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_i64, c_void_p, c_int, c_void_p,
                              c_int, c_int, c_void_p]),
    "fd_sweep_assemble_workspace_bytes": (c_size_t, [c_i64]),
    "fd_sweep_assemble": (c_int, [c_void_p, c_int, c_int, c_i64, c_void_p, c_int, c_float, c_void_p, c_void_p, c_void_p,
                                  c_size_t, c_void_p]),
    "fd_deform_adapt_packed_weight_bytes": (c_size_t, [c_int]),
    "fd_deform_adapt_pack_weight": (c_int, [c_void_p, c_void_p, c_int, c_void_p]),
    "fd_deform_adapt_nhwc": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "fd_deform_adapt_backward_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "fd_deform_adapt_backward": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p,
                                         c_void_p, c_void_p, c_size_t, c_void_p]),
    "fd_deform_adapt_pack_weight_device": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p]),
    "fd_spconv_wgrad_workspace_bytes": (c_size_t, [c_int, c_i64, c_int, c_int]),
    "fd_spconv_wgrad": (c_int, [c_void_p, c_i64, c_void_p, c_void_p, c_i64, c_int, c_i64, c_void_p, c_int, c_int, c_void_p, c_void_p, c_size_t,
                                c_void_p]),
    "fd_rulebook_transpose": (c_int, [c_void_p, c_i64, c_int, c_i64, c_void_p, c_i64, c_void_p, c_i64, c_void_p]),
    "fd_spconv_pack_weight_device": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "fd_spconv_wgrad_bf16_workspace_bytes": (c_size_t, [c_int, c_i64, c_int, c_int]),
    "fd_spconv_wgrad_bf16": (c_int, [c_void_p, c_i64, c_void_p, c_void_p, c_i64, c_int, c_i64, c_void_p, c_int, c_int, c_void_p, c_void_p, c_size_t,
                                     c_void_p]),
    "fd_spconv_pack_weight_device_bf16": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "fd_conv2d_pack_weight_dev": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "fd_conv2d_wgrad_bf16_chunk": (c_int, []),
    "fd_conv2d_wgrad_bf16_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int, c_int]),
    "fd_conv2d_wgrad_bf16": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_size_t, c_void_p, c_void_p]),
    "fd_conv2d_s2_dgrad_bf16": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "fd_conv2d_wgrad_s2_bf16_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    "fd_conv2d_wgrad_s2_bf16": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_size_t, c_void_p, c_void_p]),
    "fd_conv2d_down2_bf16": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p]),
    "fd_conv2d_packed_weight_2x2_bytes": (c_size_t, [c_int, c_int, c_int]),
    "fd_conv2d_pack_weight_2x2_dev": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "fd_conv2d_wgrad_2x2_bf16_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    "fd_conv2d_wgrad_2x2_bf16": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_size_t, c_void_p, c_void_p]),
    "fd_head_tail_bf16_max_groups": (c_int, []),
    "fd_head_tail_wgrad_bf16_chunk": (c_int, []),
    "fd_head_tail_wgrad_bf16_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "fd_head_tail_forward_bf16": (c_int, [ctypes.POINTER(HeadTailGroup), c_int, c_int, c_int, c_int, c_void_p]),
    "fd_head_tail_dgrad_bf16": (c_int, [ctypes.POINTER(HeadTailGroup), c_int, c_int, c_int, c_int, c_void_p]),
    "fd_head_tail_wgrad_bf16": (c_int, [ctypes.POINTER(HeadTailGroup), c_int, c_int, c_int, c_int, c_void_p, c_size_t, c_void_p]),
    "fd_dense_gather": (c_int, [c_void_p, c_i64, c_i64, c_i64, c_i64, c_int, c_void_p, c_i64, c_void_p, c_int, c_void_p, c_void_p]),
    "fd_pillar_train_workspace_bytes": (c_size_t, [c_i64, c_int]),
    "fd_pillar_train_forward": (c_int, [c_void_p, c_void_p, c_void_p, c_i64, c_int, c_int, c_int, c_float, c_float, c_float, c_float,
                                        c_void_p, c_void_p, c_void_p, c_int, c_float, c_void_p, c_void_p, c_void_p, c_int, c_float,
                                        c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "fd_pillar_train_backward": (c_int, [c_void_p, c_void_p, c_void_p, c_i64, c_int, c_int, c_int, c_float, c_float, c_float, c_float,
                                         c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p,
                                         c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "fd_pillar_train_forward_dev": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_i64, c_int, c_int, c_int, c_float, c_float,
                                            c_float, c_float, c_void_p, c_void_p, c_void_p, c_int, c_float, c_void_p, c_void_p, c_void_p,
                                            c_int, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "fd_pillar_train_backward_dev": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_i64, c_int, c_int, c_int, c_float, c_float,
                                             c_float, c_float, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int,
                                             c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t,
                                             c_void_p]),
    "fd_pillar_train_running_stats_dev": (c_int, [c_void_p, c_void_p, c_int, ctypes.c_double, c_void_p, c_int, c_i64, c_int, c_void_p,
                                                  c_void_p, c_void_p, c_void_p]),
    "fd_targets_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "fd_assign_targets": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, ctypes.POINTER(TargetsCfg), c_void_p, c_void_p, c_void_p, c_void_p,
                                  c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "fd_optim_chunk": (c_int, []),
    "fd_optim_zero_grad": (c_int, [ctypes.POINTER(OptimTable), c_void_p]),
    "fd_optim_adam_step": (c_int, [ctypes.POINTER(OptimTable)] + [ctypes.c_double] * 6 + [c_void_p]),
    "fd_optim_adam_step_dev": (c_int, [ctypes.POINTER(OptimTable), c_void_p, c_int, c_void_p, c_void_p]),
    "fd_rows_colsum_chunk": (c_int, []),
    "fd_rows_colsum_workspace_bytes": (c_size_t, [c_i64, c_int]),
    "fd_rows_colsum": (c_int, [c_void_p, c_i64, c_void_p, c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "fd_levels_overflow": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    "fd_augment_points": (c_int, [c_void_p, c_i64, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "fd_augment_boxes": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "fd_gt_range_filter": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_float, c_float, c_float, c_void_p, c_void_p, c_void_p,
                                   c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "fd_augment_mask": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "fd_augment_mask_check": (c_int, [c_void_p, c_int, c_int, c_int]),
    "fd_gt_sample_select": (c_int, [c_void_p] * 9 + [c_int, c_int, c_i64, c_void_p, c_void_p, c_int, ctypes.c_double, c_int] + [c_void_p] * 8
                            + [c_int, c_int, c_int, c_int, c_void_p]),
    "fd_gt_sample_points": (c_int, [c_void_p, c_i64, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int,
                                    c_void_p]),
    "fd_points_in_boxes_workspace_bytes": (c_size_t, [c_i64, c_int]),
    "fd_points_in_boxes_count": (c_int, [c_void_p, c_i64, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "fd_points_in_boxes_extract": (c_int, [c_void_p, c_i64, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p, c_i64, c_int,
                                           c_void_p, c_void_p, c_void_p]),
    "fd_gt_min_points_filter": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                        c_int, c_int, c_int, c_void_p]),
    "fd_loss_chunk": (c_int, []),
    "fd_centerhead_loss_terms": (c_size_t, [ctypes.POINTER(LossCfg)]),
    "fd_centerhead_loss_workspace_bytes": (c_size_t, [ctypes.POINTER(LossCfg), c_int]),
    "fd_centerhead_loss_forward": (c_int, [ctypes.POINTER(LossCfg), ctypes.POINTER(LossTask), c_void_p, c_void_p, c_size_t, c_void_p]),
    "fd_centerhead_loss_backward": (c_int, [ctypes.POINTER(LossCfg), ctypes.POINTER(LossTask), c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "fd_sparse_bn_chunk": (c_int, []),
    "fd_sparse_bn_workspace_bytes": (c_size_t, [c_i64, c_int]),
    "fd_sparse_bn_train_forward": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_i64, c_void_p, c_int, c_int, c_float, ctypes.c_double,
                                           c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "fd_sparse_bn_train_backward": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_i64, c_void_p, c_int, c_int,
                                            c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "fd_dense_bn_chunk": (c_int, []),
    "fd_dense_bn_workspace_bytes": (c_size_t, [c_i64, c_int, c_i64]),
    "fd_dense_bn_train_forward": (c_int, [c_void_p, c_void_p, c_void_p, c_i64, c_int, c_i64, c_int, c_float, ctypes.c_double,
                                          c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "fd_dense_bn_train_backward": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_i64, c_int, c_i64, c_int,
                                           c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "fd_dense_bn_nhwc_chunk": (c_int, []),
    "fd_dense_bn_nhwc_stat_groups": (c_int, []),
    "fd_dense_bn_nhwc_apply_blocks": (c_int, []),
    "fd_dense_bn_nhwc_workspace_bytes": (c_size_t, [c_i64, c_int]),
    "fd_dense_bn_nhwc_train_forward_bf16": (c_int, [c_void_p, ctypes.POINTER(DenseBnNhwcGroup), c_int, c_i64, c_int, c_int, c_void_p, c_void_p,
                                                    c_void_p, c_size_t, c_void_p]),
    "fd_dense_bn_nhwc_train_backward_bf16": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, ctypes.POINTER(DenseBnNhwcGroup), c_int, c_i64, c_int,
                                                     c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
}
for _name in ("fd_sparse_bn_train_forward", "fd_sparse_bn_train_backward"):  # bf16 rows: the same argument lists
    SIGNATURES[_name + "_bf16"] = SIGNATURES[_name]



class FutureDetHipError(RuntimeError):
    pass


def load():
    """Loads the HIP library; raises (never falls back) when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.isfile(LIB_PATH):
            raise FutureDetHipError(
                "libfuturedet_hip.so is not built (%s). Run `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `python futuredet_amd/build.py`; there is no CPU fallback for this path." % LIB_PATH)
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)  # AttributeError = ABI mismatch, let it propagate
            fn.restype = res
            fn.argtypes = args
        if L.fd_abi_version() != ABI_VERSION:  # a stale build would read the structs below with another layout
            raise FutureDetHipError("%s reports ABI %d, these bindings are written for %d: rebuild it (python futuredet_amd/build.py --force)"
                                    % (LIB_PATH, L.fd_abi_version(), ABI_VERSION))
        _lib = L
    return _lib


def check(status, what):
    if status != 0:
        msg = load().fd_last_error()
        raise FutureDetHipError("%s failed (%d): %s" % (what, status, msg.decode() if msg else "?"))
