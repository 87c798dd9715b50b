"""The C signatures of libgsraster.so as the ctypes binding declares them: name -> (restype, argtypes), one entry per
entry point of include/gsraster.h that this package (or simple_knn) calls.  Data only: `_load()` applies the table once,
to the symbols the loaded library exports, and tests/test_signatures.py checks every entry against the header's prototype
-- parameter count, the kind of every position, the return kind.  A new entry point is declared here and nowhere else.

Every pointer parameter, struct pointers included, is a c_void_p: it takes None, an address (`tensor.data_ptr()`), a
ctypes array and `byref(...)` alike, and the header decides what it points at.
"""
import ctypes

PTR, I32, I64, U32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint32
F32, F64, INT = ctypes.c_float, ctypes.c_double, ctypes.c_int

CHUNK_FN = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_int64)   # gsr_chunk_fn


def _p(n):
    return (PTR,) * n


_OUT3 = _p(3)                 # out_color, out_objects, radii
_KEEP = _p(3)                 # ctx_out, num_rendered, stream
_AUX_KEEP = _p(5)             # ctx_out, num_rendered, out_depth, out_alpha, stream

SIGNATURES = {
    # ---- rasteriser: classic surface (settings, P, K, 8 inputs, ...)
    "gsr_forward": (INT, (PTR, I32, I32) + _p(8) + _OUT3 + _KEEP),
    "gsr_forward_aux": (INT, (PTR, I32, I32) + _p(8) + _OUT3 + _AUX_KEEP),
    "gsr_backward": (INT, _p(13)),
    # ---- raw parameters (settings, P, 7 inputs, ...)
    "gsr_forward_raw": (INT, (PTR, I32) + _p(7) + _OUT3 + _KEEP),
    "gsr_forward_raw_aux": (INT, (PTR, I32) + _p(7) + _OUT3 + _AUX_KEEP),
    "gsr_backward_raw": (INT, _p(12)),
    "gsr_backward_raw_into": (INT, _p(11) + (I32, PTR)),
    "gsr_backward_raw_chunked": (INT, _p(11) + (I32, I32, CHUNK_FN, PTR, PTR)),
    # ---- two models as one scene (settings, Pa, 7 inputs, Pb, 7 inputs, ...)
    "gsr_forward_raw2": (INT, (PTR, I32) + _p(7) + (I32,) + _p(7) + _OUT3 + _p(2)),
    "gsr_forward_raw2_keep": (INT, (PTR, I32) + _p(7) + (I32,) + _p(7) + _OUT3 + _KEEP),
    # ---- batches of views (settings[B], B, P, 6 inputs -- 7 with object features --, ...)
    "gsr_forward_raw_batch": (INT, (PTR, I32, I32) + _p(6) + _p(2) + _KEEP),
    "gsr_forward_raw_batch_aux": (INT, (PTR, I32, I32) + _p(6) + _p(2) + _AUX_KEEP),
    "gsr_forward_raw_batch_obj": (INT, (PTR, I32, I32) + _p(7) + _OUT3 + _KEEP),
    "gsr_forward_raw2_batch": (INT, (PTR, I32, I32) + _p(6) + (I32,) + _p(6) + _p(2) + _KEEP),
    "gsr_forward_raw2_batch_obj": (INT, (PTR, I32, I32) + _p(7) + (I32,) + _p(7) + _OUT3 + _KEEP),
    "gsr_backward_raw_batch_into": (INT, _p(9) + (I32, PTR)),
    "gsr_backward_raw_batch_views": (INT, _p(9) + (I64, PTR)),
    "gsr_backward_raw_batch_obj_into": (INT, _p(11) + (I32, PTR)),
    "gsr_backward_raw_batch_obj_views": (INT, _p(11) + (I64, PTR)),
    # ---- kept contexts
    "gsr_ctx_rerender": (INT, _p(8) + (U32, PTR)),
    "gsr_ctx_free": (None, (PTR,)),
    "gsr_ctx_set_aux_grads": (INT, _p(3)),
    "gsr_ctx_request_sumsq": (INT, _p(2)),
    "gsr_ctx_info": (INT, (PTR, I32, PTR)),
    "gsr_ctx_export": (INT, (PTR, I32, PTR, I64, PTR)),
    # ---- steps, visibility, neighbours
    "gsr_mark_visible": (INT, (PTR, I32) + _p(3)),
    "gsr_pgd_step": (INT, _p(3) + (I64, I32, F32, F32, I32, PTR)),
    "gsr_pgd_step_normed": (INT, _p(3) + (I64, I32, F32, F32, PTR, PTR)),
    "gsr_pgd_step_multi": (INT, (I32,) + _p(7) + (I32, PTR, PTR)),
    "gsr_adam_step_multi": (INT, (I32,) + _p(10) + (I64, PTR, I64, I64, PTR)),
    "gsr_densify_stats": (INT, _p(3) + (I32, I64) + _p(4)),
    "gsr_densify_plan_bytes": (INT, (I64, PTR)),
    "gsr_densify_plan": (INT, _p(5) + (I64, F64, F64, F64, F64, F64, I32, U32, PTR, I64, PTR, PTR)),
    "gsr_densify_plan_prune": (INT, (PTR, I64, PTR, I64, PTR, PTR)),
    "gsr_densify_apply": (INT, (PTR, I64, I64, PTR, I32) + _p(9) + (I32, U32) + _p(6)),
    "gsr_knn_dist2": (INT, (PTR, I32, PTR, PTR)),
    "gsr_knn_query": (INT, (PTR, I32, PTR, I32, I32, U32) + _p(3)),
    "gsr_knn_gather_mean": (INT, (PTR, I32, I32, I32, I32) + _p(4)),
    # ---- groups
    "gsr_group_classify": (INT, (PTR, I32, PTR, PTR, I32, PTR, I32, F32) + _p(3)),
    "gsr_convex_hull_planes": (INT, (PTR, I64, PTR, I64, PTR, PTR)),
    "gsr_points_in_hull": (INT, (PTR, I32, PTR, I32, PTR, F64) + _p(3)),
    # ---- image front end
    "gsr_image_resample": (INT, _p(4)),
    "gsr_image_resample_backward": (INT, _p(4) + (I32, PTR)),
    "gsr_image_to_u8": (INT, (PTR, I32, I32, I32, PTR, PTR)),
    # ---- detector output, detection metrics, detection loss, set-prediction detector
    "gsr_det_workspace_bytes": (INT, _p(2)),
    "gsr_det_postprocess": (INT, _p(3) + (I64,) + _p(3)),
    "gsr_det_nms": (INT, (I32, I32) + _p(4) + (F32, I32, PTR, I64) + _p(3)),
    "gsr_det_box_iou": (INT, (PTR, I32, PTR, I32, PTR, PTR)),
    "gsr_det_verdict": (INT, (PTR, PTR, I32, I32, PTR, I32, I32, I32, F32) + _p(3)),
    "gsr_deteval_workspace_bytes": (INT, (PTR, I64, PTR)),
    "gsr_deteval_match": (INT, (PTR, I32) + _p(11)),
    "gsr_deteval_accumulate": (INT, (PTR, I64) + _p(9) + (I64,) + _p(5)),
    "gsr_deteval_summarize": (INT, _p(5)),
    "gsr_detloss_workspace_bytes": (INT, _p(2)),
    "gsr_detloss": (INT, _p(5) + (I64,) + _p(5)),
    "gsr_setdet_workspace_bytes": (INT, _p(2)),
    "gsr_setdet_loss": (INT, _p(6) + (I64,) + _p(6)),
    "gsr_setdet_postprocess": (INT, _p(6)),
    # ---- two-stage detector: sampler, RoIAlign, box-head loss, output
    "gsr_rcnn_sample": (INT, _p(11)),
    "gsr_roi_align": (INT, _p(4) + (I32,) + _p(2)),
    "gsr_roi_align_backward": (INT, _p(3) + (I32,) + _p(2) + (I32, PTR)),
    "gsr_rcnn_workspace_bytes": (INT, _p(2)),
    "gsr_rcnn_loss": (INT, _p(8) + (I64,) + _p(4)),
    "gsr_rcnn_postprocess": (INT, _p(6) + (I64,) + _p(3)),
    "gsr_rpn_workspace_bytes": (INT, _p(2)),
    "gsr_rpn_select": (INT, _p(8)),
    "gsr_rpn_nms": (INT, _p(5) + (I64,) + _p(5)),
    # ---- FPN RoI pooler (features / grad_features: host arrays of device pointers)
    "gsr_fpn_pool": (INT, _p(4) + (I32,) + _p(5)),
    "gsr_fpn_pool_backward": (INT, _p(6) + (I32, PTR)),
    # ---- fused image losses
    "gsr_imgloss_workspace_bytes": (INT, _p(2)),
    "gsr_imgloss": (INT, _p(4) + (I64,) + _p(4)),
    # ---- RPN loss stage (cell_anchors / logits / deltas / grad_*: host arrays of device pointers)
    "gsr_rpnloss_workspace_bytes": (INT, _p(2)),
    "gsr_rpnloss_label": (INT, _p(5) + (I64,) + _p(5)),
    "gsr_rpnloss": (INT, _p(8) + (I64,) + _p(4)),
    # ---- object-map classifier
    "gsr_objmap_workspace_bytes": (INT, _p(2)),
    "gsr_objmap": (INT, _p(7) + (I64,) + _p(7)),
    # ---- library state, profiling, test hooks
    "gsr_query": (INT, (I32, PTR)),
    "gsr_trim_pool": (None, ()),
    "gsr_profile": (None, (I32,)),
    "gsr_profile_read": (INT, _p(2)),
    "gsr_last_error": (ctypes.c_char_p, ()),
    "gsr_test_scan": (INT, (PTR, PTR, U32, PTR)),
    "gsr_test_sort_pairs": (INT, (PTR, PTR, U32, I32, I32, I32, PTR)),
    "gsr_test_scan_ex": (INT, (PTR, PTR, U32, PTR, PTR, U32, U32, PTR)),
    "gsr_test_sort_pairs_ex": (INT, (PTR, PTR, U32, PTR, I32, I32, I32, I32, PTR, U32, PTR)),
}
