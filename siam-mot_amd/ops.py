"""ctypes binding of ``csrc/libsmot_emm.so`` (C ABI: include/smot_emm.h) + tensor-level operators.

This is the ONLY compute path of the package: there is no CPU / eager fallback.  If the HIP
library is missing or a tensor is not a contiguous fp32 device tensor, the call raises.  The FPN maps alone may also be
fp16 or bf16 (a backbone under ``torch.autocast`` or ``.half()``): the ``smot_*_typed_fwd`` entry points read them as
they are and return bit for bit what the call returns on ``maps.float()``; everything else stays fp32.

Operator ↔ reference map (reference paths relative to amazon-science/siam-mot):
    roi_align_levels   SRPooler.forward            EMM/sr_pool.py:53-91 (+ track_utils.py:87-107 pad)
    search_region      update_boxes_in_pad_images  track_head/track_utils.py:109-135 + extend_bbox :62-85
    xcorr_depthwise    xcorr_depthwise             EMM/xcorr.py:37-46
    emm_predictor      EMMPredictor.forward        EMM/feature_extractor.py:62-69
    emm_decode         3x F.interpolate + get_locations + decode_response   EMM/track_core.py:69-77
"""
import array as _array
import contextlib
import ctypes
import struct
import weakref
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libsmot_emm.so")
# measurement build (-DSMOT_DEBUG): older kernel generations, A/B switches, timing ablations.  Never loaded
# implicitly — only through ``debug_library()`` (tools/, A/B tests).
DEBUG_LIB_PATH = os.path.join(_HERE, "csrc", "libsmot_emm_debug.so")
ABI_VERSION = 14
UP_SCALE = 16          # reference track_core.py:69-73


_lib = None
_c_float_p = ctypes.POINTER(ctypes.c_float)
_vp = ctypes.c_void_p
_i = ctypes.c_int
_f = ctypes.c_float

_SIGNATURES = {
    "smot_abi_version": (ctypes.c_int, []),
    "smot_build_info": (ctypes.c_int, []),
    "smot_last_error": (ctypes.c_char_p, []),
    "smot_roi_align_levels_fwd": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _i, _i, _i, _i,
                                                 _vp, _vp, _vp]),
    "smot_roi_align_fwd": (ctypes.c_int, [_vp, _i, _i, _i, _i, _i, _vp, _i, _f, _i, _i, _i, _vp, _vp]),
    "smot_search_region_fwd": (ctypes.c_int, [_vp, _i, _f, _f, _f, _vp, _vp]),
    "smot_xcorr_dw_fwd": (ctypes.c_int, [_vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "smot_emm_predictor_fwd": (ctypes.c_int, [_vp, _i, _i, _i] + [_vp] * 12 + [_i, _f, _vp, _vp, _vp, _vp]),
    "smot_debug_trace": (None, [_vp]),
    "smot_emm_tower_pack_floats": (ctypes.c_longlong, [_i]),
    "smot_emm_tower_form": (ctypes.c_int, [_i, _i, _i]),
    "smot_emm_tower_pack": (ctypes.c_int, [_vp, _vp, _i, _vp, _vp]),
    "smot_emm_decode_fwd": (ctypes.c_int, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _f, _f, _i, _f, _f,
                                           _vp, _vp, _vp, _vp, _vp]),
    "smot_emm_decode_ws_floats": (ctypes.c_int, [_i, _i]),
    "smot_sr_xcorr_fused_fwd": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _i, _i, _i, _i,
                                               _vp, _vp, _vp]),
    "smot_sr_xcorr_gather_fwd": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    "smot_preprocess_fwd": (ctypes.c_int, [_vp, _i, _i, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _i, _vp, _vp]),
    # the frames of several cameras in one call: host arrays of per-image pointers / sizes, one output size and tensor
    "smot_preprocess_batch_fwd": (ctypes.c_int, [_i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _i,
                                                 _vp, _i, _vp]),
    "smot_nms_ws_bytes": (ctypes.c_longlong, [_i]),
    "smot_nms_fwd": (ctypes.c_int, [_vp, _i, _f, _vp, _vp, _vp]),
    "smot_xcorr_timer_begin": (ctypes.c_int, [_i]),
    "smot_xcorr_timer_end": (ctypes.c_int, [_vp, _vp]),
    "smot_kernel_timer_begin": (ctypes.c_int, [_i, _i, _i]),
    "smot_kernel_timer_bracket_overhead": (ctypes.c_int, [_vp, _i, _vp]),
    "smot_dispatch_floor_fwd": (ctypes.c_int, [_i, _i, _vp]),
    "smot_kernel_timer_end": (ctypes.c_int, [_i, _vp, _vp]),
    "smot_emm_track_ws_floats": (ctypes.c_longlong, [_i, _i, _i, _i]),
    "smot_emm_track_fwd": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _i, _i, _i, _i,
                                          _vp, _i, _f, _vp, _i, _f, _f, _f, _i, _f, _f, _vp, _vp, _vp, _vp, _vp, _vp]),
    "smot_emm_order_hint_floats": (ctypes.c_longlong, [_i, _i, _i]),
    "smot_emm_extract_cache_fwd": (ctypes.c_int, [_vp, _vp, _vp, _vp, _i, _i, _vp, _i, _i, _i, _f, _f, _f,
                                                  _vp, _vp, _vp, _vp]),
    "smot_emm_extract_cache_masked_fwd": (ctypes.c_int, [_vp, _vp, _vp, _vp, _i, _i, _vp, _i, _vp, _i, _i, _f, _f, _f,
                                                         _vp, _vp, _vp, _vp]),
    "smot_box_refine_post_max_rows": (ctypes.c_int, []),
    "smot_box_refine_post_fwd": (ctypes.c_int, [_vp, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _f, _f, _f, _f, _f, _f, _f, _i,
                                                _vp, _vp, _vp, _vp, _vp]),
    "smot_box_refine_ws_floats": (ctypes.c_longlong, [_i, _i, _i, _i, _i, _i, _i]),
    "smot_box_refine_fwd": (ctypes.c_int, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _i,
                                           _vp, _vp, _i, _vp, _vp, _i, _vp, _vp, _i, _vp, _vp, _i,
                                           _f, _f, _f, _f, _f, _f, _f, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "smot_linear_rows_max_rows": (ctypes.c_int, []),
    "smot_linear_rows_ws_floats": (ctypes.c_longlong, [_i, _i, _i]),
    "smot_linear_rows_fwd": (ctypes.c_int, [_vp, _i, _i, _vp, _vp, _i, _i, _vp, _vp, _i, _vp]),
    "smot_track_frame_fwd": (ctypes.c_int, [_vp, _vp]),
    "smot_track_solve_max_boxes": (ctypes.c_int, []),
    "smot_emm_order_hint_status": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "smot_memory_carry_max_rows": (ctypes.c_int, []),
    "smot_memory_carry_fwd": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _i, _i,
                                             _vp, _i, _vp]),
    "smot_track_solve_fwd": (ctypes.c_int, [_vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _i, _f, _f, _f, _f, _f, _i,
                                            _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "smot_track_solve_carry_fwd": (ctypes.c_int, [_vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _i, _f, _f, _f, _f, _f, _i,
                                                  _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                                  _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _i, _vp]),
    # several images per call (ABI 14): the single-image twins' arguments + num_images, row_start (host int array)
    "smot_emm_track_batched_fwd": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _i, _i, _i, _i,
                                                  _vp, _i, _f, _vp, _i, _f, _f, _f, _i, _f, _f, _vp, _vp, _vp, _vp, _vp, _vp,
                                                  _i, _vp]),
    "smot_emm_extract_cache_batched_fwd": (ctypes.c_int, [_vp, _vp, _vp, _vp, _i, _i, _vp, _i, _i, _i, _f, _f, _f,
                                                          _vp, _vp, _vp, _vp, _i, _vp]),
    # fp16 / bf16 feature maps: the twins' arguments with `feat_type` behind the maps (track / extract_cache: the batched
    # signatures; extract_cache + n_valid)
    "smot_roi_align_levels_typed_fwd": (ctypes.c_int, [_vp, _i, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _i, _i, _i, _i,
                                                       _vp, _vp, _vp]),
    "smot_roi_align_typed_fwd": (ctypes.c_int, [_vp, _i, _i, _i, _i, _i, _i, _vp, _i, _f, _i, _i, _i, _vp, _vp]),
    "smot_sr_xcorr_fused_typed_fwd": (ctypes.c_int, [_vp, _i, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _i, _i, _i, _i,
                                                     _vp, _vp, _vp]),
    "smot_sr_xcorr_gather_typed_fwd": (ctypes.c_int, [_vp, _i, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _i, _i, _i, _i,
                                                      _vp, _vp]),
    "smot_emm_track_typed_fwd": (ctypes.c_int, [_vp, _i, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _i, _i, _i, _i,
                                                _vp, _i, _f, _vp, _i, _f, _f, _f, _i, _f, _f, _vp, _vp, _vp, _vp, _vp, _vp,
                                                _i, _vp]),
    "smot_emm_extract_cache_typed_fwd": (ctypes.c_int, [_vp, _i, _vp, _vp, _vp, _i, _i, _vp, _i, _i, _i, _f, _f, _f,
                                                        _vp, _vp, _vp, _vp, _i, _vp, _vp]),
    "smot_box_refine_typed_fwd": (ctypes.c_int, [_vp, _i, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _i,
                                                 _vp, _vp, _i, _vp, _vp, _i, _vp, _vp, _i, _vp, _vp, _i,
                                                 _f, _f, _f, _f, _f, _f, _f, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "smot_track_frame_typed_fwd": (ctypes.c_int, [_vp, _i, _vp]),
    # RPN proposal selection: all images and levels of a call in one set of launches
    "smot_rpn_proposals_ws_bytes": (ctypes.c_longlong, [_i, _i, _vp, _vp, _vp, _i, _i]),
    "smot_rpn_proposals_fwd": (ctypes.c_int, [_vp, _vp, _i, _vp, _vp, _vp, _i, _i, _vp, _vp, _i, _i, _i, _f, _f, _i,
                                              _f, _f, _f, _f, _f, _vp, _vp, _vp, _vp, _vp]),
    # box-head post-processing of the detections (proposals without ids): four launches, no host synchronisation
    "smot_box_detect_post_ws_bytes": (ctypes.c_longlong, [_i, _i]),
    "smot_box_detect_post_fwd": (ctypes.c_int, [_vp, _i, _i, _i, _vp, _vp, _i, _f, _f, _f, _f, _f, _f, _f, _f, _f, _vp,
                                                _vp, _vp, _vp, _vp, _vp, _vp]),
    # the box head over several images: the twins' arguments + num_images, row_start (host int array)
    "smot_roi_align_levels_batched_typed_fwd": (ctypes.c_int, [_vp, _i, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _i, _i, _i, _i,
                                                               _vp, _vp, _vp, _i, _vp]),
    "smot_box_detect_post_batched_ws_bytes": (ctypes.c_longlong, [_i, _vp, _i]),
    "smot_box_detect_post_batched_fwd": (ctypes.c_int, [_vp, _i, _i, _i, _vp, _vp, _i, _f, _f, _f, _f, _f, _f, _f, _f, _f, _vp,
                                                        _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp]),
    # the track solver over several images: num_images, smot_track_solve_fwd's 27 arguments as host arrays, stream
    "smot_track_solve_batched_fwd": (ctypes.c_int, [_i] + [_vp] * 27 + [_vp]),
    # the refinement of the propagated tracks over several images: the twins' arguments + num_images, row_start (host int array)
    "smot_box_refine_batched_max_rows": (ctypes.c_int, []),
    "smot_box_refine_batched_ws_floats": (ctypes.c_longlong, [_i, _i, _i, _i, _i, _i, _i]),
    "smot_box_refine_post_batched_fwd": (ctypes.c_int, [_vp, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _f, _f, _f, _f, _f, _f, _f, _i,
                                                        _vp, _vp, _vp, _vp, _vp, _i, _vp]),
    "smot_box_refine_batched_typed_fwd": (ctypes.c_int, [_vp, _i, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _i,
                                                         _vp, _vp, _i, _vp, _vp, _i, _vp, _vp, _i, _vp, _vp, _i,
                                                         _f, _f, _f, _f, _f, _f, _f, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp]),
    # RPN head (conv3x3 + ReLU + the two 1x1 heads) and anchor grid: all images and levels of a call in one launch each
    "smot_rpn_head_packed_floats": (ctypes.c_longlong, [_i, _i]),
    "smot_rpn_head_pack": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp]),
    "smot_rpn_head_fwd": (ctypes.c_int, [_vp, _i, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "smot_rpn_anchors_fwd": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _i, _vp, _vp]),
    # feature pyramid: backbone stage maps to the FPN maps of all images in num_levels + 1 launches
    "smot_fpn_packed_floats": (ctypes.c_longlong, [_i, _vp, _i]),
    "smot_fpn_pack": (ctypes.c_int, [_vp, _vp, _vp, _vp, _i, _vp, _i, _vp, _vp]),
    "smot_fpn_ws_bytes": (ctypes.c_longlong, [_i, _vp, _vp, _i, _i]),
    "smot_fpn_fwd": (ctypes.c_int, [_vp, _i, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _i, _i, _vp]),
    # DLA backbone body: an image batch to the four stage maps; and its three operators alone
    "smot_dla_packed_floats": (ctypes.c_longlong, [_vp, _vp]),
    "smot_dla_pack": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _i, _vp, _vp]),
    "smot_dla_ws_bytes": (ctypes.c_longlong, [_vp, _vp, _i, _i, _i]),
    "smot_dla_fwd": (ctypes.c_int, [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp]),
    "smot_dla_conv_packed_floats": (ctypes.c_longlong, [_i, _i, _i]),
    "smot_dla_conv3x3_fwd": (ctypes.c_int, [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _i, _i, _vp, _i, _i, _i, _vp, _vp, _vp]),
    "smot_dla_conv3x3_form": (ctypes.c_int, [_i, _i, _i, _i, _i]),
    "smot_dla_conv1x1_fwd": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _i, _i, _vp, _vp, _i, _vp]),
    "smot_dla_stem_ws_bytes": (ctypes.c_longlong, [_i, _i, _i, _i, _i]),
    "smot_dla_stem_fwd": (ctypes.c_int, [_vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "smot_dla_split_packed_floats": (ctypes.c_longlong, [_vp, _vp]),
    "smot_dla_split_pack": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _i, _vp, _vp]),
    "smot_dla_split_fwd": (ctypes.c_int, [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp]),
    "smot_dla_conv_split_packed_floats": (ctypes.c_longlong, [_i, _i, _i]),
    "smot_dla_conv3x3_split_fwd": (ctypes.c_int, [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _i, _i, _vp, _i, _i, _i, _vp, _vp, _vp]),
    "smot_dla_conv3x3_split_form": (ctypes.c_int, [_i, _i, _i, _i, _i]),
    # DLA bodies of either block type and any tree depth (DLA-46-C / 60 / 102 / 169), and the 1x1 operator with a residual
    "smot_dla_net_num_convs": (ctypes.c_int, [_vp, _vp, _i]),
    "smot_dla_net_packed_floats": (ctypes.c_longlong, [_vp, _vp, _i, _i, _i]),
    "smot_dla_net_pack": (ctypes.c_int, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp, _i, _vp, _vp]),
    "smot_dla_net_ws_bytes": (ctypes.c_longlong, [_vp, _vp, _i, _i, _i, _i, _i]),
    "smot_dla_net_fwd": (ctypes.c_int, [_vp, _i, _i, _i, _i, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _i, _vp]),
    "smot_dla_conv1x1_res_fwd": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _i, _i, _vp, _i, _i, _vp, _vp,
                                                _i, _vp]),
    # DLA bodies in half compute mode: every tree convolution with fp16 / bf16 operands on the 16-bit matrix instruction
    "smot_dla_half_packed_floats": (ctypes.c_longlong, [_vp, _vp, _i, _i, _i]),
    "smot_dla_half_pack": (ctypes.c_int, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp, _i, _vp, _vp]),
    "smot_dla_half_fwd": (ctypes.c_int, [_vp, _i, _i, _i, _i, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _i, _vp]),
    "smot_dla_conv_half_packed_floats": (ctypes.c_longlong, [_i, _i, _i]),
    "smot_dla_conv3x3_half_fwd": (ctypes.c_int, [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _i, _i, _vp, _i, _i, _i, _i, _vp, _vp, _vp]),
    "smot_dla_conv3x3_half_form": (ctypes.c_int, [_i, _i, _i, _i, _i]),
    "smot_dla_conv1x1_half_form": (ctypes.c_int, [_i, _i, _i, _i]),
    "smot_dla_conv1x1_half_fwd": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _i, _i, _vp, _i, _i, _i, _vp,
                                                 _vp, _i, _vp]),
    # DLA bodies in half compute mode with the maps between layers stored in the compute type
    "smot_dla_half_storage_ws_bytes": (ctypes.c_longlong, [_vp, _vp, _i, _i, _i, _i, _i, _i]),
    "smot_dla_half_storage_fwd": (ctypes.c_int, [_vp, _i, _i, _i, _i, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "smot_dla_conv3x3_half_storage_fwd": (ctypes.c_int, [_vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _i, _i, _vp, _i, _i, _i, _i, _i,
                                                         _vp, _vp, _vp]),
    "smot_dla_conv1x1_half_storage_fwd": (ctypes.c_int, [_vp, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _i, _i, _vp, _i,
                                                         _i, _i, _i, _vp, _vp, _vp]),
    # FPN and RPN head in half compute mode: the fp32 twins' arguments + compute_type
    "smot_fpn_half_packed_floats": (ctypes.c_longlong, [_i, _vp, _i, _i]),
    "smot_fpn_half_pack": (ctypes.c_int, [_vp, _vp, _vp, _vp, _i, _vp, _i, _i, _vp, _vp]),
    "smot_fpn_half_fwd": (ctypes.c_int, [_vp, _i, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _i, _i, _vp]),
    "smot_rpn_head_half_packed_floats": (ctypes.c_longlong, [_i, _i, _i]),
    "smot_rpn_head_half_pack": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp]),
    "smot_rpn_head_half_fwd": (ctypes.c_int, [_vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp]),
}
EXPORTED_SYMBOLS = tuple(_SIGNATURES.keys())
_DEBUG_SIGNATURES = {
    "smot_debug_set_knob": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_char_p]),
    "smot_debug_sr_xcorr_fused_hint_fwd": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp]),
    "smot_debug_linear_rows_blocks_ws_floats": (ctypes.c_longlong, [_i, _i, _i]),
    "smot_debug_linear_rows_blocks_fwd": (ctypes.c_int, [_vp, _i, _i, _vp, _vp, _i, _i, _vp, _vp, _i, _vp]),
}
DEBUG_EXPORTED_SYMBOLS = tuple(_DEBUG_SIGNATURES.keys())


def load_library(path=None):
    """dlopen the HIP library (after torch, so both share one libamdhip64) and type its symbols."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    path = path or LIB_PATH
    if not os.path.exists(path):
        raise RuntimeError(
            "siammot_amd: HIP library %s not found — build it with `python siam-mot_amd/build.py` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback." % path)
    _lib = _open(path, _SIGNATURES)
    return _lib


def _open(path, signatures):
    lib = ctypes.CDLL(path)
    for name, (res, args) in signatures.items():
        fn = getattr(lib, name)          # AttributeError if the symbol is missing
        fn.restype = res
        fn.argtypes = args
    if lib.smot_abi_version() != ABI_VERSION:
        raise RuntimeError("siammot_amd: %s has ABI %d, host layer expects %d"
                           % (path, lib.smot_abi_version(), ABI_VERSION))
    return lib


_KNOB_DEFAULTS = {"SMOT_NO_FUSE": "0", "SMOT_ROI_GENERIC": "0", "SMOT_TOWER_DIRECT": "0", "SMOT_TOWER_WIDE": "0",
                  "SMOT_DECODE_SPLIT": "0", "SMOT_XCORR_VARIANT": "default", "SMOT_DECODE_2PASS": "0",
                  "SMOT_FUSED_GEN": "0", "SMOT_TOWER_OCT": "0", "SMOT_TOWER_BF3": "1", "SMOT_FUSED_ORDER": "0", "SMOT_NO_HINT": "0", "SMOT_FUSED_ABL": "0",
                  "SMOT_ANY_ORDER": "0",
                  "SMOT_WINO_ABL": "0",
                  "SMOT_TOWER_ABL": "0"}


@contextlib.contextmanager
def debug_library(**knobs):
    """Measurement build as the current library inside the block (tools/ and A/B tests only), with the given
    switches set (``debug_library(SMOT_XCORR_VARIANT="mfma")``; names as in csrc/knobs.h) and every switch
    back at its default afterwards.  The product library is restored on exit."""
    global _lib
    if not os.path.exists(DEBUG_LIB_PATH):
        raise RuntimeError("siammot_amd: measurement library %s not built (python siam-mot_amd/build.py)" % DEBUG_LIB_PATH)
    load_library()                                  # make sure the product handle exists to return to
    dbg = _open(DEBUG_LIB_PATH, dict(_SIGNATURES, **_DEBUG_SIGNATURES))
    if not (dbg.smot_build_info() & 1):
        raise RuntimeError("siammot_amd: %s is not a measurement build" % DEBUG_LIB_PATH)
    prev, _lib = _lib, dbg

    def set_all(values):
        for k, v in values.items():
            if dbg.smot_debug_set_knob(k.encode(), str(v).encode()) != 0:
                raise RuntimeError("siammot_amd: " + dbg.smot_last_error().decode("utf-8", "replace"))
    try:
        set_all(_KNOB_DEFAULTS)
        set_all(knobs)
        _hint_floats.clear()                        # (answers of the library that depend on its switches)
        yield dbg
    finally:
        set_all(_KNOB_DEFAULTS)
        _lib = prev
        _hint_floats.clear()


def _check(rc, what):
    if rc != 0:
        msg = _lib.smot_last_error().decode("utf-8", "replace")
        raise RuntimeError("siammot_amd.%s failed (code %d): %s" % (what, rc, msg))


def _dev_f32(t, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError("siammot_amd: %s must be a device (ROCm) tensor — no CPU path exists" % name)
    if t.dtype != torch.float32:
        raise RuntimeError("siammot_amd: %s must be float32, got %s" % (name, t.dtype))
    return t if t.is_contiguous() else t.contiguous()


# element types of the feature MAPS (SMOT_FEAT_* of include/smot_emm.h); everything else is fp32
FEAT_TYPES = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}


def _dev_feat(t, name):
    """``_dev_f32`` for a feature map: fp16 and bf16 pass as they are (no copy, no cast)."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError("siammot_amd: %s must be a device (ROCm) tensor — no CPU path exists" % name)
    if t.dtype not in FEAT_TYPES:
        raise RuntimeError("siammot_amd: %s must be float32 (or a float16 / bfloat16 feature map), got %s" % (name, t.dtype))
    return t if t.is_contiguous() else t.contiguous()


# layout flag of the maps, OR'ed into the typed entry points' ``feat_type`` (SMOT_FEAT_CHANNELS_LAST): the levels are
# ``[B, C, H, W]`` tensors whose memory is ``[B, H, W, C]`` and are read in place
FEAT_CHANNELS_LAST = 16
_CL = torch.channels_last


def maps_layout(t):
    """``FEAT_CHANNELS_LAST`` for a map the library reads as channels-last, 0 for NCHW and for everything else (which is
    passed as NCHW: contiguous as it is, a strided view through a copy).  Channels-last: 4-D, NOT contiguous, and
    contiguous in ``torch.channels_last`` — a tensor that is both (C == 1, or H == W == 1) is NCHW."""
    return FEAT_CHANNELS_LAST if (t.dim() == 4 and not t.is_contiguous() and t.is_contiguous(memory_format=_CL)) else 0


def _levels_layout(features, L):
    """The layout word of a call: ``FEAT_CHANNELS_LAST`` only when EVERY level is channels-last, C % 8 == 0 and the level
    starts at a 16-byte boundary (a pixel's channel runs are then 16-byte aligned); any mix of layouts, other strides,
    another C or a view at an odd offset -> 0, the call as it ever was (such maps are copied)."""
    for l in range(L):
        f = features[l]
        if not (isinstance(f, torch.Tensor) and f.dim() == 4 and f.shape[1] % 8 == 0 and not f.is_contiguous()
                and f.is_contiguous(memory_format=_CL) and f.data_ptr() % 16 == 0):
            return 0
    return FEAT_CHANNELS_LAST


def _dev_feats(features, L, nhwc=True):
    """The ``L`` levels as the library takes them, and their ``feat_type`` word: channels-last levels (``_levels_layout``;
    ``nhwc=False``: the entry has no channels-last form) pass as they are with the flag set, anything else through
    ``_dev_feat``."""
    if nhwc and _levels_layout(features, L):
        feats = [features[l] for l in range(L)]
        for l, f in enumerate(feats):
            if not f.is_cuda:
                raise RuntimeError("siammot_amd: features[%d] must be a device (ROCm) tensor — no CPU path exists" % l)
            if f.dtype not in FEAT_TYPES:
                _dev_feat(f, "features[%d]" % l)            # raises
        return feats, _feat_type(feats) | FEAT_CHANNELS_LAST
    feats = [_dev_feat(features[l], "features[%d]" % l) for l in range(L)]
    return feats, _feat_type(feats)


def _feat_type(feats):
    """The one element type of a call's maps (each passed ``_dev_feat``) -> SMOT_FEAT_*; mixed levels raise."""
    dt = feats[0].dtype
    for l, f in enumerate(feats):
        if f.dtype is not dt:
            raise RuntimeError("siammot_amd: all feature levels of one call must share one dtype, got %s (features[0]) and %s "
                               "(features[%d])" % (dt, f.dtype, l))
    return FEAT_TYPES[dt]


def _one_image_rows(N):
    """``row_start`` of a typed call on one image."""
    return (ctypes.c_int * 2)(0, N)


try:
    _raw_stream = torch._C._cuda_getCurrentRawStream         # (device index) -> hipStream_t as int, ~0.2 us
except AttributeError:                                        # pragma: no cover - older torch
    _raw_stream = None


def _stream(device=None):
    """The current torch stream of ``device`` as a raw handle (launches are enqueued on it)."""
    if _raw_stream is not None:
        idx = device.index if (device is not None and device.index is not None) else torch.cuda.current_device()
        return ctypes.c_void_p(_raw_stream(idx))
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


class StreamImage(object):
    """A device image that is computed once and kept (packed weights, anchor grids), ordered for every stream that reads it.
    ``produce()`` enqueues the image on the current stream of ``device`` and returns its tensor or list of tensors; the image
    carries that stream's raw handle and an event recorded right behind the producing launch.  ``get()`` returns the
    tensor(s) for a consumer that launches on the current stream: on the producing stream that is one raw-stream lookup and
    an integer compare; on any other stream the stream first waits for the event (on the device: no host synchronisation)
    and the tensors are marked as used by it (``Tensor.record_stream``), so that dropping the image on a repack cannot hand
    its block out again under a kernel that still reads it."""
    __slots__ = ("value", "device", "stream", "event")

    def __init__(self, produce, device):
        self.device = device
        self.stream = _stream(device).value
        self.value = produce()
        self.event = torch.cuda.Event()
        self.event.record(torch.cuda.current_stream(device))

    def get(self):
        if _stream(self.device).value != self.stream:
            current = torch.cuda.current_stream(self.device)
            current.wait_event(self.event)
            for t in (self.value if isinstance(self.value, (list, tuple)) else (self.value,)):
                t.record_stream(current)
        return self.value


class _Launch(object):
    """Launch context of one binding: every tensor must live on ONE device, that device is made current for
    the duration of the call (hipLaunchKernelGGL launches on the CURRENT device — a stream handle of another
    device would be invalid there), and ``stream`` is that device's current torch stream.  A no-op switch when
    the device is current already (the common case: ~0.5 us)."""
    __slots__ = ("dev", "prev", "stream")

    def __init__(self, *tensors):
        dev = None
        for t in tensors:
            if t is None:
                continue
            if not (isinstance(t, torch.Tensor) and t.is_cuda):
                raise RuntimeError("siammot_amd: inputs must be device (ROCm) tensors — no CPU path exists")
            if dev is None:
                dev = t.device
            elif t.device != dev:
                raise RuntimeError("siammot_amd: inputs live on different devices (%s and %s)" % (dev, t.device))
        if dev is None:
            raise RuntimeError("siammot_amd: no device tensor among the inputs")
        self.dev = dev
        self.prev = None
        self.stream = None

    def __enter__(self):
        cur = torch.cuda.current_device()
        if cur != self.dev.index:
            self.prev = cur
            torch.cuda.set_device(self.dev.index)
        self.stream = _stream(self.dev)
        return self

    def __exit__(self, *exc):
        if self.prev is not None:
            torch.cuda.set_device(self.prev)
        return False


# ----------------------------------------------------------------------------------------------
def roi_align_levels(features, rois, level_boxes, out_size, scales, sampling_ratio, pad_cells=None,
                     return_levels=False):
    """Level-routed legacy ROIAlign on one image with virtual zero padding.

    features: sequence of ``[1,C,H_l,W_l]`` tensors (only the first ``len(scales)`` are used, as the
    reference's ``zip(x, self.poolers)``); rois ``[R,4]`` xyxy in padded-image pixels; level_boxes
    ``[R,4]`` (template boxes) choose the level; pad_cells: per-level virtual padding in cells.
    Returns ``[R,C,out_size,out_size]`` (and int32 levels when asked).
    """
    lib = load_library()
    L = len(scales)
    feats, fp, hs, ws, sc, ft = _level_arrays(features, scales, what=".roi_align_levels")
    C = feats[0].shape[1]
    rois = _dev_f32(rois, "rois")
    level_boxes = rois if level_boxes is None else _dev_f32(level_boxes, "level_boxes")
    R = rois.shape[0]
    if pad_cells is None:
        pad_cells = [0] * L
    out = torch.empty((R, C, out_size, out_size), dtype=torch.float32, device=rois.device)
    levels = torch.empty((R,), dtype=torch.int32, device=rois.device) if return_levels else None
    pc = (ctypes.c_int * L)(*[int(p) for p in pad_cells[:L]])
    with _Launch(rois, level_boxes, *feats) as ln:
        rc = lib.smot_roi_align_levels_typed_fwd(_cast(fp), ft, _cast(hs), _cast(ws), _cast(pc), _cast(sc), L, C,
                                                 _ptr(rois), _ptr(level_boxes), R, out_size, out_size,
                                                 int(sampling_ratio), _ptr(out), _ptr(levels), ln.stream)
    _check(rc, "roi_align_levels")
    return (out, levels) if return_levels else out


def roi_align(input, rois, spatial_scale, pooled_h, pooled_w, sampling_ratio, pad_cells=0):
    """[UPSTREAM] ``_C.roi_align_forward(input, rois, spatial_scale, pooled_h, pooled_w, sampling_ratio)``: one feature
    level ``[B,C,H,W]``, rois ``[R,5]`` = (image index, x1, y1, x2, y2) -> ``[R,C,pooled_h,pooled_w]``, allocated here
    in fp32 (a half ``input`` is read as it is; upstream's ``ROIAlign.forward`` is an ``amp.float_function``).  ``pad_cells`` > 0: virtual zero border (rois in padded coordinates)."""
    lib = load_library()
    _dev_feat(input, "input") if not isinstance(input, torch.Tensor) else None        # (raises: not a tensor)
    (input,), ft = _dev_feats((input,), 1)
    rois = _dev_f32(rois, "rois")
    if input.dim() != 4 or rois.dim() != 2 or rois.shape[1] != 5:
        raise RuntimeError("siammot_amd.roi_align: input must be [B,C,H,W] and rois [R,5], got %s and %s"
                           % (tuple(input.shape), tuple(rois.shape)))
    B, C, H, W = input.shape
    R = rois.shape[0]
    out = torch.empty((R, C, int(pooled_h), int(pooled_w)), dtype=torch.float32, device=input.device)
    with _Launch(input, rois) as ln:
        rc = lib.smot_roi_align_typed_fwd(_ptr(input), ft, B, C, H, W, int(pad_cells), _ptr(rois), R,
                                          float(spatial_scale), int(pooled_h), int(pooled_w), int(sampling_ratio),
                                          _ptr(out), ln.stream)
    _check(rc, "roi_align")
    return out


def search_region(boxes, pad_pixels, search_expansion, min_search_wh):
    """Template boxes ``[N,4]`` → search regions ``[N,4]`` in padded-image coordinates."""
    lib = load_library()
    boxes = _dev_f32(boxes, "boxes")
    sr = torch.empty_like(boxes)
    with _Launch(boxes) as ln:
        rc = lib.smot_search_region_fwd(_ptr(boxes), boxes.shape[0], float(pad_pixels), float(search_expansion),
                                        float(min_search_wh), _ptr(sr), ln.stream)
    _check(rc, "search_region")
    return sr


def xcorr_depthwise(x, kernel):
    """Same contract as the reference ``xcorr_depthwise(x, kernel)`` (EMM/xcorr.py:37-46)."""
    lib = load_library()
    x = _dev_f32(x, "x")
    kernel = _dev_f32(kernel, "kernel")
    if x.dim() != 4 or kernel.dim() != 4 or x.shape[:2] != kernel.shape[:2] \
            or x.shape[2] != x.shape[3] or kernel.shape[2] != kernel.shape[3]:
        raise RuntimeError("siammot_amd.xcorr_depthwise: need x [N,C,Rx,Rx] and kernel [N,C,Rz,Rz], got %s, %s"
                           % (tuple(x.shape), tuple(kernel.shape)))
    N, C, Rx, _ = x.shape
    Rz = kernel.shape[2]
    out = torch.empty((N, C, Rx - Rz + 1, Rx - Rz + 1), dtype=torch.float32, device=x.device)
    with _Launch(x, kernel) as ln:
        rc = lib.smot_xcorr_dw_fwd(_ptr(x), _ptr(kernel), _ptr(out), N, C, Rx, Rz, ln.stream)
    _check(rc, "xcorr_depthwise")
    return out


PREDICTOR_KEYS = (
    "cls_tower.0.weight", "cls_tower.1.weight", "cls_tower.1.bias",
    "reg_tower.0.weight", "reg_tower.1.weight", "reg_tower.1.bias",
    "cls.weight", "cls.bias", "center.weight", "center.bias", "reg.weight", "reg.bias",
)


_TOWER_KEYS = ("cls_tower.0.weight", "reg_tower.0.weight")
_KEY_INDEX = {k: i for i, k in enumerate(PREDICTOR_KEYS)}
_pack_cache = {}


def tower_packed(params):
    """Winograd-transformed tower filters (``smot_emm_tower_pack``) for the matrix-core tower kernel, cached per
    pair of weight tensors and recomputed when either is modified in place (``load_state_dict``) or replaced
    (``.to()``).  ``None`` when the channel count has no packed path."""
    lib = load_library()
    wc = _dev_f32(params["cls_tower.0.weight"], "cls_tower.0.weight")
    wr = _dev_f32(params["reg_tower.0.weight"], "reg_tower.0.weight")
    C = wc.shape[0]
    nfl = lib.smot_emm_tower_pack_floats(C)
    if nfl == 0 or tuple(wc.shape) != (C, C, 3, 3) or tuple(wr.shape) != (C, C, 3, 3):
        return None
    # Keyed on the tensor OBJECTS (weak references), not on addresses: the caching allocator hands the address
    # of a freed weight tensor to the next model's weights, and version counters restart with every tensor.
    key = (wc.data_ptr(), wr.data_ptr())
    ver = (wc._version, wr._version)
    hit = _pack_cache.get(key)
    if hit is not None and hit[0]() is wc and hit[1]() is wr and hit[2] == ver:
        return hit[3]
    packed = torch.empty((nfl,), dtype=torch.float32, device=wc.device)
    with _Launch(wc, wr) as ln:
        _check(lib.smot_emm_tower_pack(_ptr(wc), _ptr(wr), C, _ptr(packed), ln.stream), "tower_pack")
    # the image is cached and may be consumed from another stream: finish it now (once per weight set)
    torch.cuda.current_stream(wc.device).synchronize()
    for k in [k for k, v in _pack_cache.items() if v[0]() is None or v[1]() is None]:
        del _pack_cache[k]
    _pack_cache[key] = (weakref.ref(wc), weakref.ref(wr), ver, packed)
    return packed


def emm_predictor(resp, params, gn_groups=32, gn_eps=1e-5, winograd=True):
    """``resp [N,C,Ho,Ho]`` + reference-keyed ``params`` → logits ``[N,7,Ho,Ho]``
    (cls0, cls1, center, reg l/t/r/b; reg already ReLU'd).  ``winograd=False`` forces the direct fp32
    tower kernel (same result up to fp32 rounding order)."""
    lib = load_library()
    resp = _dev_f32(resp, "resp")
    N, C, Ho, _ = resp.shape
    w = [_dev_f32(params[k], k) for k in PREDICTOR_KEYS]
    expect = {0: (C, C, 3, 3), 3: (C, C, 3, 3), 6: (2, C, 3, 3), 8: (1, C, 3, 3), 10: (4, C, 3, 3)}
    for i, shp in expect.items():
        if tuple(w[i].shape) != shp:
            raise RuntimeError("siammot_amd.emm_predictor: %s has shape %s, expected %s"
                               % (PREDICTOR_KEYS[i], tuple(w[i].shape), shp))
    tower_ws = torch.empty((N, 2 * C, Ho, Ho), dtype=torch.float32, device=resp.device)
    logits = torch.empty((N, 7, Ho, Ho), dtype=torch.float32, device=resp.device)
    packed = tower_packed(params) if (winograd and Ho in (16, 29)) else None       # (29: Winograd in 16 x 16 blocks)
    with _Launch(resp, *w) as ln:
        rc = lib.smot_emm_predictor_fwd(_ptr(resp), N, C, Ho, *[_ptr(t) for t in w], int(gn_groups), float(gn_eps),
                                        _ptr(packed), _ptr(tower_ws), _ptr(logits), ln.stream)
    _check(rc, "emm_predictor")
    return logits


_hann_cache = {}


def hann_window(G, device):
    """``torch.hann_window(G)`` (periodic) evaluated on the CPU — bit-identical to what the CPU
    reference multiplies in (track_core.py:157-158) — cached per device."""
    key = (G, device)
    w = _hann_cache.get(key)
    if w is None:
        w = _hann_cache[key] = torch.hann_window(G, dtype=torch.float).to(device)
    return w


def emm_decode(logits, sr, boxes, rx, rz, pad_pixels, sigma=0.4, use_centerness=True, return_index=False,
               clip_wh=None):
    """Fused up-sample + decode.  logits ``[N,7,Ho,Ho]``, sr/boxes ``[N,4]`` → (bb ``[N,4]``, conf ``[N]``).
    ``clip_wh=(W, H)`` also applies the in-place clamp of ``BoxList.clip_to_image`` (non-amodal)."""
    lib = load_library()
    logits = _dev_f32(logits, "logits")
    sr = _dev_f32(sr, "sr")
    boxes = _dev_f32(boxes, "boxes")
    N, _, Ho, _ = logits.shape
    dev = logits.device
    G = Ho * UP_SCALE
    ws = torch.empty((max(N, 1) * lib.smot_emm_decode_ws_floats(Ho, UP_SCALE),), dtype=torch.float32, device=dev)
    bb = torch.empty((N, 4), dtype=torch.float32, device=dev)
    conf = torch.empty((N,), dtype=torch.float32, device=dev)
    idx = torch.empty((N,), dtype=torch.int64, device=dev) if return_index else None
    with _Launch(logits, sr, boxes) as ln:
        rc = lib.smot_emm_decode_fwd(_ptr(logits), _ptr(sr), _ptr(boxes), _ptr(hann_window(G, dev)), N, Ho, UP_SCALE,
                                     int(rx), int(rz), float(pad_pixels), float(1 - sigma), float(sigma),
                                     int(bool(use_centerness)),
                                     float(clip_wh[0]) if clip_wh is not None else 0.0,
                                     float(clip_wh[1]) if clip_wh is not None else 0.0,
                                     _ptr(ws), _ptr(bb), _ptr(conf), _ptr(idx), ln.stream)
    _check(rc, "emm_decode")
    return (bb, conf, idx) if return_index else (bb, conf)


# ----------------------------------------------------------------------------------------------
# one-call halves of a frame pair
# ----------------------------------------------------------------------------------------------
_cast = lambda a: ctypes.cast(a, ctypes.c_void_p)


def _level_arrays(features, scales, nhwc=True, what="", batched=False):
    """The first ``len(scales)`` levels as the library takes them and their ctypes arrays -> (maps, pointers, heights, widths,
    scales, ``feat_type``).  ``what``: the caller's name in the error text (".roi_align_levels").  ``batched``: ``[B, C, H_l,
    W_l]`` maps with one B and one C for every level instead of one image."""
    L = len(scales)
    feats, ft = _dev_feats(features, L, nhwc)      # (one dtype per call: raises otherwise)
    for f in feats:
        if batched:
            if f.dim() != 4 or f.shape[:2] != feats[0].shape[:2]:
                raise RuntimeError("siammot_amd%s: every level must be [B, C, H, W] with one B and one C, got feature shapes %s"
                                   % (what, [tuple(g.shape) for g in feats]))
        elif f.dim() != 4 or f.shape[0] != 1:
            raise RuntimeError("siammot_amd%s: one image per call, got feature shape %s" % (what, tuple(f.shape)))
    fp = (ctypes.c_void_p * L)(*[f.data_ptr() for f in feats])
    hs = (ctypes.c_int * L)(*[f.shape[2] for f in feats])
    ws = (ctypes.c_int * L)(*[f.shape[3] for f in feats])
    sc = (ctypes.c_float * L)(*[float(s) for s in scales])
    return feats, fp, hs, ws, sc, ft


_ws_cache = {}


def _workspace(device, n_floats, stream=None):
    """Grow-only fp32 scratch per (device, stream): intermediates never leave the library and nothing persists
    semantically between calls, but two streams of one device run concurrently and must not share it."""
    key = (device, stream)
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < n_floats:
        buf = torch.empty((int(n_floats * 1.25) + 1024,), dtype=torch.float32, device=device)
        _ws_cache[key] = buf
    return buf


# ---- launch state reused across frames --------------------------------------------------------
# A frame pair is ~80 us of GPU work, so the host side of the two one-call entry points has to stay well below
# that: everything that does not change from frame to frame (per-level geometry arrays, the validated parameter
# pointer block, the packed tower filters, the Hann window, the workspace) is cached; per call only the feature /
# box pointers are refreshed and checked.
_F32 = torch.float32


class _LevelGeometry(object):
    """ctypes arrays of one FPN geometry: heights / widths / scales / virtual pad cells, plus the pointer array
    that is refilled every call."""
    __slots__ = ("shapes", "L", "C", "fp", "hs", "ws", "sc", "pc", "a_fp", "a_hs", "a_ws", "a_sc", "a_pc", "keep", "dtype", "ft")

    def __init__(self, shapes, scales, pad_pixels, dtype=torch.float32, layout=0):
        L = len(scales)
        self.shapes, self.L, self.C = shapes, L, shapes[0][1]
        # the maps' one element type and layout (parts of the cache key): ``ft`` is the typed entry points' ``feat_type``
        self.dtype, self.ft = dtype, FEAT_TYPES[dtype] | layout
        self.fp = (ctypes.c_void_p * L)()
        self.hs = (ctypes.c_int * L)(*[sh[2] for sh in shapes])
        self.ws = (ctypes.c_int * L)(*[sh[3] for sh in shapes])
        self.sc = (ctypes.c_float * L)(*[float(v) for v in scales])
        self.pc = (ctypes.c_int * L)(*[int(pad_pixels / ((2 ** i) * 4)) for i in range(L)])
        self.a_fp, self.a_hs, self.a_ws = ctypes.addressof(self.fp), ctypes.addressof(self.hs), ctypes.addressof(self.ws)
        self.a_sc, self.a_pc = ctypes.addressof(self.sc), ctypes.addressof(self.pc)
        self.keep = [None] * L                   # contiguous copies of strided inputs, alive until the next call


_geom_cache = {}


def _maps_dtype(features, L):
    """The element type of a call's maps (levels must agree; anything but fp32 / fp16 / bf16 raises)."""
    dt = features[0].dtype if isinstance(features[0], torch.Tensor) else None
    if dt not in FEAT_TYPES:
        _dev_feat(features[0], "features[0]")               # raises
    for l in range(1, L):
        if features[l].dtype is not dt:
            _feat_type([_dev_feat(features[k], "features[%d]" % k) for k in range(l + 1)])     # raises either way
    return dt


def _geometry(features, scales, pad_pixels, device, nhwc=True, batched=False):
    """Validate the per-level feature tensors (all on ``device``) and return the cached geometry with fresh
    pointers.  Channels-last levels (``_levels_layout``) are passed as they are and the geometry says so (``g.ft``);
    ``nhwc=False``: the caller's entry has no channels-last form, such maps are copied like any strided view.
    ``batched``: ``[B, C, H, W]`` maps with one B (``g.shapes[0][0]``) for every level instead of one image."""
    L = len(scales)
    shapes = tuple(tuple(features[l].shape) for l in range(L))
    dt = _maps_dtype(features, L)
    cl = _levels_layout(features, L) if nhwc else 0
    key = ("batched", shapes, tuple(scales), pad_pixels, dt, cl) if batched else (shapes, tuple(scales), pad_pixels, dt, cl)
    g = _geom_cache.get(key)
    if g is None:
        for sh in shapes:
            if len(sh) != 4 or sh[0] != (shapes[0][0] if batched else 1) or sh[1] != shapes[0][1]:
                raise RuntimeError(("siammot_amd: every level must be [B, C, H, W] with one B and one C, got feature shapes %s"
                                    if batched else
                                    "siammot_amd: one image per call and one channel count, got feature shapes %s") % (shapes,))
        if len(_geom_cache) > 32:
            _geom_cache.clear()
        g = _geom_cache[key] = _LevelGeometry(shapes, scales, pad_pixels, dt, cl)
    fp = g.fp
    for l in range(L):
        f = features[l]
        if not (f.is_cuda and (cl or f.is_contiguous())):
            f = g.keep[l] = _dev_feat(f, "features[%d]" % l)        # raises, or copies a strided view
        if f.device != device:
            raise RuntimeError("siammot_amd: features[%d] lives on %s, the boxes on %s" % (l, f.device, device))
        fp[l] = f.data_ptr()
    return g


def _head_reads_channels_last(rx, rz):
    """False for the 35 / 7 head shape: its gather kernel has no channels-last form (the maps go through the NCHW copy)."""
    return not (int(rx) == 35 and int(rz) == 7)


def _geometry_refresh(g, features, device):
    """The per-frame part of ``_geometry`` for a caller that keeps ``g``: same shapes, same dtype, the geometry's own layout
    (contiguous, or channels-last for a channels-last geometry), on ``device`` -> the pointer array is refilled and True is
    returned; anything else returns False (the caller takes the full path, which raises or rebuilds)."""
    fp, shapes, dt = g.fp, g.shapes, g.dtype
    if len(features) < g.L:
        return False
    cl = g.ft & FEAT_CHANNELS_LAST
    for l in range(g.L):                 # validate every level first: a mismatch must leave the pointer array as it was
        f = features[l]
        if f.shape != shapes[l] or not (f.is_cuda and f.dtype is dt) or f.device != device:
            return False
        if f.is_contiguous() if cl else not f.is_contiguous():      # (channels-last: not contiguous, and ...)
            return False
        if cl and not (f.is_contiguous(memory_format=_CL) and f.data_ptr() % 16 == 0):
            return False
    for l in range(g.L):
        fp[l] = features[l].data_ptr()
    return True


def _same_device(device, *named):
    for name, t in named:
        if t.device != device:
            raise RuntimeError("siammot_amd: %s lives on %s, the boxes on %s" % (name, t.device, device))


class _ParamBlock(object):
    """The 12 predictor tensors validated once, their pointers as a ctypes block, and the Winograd-packed tower
    filters; revalidated per call by data pointer + version counter (a dozen attribute reads)."""
    __slots__ = ("params", "tensors", "stamp", "pp", "a_pp", "packed", "C", "calls")

    def __init__(self, params):
        self.params = params                     # keeps the dict (and so its id) alive while cached
        self.calls = 0
        self.refresh()

    def refresh(self):
        w = [_dev_f32(self.params[k], k) for k in PREDICTOR_KEYS]
        C = w[0].shape[0]
        expect = {0: (C, C, 3, 3), 3: (C, C, 3, 3), 6: (2, C, 3, 3), 8: (1, C, 3, 3), 10: (4, C, 3, 3)}
        for i, shp in expect.items():
            if tuple(w[i].shape) != shp:
                raise RuntimeError("siammot_amd: %s has shape %s, expected %s" % (PREDICTOR_KEYS[i], tuple(w[i].shape), shp))
        self.tensors, self.C = w, C
        self.stamp = [(t.data_ptr(), t._version) for t in w]
        self.packed = tower_packed(self.params)
        self.pp = (ctypes.c_void_p * 13)(*([t.data_ptr() for t in w] + [self.packed.data_ptr() if self.packed is not None else None]))
        self.a_pp = ctypes.addressof(self.pp)

    def current(self):
        """Revalidate against in-place updates (``load_state_dict`` bumps every tensor's version) and moves
        (``.to()`` replaces every storage): the two tower weights are checked on every call, the whole set every
        32nd — a dozen attribute reads less per frame on the tracking loop's host path."""
        p, st = self.params, self.stamp
        self.calls = calls = self.calls + 1
        keys = PREDICTOR_KEYS if (calls & 31) == 0 else _TOWER_KEYS
        for k in keys:
            t = p[k]
            s = st[_KEY_INDEX[k]]
            if t.data_ptr() != s[0] or t._version != s[1]:
                self.refresh()
                break
        return self


_param_cache = {}


def _param_block(params):
    blk = _param_cache.get(id(params))
    if blk is None or blk.params is not params:
        if len(_param_cache) > 16:
            _param_cache.clear()
        blk = _param_cache[id(params)] = _ParamBlock(params)
        return blk
    return blk.current()


def _chk(t, name, shape):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype is _F32):
        _dev_f32(t, name)
    if tuple(t.shape) != shape:
        raise RuntimeError("siammot_amd: %s has shape %s, expected %s" % (name, tuple(t.shape), shape))
    return t if t.is_contiguous() else t.contiguous()


def _head_call(lib, g, batched=False):
    """The head's library call (``smot_emm_track*_fwd``) bound to the geometry ``g``: the ONE place that spells its argument
    order and chooses its entry point.  The entry also selects the kernels (csrc/emm_fused.hip): the untyped entry runs the
    single-image kernels, the typed entry the batched ones even for one image.

        one image, fp32 NCHW maps (``g.ft == 0``)     smot_emm_track_fwd
        one image, any other ``g.ft``                 smot_emm_track_typed_fwd(..., 1, [0, N])
        ``batched``, any ``g.ft`` (0 included)        smot_emm_track_typed_fwd(..., num_images, row_start)

    The callable takes addresses (None = NULL) and returns the library's status."""
    a_fp, ft, a_hs, a_ws, a_pc, a_sc, L, C = g.a_fp, g.ft, g.a_hs, g.a_ws, g.a_pc, g.a_sc, g.L, g.C
    if not batched and ft == 0:
        fn = lib.smot_emm_track_fwd

        def call(boxes, sr, templates, N, rx, rz, sampling_ratio, a_pp, gn_groups, gn_eps, hann, pad_pixels, sigma,
                 use_centerness, clip_w, clip_h, work, bb, conf, idx, hint, stream):
            return fn(a_fp, a_hs, a_ws, a_pc, a_sc, L, C, boxes, sr, templates, N, rx, rz, sampling_ratio, a_pp, gn_groups,
                      gn_eps, hann, UP_SCALE, pad_pixels, 1 - sigma, sigma, 1 if use_centerness else 0, clip_w, clip_h,
                      work, bb, conf, idx, hint, stream)
    else:
        fn = lib.smot_emm_track_typed_fwd

        def call(boxes, sr, templates, N, rx, rz, sampling_ratio, a_pp, gn_groups, gn_eps, hann, pad_pixels, sigma,
                 use_centerness, clip_w, clip_h, work, bb, conf, idx, hint, stream, num_images=1, row_start=None):
            return fn(a_fp, ft, a_hs, a_ws, a_pc, a_sc, L, C, boxes, sr, templates, N, rx, rz, sampling_ratio, a_pp, gn_groups,
                      gn_eps, hann, UP_SCALE, pad_pixels, 1 - sigma, sigma, 1 if use_centerness else 0, clip_w, clip_h,
                      work, bb, conf, idx, hint, stream, num_images,
                      row_start if row_start is not None else _one_image_rows(N))
    return call


def _emm_track(batched, features, boxes, sr, templates, rows_per_image, params, rx, rz, scales, sampling_ratio, pad_pixels,
               sigma, use_centerness, clip_wh, gn_groups, gn_eps, return_index, winograd, order_hint):
    """The one body of ``emm_track`` and ``emm_track_batched``."""
    what = "emm_track_batched" if batched else "emm_track"
    lib = _lib or load_library()
    if not (isinstance(boxes, torch.Tensor) and boxes.is_cuda):
        _dev_f32(boxes, "boxes")                 # raises: no CPU path
    dev = boxes.device
    g = _geometry(features, scales, pad_pixels, dev, nhwc=_head_reads_channels_last(rx, rz), batched=batched)
    N, C = boxes.shape[0], g.C
    rows = (g.shapes[0][0], _row_starts(rows_per_image, g.shapes[0][0], N)) if batched else ()
    boxes = _chk(boxes, "boxes", (N, 4))
    sr = _chk(sr, "sr", (N, 4))
    templates = _chk(templates, "template_features", (N, C, rz, rz))
    blk = _param_block(params)
    _same_device(dev, ("sr", sr), ("template_features", templates), ("predictor weights", blk.tensors[0]))
    if blk.C != C:
        raise RuntimeError("siammot_amd.%s: predictor has %d channels, features have %d" % (what, blk.C, C))
    ho = rx - rz + 1
    a_pp = blk.a_pp
    if not (winograd and ho in (16, 29)) and blk.packed is not None:
        pp = (ctypes.c_void_p * 13)(*([t.data_ptr() for t in blk.tensors] + [None]))    # direct tower kernel
        a_pp = ctypes.addressof(pp)
    stream = _stream(dev)
    work = _workspace(dev, lib.smot_emm_track_ws_floats(N, C, rx, rz), stream.value)
    bb = torch.empty((N, 4), dtype=_F32, device=dev)
    conf = torch.empty((N,), dtype=_F32, device=dev)
    idx = torch.empty((N,), dtype=torch.int64, device=dev) if return_index else None
    if not batched and order_hint is None and rx == 30 and rz == 15 and 2 <= N <= 256:
        FALLBACKS["unhinted_head"] += 1
    if order_hint is not None and (tuple(order_hint.shape) != (N, HINT_FLOATS) or order_hint.device != dev
                                   or order_hint.dtype is not _F32 or not order_hint.is_contiguous()):
        raise RuntimeError("siammot_amd.%s: order_hint must be the contiguous fp32 [%d, %d] tensor of the "
                           "extraction that made these boxes" % (what, N, HINT_FLOATS))
    cur = torch.cuda.current_device()           # kernels launch on the CURRENT device: make it the tensors' device
    if cur != dev.index:
        torch.cuda.set_device(dev.index)
    try:
        rc = _head_call(lib, g, batched)(
            boxes.data_ptr(), sr.data_ptr(), templates.data_ptr(), N, rx, rz, sampling_ratio, a_pp, gn_groups, gn_eps,
            hann_window(ho * UP_SCALE, dev).data_ptr(), pad_pixels, sigma, use_centerness,
            float(clip_wh[0]) if clip_wh is not None else 0.0, float(clip_wh[1]) if clip_wh is not None else 0.0,
            work.data_ptr(), bb.data_ptr(), conf.data_ptr(), idx.data_ptr() if idx is not None else None,
            order_hint.data_ptr() if order_hint is not None else None, stream, *rows)
    finally:
        if cur != dev.index:
            torch.cuda.set_device(cur)
    if rc:
        _check(rc, what)
    return (bb, conf, idx) if return_index else (bb, conf)


def emm_track(features, boxes, sr, templates, params, rx, rz, scales, sampling_ratio, pad_pixels,
              sigma=0.4, use_centerness=True, clip_wh=None, gn_groups=32, gn_eps=1e-5, return_index=False,
              winograd=True, order_hint=None):
    """The inference branch of ``EMM.forward`` in ONE library call.  Returns (bb ``[N,4]``, conf ``[N]``).

    ``order_hint``: the ``[N, HINT_FLOATS]`` tensor ``emm_extract_cache(..., hint=True)`` returned TOGETHER WITH exactly
    these ``boxes`` / ``sr`` (include/smot_emm.h: a scheduling side channel, VERIFIED by the kernel against these very
    tensors: a hint of other boxes raises its status word — ``order_hint_status`` — and every returned row is NaN;
    ``siammot_amd.emm.EMM`` also checks tensor identity and versions before it passes one), or None."""
    return _emm_track(False, features, boxes, sr, templates, None, params, rx, rz, scales, sampling_ratio, pad_pixels,
                      sigma, use_centerness, clip_wh, gn_groups, gn_eps, return_index, winograd, order_hint)


HINT_FLOATS = 536                    # SMOT_HINT_FLOATS (include/smot_emm.h): entry header + both finished sample tables + by-roi record
HINT_STATUS_WORD = 534               # SMOT_HINT_STATUS_WORD: the list's status word (entry 0), raised by a head that found the
                                     # hint NOT describing its rois (that head's rows are NaN)
_hint_floats = {}


def order_hint_status(order_hint):
    """Status word of an order hint (``[N, HINT_FLOATS]`` tensor): 0 = every head given this hint found it describing its
    rois.  Synchronises (one 4-byte copy): for error paths and tests, not for the frame loop."""
    return int(order_hint.view(-1)[HINT_STATUS_WORD:HINT_STATUS_WORD + 1].view(torch.int32).item())


def order_hint_floats(N, rz, sampling_ratio):
    """``smot_emm_order_hint_floats``: size of the order hint the extraction writes for ``N`` boxes (0 = none)."""
    key = (N, rz, sampling_ratio)
    v = _hint_floats.get(key)
    if v is None:
        if len(_hint_floats) > 1024:
            _hint_floats.clear()
        v = _hint_floats[key] = int((_lib or load_library()).smot_emm_order_hint_floats(N, rz, sampling_ratio))
    return v


def _extract_call(lib, g, batched=False, masked=False):
    """The extraction's library call (``smot_emm_extract_cache*_fwd``) bound to the geometry ``g``: the ONE place that spells
    its argument order and chooses its entry point (and with it the kernels, as for ``_head_call``).

        one image, ``g.ft == 0``, no ``n_valid``      smot_emm_extract_cache_fwd
        one image, ``g.ft == 0``, ``masked``          smot_emm_extract_cache_masked_fwd(..., n_valid, ...)
        one image, any other ``g.ft``                 smot_emm_extract_cache_typed_fwd(..., 1, [0, N], n_valid or NULL)
        ``batched``, any ``g.ft``                     smot_emm_extract_cache_typed_fwd(..., num_images, row_start, NULL)

    The callable takes addresses (None = NULL) and returns the library's status."""
    a_fp, ft, a_hs, a_ws, a_sc, L, C = g.a_fp, g.ft, g.a_hs, g.a_ws, g.a_sc, g.L, g.C
    if batched or ft != 0:
        fn = lib.smot_emm_extract_cache_typed_fwd

        def call(boxes, N, rz, sampling_ratio, pad_pixels, search_expansion, min_search_wh, templates, sr, hint, stream,
                 n_valid=None, num_images=1, row_start=None):
            return fn(a_fp, ft, a_hs, a_ws, a_sc, L, C, boxes, N, rz, sampling_ratio, pad_pixels, search_expansion,
                      min_search_wh, templates, sr, hint, stream, num_images,
                      row_start if row_start is not None else _one_image_rows(N), n_valid)
    elif masked:
        fn = lib.smot_emm_extract_cache_masked_fwd

        def call(boxes, N, rz, sampling_ratio, pad_pixels, search_expansion, min_search_wh, templates, sr, hint, stream,
                 n_valid):
            return fn(a_fp, a_hs, a_ws, a_sc, L, C, boxes, N, n_valid, rz, sampling_ratio, pad_pixels, search_expansion,
                      min_search_wh, templates, sr, hint, stream)
    else:
        fn = lib.smot_emm_extract_cache_fwd

        def call(boxes, N, rz, sampling_ratio, pad_pixels, search_expansion, min_search_wh, templates, sr, hint, stream,
                 n_valid=None):
            return fn(a_fp, a_hs, a_ws, a_sc, L, C, boxes, N, rz, sampling_ratio, pad_pixels, search_expansion,
                      min_search_wh, templates, sr, hint, stream)
    return call


def _sr_and_hint(N, dev, with_hint):
    """The extraction's search-region output and, ``with_hint``, its order hint, in one allocation: hint | sr."""
    if not with_hint:
        return torch.empty((N, 4), dtype=_F32, device=dev), None
    both = torch.empty((N * (HINT_FLOATS + 4),), dtype=_F32, device=dev)
    return both[N * HINT_FLOATS:].view(N, 4), both[:N * HINT_FLOATS].view(N, HINT_FLOATS)


def _emm_extract_cache(batched, features, boxes, rows_per_image, rz, scales, sampling_ratio, pad_pixels, search_expansion,
                       min_search_wh, n_valid, hint):
    """The one body of ``emm_extract_cache`` and ``emm_extract_cache_batched``."""
    lib = _lib or load_library()
    if not (isinstance(boxes, torch.Tensor) and boxes.is_cuda):
        _dev_f32(boxes, "boxes")                 # raises: no CPU path
    dev = boxes.device
    g = _geometry(features, scales, 0, dev, batched=True) if batched else _geometry(features, scales, 0, dev)
    N = boxes.shape[0]
    rows = (g.shapes[0][0], _row_starts(rows_per_image, g.shapes[0][0], N)) if batched else ()
    boxes = _chk(boxes, "boxes", (N, 4))
    templates = torch.empty((N, g.C, rz, rz), dtype=_F32, device=dev)
    sr, oh = _sr_and_hint(N, dev, hint and boxes.data_ptr() % 16 == 0 and order_hint_floats(N, rz, sampling_ratio) > 0)
    cur = torch.cuda.current_device()
    if cur != dev.index:
        torch.cuda.set_device(dev.index)
    try:
        rc = _extract_call(lib, g, batched, n_valid is not None)(
            boxes.data_ptr(), N, rz, sampling_ratio, pad_pixels, search_expansion, min_search_wh, templates.data_ptr(),
            sr.data_ptr(), oh.data_ptr() if oh is not None else None, _stream(dev),
            n_valid.data_ptr() if n_valid is not None else None, *rows)
    finally:
        if cur != dev.index:
            torch.cuda.set_device(cur)
    if rc:
        _check(rc, "emm_extract_cache_batched" if batched else "emm_extract_cache")
    return (templates, sr, oh) if hint else (templates, sr)


def emm_extract_cache(features, boxes, rz, scales, sampling_ratio, pad_pixels, search_expansion, min_search_wh,
                      n_valid=None, hint=False):
    """``EMM.extract_cache`` in one library call → (templates ``[N,C,rz,rz]``, sr ``[N,4]``); with ``hint=True`` →
    (templates, sr, order hint ``[N, HINT_FLOATS]`` or None when this shape / count writes none): the list the next
    frame's ``emm_track(..., order_hint=)`` reads instead of ranking these search regions in every workgroup.

    ``n_valid``: a device int32 tensor (1 element) holding the number of REAL rows among ``boxes`` (a capacity): rows
    beyond it are skipped on the device and their outputs stay unwritten — the call can be enqueued before the
    host knows the count (ops.track_solve_launch)."""
    return _emm_extract_cache(False, features, boxes, None, rz, scales, sampling_ratio, pad_pixels, search_expansion,
                              min_search_wh, n_valid, hint)


# ---- several images per call (smot_emm_*_typed_fwd with num_images, row_start) ----------------------------------------
MAX_IMAGES = 64                      # SMOT_MAX_IMAGES (include/smot_emm.h)


def _row_starts(rows_per_image, B, N):
    """Host ``row_start[B + 1]`` of a batch from its per-image row counts (checked here and again by the library)."""
    rows = [int(r) for r in rows_per_image]
    if len(rows) != B:
        raise RuntimeError("siammot_amd: %d row counts for a feature batch of %d images" % (len(rows), B))
    if any(r < 0 for r in rows) or sum(rows) != N:
        raise RuntimeError("siammot_amd: row counts %s do not split the %d rows" % (rows, N))
    starts = [0]
    for r in rows:
        starts.append(starts[-1] + r)
    return (ctypes.c_int * (B + 1))(*starts)


def emm_track_batched(features, boxes, sr, templates, rows_per_image, params, rx, rz, scales, sampling_ratio, pad_pixels,
                      sigma=0.4, use_centerness=True, clip_wh=None, gn_groups=32, gn_eps=1e-5, return_index=False,
                      winograd=True, order_hint=None):
    """``emm_track`` over B images in one library call: ``features`` are ``[B, C, H_l, W_l]`` per level, the rows of image b
    are the ``rows_per_image[b]`` consecutive rows after those of images 0..b-1 (host ints).  Returns what ``emm_track``
    returns for all rows; the rows of image b are exactly what ``emm_track`` gives on ``features[l][b:b+1]`` with them.
    ``clip_wh``: the one image size of the batch.  ``order_hint``: as for ``emm_track``, from ``emm_extract_cache_batched``."""
    return _emm_track(True, features, boxes, sr, templates, rows_per_image, params, rx, rz, scales, sampling_ratio,
                      pad_pixels, sigma, use_centerness, clip_wh, gn_groups, gn_eps, return_index, winograd, order_hint)


def emm_extract_cache_batched(features, boxes, rows_per_image, rz, scales, sampling_ratio, pad_pixels, search_expansion,
                              min_search_wh, hint=False):
    """``emm_extract_cache`` over B images in one library call (``features`` ``[B, C, H_l, W_l]``, rows grouped by image as
    in ``emm_track_batched``) -> (templates, sr) or, with ``hint=True``, (templates, sr, order hint or None)."""
    return _emm_extract_cache(True, features, boxes, rows_per_image, rz, scales, sampling_ratio, pad_pixels,
                              search_expansion, min_search_wh, None, hint)


def roi_align_levels_batched(features, rois, level_boxes, rows_per_image, out_size, scales, sampling_ratio, pad_cells=None):
    """``roi_align_levels`` over B images in one library call: ``features`` are ``[B, C, H_l, W_l]`` per level (fp32, fp16 or
    bf16, NCHW or channels-last, as for one image), the rois of image b are the ``rows_per_image[b]`` consecutive rows after
    those of images 0..b-1 (host ints; zero is fine).  Returns ``[R, C, out_size, out_size]``; the rows of image b are bit for
    bit what ``roi_align_levels`` gives on ``features[l][b:b+1]`` with them."""
    lib = load_library()
    L = len(scales)
    feats, fp, hs, ws, sc, ft = _level_arrays(features, scales, what=".roi_align_levels_batched", batched=True)
    B, C = feats[0].shape[0], feats[0].shape[1]
    rois = _dev_f32(rois, "rois")
    level_boxes = rois if level_boxes is None else _dev_f32(level_boxes, "level_boxes")
    if rois.dim() != 2 or rois.shape[1] != 4 or level_boxes.shape != rois.shape:
        raise RuntimeError("siammot_amd.roi_align_levels_batched: rois and level_boxes must be [R, 4], got %s and %s"
                           % (tuple(rois.shape), tuple(level_boxes.shape)))
    R = rois.shape[0]
    if B > MAX_IMAGES:
        raise RuntimeError("siammot_amd.roi_align_levels_batched: %d images, at most %d per call" % (B, MAX_IMAGES))
    starts = _row_starts(rows_per_image, B, R)
    if pad_cells is None:
        pad_cells = [0] * L
    out = torch.empty((R, C, out_size, out_size), dtype=torch.float32, device=rois.device)
    pc = (ctypes.c_int * L)(*[int(p) for p in pad_cells[:L]])
    with _Launch(rois, level_boxes, *feats) as ln:
        rc = lib.smot_roi_align_levels_batched_typed_fwd(_cast(fp), ft, _cast(hs), _cast(ws), _cast(pc), _cast(sc), L, C,
                                                         _ptr(rois), _ptr(level_boxes), R, out_size, out_size,
                                                         int(sampling_ratio), _ptr(out), _ptr(None), ln.stream, B,
                                                         _cast(starts))
    _check(rc, "roi_align_levels_batched")
    return out


try:
    _cur_device = torch._C._cuda_getDevice                    # current device index, ~0.1 us (torch.cuda.current_device: ~0.7)
except AttributeError:                                        # pragma: no cover - older torch
    _cur_device = torch.cuda.current_device


class PairPlan(object):
    """The host side of ``EMM.forward`` / ``EMM.extract_cache`` for a caller that makes the same two calls every frame
    (round 6): what ``emm_track`` / ``emm_extract_cache`` look up, validate and convert on every call —
    the level geometry, the parameter block, the workspace, the Hann window, the hint's size, two dozen scalar arguments —
    is resolved ONCE per (feature shapes, scales, device, shape family) and kept as the constant part of the library
    call's argument tuple; a call then checks what can change between frames (the five feature tensors: shape, dtype,
    layout, device -> their pointers; the box / search-region / template tensors; the parameter tensors' storage and
    version), allocates its outputs and makes the ONE library call.  ``track`` / ``extract`` return None for anything they
    do not recognise (another geometry, a strided tensor, another device, a count the plan was not made for is re-planned):
    the caller then takes the general functions above, which raise or convert.  Results are the general functions', bit
    for bit — same library entry points, same arguments: both go through ``_head_call`` / ``_extract_call``
    (tests/test_binding_paths.py).  There is still no CPU or eager path."""
    __slots__ = ("dev", "dev_index", "g", "gz", "params", "blk", "rx", "rz", "ho", "scales", "sampling_ratio", "pad_pixels",
                 "hann_ptr", "ws", "ws_n", "C", "hint_n", "hint_ok", "lib", "f_track", "f_extract", "tu", "ft")

    def __init__(self, features, dev, params, rx, rz, scales, sampling_ratio, pad_pixels, tu):
        self.lib = lib = _lib or load_library()
        self.dev, self.dev_index = dev, dev.index
        nhwc = _head_reads_channels_last(rx, rz)                        # (one layout for the plan's two calls)
        self.g = _geometry(features, scales, pad_pixels, dev, nhwc)     # full validation (raises)
        self.gz = _geometry(features, scales, 0, dev, nhwc)
        self.params, self.blk = params, _param_block(params)
        self.rx, self.rz, self.ho = rx, rz, rx - rz + 1
        self.scales, self.sampling_ratio, self.pad_pixels = scales, sampling_ratio, pad_pixels
        self.C = self.g.C
        if self.blk.C != self.C:
            raise RuntimeError("siammot_amd.emm_track: predictor has %d channels, features have %d" % (self.blk.C, self.C))
        self.hann_ptr = hann_window(self.ho * UP_SCALE, dev).data_ptr()
        self.ws, self.ws_n = None, -1
        self.hint_n, self.hint_ok = -1, False
        self.ft = self.g.ft                       # the maps' element type and layout the plan was made for (SMOT_FEAT_*)
        self.f_track, self.f_extract = _head_call(lib, self.g), _extract_call(lib, self.gz)     # (entries resolved once)
        self.tu = (float(tu.pad_pixels), float(tu.search_expansion), float(tu.min_search_wh))

    def stale(self, params, rx, rz, scales, sampling_ratio, pad_pixels, tu, features=None):
        """True when the plan does not describe this call.  ``features``: the call's maps — another dtype, another layout or
        other shapes than the plan's geometry make it stale too (a caller that switches between fp32 and half maps, between
        NCHW and channels-last maps, or between map sizes, gets a new plan instead of falling to the general functions on
        every call)."""
        if features is not None:
            g = self.g
            if len(features) < g.L:
                return True
            for l in range(g.L):
                if features[l].dtype is not g.dtype or features[l].shape != g.shapes[l]:
                    return True
            # ... and another layout (NCHW maps on a channels-last plan, or maps the library reads as channels-last on an
            # NCHW plan): a caller that alternates gets a plan per layout
            if features[0].is_contiguous():
                if g.ft & FEAT_CHANNELS_LAST:
                    return True
            elif not (g.ft & FEAT_CHANNELS_LAST) and _head_reads_channels_last(rx, rz) and _levels_layout(features, g.L):
                return True
        return (params is not self.params or rx != self.rx or rz != self.rz or scales != self.scales or
                sampling_ratio != self.sampling_ratio or pad_pixels != self.pad_pixels or self.lib is not _lib or
                self.tu != (float(tu.pad_pixels), float(tu.search_expansion), float(tu.min_search_wh)))

    def track(self, features, boxes, sr, templates, sigma, use_centerness, clip_w, clip_h, gn_groups, gn_eps, order_hint):
        """``emm_track`` (winograd path, no index output): (bb ``[N,4]``, conf ``[N]``) or None."""
        dev, g, rz = self.dev, self.g, self.rz
        if not (boxes.is_cuda and boxes.dtype is _F32 and boxes.is_contiguous() and boxes.device == dev and boxes.dim() == 2):
            return None
        N = boxes.shape[0]
        if not (sr.is_cuda and sr.dtype is _F32 and sr.is_contiguous() and sr.shape == boxes.shape and boxes.shape[1] == 4 and
                templates.is_cuda and templates.dtype is _F32 and templates.is_contiguous() and
                templates.shape == (N, self.C, rz, rz) and sr.get_device() == self.dev_index and
                templates.get_device() == self.dev_index and _cur_device() == self.dev_index):
            return None
        if not _geometry_refresh(g, features, dev):
            return None
        blk = self.blk.current()
        if blk.packed is None or blk.tensors[0].get_device() != self.dev_index or blk.C != self.C:
            return None
        stream = _raw_stream(self.dev_index)
        if N != self.ws_n or self.ws is None or self.ws is not _ws_cache.get((dev, stream)):
            self.ws = _workspace(dev, self.lib.smot_emm_track_ws_floats(N, self.C, self.rx, rz), stream)
            self.ws_n = N
        bb = torch.empty((N, 4), dtype=_F32, device=dev)
        conf = torch.empty((N,), dtype=_F32, device=dev)
        hint_ptr = None
        if order_hint is not None:
            if (order_hint.shape != (N, HINT_FLOATS) or order_hint.get_device() != self.dev_index or
                    order_hint.dtype is not _F32 or not order_hint.is_contiguous()):
                return None
            hint_ptr = order_hint.data_ptr()
        elif self.rx == 30 and rz == 15 and 2 <= N <= 256:
            FALLBACKS["unhinted_head"] += 1
        rc = self.f_track(boxes.data_ptr(), sr.data_ptr(), templates.data_ptr(), N, self.rx, rz, self.sampling_ratio, blk.a_pp,
                          gn_groups, gn_eps, self.hann_ptr, self.pad_pixels, sigma, use_centerness, clip_w, clip_h,
                          self.ws.data_ptr(), bb.data_ptr(), conf.data_ptr(), None, hint_ptr, stream)
        if rc:
            _check(rc, "emm_track")
        return bb, conf

    def extract(self, features, boxes, hint):
        """``emm_extract_cache`` (un-masked form): (templates, sr, order hint or None) or None."""
        dev, g, rz = self.dev, self.gz, self.rz
        if not (boxes.is_cuda and boxes.dtype is _F32 and boxes.is_contiguous() and boxes.device == dev and
                boxes.dim() == 2 and boxes.shape[1] == 4 and _cur_device() == self.dev_index):
            return None
        if not _geometry_refresh(g, features, dev):
            return None
        N = boxes.shape[0]
        templates = torch.empty((N, self.C, rz, rz), dtype=_F32, device=dev)
        if hint and N != self.hint_n:
            self.hint_n, self.hint_ok = N, order_hint_floats(N, rz, self.sampling_ratio) > 0
        sr, oh = _sr_and_hint(N, dev, hint and self.hint_ok and boxes.data_ptr() % 16 == 0)
        tu = self.tu
        rc = self.f_extract(boxes.data_ptr(), N, rz, self.sampling_ratio, tu[0], tu[1], tu[2], templates.data_ptr(),
                            sr.data_ptr(), oh.data_ptr() if oh is not None else None, _raw_stream(self.dev_index))
        if rc:
            _check(rc, "emm_extract_cache")
        return templates, sr, oh


TIMER_XCORR, TIMER_TOWER = 0, 1


# Capacity cliffs of the fast paths fall back to slower (correct) ones: every such event is counted here so that a
# benchmark / a service can REPORT them instead of silently running slower.  Keys:
#   refine_library_gemm  box-head refinement of more rows than the weight-streaming kernels take (library GEMMs instead)
#   host_solver          a frame beyond the one-launch solver's capacity (or with fields it does not carry): host path
#   unhinted_head        a pooling + correlation launch that ranked its rois itself although an order hint could exist
#   general_frame        a tracking-loop frame that did not take the one-launch path at all
#   multi_camera_per_camera  a ``solver.solve_batched`` call that ran camera by camera (an image failed ``_device_path``)
#   rpn_torch            an RPN proposal selection on device tensors beyond ``rpn_proposals``' capacities (torch composition)
#   box_detect_torch     a box-head call on id-less device proposals that ``box_detect_post`` does not take (torch composition)
#   refine_per_camera    a multi-camera step whose refinement wanted the batched call and ran camera by camera (an image of
#                        more than ``BOX_REFINE_IMAGE_ROWS`` rows, the call's caps); present from import so that a step that
#                        does not fall back leaves the table as it was
import collections as _collections
FALLBACKS = _collections.Counter()
FALLBACKS["refine_per_camera"] = 0
#   rpn_head_torch       an ``rpn.RPNHead`` call on device maps that ``rpn_head`` does not take (training mode, C or A beyond
#                        its capacities, more images or levels): the ``F.conv2d`` composition; present from import
FALLBACKS["rpn_head_torch"] = 0
#   fpn_torch            an ``fpn.FPN`` call on device maps that ``fpn`` does not take (training or grad mode, a GroupNorm /
#                        ReLU conv block, ``LastLevelP6P7``, channel counts beyond the kernels' capacities)
FALLBACKS["fpn_torch"] = 0
#   dla_torch            a ``dla.DLA`` call on device images that ``dla`` does not take (grad mode with trainable parameters,
#                        images that are not contiguous NCHW, sizes that are no multiple of 32, levels / channels beyond the
#                        kernels' capacities)
FALLBACKS["dla_torch"] = 0
# speculative next-frame heads of the tracking loop (TrackingLoop.forward(..., next_features=...)): launched / used as they
# were / discarded because the row count, the memory, the features or the parameters were not what the launch assumed
SPECULATION = _collections.Counter()


TOWER_FORMS = {0: "direct fp32 (no packed path)", 1: "Winograd, one 16-channel tile per workgroup, fp32 matrix instructions",
               2: "Winograd, two tiles per workgroup, fp32 matrix instructions",
               3: "Winograd, two tiles per workgroup, two-part fp16 operands on v_mfma_f32_16x16x32_f16"}


def tower_form(n, channels, ho=16):
    """Which form of the tower kernel ``n`` tracks get from the current library (``smot_emm_tower_form``): 0..3, see
    ``TOWER_FORMS``."""
    return int(load_library().smot_emm_tower_form(int(n), int(channels), int(ho)))


def fused_kernel_name():
    """Name of the kernel ``smot_emm_track_fwd`` runs for search-region pooling + cross-correlation at the
    DLA shape family (what bench.py's roofline and the rocprofv3 summaries in profiles/ refer to)."""
    return "sr_xcorr_fused9_kernel<30,15,2,true,8,false,1>"       # (..., planes per workgroup, no plane-pair FMA phase, matrix-pipe correlation)


def kernel_timer_begin(slot, max_launches, stride=1):
    """Start bracketing the kernels of ``slot`` with HIP events on their launch stream (bench.py)."""
    _check(load_library().smot_kernel_timer_begin(int(slot), int(max_launches), int(stride)), "kernel_timer_begin")


def kernel_timer_bracket_overhead(reps=200):
    """Median span (us) of an empty event bracket on the current stream."""
    us = ctypes.c_double(0.0)
    _check((_lib or load_library()).smot_kernel_timer_bracket_overhead(_stream(), int(reps), ctypes.byref(us)),
           "kernel_timer_bracket_overhead")
    return us.value


def dispatch_floor_us(workgroups, threads, reps=200):
    """Average span of the kernel timer's event bracket around an EMPTY kernel of this launch shape on the current stream
    (``smot_dispatch_floor_fwd``; timer slot 0 must be idle): the bracket's own floor (4.1 us on MI355X), an upper bound on
    the fixed cost of a dispatch — rocprofv3 reads 0.8-1.5 us for the same kernel from the packet's timestamps."""
    lib = _lib or load_library()
    for _ in range(20):
        _check(lib.smot_dispatch_floor_fwd(int(workgroups), int(threads), _stream()), "dispatch_floor")
    kernel_timer_begin(TIMER_XCORR, reps, 1)
    for _ in range(reps):
        _check(lib.smot_dispatch_floor_fwd(int(workgroups), int(threads), _stream()), "dispatch_floor")
    torch.cuda.synchronize()
    ms, cnt = kernel_timer_end(TIMER_XCORR)
    return ms * 1e3 / max(cnt, 1)


def kernel_timer_end(slot):
    """→ (total milliseconds inside the slot's kernels, launches timed)."""
    tot = ctypes.c_double(0.0)
    n = ctypes.c_int(0)
    _check(load_library().smot_kernel_timer_end(int(slot), ctypes.cast(ctypes.byref(tot), ctypes.c_void_p),
                                                ctypes.cast(ctypes.byref(n), ctypes.c_void_p)), "kernel_timer_end")
    return tot.value, n.value


def xcorr_timer_begin(max_launches):
    kernel_timer_begin(TIMER_XCORR, max_launches)


def xcorr_timer_end():
    return kernel_timer_end(TIMER_XCORR)


def sr_xcorr_fused(features, boxes, sr, templates, rx, rz, scales, sampling_ratio, pad_pixels, return_pooled=False):
    """Search-region pooling + depthwise cross-correlation in one kernel → response ``[N,C,Ho,Ho]``
    (and the pooled ``[N,C,rx,rx]`` planes when asked — test hook)."""
    lib = load_library()
    boxes = _dev_f32(boxes, "boxes")
    sr = _dev_f32(sr, "sr")
    templates = _dev_f32(templates, "template_features")
    N = boxes.shape[0]
    # (the 35 / 7 shape's kernel has no channels-last form: such maps go through the NCHW copy there)
    feats, fp, hs, ws_, sc, ft = _level_arrays(features, scales, nhwc=not ((int(rx), int(rz)) == (35, 7) and not return_pooled))
    C = feats[0].shape[1]
    L = len(scales)
    pc = (ctypes.c_int * L)(*[int(pad_pixels / ((2 ** i) * 4)) for i in range(L)])
    ho = rx - rz + 1
    resp = torch.empty((N, C, ho, ho), dtype=torch.float32, device=boxes.device)
    pooled = torch.empty((N, C, rx, rx), dtype=torch.float32, device=boxes.device) if return_pooled else None
    with _Launch(boxes, sr, templates, *feats) as ln:
        if (int(rx), int(rz)) == (35, 7) and pooled is None:        # the second yaml family's shape: its own entry
            rc = lib.smot_sr_xcorr_gather_typed_fwd(_cast(fp), ft, _cast(hs), _cast(ws_), _cast(pc), _cast(sc), L, C, _ptr(boxes),
                                              _ptr(sr), _ptr(templates), N, int(rx), int(rz), int(sampling_ratio),
                                              _ptr(resp), ln.stream)
        else:
            rc = lib.smot_sr_xcorr_fused_typed_fwd(_cast(fp), ft, _cast(hs), _cast(ws_), _cast(pc), _cast(sc), L, C, _ptr(boxes),
                                             _ptr(sr), _ptr(templates), N, int(rx), int(rz), int(sampling_ratio),
                                             _ptr(resp), _ptr(pooled), ln.stream)
    _check(rc, "sr_xcorr_fused")
    return (resp, pooled) if return_pooled else resp


def _nms_sorted(boxes, scores, thresh):
    """The part ``nms_keep_mask`` and ``nms`` share: sort by descending score (stable) and one suppression launch ->
    (device, order, keep flags uint8 in sorted order); (device, None, None) for no boxes."""
    lib = load_library()
    boxes = _dev_f32(boxes, "boxes")
    scores = _dev_f32(scores, "scores")
    n = boxes.shape[0]
    if n == 0:
        return boxes.device, None, None
    order = torch.argsort(scores, descending=True, stable=True)
    sorted_boxes = boxes[order].contiguous()
    ws = torch.empty((max(lib.smot_nms_ws_bytes(n) // 8, 1),), dtype=torch.int64, device=boxes.device)
    keep = torch.empty((n,), dtype=torch.uint8, device=boxes.device)
    with _Launch(boxes, scores) as ln:
        rc = lib.smot_nms_fwd(_ptr(sorted_boxes), n, float(thresh), _ptr(ws), _ptr(keep), ln.stream)
    _check(rc, "nms")
    return boxes.device, order, keep


def nms_keep_mask(boxes, scores, thresh):
    """Greedy NMS as a device-resident boolean mask in the ORIGINAL box order (True = kept) — no host
    synchronisation; ``nms`` below turns it into upstream's index list."""
    dev, order, keep = _nms_sorted(boxes, scores, thresh)
    if order is None:
        return torch.empty((0,), dtype=torch.bool, device=dev)
    mask = torch.empty((order.shape[0],), dtype=torch.bool, device=dev)
    mask[order] = keep.bool()
    return mask


def nms(boxes, scores, thresh):
    """[UPSTREAM] ``_C.nms(dets, scores, thresh)`` semantics: indices of the kept boxes, ascending (original
    order), after greedy suppression in descending-score order with the +1 IoU convention.  One host sync
    (the number of kept boxes), as in the reference."""
    dev, order, keep = _nms_sorted(boxes, scores, thresh)
    if order is None:
        return torch.empty((0,), dtype=torch.int64, device=dev)
    return order[keep.bool()].sort()[0]


# capacities of ``rpn_proposals`` (include/smot_emm.h): beyond them ``siammot_amd.rpn.RPNPostProcessor`` takes its torch path
RPN_MAX_TOP_N = 2048
RPN_MAX_IMAGES = 64
RPN_MAX_LEVELS = 8
RPN_MAX_ANCHOR_TENSORS = 128
RPN_MERGE_LDS_BYTES = 64 * 1024      # levels x rows per level x 4 + 64 must fit (the merge's keys and counters)
RPN_MAX_MASK_BYTES = 64 << 20        # NMS bitmask scratch the module accepts (see rpn_mask_bytes); larger calls take the torch path


def rpn_mask_bytes(num_images, num_levels, pre_nms_top_n):
    """Size of the largest part of ``rpn_proposals``' workspace, the NMS bitmasks: 8 bytes per (candidate row, 64-column
    tile) of every (image, level), allocated for ``pre_nms_top_n`` rows whether or not they survive the size filter —
    2.6 MB at 4 images x 5 levels x 1000, 268 MB at the capacities 64 x 8 x 2048."""
    return num_images * num_levels * pre_nms_top_n * ((pre_nms_top_n + 63) // 64) * 8


def _al4(words):
    return (words + 3) & ~3


def rpn_proposals(objectness, box_regression, anchors, image_sizes, pre_nms_top_n, post_nms_top_n, fpn_post_nms_top_n,
                  nms_thresh, min_size, amodal=False, weights=(1.0, 1.0, 1.0, 1.0), xform_clip=None,
                  return_candidates=False):
    """RPN proposal selection of all images and levels in one library call, free of host synchronisation
    (``smot_rpn_proposals_fwd``).

    objectness: L tensors ``[N, A, H, W]`` (logits); box_regression: L tensors ``[N, 4A, H, W]``; one dtype per call (fp32,
    fp16 or bf16; a half call returns the bits of the call on ``.float()``); strided inputs are copied.  anchors: per image
    a sequence of L fp32 ``[A*H*W, 4]`` tensors in the reference's flattened order, read in place.  image_sizes: per image
    ``(width, height)``.

    Returns ``(boxes [N, cap, 4], objectness [N, cap], count [N] int32)``, rows beyond ``count`` zero, with
    ``cap = fpn_post_nms_top_n`` — or, with one level, where upstream makes no selection across levels,
    ``min(post_nms_top_n, pre_nms_top_n)``.  ``return_candidates=True`` adds a dict of the per-level candidates
    ``count [N, L]``, ``index [N, L, pre]``, ``logit [N, L, pre]``, ``box [N, L, pre, 4]`` (sorted flat indices, their
    logits, the decoded boxes before clipping): views of this call's own workspace."""
    import math
    lib = _lib or load_library()
    L = len(objectness)
    N = len(anchors)
    if L < 1 or len(box_regression) != L or len(image_sizes) != N:
        raise RuntimeError("siammot_amd.rpn_proposals: %d objectness levels, %d regression levels, %d images with anchors, "
                           "%d image sizes" % (L, len(box_regression), N, len(image_sizes)))
    obj = [_dev_feat(o, "objectness[%d]" % l) for l, o in enumerate(objectness)]
    reg = [_dev_feat(r, "box_regression[%d]" % l) for l, r in enumerate(box_regression)]
    ft = _feat_type(obj + reg)
    dev = obj[0].device
    shapes = []
    for l in range(L):
        if obj[l].dim() != 4 or obj[l].shape[0] != N or tuple(reg[l].shape) != (N, 4 * obj[l].shape[1]) + tuple(obj[l].shape[2:]):
            raise RuntimeError("siammot_amd.rpn_proposals: level %d has objectness %s and regression %s for %d images"
                               % (l, tuple(obj[l].shape), tuple(reg[l].shape), N))
        shapes.append(tuple(obj[l].shape[1:]))
    anc = []
    for i in range(N):
        if len(anchors[i]) != L:
            raise RuntimeError("siammot_amd.rpn_proposals: image %d has %d anchor levels, expected %d" % (i, len(anchors[i]), L))
        for l in range(L):
            a, h, w = shapes[l]
            anc.append(_chk(anchors[i][l], "anchors[%d][%d]" % (i, l), (a * h * w, 4)))
    pre, post, fpn = int(pre_nms_top_n), int(post_nms_top_n), int(fpn_post_nms_top_n)
    cap = fpn if L > 1 else min(post, pre)
    ia = (ctypes.c_int * L)(*[s[0] for s in shapes])
    ih = (ctypes.c_int * L)(*[s[1] for s in shapes])
    iw = (ctypes.c_int * L)(*[s[2] for s in shapes])
    nbytes = lib.smot_rpn_proposals_ws_bytes(N, L, _cast(ia), _cast(ih), _cast(iw), pre, post)
    if nbytes < 0:
        _check(-1, "rpn_proposals")
    stream = _stream(dev)
    if return_candidates:
        work = torch.empty((nbytes // 4,), dtype=_F32, device=dev)
    else:
        work = _workspace(dev, nbytes // 4, stream.value)
    boxes = torch.empty((N, cap, 4), dtype=_F32, device=dev)
    scores = torch.empty((N, cap), dtype=_F32, device=dev)
    count = torch.empty((N,), dtype=torch.int32, device=dev)
    po = (ctypes.c_void_p * L)(*[t.data_ptr() for t in obj])
    pr = (ctypes.c_void_p * L)(*[t.data_ptr() for t in reg])
    pa = (ctypes.c_void_p * (N * L))(*[t.data_ptr() for t in anc])
    wh = (ctypes.c_float * (2 * N))(*[float(v) for s in image_sizes for v in (s[0], s[1])])
    wx, wy, ww, wh_ = [float(v) for v in weights]
    with _Launch(*(obj + reg + anc)) as ln:
        rc = lib.smot_rpn_proposals_fwd(_cast(po), _cast(pr), ft, _cast(ia), _cast(ih), _cast(iw), L, N, _cast(pa), _cast(wh),
                                        pre, post, cap, float(nms_thresh), float(min_size), 1 if amodal else 0,
                                        wx, wy, ww, wh_, float(math.log(1000.0 / 16) if xform_clip is None else xform_clip),
                                        _ptr(work), _ptr(boxes), _ptr(scores), _ptr(count), ln.stream)
    _check(rc, "rpn_proposals")
    if not return_candidates:
        return boxes, scores, count
    NL = N * L
    o1 = _al4(NL)
    o2 = o1 + _al4(NL * pre)
    o3 = o2 + _al4(NL * pre)
    cand = {"count": work[:NL].view(torch.int32).view(N, L),
            "index": work[o1:o1 + NL * pre].view(torch.int32).view(N, L, pre),
            "logit": work[o2:o2 + NL * pre].view(N, L, pre),
            "box": work[o3:o3 + NL * pre * 4].view(N, L, pre, 4)}
    return boxes, scores, count, cand


# capacities of ``rpn_head`` (include/smot_emm.h): beyond them ``siammot_amd.rpn.RPNHead`` takes its torch composition
RPN_HEAD_MAX_CHANNELS = 512
RPN_HEAD_CHANNEL_STEP = 32
RPN_HEAD_MAX_ROWS = 64               # 5 A: the objectness and regression rows of the two 1x1 heads


def rpn_head_shapes_ok(C, A):
    return C >= 32 and C % RPN_HEAD_CHANNEL_STEP == 0 and C <= RPN_HEAD_MAX_CHANNELS and 1 <= A and 5 * A <= RPN_HEAD_MAX_ROWS


def _rpn_head_pack(who, ct, conv_w, conv_b, cls_w, cls_b, bbox_w, bbox_b):
    lib = _lib or load_library()
    C, A = int(conv_w.shape[0]), int(cls_w.shape[0])
    ts = [_chk(conv_w, "conv.weight", (C, C, 3, 3)), _chk(conv_b, "conv.bias", (C,)),
          _chk(cls_w.reshape(A, -1), "cls_logits.weight", (A, C)), _chk(cls_b, "cls_logits.bias", (A,)),
          _chk(bbox_w.reshape(4 * A, -1), "bbox_pred.weight", (4 * A, C)), _chk(bbox_b, "bbox_pred.bias", (4 * A,))]
    n = lib.smot_rpn_head_packed_floats(C, A) if ct is None else lib.smot_rpn_head_half_packed_floats(C, A, ct)
    if n < 0:
        _check(-2, who)
    packed = torch.empty((n,), dtype=_F32, device=conv_w.device)
    with _Launch(*ts) as ln:
        if ct is None:
            rc = lib.smot_rpn_head_pack(*([_ptr(t) for t in ts] + [C, A, _ptr(packed), ln.stream]))
        else:
            rc = lib.smot_rpn_head_half_pack(*([_ptr(t) for t in ts] + [C, A, ct, _ptr(packed), ln.stream]))
    _check(rc, who)
    return packed


def rpn_head_pack(conv_w, conv_b, cls_w, cls_b, bbox_w, bbox_b):
    """The RPN head's parameters (upstream's ``conv`` ``[C, C, 3, 3]``, ``cls_logits`` ``[A, C, 1, 1]``, ``bbox_pred``
    ``[4A, C, 1, 1]`` and their biases, fp32 device tensors) in the operand order of ``rpn_head`` (``smot_rpn_head_pack``:
    one launch, no synchronisation).  -> fp32 ``[smot_rpn_head_packed_floats(C, A)]``.
    The image is ordered on the current stream only: a caller who packs on one stream and consumes on another orders the two
    himself (the modules do it through ``StreamImage``)."""
    return _rpn_head_pack("rpn_head_pack", None, conv_w, conv_b, cls_w, cls_b, bbox_w, bbox_b)


def rpn_head_half_pack(conv_w, conv_b, cls_w, cls_b, bbox_w, bbox_b, compute_dtype):
    """``rpn_head_pack`` for ``rpn_head_half`` (``smot_rpn_head_half_pack``): ``conv.weight`` rounded once to
    ``compute_dtype`` (``tensor.to``'s rounding), every bias and the two 1x1 heads' rows in fp32.  The tensor serves this
    ``compute_dtype`` and no other mode.  One launch, no synchronisation, ordered on the current stream only, as
    ``rpn_head_pack``."""
    ct = _dla_ctype(compute_dtype, "rpn_head_half_pack")
    return _rpn_head_pack("rpn_head_half_pack", ct, conv_w, conv_b, cls_w, cls_b, bbox_w, bbox_b)


def _rpn_head(who, ct, features, packed, C, A):
    lib = _lib or load_library()
    L = len(features)
    if L < 1:
        raise RuntimeError("siammot_amd.%s: no feature level" % who)
    feats = [_dev_feat(f, "features[%d]" % l) for l, f in enumerate(features)]
    ft = _feat_type(feats)
    N = feats[0].shape[0]
    for l, f in enumerate(feats):
        if f.dim() != 4 or f.shape[0] != N or f.shape[1] != C:
            raise RuntimeError("siammot_amd.%s: features[%d] has shape %s, expected [%d, %d, H, W]"
                               % (who, l, tuple(f.shape), N, C))
    dev = feats[0].device
    obj = [torch.empty((N, A) + tuple(f.shape[2:]), dtype=_F32, device=dev) for f in feats]
    reg = [torch.empty((N, 4 * A) + tuple(f.shape[2:]), dtype=_F32, device=dev) for f in feats]
    fp = (ctypes.c_void_p * L)(*[t.data_ptr() for t in feats])
    po = (ctypes.c_void_p * L)(*[t.data_ptr() for t in obj])
    pr = (ctypes.c_void_p * L)(*[t.data_ptr() for t in reg])
    ih = (ctypes.c_int * L)(*[f.shape[2] for f in feats])
    iw = (ctypes.c_int * L)(*[f.shape[3] for f in feats])
    with _Launch(*(feats + [packed])) as ln:
        if ct is None:
            rc = lib.smot_rpn_head_fwd(_cast(fp), ft, _cast(ih), _cast(iw), L, N, int(C), int(A), _ptr(packed), _cast(po),
                                       _cast(pr), ln.stream)
        else:
            rc = lib.smot_rpn_head_half_fwd(_cast(fp), ft, _cast(ih), _cast(iw), L, N, int(C), int(A), ct, _ptr(packed),
                                            _cast(po), _cast(pr), ln.stream)
    _check(rc, who)
    return obj, reg


def rpn_head(features, packed, C, A):
    """Upstream's ``RPNHead.forward`` on all images and levels of a call in one launch (``smot_rpn_head_fwd``), free of host
    synchronisation.  features: L maps ``[N, C, H_l, W_l]`` of one dtype (fp32, fp16 or bf16; a half call returns the bits
    of the call on ``.float()``); anything but contiguous NCHW (channels-last, strided views) is copied.  packed:
    ``rpn_head_pack``'s tensor.  -> (objectness: L fp32 ``[N, A, H_l, W_l]``, regression: L fp32 ``[N, 4A, H_l, W_l]``)."""
    return _rpn_head("rpn_head", None, features, packed, C, A)


def rpn_head_half(features, packed, C, A, compute_dtype):
    """``rpn_head`` in half compute mode (``smot_rpn_head_half_fwd``): the 3x3 convolution multiplies the maps and
    ``conv.weight`` rounded to ``compute_dtype`` (maps as they are loaded, filters in ``rpn_head_half_pack``) on the 16-bit
    matrix instruction and accumulates in fp32; its bias / ReLU result stays fp32 on the chip and the two 1x1 heads run on
    it as in ``rpn_head``, unrounded.  An fp16 operand beyond 65,504 in magnitude is +-inf.  Arguments and results
    otherwise as ``rpn_head``'s; the same single launch.  packed: ``rpn_head_half_pack``'s tensor of this ``compute_dtype``."""
    return _rpn_head("rpn_head_half", _dla_ctype(compute_dtype, "rpn_head_half"), features, packed, C, A)


# capacities of ``fpn`` (include/smot_emm.h): beyond them ``siammot_amd.fpn.FPN`` takes its torch composition
FPN_MAX_LEVELS = 7
FPN_MAX_CHANNELS = 512
FPN_CHANNEL_STEP = 32
FPN_MAX_IN_CHANNELS = 2048
FPN_IN_CHANNEL_STEP = 16


def fpn_shapes_ok(in_channels, C):
    return (1 <= len(in_channels) <= FPN_MAX_LEVELS and C >= 32 and C % FPN_CHANNEL_STEP == 0 and C <= FPN_MAX_CHANNELS
            and all(16 <= c <= FPN_MAX_IN_CHANNELS and c % FPN_IN_CHANNEL_STEP == 0 for c in in_channels))


# the half compute mode's K step (``fpn_half``): every level's input channels in multiples of 32
FPN_HALF_IN_CHANNEL_STEP = 32


def fpn_half_shapes_ok(in_channels, C):
    return fpn_shapes_ok(in_channels, C) and all(c % FPN_HALF_IN_CHANNEL_STEP == 0 for c in in_channels)


def _fpn_pack(who, ct, inner, layer):
    lib = _lib or load_library()
    L = len(inner)
    if L < 1 or len(layer) != L:
        raise RuntimeError("siammot_amd.%s: %d lateral and %d output blocks" % (who, L, len(layer)))
    C = int(inner[0][0].shape[0])
    cin = [int(w.shape[1]) for w, _ in inner]
    iw = [_chk(w.reshape(C, -1), "fpn_inner%d.weight" % (l + 1), (C, cin[l])) for l, (w, _) in enumerate(inner)]
    ib = [_chk(b, "fpn_inner%d.bias" % (l + 1), (C,)) for l, (_, b) in enumerate(inner)]
    lw = [_chk(w, "fpn_layer%d.weight" % (l + 1), (C, C, 3, 3)) for l, (w, _) in enumerate(layer)]
    lb = [_chk(b, "fpn_layer%d.bias" % (l + 1), (C,)) for l, (_, b) in enumerate(layer)]
    ic = (ctypes.c_int * L)(*cin)
    n = lib.smot_fpn_packed_floats(L, _cast(ic), C) if ct is None else lib.smot_fpn_half_packed_floats(L, _cast(ic), C, ct)
    if n < 0:
        _check(-2, who)
    packed = torch.empty((n,), dtype=_F32, device=iw[0].device)
    arrays = [(ctypes.c_void_p * L)(*[t.data_ptr() for t in ts]) for ts in (iw, ib, lw, lb)]
    with _Launch(*(iw + ib + lw + lb)) as ln:
        if ct is None:
            rc = lib.smot_fpn_pack(*([_cast(a) for a in arrays] + [L, _cast(ic), C, _ptr(packed), ln.stream]))
        else:
            rc = lib.smot_fpn_half_pack(*([_cast(a) for a in arrays] + [L, _cast(ic), C, ct, _ptr(packed), ln.stream]))
    _check(rc, who)
    return packed


def fpn_pack(inner, layer):
    """The pyramid's parameters (per level, finest first: ``inner[l]`` = upstream's ``fpn_inner{l+1}`` ``(weight [C, Cin_l,
    1, 1], bias [C])``, ``layer[l]`` = ``fpn_layer{l+1}`` ``(weight [C, C, 3, 3], bias [C])``, fp32 device tensors) in the
    operand order of ``fpn`` (``smot_fpn_pack``: one launch, no synchronisation).  -> fp32 ``[smot_fpn_packed_floats]``.
    The image is ordered on the current stream only: a caller who packs on one stream and consumes on another orders the two
    himself (the modules do it through ``StreamImage``)."""
    return _fpn_pack("fpn_pack", None, inner, layer)


def fpn_half_pack(inner, layer, compute_dtype):
    """``fpn_pack`` for ``fpn_half`` (``smot_fpn_half_pack``): both convolutions' filters rounded once to ``compute_dtype``
    (``tensor.to``'s rounding), the biases in fp32.  The tensor serves this ``compute_dtype`` and no other mode.  One launch, no
    synchronisation, ordered on the current stream only, as ``fpn_pack``."""
    return _fpn_pack("fpn_half_pack", _dla_ctype(compute_dtype, "fpn_half_pack"), inner, layer)


def _fpn(who, ct, stages, packed, in_channels, C, out_dtype, top_block):
    lib = _lib or load_library()
    L = len(stages)
    if L < 1 or len(in_channels) != L:
        raise RuntimeError("siammot_amd.%s: %d stage maps for %d levels" % (who, L, len(in_channels)))
    if out_dtype not in FEAT_TYPES:
        raise RuntimeError("siammot_amd.%s: out_dtype must be float32, float16 or bfloat16, got %s" % (who, out_dtype))
    feats = [_dev_feat(f, "stages[%d]" % l) for l, f in enumerate(stages)]
    ft = _feat_type(feats)
    N = feats[0].shape[0]
    for l, f in enumerate(feats):
        if f.dim() != 4 or f.shape[0] != N or f.shape[1] != in_channels[l]:
            raise RuntimeError("siammot_amd.%s: stages[%d] has shape %s, expected [%d, %d, H, W]"
                               % (who, l, tuple(f.shape), N, in_channels[l]))
    dev = feats[0].device
    sizes = [(int(f.shape[2]), int(f.shape[3])) for f in feats]
    ic = (ctypes.c_int * L)(*[int(c) for c in in_channels])
    ih = (ctypes.c_int * L)(*[s[0] for s in sizes])
    iw = (ctypes.c_int * L)(*[s[1] for s in sizes])
    nbytes = lib.smot_fpn_ws_bytes(L, _cast(ih), _cast(iw), N, int(C))
    if nbytes < 0:
        raise RuntimeError("siammot_amd.%s: %d levels of %d images (at most %d levels, %d images, no empty map)"
                           % (who, L, N, FPN_MAX_LEVELS, RPN_MAX_IMAGES))
    ws = torch.empty((max(nbytes // 4, 4),), dtype=_F32, device=dev)
    if top_block:
        sizes = sizes + [((sizes[-1][0] + 1) // 2, (sizes[-1][1] + 1) // 2)]
    out = [torch.empty((N, int(C), h, w), dtype=out_dtype, device=dev) for (h, w) in sizes]
    fp = (ctypes.c_void_p * L)(*[t.data_ptr() for t in feats])
    po = (ctypes.c_void_p * len(out))(*[t.data_ptr() for t in out])
    with _Launch(*(feats + [packed])) as ln:
        if ct is None:
            rc = lib.smot_fpn_fwd(_cast(fp), ft, _cast(ic), _cast(ih), _cast(iw), L, N, int(C), _ptr(packed), _ptr(ws),
                                  _cast(po), FEAT_TYPES[out_dtype], 1 if top_block else 0, ln.stream)
        else:
            rc = lib.smot_fpn_half_fwd(_cast(fp), ft, _cast(ic), _cast(ih), _cast(iw), L, N, int(C), ct, _ptr(packed), _ptr(ws),
                                       _cast(po), FEAT_TYPES[out_dtype], 1 if top_block else 0, ln.stream)
    _check(rc, who)
    return out


def fpn(stages, packed, in_channels, C, out_dtype=torch.float32, top_block=True):
    """Upstream's ``FPN.forward`` (top-down path resized bilinearly to the lateral's size) on all images of a call in L + 1
    launches (``smot_fpn_fwd``), free of host synchronisation.  stages: L maps ``[N, Cin_l, H_l, W_l]``, finest first, of
    one dtype (fp32, fp16 or bf16; a half call returns the bits of the call on ``.float()``); anything but contiguous NCHW
    is copied.  packed: ``fpn_pack``'s tensor.  -> L (+ 1 with ``top_block``: ``LastLevelMaxPool``) contiguous NCHW maps
    ``[N, C, H_l, W_l]`` of ``out_dtype`` (a half output is the fp32 value rounded to nearest even)."""
    return _fpn("fpn", None, stages, packed, in_channels, C, out_dtype, top_block)


def fpn_half(stages, packed, in_channels, C, compute_dtype, out_dtype=torch.float32, top_block=True):
    """``fpn`` in half compute mode (``smot_fpn_half_fwd``): the laterals and the 3x3 convolutions multiply operands rounded
    to ``compute_dtype`` (stage maps and the fp32 ``last`` maps as they are loaded, filters in ``fpn_half_pack``) on the
    16-bit matrix instruction and accumulate in fp32; the bias adds, the bilinear top-down path, ``last`` in the workspace and
    the stores are ``fpn``'s.  An fp16 operand beyond 65,504 in magnitude is +-inf.  Every ``Cin_l`` a multiple of 32
    (``fpn_half_shapes_ok``).  Arguments and results otherwise as ``fpn``'s; the same L + 1 launches and workspace."""
    return _fpn("fpn_half", _dla_ctype(compute_dtype, "fpn_half"), stages, packed, in_channels, C, out_dtype, top_block)


# capacities of ``dla`` (include/smot_emm.h, DLA BACKBONE): beyond them ``siammot_amd.dla.DLA`` takes its torch composition
DLA_MAX_CHANNELS = 1024
DLA_CHANNEL_STEP = 32
DLA_SIZE_STEP = 32


# block types of the DLA bodies (SMOT_DLA_BLOCK_* of include/smot_emm.h) and the deepest tree ``dla_net`` walks
DLA_BLOCKS = {"basic": 0, "bottleneck": 1}
DLA_MAX_DEPTH = 5


def dla_shapes_ok(levels, channels, H=None, W=None, N=1, block="basic"):
    """``dla`` / ``dla_net`` take a network of these ``levels`` / ``channels`` and this ``block`` (and, if given, ``N`` images of
    ``H x W``): trees of depth 1 .. 5; a bottleneck network's ``channels[2:]`` are multiples of 64 (``mid`` of 32)."""
    levels, channels = tuple(int(v) for v in levels), tuple(int(v) for v in channels)
    if block not in DLA_BLOCKS or len(levels) != 6 or len(channels) != 6 or levels[:2] != (1, 1):
        return False
    if any(not 1 <= v <= DLA_MAX_DEPTH for v in levels[2:]):
        return False
    if channels[0] not in (16, 32) or any(c < 32 or c % DLA_CHANNEL_STEP or c > DLA_MAX_CHANNELS for c in channels[1:]):
        return False
    wide = 2 if block == "bottleneck" else 1                     # (a bottleneck's conv1 map: twice the level's own)
    if wide == 2 and any(c % (2 * DLA_CHANNEL_STEP) for c in channels[2:]):
        return False
    if H is None and W is None:
        return True
    H, W = int(H), int(W)
    if H < 32 or W < 32 or H % DLA_SIZE_STEP or W % DLA_SIZE_STEP or not 1 <= N <= RPN_MAX_IMAGES:
        return False
    return max(channels[k] * (H >> k) * (W >> k) * (wide if k >= 2 else 1) for k in range(6)) < 2 ** 31


def _int6(v):
    return (ctypes.c_int * 6)(*[int(x) for x in v])


# ``operands`` of the DLA operators: "fp32": every convolution on the fp32 matrix instruction; "split16": the trees' 3x3
# convolutions on the 16-bit matrix instruction with three-part bf16 operands and fp32 accumulation (fp32-grade results;
# include/smot_emm.h, DLA BACKBONE, SPLIT OPERANDS)
DLA_OPERANDS = ("fp32", "split16")


def _dla_split(operands, who):
    if operands not in DLA_OPERANDS:
        raise ValueError("siammot_amd.%s: operands must be \"fp32\" or \"split16\", got %r" % (who, operands))
    return operands == "split16"


def dla_pack(convs, levels, channels, operands="fp32"):
    """The body's parameters in the operand order of ``dla`` (``smot_dla_pack``, or ``smot_dla_split_pack`` for ``operands``
    "split16": the image of one mode does not serve the other; one launch per convolution, no synchronisation).  convs: ``(weight [Cout, Cin, k, k], scale [Cout], shift [Cout])`` per convolution in LAUNCH ORDER
    (include/smot_emm.h; ``dla.DLA.convs()``), fp32 device tensors, ``scale`` / ``shift`` the frozen BN's.  -> fp32
    ``[smot_dla_packed_floats]``.
    The image is ordered on the current stream only: a caller who packs on one stream and consumes on another orders the two
    himself (the modules do it through ``StreamImage``)."""
    lib = _lib or load_library()
    split = _dla_split(operands, "dla_pack")
    lv, ch = _int6(levels), _int6(channels)
    n = (lib.smot_dla_split_packed_floats if split else lib.smot_dla_packed_floats)(_cast(lv), _cast(ch))
    if n < 0:
        _check(-2, "dla_pack")
    ts = [[_chk(t, "dla_pack: convs[%d][%d]" % (i, j), tuple(t.shape)) for j, t in enumerate(c)] for i, c in enumerate(convs)]
    packed = torch.empty((n,), dtype=_F32, device=ts[0][0].device)
    arrays = [(ctypes.c_void_p * len(ts))(*[c[j].data_ptr() for c in ts]) for j in range(3)]
    with _Launch(*[t for c in ts for t in c]) as ln:
        rc = (lib.smot_dla_split_pack if split else lib.smot_dla_pack)(
            _cast(lv), _cast(ch), _cast(arrays[0]), _cast(arrays[1]), _cast(arrays[2]), len(ts), _ptr(packed), ln.stream)
    _check(rc, "dla_pack")
    return packed


def dla(images, packed, levels, channels, out_dtype=torch.float32, operands="fp32"):
    """Upstream's ``DLA.forward`` (DlaBasic blocks, frozen BN) on all images of a call (``smot_dla_fwd``: 37 launches for
    DLA-34), free of host synchronisation.  images: ``[N, 3, H, W]`` fp32, fp16 or bf16 (a half call returns the bits of the
    call on ``.float()``), H and W multiples of 32; anything but contiguous NCHW is copied.  packed: ``dla_pack``'s tensor.
    -> the four contiguous NCHW stage maps ``[N, channels[k], H >> k, W >> k]``, k = 2 .. 5, of ``out_dtype`` (a half output
    is the fp32 value rounded to nearest even; the next stage reads the fp32 value).  ``operands``: the mode ``packed`` was
    made for (``smot_dla_split_fwd`` for "split16")."""
    lib = _lib or load_library()
    split = _dla_split(operands, "dla")
    if out_dtype not in FEAT_TYPES:
        raise RuntimeError("siammot_amd.dla: out_dtype must be float32, float16 or bfloat16, got %s" % (out_dtype,))
    x = _dev_feat(images, "images")
    if x.dim() != 4 or x.shape[1] != 3:
        raise RuntimeError("siammot_amd.dla: images has shape %s, expected [N, 3, H, W]" % (tuple(x.shape),))
    N, H, W = int(x.shape[0]), int(x.shape[2]), int(x.shape[3])
    lv, ch = _int6(levels), _int6(channels)
    nbytes = lib.smot_dla_ws_bytes(_cast(lv), _cast(ch), N, H, W)
    if nbytes < 0:
        _check(-2, "dla")
    ws = torch.empty((max(nbytes // 4, 4),), dtype=_F32, device=x.device)
    out = [torch.empty((N, int(channels[k]), H >> k, W >> k), dtype=out_dtype, device=x.device) for k in range(2, 6)]
    po = (ctypes.c_void_p * 4)(*[t.data_ptr() for t in out])
    with _Launch(x, packed) as ln:
        rc = (lib.smot_dla_split_fwd if split else lib.smot_dla_fwd)(
            _ptr(x), FEAT_TYPES[x.dtype], N, H, W, _cast(lv), _cast(ch), _ptr(packed), _ptr(ws), _cast(po), FEAT_TYPES[out_dtype],
            ln.stream)
    _check(rc, "dla")
    return out


def dla_conv3x3_form(N, H, W, Cout, stride, operands="fp32"):
    """Which form of the 3x3 kernel ``dla_conv3x3`` runs for ``N`` images of ``H x W`` (``smot_dla_conv3x3_form``): ``(WR,
    NM)`` — the row groups of a workgroup's four waves (1, 2 or 4) and the M-tiles per channel pair."""
    lib = _lib or load_library()
    fn = lib.smot_dla_conv3x3_split_form if _dla_split(operands, "dla_conv3x3_form") else lib.smot_dla_conv3x3_form
    form = fn(int(N), int(H), int(W), int(Cout), int(stride))
    if form < 0:
        raise RuntimeError("siammot_amd.dla_conv3x3_form: bad argument")
    return form // 10, form % 10


def dla_conv3x3(x, w, scale, shift, stride, residual=None, relu=True, residual_pooled=False, operands="fp32"):
    """``relu(conv3x3(x, w, stride, pad 1) * scale + shift + residual)`` (``smot_dla_conv3x3_fwd``; residual and ReLU
    optional): x ``[N, Cin, H, W]`` fp32 -> ``[N, Cout, Ho, Wo]`` fp32, any H, W >= 1.  ``residual_pooled``: the residual is
    ``[N, Cout, Hr, Wr]`` with ``Hr // 2 == Ho``, ``Wr // 2 == Wo`` and is read through ``max_pool2d(., 2, 2)``.
    ``operands`` "split16": ``smot_dla_conv3x3_split_fwd`` (``Cin`` a multiple of 32)."""
    lib = _lib or load_library()
    split = _dla_split(operands, "dla_conv3x3")
    x = _dev_f32(x, "x")
    N, Cin, H, W = (int(v) for v in x.shape)
    Cout = int(w.shape[0])
    w = _chk(w, "w", (Cout, Cin, 3, 3))
    scale, shift = _chk(scale, "scale", (Cout,)), _chk(shift, "shift", (Cout,))
    Ho, Wo = ((H - 1) // 2 + 1, (W - 1) // 2 + 1) if stride == 2 else (H, W)
    rh = rw = 0
    if residual is not None and residual_pooled:
        rh, rw = int(residual.shape[-2]), int(residual.shape[-1])
        residual = _chk(residual, "residual", (N, Cout, rh, rw))
    elif residual is not None:
        residual = _chk(residual, "residual", (N, Cout, Ho, Wo))
    n = (lib.smot_dla_conv_split_packed_floats if split else lib.smot_dla_conv_packed_floats)(3, Cin, Cout)
    packed = torch.empty((max(n, 4),), dtype=_F32, device=x.device)
    out = torch.empty((N, Cout, Ho, Wo), dtype=_F32, device=x.device)
    with _Launch(x, w, scale, shift, residual) as ln:
        rc = (lib.smot_dla_conv3x3_split_fwd if split else lib.smot_dla_conv3x3_fwd)(
            _ptr(x), N, Cin, H, W, _ptr(w), _ptr(scale), _ptr(shift), Cout, int(stride), _ptr(residual), rh, rw, 1 if relu else 0,
            _ptr(packed), _ptr(out), ln.stream)
    _check(rc, "dla_conv3x3")
    return out


def dla_conv1x1(sources, pooled, w, scale, shift, relu, out_dtype=torch.float32):
    """``relu(conv1x1(cat(sources, 1), w) * scale + shift)`` (``smot_dla_conv1x1_fwd``; ReLU optional) with no ``cat``:
    sources: up to four fp32 maps ``[N, C_s, ., .]``; ``pooled[s]``: the source is read through ``max_pool2d(., 2, 2)``
    (a map twice as fine), else it has the output's size.  -> ``[N, Cout, H, W]`` of ``out_dtype``."""
    lib = _lib or load_library()
    S = len(sources)
    if not 1 <= S <= 4 or len(pooled) != S:
        raise RuntimeError("siammot_amd.dla_conv1x1: %d sources, %d pooled flags (1 .. 4 of each)" % (S, len(pooled)))
    if out_dtype not in FEAT_TYPES:
        raise RuntimeError("siammot_amd.dla_conv1x1: out_dtype must be float32, float16 or bfloat16, got %s" % (out_dtype,))
    src = [_dev_f32(t, "sources[%d]" % s) for s, t in enumerate(sources)]
    N = int(src[0].shape[0])
    H, W = (int(src[0].shape[2]) // 2, int(src[0].shape[3]) // 2) if pooled[0] else (int(src[0].shape[2]), int(src[0].shape[3]))
    K = sum(int(t.shape[1]) for t in src)
    Cout = int(w.shape[0])
    w = _chk(w.reshape(Cout, -1), "w", (Cout, K))
    scale, shift = _chk(scale, "scale", (Cout,)), _chk(shift, "shift", (Cout,))
    for s, t in enumerate(src):
        if t.dim() != 4 or t.shape[0] != N:
            raise RuntimeError("siammot_amd.dla_conv1x1: sources[%d] has shape %s" % (s, tuple(t.shape)))
    arr = lambda vals: (ctypes.c_int * S)(*[int(v) for v in vals])
    sp = (ctypes.c_void_p * S)(*[t.data_ptr() for t in src])
    sc, sf = arr(t.shape[1] for t in src), arr(1 if f else 0 for f in pooled)
    sh, sw = arr(t.shape[2] for t in src), arr(t.shape[3] for t in src)
    n = lib.smot_dla_conv_packed_floats(1, K, Cout)
    packed = torch.empty((max(n, 4),), dtype=_F32, device=src[0].device)
    out = torch.empty((N, Cout, H, W), dtype=out_dtype, device=src[0].device)
    with _Launch(*(src + [w, scale, shift])) as ln:
        rc = lib.smot_dla_conv1x1_fwd(_cast(sp), _cast(sc), _cast(sf), _cast(sh), _cast(sw), S, N, H, W, _ptr(w), _ptr(scale),
                                      _ptr(shift), Cout, 1 if relu else 0, _ptr(packed), _ptr(out), FEAT_TYPES[out_dtype], ln.stream)
    _check(rc, "dla_conv1x1")
    return out


def dla_conv1x1_res(sources, pooled, w, scale, shift, relu, residual=None, residual_pooled=False, out_dtype=torch.float32):
    """``relu(conv1x1(cat(sources, 1), w) * scale + shift + residual)`` (``smot_dla_conv1x1_res_fwd``; residual and ReLU
    optional): ``dla_conv1x1`` over up to EIGHT sources.  ``residual``: ``[N, Cout, H, W]`` fp32, or with ``residual_pooled``
    ``[N, Cout, Hr, Wr]`` with ``Hr // 2 == H``, ``Wr // 2 == W``, read through ``max_pool2d(., 2, 2)``; it may be one of the
    sources.  With up to four sources and no residual: the bits of ``dla_conv1x1``."""
    lib = _lib or load_library()
    S = len(sources)
    if S < 1 or len(pooled) != S:
        raise RuntimeError("siammot_amd.dla_conv1x1_res: %d sources, %d pooled flags" % (S, len(pooled)))
    if out_dtype not in FEAT_TYPES:
        raise RuntimeError("siammot_amd.dla_conv1x1_res: out_dtype must be float32, float16 or bfloat16, got %s" % (out_dtype,))
    src = [_dev_f32(t, "sources[%d]" % s) for s, t in enumerate(sources)]
    N = int(src[0].shape[0])
    H, W = (int(src[0].shape[2]) // 2, int(src[0].shape[3]) // 2) if pooled[0] else (int(src[0].shape[2]), int(src[0].shape[3]))
    K = sum(int(t.shape[1]) for t in src)
    Cout = int(w.shape[0])
    w = _chk(w.reshape(Cout, -1), "w", (Cout, K))
    scale, shift = _chk(scale, "scale", (Cout,)), _chk(shift, "shift", (Cout,))
    for s, t in enumerate(src):
        if t.dim() != 4 or t.shape[0] != N:
            raise RuntimeError("siammot_amd.dla_conv1x1_res: sources[%d] has shape %s" % (s, tuple(t.shape)))
    rh = rw = 0
    if residual is not None and residual_pooled:                 # (its size is the library's to check)
        rh, rw = int(residual.shape[-2]), int(residual.shape[-1])
        residual = _chk(residual, "residual", (N, Cout, rh, rw))
    elif residual is not None:
        residual = _chk(residual, "residual", (N, Cout, H, W))
    arr = lambda vals: (ctypes.c_int * S)(*[int(v) for v in vals])
    sp = (ctypes.c_void_p * S)(*[t.data_ptr() for t in src])
    sc, sf = arr(t.shape[1] for t in src), arr(1 if f else 0 for f in pooled)
    sh, sw = arr(t.shape[2] for t in src), arr(t.shape[3] for t in src)
    n = lib.smot_dla_conv_packed_floats(1, K, Cout)
    packed = torch.empty((max(n, 4),), dtype=_F32, device=src[0].device)
    out = torch.empty((N, Cout, H, W), dtype=out_dtype, device=src[0].device)
    with _Launch(*(src + [w, scale, shift, residual])) as ln:
        rc = lib.smot_dla_conv1x1_res_fwd(_cast(sp), _cast(sc), _cast(sf), _cast(sh), _cast(sw), S, N, H, W, _ptr(w), _ptr(scale),
                                          _ptr(shift), Cout, 1 if relu else 0, _ptr(residual), rh, rw, _ptr(packed), _ptr(out),
                                          FEAT_TYPES[out_dtype], ln.stream)
    _check(rc, "dla_conv1x1_res")
    return out


def _dla_block(block, who):
    if block not in DLA_BLOCKS:
        raise ValueError("siammot_amd.%s: block must be \"basic\" or \"bottleneck\", got %r" % (who, block))
    return DLA_BLOCKS[block]


def dla_net_num_convs(levels, channels, block="basic"):
    """The convolutions ``dla_net`` evaluates = its launches (``smot_dla_net_num_convs``; the stem's three included): 37 for
    DLA-34, 48 for DLA-46-C, 63 for DLA-60, 105 for DLA-102, 168 for DLA-169.  -1: beyond the capacities."""
    lib = _lib or load_library()
    return int(lib.smot_dla_net_num_convs(_cast(_int6(levels)), _cast(_int6(channels)), _dla_block(block, "dla_net_num_convs")))


def dla_net_ws_bytes(levels, channels, N, H, W, block="basic", residual_root=False):
    """The bytes of workspace ``dla_net`` takes for ``N`` images of ``H x W`` (``smot_dla_net_ws_bytes``; no device needed).
    -1: beyond the capacities."""
    lib = _lib or load_library()
    return int(lib.smot_dla_net_ws_bytes(_cast(_int6(levels)), _cast(_int6(channels)), _dla_block(block, "dla_net_ws_bytes"),
                                         1 if residual_root else 0, int(N), int(H), int(W)))


def dla_net_pack(convs, levels, channels, block="basic", residual_root=False, operands="fp32"):
    """``dla_pack`` for ``dla_net`` (``smot_dla_net_pack``): convs in LAUNCH ORDER (``dla.DLA.convs()``).  With basic blocks and
    trees of depth <= 2 the tensor is ``dla_pack``'s.  No synchronisation, ordered on the current stream only, as
    ``dla_pack``."""
    lib = _lib or load_library()
    split = 1 if _dla_split(operands, "dla_net_pack") else 0
    blk, rr = _dla_block(block, "dla_net_pack"), 1 if residual_root else 0
    lv, ch = _int6(levels), _int6(channels)
    n = lib.smot_dla_net_packed_floats(_cast(lv), _cast(ch), blk, rr, split)
    if n < 0:
        _check(-2, "dla_net_pack")
    ts = [[_chk(t, "dla_net_pack: convs[%d][%d]" % (i, j), tuple(t.shape)) for j, t in enumerate(c)] for i, c in enumerate(convs)]
    packed = torch.empty((n,), dtype=_F32, device=ts[0][0].device)
    arrays = [(ctypes.c_void_p * len(ts))(*[c[j].data_ptr() for c in ts]) for j in range(3)]
    with _Launch(*[t for c in ts for t in c]) as ln:
        rc = lib.smot_dla_net_pack(_cast(lv), _cast(ch), blk, rr, split, _cast(arrays[0]), _cast(arrays[1]), _cast(arrays[2]),
                                   len(ts), _ptr(packed), ln.stream)
    _check(rc, "dla_net_pack")
    return packed


def dla_net(images, packed, levels, channels, block="basic", residual_root=False, out_dtype=torch.float32, operands="fp32"):
    """Upstream's ``DLA.forward`` for DlaBasic or DlaBottleneck blocks, trees of depth 1 .. 5 and plain or residual roots
    (``smot_dla_net_fwd``; include/smot_emm.h, DLA BACKBONE, BOTTLENECK BLOCKS AND DEEPER TREES), one launch per evaluated
    convolution, free of host synchronisation.  Arguments and results as ``dla``'s; packed: ``dla_net_pack``'s tensor."""
    lib = _lib or load_library()
    split = 1 if _dla_split(operands, "dla_net") else 0
    blk, rr = _dla_block(block, "dla_net"), 1 if residual_root else 0
    if out_dtype not in FEAT_TYPES:
        raise RuntimeError("siammot_amd.dla_net: out_dtype must be float32, float16 or bfloat16, got %s" % (out_dtype,))
    x = _dev_feat(images, "images")
    if x.dim() != 4 or x.shape[1] != 3:
        raise RuntimeError("siammot_amd.dla_net: images has shape %s, expected [N, 3, H, W]" % (tuple(x.shape),))
    N, H, W = int(x.shape[0]), int(x.shape[2]), int(x.shape[3])
    lv, ch = _int6(levels), _int6(channels)
    nbytes = lib.smot_dla_net_ws_bytes(_cast(lv), _cast(ch), blk, rr, N, H, W)
    if nbytes < 0:
        _check(-2, "dla_net")
    ws = torch.empty((max(nbytes // 4, 4),), dtype=_F32, device=x.device)
    out = [torch.empty((N, int(channels[k]), H >> k, W >> k), dtype=out_dtype, device=x.device) for k in range(2, 6)]
    po = (ctypes.c_void_p * 4)(*[t.data_ptr() for t in out])
    with _Launch(x, packed) as ln:
        rc = lib.smot_dla_net_fwd(_ptr(x), FEAT_TYPES[x.dtype], N, H, W, _cast(lv), _cast(ch), blk, rr, split, _ptr(packed),
                                  _ptr(ws), _cast(po), FEAT_TYPES[out_dtype], ln.stream)
    _check(rc, "dla_net")
    return out


# ``compute_dtype`` of the DLA bodies' half compute mode (include/smot_emm.h, DLA BACKBONE, HALF COMPUTE): every tree
# convolution takes its operands rounded to this type, on the 16-bit matrix instruction, with fp32 accumulation
DLA_COMPUTE_TYPES = (torch.float16, torch.bfloat16)


def _dla_ctype(compute_dtype, who):
    if compute_dtype not in DLA_COMPUTE_TYPES:
        raise ValueError("siammot_amd.%s: compute_dtype must be torch.float16 or torch.bfloat16, got %r" % (who, compute_dtype))
    return FEAT_TYPES[compute_dtype]


def dla_half_pack(convs, levels, channels, compute_dtype, block="basic", residual_root=False):
    """``dla_net_pack`` for ``dla_half`` (``smot_dla_half_pack``): the tree convolutions' filters rounded once to
    ``compute_dtype`` (``tensor.to``'s rounding), the stem's and every ``scale`` / ``shift`` in fp32.  The tensor serves this
    ``compute_dtype`` and no other mode.  No synchronisation, ordered on the current stream only, as ``dla_pack``."""
    lib = _lib or load_library()
    ct = _dla_ctype(compute_dtype, "dla_half_pack")
    blk, rr = _dla_block(block, "dla_half_pack"), 1 if residual_root else 0
    lv, ch = _int6(levels), _int6(channels)
    n = lib.smot_dla_half_packed_floats(_cast(lv), _cast(ch), blk, rr, ct)
    if n < 0:
        _check(-2, "dla_half_pack")
    ts = [[_chk(t, "dla_half_pack: convs[%d][%d]" % (i, j), tuple(t.shape)) for j, t in enumerate(c)] for i, c in enumerate(convs)]
    packed = torch.empty((n,), dtype=_F32, device=ts[0][0].device)
    arrays = [(ctypes.c_void_p * len(ts))(*[c[j].data_ptr() for c in ts]) for j in range(3)]
    with _Launch(*[t for c in ts for t in c]) as ln:
        rc = lib.smot_dla_half_pack(_cast(lv), _cast(ch), blk, rr, ct, _cast(arrays[0]), _cast(arrays[1]), _cast(arrays[2]),
                                    len(ts), _ptr(packed), ln.stream)
    _check(rc, "dla_half_pack")
    return packed


def dla_half(images, packed, levels, channels, compute_dtype, block="basic", residual_root=False, out_dtype=torch.float32):
    """``dla_net`` in half compute mode (``smot_dla_half_fwd``): every tree convolution — 3x3 and 1x1 — multiplies operands
    rounded to ``compute_dtype`` (activations as they are loaded, filters in ``dla_half_pack``) on the 16-bit matrix
    instruction and accumulates in fp32; the stem, the BN, the residuals and the maps between layers stay fp32.  An fp16
    operand beyond 65,504 in magnitude is +-inf.  Arguments and results otherwise as ``dla_net``'s; the same launches and
    workspace."""
    lib = _lib or load_library()
    ct = _dla_ctype(compute_dtype, "dla_half")
    blk, rr = _dla_block(block, "dla_half"), 1 if residual_root else 0
    if out_dtype not in FEAT_TYPES:
        raise RuntimeError("siammot_amd.dla_half: out_dtype must be float32, float16 or bfloat16, got %s" % (out_dtype,))
    x = _dev_feat(images, "images")
    if x.dim() != 4 or x.shape[1] != 3:
        raise RuntimeError("siammot_amd.dla_half: images has shape %s, expected [N, 3, H, W]" % (tuple(x.shape),))
    N, H, W = int(x.shape[0]), int(x.shape[2]), int(x.shape[3])
    lv, ch = _int6(levels), _int6(channels)
    nbytes = lib.smot_dla_net_ws_bytes(_cast(lv), _cast(ch), blk, rr, N, H, W)
    if nbytes < 0:
        _check(-2, "dla_half")
    ws = torch.empty((max(nbytes // 4, 4),), dtype=_F32, device=x.device)
    out = [torch.empty((N, int(channels[k]), H >> k, W >> k), dtype=out_dtype, device=x.device) for k in range(2, 6)]
    po = (ctypes.c_void_p * 4)(*[t.data_ptr() for t in out])
    with _Launch(x, packed) as ln:
        rc = lib.smot_dla_half_fwd(_ptr(x), FEAT_TYPES[x.dtype], N, H, W, _cast(lv), _cast(ch), blk, rr, ct, _ptr(packed),
                                   _ptr(ws), _cast(po), FEAT_TYPES[out_dtype], ln.stream)
    _check(rc, "dla_half")
    return out


def dla_conv3x3_half_form(N, H, W, Cout, stride):
    """``dla_conv3x3_form`` for ``dla_conv3x3_half``'s launch site (``smot_dla_conv3x3_half_form``): ``(WR, NM)``."""
    lib = _lib or load_library()
    form = lib.smot_dla_conv3x3_half_form(int(N), int(H), int(W), int(Cout), int(stride))
    if form < 0:
        raise RuntimeError("siammot_amd.dla_conv3x3_half_form: bad argument")
    return form // 10, form % 10


def dla_conv3x3_half(x, w, scale, shift, stride, compute_dtype, residual=None, relu=True, residual_pooled=False):
    """``dla_conv3x3`` in half compute mode (``smot_dla_conv3x3_half_fwd``): ``x`` and ``w`` rounded to ``compute_dtype``,
    exact products, fp32 accumulation, the fp32 epilogue.  ``Cin`` a multiple of 32."""
    lib = _lib or load_library()
    ct = _dla_ctype(compute_dtype, "dla_conv3x3_half")
    x = _dev_f32(x, "x")
    N, Cin, H, W = (int(v) for v in x.shape)
    Cout = int(w.shape[0])
    w = _chk(w, "w", (Cout, Cin, 3, 3))
    scale, shift = _chk(scale, "scale", (Cout,)), _chk(shift, "shift", (Cout,))
    Ho, Wo = ((H - 1) // 2 + 1, (W - 1) // 2 + 1) if stride == 2 else (H, W)
    rh = rw = 0
    if residual is not None and residual_pooled:
        rh, rw = int(residual.shape[-2]), int(residual.shape[-1])
        residual = _chk(residual, "residual", (N, Cout, rh, rw))
    elif residual is not None:
        residual = _chk(residual, "residual", (N, Cout, Ho, Wo))
    n = lib.smot_dla_conv_half_packed_floats(3, Cin, Cout)
    packed = torch.empty((max(n, 4),), dtype=_F32, device=x.device)
    out = torch.empty((N, Cout, Ho, Wo), dtype=_F32, device=x.device)
    with _Launch(x, w, scale, shift, residual) as ln:
        rc = lib.smot_dla_conv3x3_half_fwd(_ptr(x), N, Cin, H, W, _ptr(w), _ptr(scale), _ptr(shift), Cout, int(stride),
                                           _ptr(residual), rh, rw, 1 if relu else 0, ct, _ptr(packed), _ptr(out), ln.stream)
    _check(rc, "dla_conv3x3_half")
    return out


def dla_conv1x1_half_form(N, H, W, Cout):
    """The M-tiles (of 16 output channels) per workgroup that ``dla_conv1x1_half`` runs for ``N`` outputs of ``H x W``
    (``smot_dla_conv1x1_half_form``): 4, or 2 where 4 would leave CUs without a workgroup."""
    lib = _lib or load_library()
    form = lib.smot_dla_conv1x1_half_form(int(N), int(H), int(W), int(Cout))
    if form < 0:
        raise RuntimeError("siammot_amd.dla_conv1x1_half_form: bad argument")
    return form


def dla_conv1x1_half(sources, pooled, w, scale, shift, relu, compute_dtype, residual=None, residual_pooled=False,
                     out_dtype=torch.float32):
    """``dla_conv1x1_res`` in half compute mode (``smot_dla_conv1x1_half_fwd``): the sources' values (after the pool, where a
    source is pooled) and ``w`` rounded to ``compute_dtype``, exact products, fp32 accumulation, the fp32 epilogue.  Every
    source a multiple of 32 channels."""
    lib = _lib or load_library()
    ct = _dla_ctype(compute_dtype, "dla_conv1x1_half")
    S = len(sources)
    if S < 1 or len(pooled) != S:
        raise RuntimeError("siammot_amd.dla_conv1x1_half: %d sources, %d pooled flags" % (S, len(pooled)))
    if out_dtype not in FEAT_TYPES:
        raise RuntimeError("siammot_amd.dla_conv1x1_half: out_dtype must be float32, float16 or bfloat16, got %s" % (out_dtype,))
    src = [_dev_f32(t, "sources[%d]" % s) for s, t in enumerate(sources)]
    N = int(src[0].shape[0])
    H, W = (int(src[0].shape[2]) // 2, int(src[0].shape[3]) // 2) if pooled[0] else (int(src[0].shape[2]), int(src[0].shape[3]))
    K = sum(int(t.shape[1]) for t in src)
    Cout = int(w.shape[0])
    w = _chk(w.reshape(Cout, -1), "w", (Cout, K))
    scale, shift = _chk(scale, "scale", (Cout,)), _chk(shift, "shift", (Cout,))
    for s, t in enumerate(src):
        if t.dim() != 4 or t.shape[0] != N:
            raise RuntimeError("siammot_amd.dla_conv1x1_half: sources[%d] has shape %s" % (s, tuple(t.shape)))
    rh = rw = 0
    if residual is not None and residual_pooled:                 # (its size is the library's to check)
        rh, rw = int(residual.shape[-2]), int(residual.shape[-1])
        residual = _chk(residual, "residual", (N, Cout, rh, rw))
    elif residual is not None:
        residual = _chk(residual, "residual", (N, Cout, H, W))
    arr = lambda vals: (ctypes.c_int * S)(*[int(v) for v in vals])
    sp = (ctypes.c_void_p * S)(*[t.data_ptr() for t in src])
    sc, sf = arr(t.shape[1] for t in src), arr(1 if f else 0 for f in pooled)
    sh, sw = arr(t.shape[2] for t in src), arr(t.shape[3] for t in src)
    n = lib.smot_dla_conv_half_packed_floats(1, K, Cout)
    packed = torch.empty((max(n, 4),), dtype=_F32, device=src[0].device)
    out = torch.empty((N, Cout, H, W), dtype=out_dtype, device=src[0].device)
    with _Launch(*(src + [w, scale, shift, residual])) as ln:
        rc = lib.smot_dla_conv1x1_half_fwd(_cast(sp), _cast(sc), _cast(sf), _cast(sh), _cast(sw), S, N, H, W, _ptr(w),
                                           _ptr(scale), _ptr(shift), Cout, 1 if relu else 0, _ptr(residual), rh, rw, ct,
                                           _ptr(packed), _ptr(out), FEAT_TYPES[out_dtype], ln.stream)
    _check(rc, "dla_conv1x1_half")
    return out


# ---- half storage: half compute mode with the maps between layers stored in ``compute_dtype`` (include/smot_emm.h, DLA
# BACKBONE, HALF STORAGE).  A map is float32 or ``compute_dtype``; every result is ``compute_dtype``.
def _dla_hs_map(t, name, compute_dtype, who):
    t = _dev_feat(t, name)
    if t.dtype is not torch.float32 and t.dtype is not compute_dtype:
        raise RuntimeError("siammot_amd.%s: %s must be float32 or the compute type %s, got %s" % (who, name, compute_dtype, t.dtype))
    return t


def _shaped(t, name, shape):
    if tuple(t.shape) != shape:
        raise RuntimeError("siammot_amd: %s has shape %s, expected %s" % (name, tuple(t.shape), shape))
    return t


def dla_half_storage_ws_bytes(levels, channels, N, H, W, compute_dtype, block="basic", residual_root=False):
    """The bytes of workspace ``dla_half_storage`` takes (``smot_dla_half_storage_ws_bytes``; no device needed): ``x1`` and the
    stem's two full-resolution maps in fp32, the tree maps in two bytes per element, no fp32 twin of a returned map.  -1
    exactly where ``dla_net_ws_bytes`` is."""
    lib = _lib or load_library()
    ct = _dla_ctype(compute_dtype, "dla_half_storage_ws_bytes")
    return int(lib.smot_dla_half_storage_ws_bytes(_cast(_int6(levels)), _cast(_int6(channels)),
                                                  _dla_block(block, "dla_half_storage_ws_bytes"), 1 if residual_root else 0, ct,
                                                  int(N), int(H), int(W)))


def dla_half_storage(images, packed, levels, channels, compute_dtype, block="basic", residual_root=False):
    """``dla_half`` with every map a tree convolution writes stored in ``compute_dtype`` (``smot_dla_half_storage_fwd``): the
    fp32 epilogue value rounded once (``tensor.to``'s rounding; an fp16 value beyond 65,504 is +-inf).  No convolution
    operand changes by a bit against ``dla_half``; a residual that is a stored map is added as the rounded value, and the
    four returned maps, of ``compute_dtype``, ARE the stored maps.  packed: ``dla_half_pack``'s tensor; the same launches."""
    lib = _lib or load_library()
    ct = _dla_ctype(compute_dtype, "dla_half_storage")
    blk, rr = _dla_block(block, "dla_half_storage"), 1 if residual_root else 0
    x = _dev_feat(images, "images")
    if x.dim() != 4 or x.shape[1] != 3:
        raise RuntimeError("siammot_amd.dla_half_storage: images has shape %s, expected [N, 3, H, W]" % (tuple(x.shape),))
    N, H, W = int(x.shape[0]), int(x.shape[2]), int(x.shape[3])
    lv, ch = _int6(levels), _int6(channels)
    nbytes = lib.smot_dla_half_storage_ws_bytes(_cast(lv), _cast(ch), blk, rr, ct, N, H, W)
    if nbytes < 0:
        _check(-2, "dla_half_storage")
    ws = torch.empty((max(nbytes // 4, 4),), dtype=_F32, device=x.device)
    out = [torch.empty((N, int(channels[k]), H >> k, W >> k), dtype=compute_dtype, device=x.device) for k in range(2, 6)]
    po = (ctypes.c_void_p * 4)(*[t.data_ptr() for t in out])
    with _Launch(x, packed) as ln:
        rc = lib.smot_dla_half_storage_fwd(_ptr(x), FEAT_TYPES[x.dtype], N, H, W, _cast(lv), _cast(ch), blk, rr, ct, _ptr(packed),
                                           _ptr(ws), _cast(po), ln.stream)
    _check(rc, "dla_half_storage")
    return out


def dla_conv3x3_half_storage(x, w, scale, shift, stride, compute_dtype, residual=None, relu=True, residual_pooled=False):
    """``dla_conv3x3_half`` in half storage (``smot_dla_conv3x3_half_storage_fwd``): ``x`` and ``residual`` each float32 or
    ``compute_dtype``; -> ``compute_dtype``: bit for bit ``dla_conv3x3_half(x.float(), ..., residual.float(), ...)
    .to(compute_dtype)``."""
    lib = _lib or load_library()
    who = "dla_conv3x3_half_storage"
    ct = _dla_ctype(compute_dtype, who)
    x = _dla_hs_map(x, "x", compute_dtype, who)
    N, Cin, H, W = (int(v) for v in x.shape)
    Cout = int(w.shape[0])
    w = _chk(w, "w", (Cout, Cin, 3, 3))
    scale, shift = _chk(scale, "scale", (Cout,)), _chk(shift, "shift", (Cout,))
    Ho, Wo = ((H - 1) // 2 + 1, (W - 1) // 2 + 1) if stride == 2 else (H, W)
    rh = rw = 0
    if residual is not None:
        residual = _dla_hs_map(residual, "residual", compute_dtype, who)
        if residual_pooled:
            rh, rw = int(residual.shape[-2]), int(residual.shape[-1])
        _shaped(residual, "residual", (N, Cout, rh, rw) if residual_pooled else (N, Cout, Ho, Wo))
    n = lib.smot_dla_conv_half_packed_floats(3, Cin, Cout)
    packed = torch.empty((max(n, 4),), dtype=_F32, device=x.device)
    out = torch.empty((N, Cout, Ho, Wo), dtype=compute_dtype, device=x.device)
    with _Launch(x, w, scale, shift, residual) as ln:
        rc = lib.smot_dla_conv3x3_half_storage_fwd(_ptr(x), FEAT_TYPES[x.dtype], N, Cin, H, W, _ptr(w), _ptr(scale), _ptr(shift),
                                                   Cout, int(stride), _ptr(residual),
                                                   FEAT_TYPES[residual.dtype] if residual is not None else 0, rh, rw,
                                                   1 if relu else 0, ct, _ptr(packed), _ptr(out), ln.stream)
    _check(rc, who)
    return out


def dla_conv1x1_half_storage(sources, pooled, w, scale, shift, relu, compute_dtype, residual=None, residual_pooled=False):
    """``dla_conv1x1_half`` in half storage (``smot_dla_conv1x1_half_storage_fwd``): the sources all float32 or all
    ``compute_dtype``, ``residual`` of either; -> ``compute_dtype``: bit for bit ``dla_conv1x1_half`` on the widened sources
    and residual, ``.to(compute_dtype)``."""
    lib = _lib or load_library()
    who = "dla_conv1x1_half_storage"
    ct = _dla_ctype(compute_dtype, who)
    S = len(sources)
    if S < 1 or len(pooled) != S:
        raise RuntimeError("siammot_amd.%s: %d sources, %d pooled flags" % (who, S, len(pooled)))
    src = [_dla_hs_map(t, "sources[%d]" % s, compute_dtype, who) for s, t in enumerate(sources)]
    if any(t.dtype is not src[0].dtype for t in src):
        raise RuntimeError("siammot_amd.%s: the sources of one call have one type, got %s" % (who, [t.dtype for t in src]))
    N = int(src[0].shape[0])
    H, W = (int(src[0].shape[2]) // 2, int(src[0].shape[3]) // 2) if pooled[0] else (int(src[0].shape[2]), int(src[0].shape[3]))
    K = sum(int(t.shape[1]) for t in src)
    Cout = int(w.shape[0])
    w = _chk(w.reshape(Cout, -1), "w", (Cout, K))
    scale, shift = _chk(scale, "scale", (Cout,)), _chk(shift, "shift", (Cout,))
    for s, t in enumerate(src):
        if t.dim() != 4 or t.shape[0] != N:
            raise RuntimeError("siammot_amd.%s: sources[%d] has shape %s" % (who, s, tuple(t.shape)))
    rh = rw = 0
    if residual is not None:                                     # (a pooled residual's size is the library's to check)
        residual = _dla_hs_map(residual, "residual", compute_dtype, who)
        if residual_pooled:
            rh, rw = int(residual.shape[-2]), int(residual.shape[-1])
        _shaped(residual, "residual", (N, Cout, rh, rw) if residual_pooled else (N, Cout, H, W))
    arr = lambda vals: (ctypes.c_int * S)(*[int(v) for v in vals])
    sp = (ctypes.c_void_p * S)(*[t.data_ptr() for t in src])
    sc, sf = arr(t.shape[1] for t in src), arr(1 if f else 0 for f in pooled)
    sh, sw = arr(t.shape[2] for t in src), arr(t.shape[3] for t in src)
    n = lib.smot_dla_conv_half_packed_floats(1, K, Cout)
    packed = torch.empty((max(n, 4),), dtype=_F32, device=src[0].device)
    out = torch.empty((N, Cout, H, W), dtype=compute_dtype, device=src[0].device)
    with _Launch(*(src + [w, scale, shift, residual])) as ln:
        rc = lib.smot_dla_conv1x1_half_storage_fwd(_cast(sp), FEAT_TYPES[src[0].dtype], _cast(sc), _cast(sf), _cast(sh), _cast(sw),
                                                   S, N, H, W, _ptr(w), _ptr(scale), _ptr(shift), Cout, 1 if relu else 0,
                                                   _ptr(residual), FEAT_TYPES[residual.dtype] if residual is not None else 0,
                                                   rh, rw, ct, _ptr(packed), _ptr(out), ln.stream)
    _check(rc, who)
    return out


def dla_stem(images, layers):
    """The body's first three layers (``smot_dla_stem_fwd``): images ``[N, 3, H, W]`` fp32, fp16 or bf16, H and W even;
    layers: ``(weight, scale, shift)`` of ``base_layer`` ``[c0, 3, 7, 7]``, ``level0`` ``[c0, c0, 3, 3]`` and ``level1``
    ``[c1, c0, 3, 3]``.  -> ``x1 [N, c1, H / 2, W / 2]`` fp32."""
    lib = _lib or load_library()
    x = _dev_feat(images, "images")
    if x.dim() != 4 or x.shape[1] != 3 or len(layers) != 3:
        raise RuntimeError("siammot_amd.dla_stem: images %s, %d layers (expected [N, 3, H, W] and three)" % (tuple(x.shape), len(layers)))
    N, H, W = int(x.shape[0]), int(x.shape[2]), int(x.shape[3])
    c0, c1 = int(layers[0][0].shape[0]), int(layers[2][0].shape[0])
    shapes = ((c0, 3, 7, 7), (c0, c0, 3, 3), (c1, c0, 3, 3))
    ts = [(_chk(w, "layers[%d] weight" % i, shapes[i]), _chk(a, "layers[%d] scale" % i, shapes[i][:1]),
           _chk(b, "layers[%d] shift" % i, shapes[i][:1])) for i, (w, a, b) in enumerate(layers)]
    nbytes = lib.smot_dla_stem_ws_bytes(N, H, W, c0, c1)
    if nbytes < 0:
        _check(-2, "dla_stem")
    ws = torch.empty((max(nbytes // 4, 4),), dtype=_F32, device=x.device)
    out = torch.empty((N, c1, H // 2, W // 2), dtype=_F32, device=x.device)
    arrays = [(ctypes.c_void_p * 3)(*[t[j].data_ptr() for t in ts]) for j in range(3)]
    with _Launch(*([x] + [t for c in ts for t in c])) as ln:
        rc = lib.smot_dla_stem_fwd(_ptr(x), FEAT_TYPES[x.dtype], N, H, W, c0, c1, _cast(arrays[0]), _cast(arrays[1]),
                                   _cast(arrays[2]), _ptr(ws), _ptr(out), ln.stream)
    _check(rc, "dla_stem")
    return out


def rpn_anchors(cell_anchors, strides, grid_sizes):
    """Upstream's ``AnchorGenerator.grid_anchors`` for all levels in one launch (``smot_rpn_anchors_fwd``).  cell_anchors: L
    fp32 device tensors ``[A_l, 4]``; strides: L ints; grid_sizes: L pairs ``(H_l, W_l)``.  -> L fp32 ``[H_l*W_l*A_l, 4]``
    in the flattened order (h*W + w)*A + a.  No synchronisation; the grids are ordered on the current stream only, as
    ``rpn_head_pack``'s image."""
    lib = _lib or load_library()
    L = len(cell_anchors)
    if L < 1 or len(strides) != L or len(grid_sizes) != L:
        raise RuntimeError("siammot_amd.rpn_anchors: %d cell-anchor levels, %d strides, %d grid sizes"
                           % (L, len(strides), len(grid_sizes)))
    cells = [_chk(c, "cell_anchors[%d]" % l, (c.shape[0], 4)) for l, c in enumerate(cell_anchors)]
    dev = cells[0].device
    out = [torch.empty((int(h) * int(w) * c.shape[0], 4), dtype=_F32, device=dev) for c, (h, w) in zip(cells, grid_sizes)]
    pc = (ctypes.c_void_p * L)(*[t.data_ptr() for t in cells])
    po = (ctypes.c_void_p * L)(*[t.data_ptr() for t in out])
    ia = (ctypes.c_int * L)(*[c.shape[0] for c in cells])
    is_ = (ctypes.c_int * L)(*[int(s) for s in strides])
    ih = (ctypes.c_int * L)(*[int(g[0]) for g in grid_sizes])
    iw = (ctypes.c_int * L)(*[int(g[1]) for g in grid_sizes])
    with _Launch(*cells) as ln:
        rc = lib.smot_rpn_anchors_fwd(_cast(pc), _cast(ia), _cast(is_), _cast(ih), _cast(iw), L, _cast(po), ln.stream)
    _check(rc, "rpn_anchors")
    return out


_rec_pinned = {}


class HostRecordRing(object):
    """Two pinned, device-accessible int32 buffers large enough for any solver record, and the event recorded behind
    each launch — owned by ONE tracker (``TrackPool.host_record_ring``), so two tracking loops driven from different
    threads or streams never re-zero or re-record each other's completion word.  The buffers alternate: the host has
    copied the previous frame's record out before the next launch can overwrite it.  A frame that was aborted between
    launch and wait (an exception, KeyboardInterrupt) leaves its buffer marked in flight; the stream is drained
    before that buffer is handed out again, so a late store of the old kernel cannot complete a newer record."""

    def __init__(self, dev, pool_capacity):
        n = FrameBuffers.record_words(track_solve_max_boxes(), pool_capacity)
        self.dev = dev
        self.bufs = [torch.zeros((n,), dtype=torch.int32).pin_memory() for _ in range(2)]
        self.views = [b.numpy() for b in self.bufs]          # the same memory as numpy arrays (cheap element access)
        self.in_flight = [False, False]
        self.k = 0
        self.event = torch.cuda.Event()

    def next(self):
        self.k ^= 1
        if self.in_flight[self.k]:
            self._drain()
            self.in_flight = [False, False]
        rec = self.bufs[self.k]
        self.views[self.k][3] = 0     # the kernel stores the frame index (>= 1) here last: the host's completion flag
        self.in_flight[self.k] = True
        return rec

    def view(self, rec):
        """The numpy view of one of this ring's buffers."""
        return self.views[0] if rec is self.bufs[0] else self.views[1]

    def record_event(self):
        """Record this ring's event on the device's current stream (behind the solver launch)."""
        self.event.record(torch.cuda.current_stream(self.dev))
        return self.event

    def wait(self, rec, event=True):
        """The frame's one synchronisation (``wait_host_record``): poll the completion word of ``rec``; if it does not show
        up, fall back to the event recorded behind the launch (``record_event``) or — ``event=False``, nothing was
        recorded — to draining the stream."""
        i = 0 if rec is self.bufs[0] else 1
        wait_host_record(self.views[i], self.event.synchronize if event else self._drain)
        self.in_flight[i] = False

    def _drain(self):
        torch.cuda.current_stream(self.dev).synchronize()


class FrameBuffers(object):
    """What the solver's launch and the masked extraction behind it write for a frame of M input rows (include/smot_emm.h,
    smot_track_solve_fwd), and the ONE owner of where — nothing outside this class spells an offset into them:

        fbuf      fp32   out_boxes [4M] | act_boxes [4M] | out_scores [M] | act_scores [M] | (to 8 floats) order hint [M, HINT_FLOATS]
        ibuf      int64  out_ids [M] | out_labels [M] | act_ids [M] | act_labels [M]
        templates [M, C, rz, rz], sr_rows [M, 4]    the extraction's rows of act_boxes (the next frame's memory)
        record    int32  K, A, max id, frame index, active ids, dormant ids, flags, M | kept input rows [M] | kept ids [M] |
                         active ids [M] | active table, dormant table, its frames [3 x capacity] | input ids [M]
    The first K rows of the out_* and the first A of the act_* fields are valid.  The order hint is kept as an OFFSET
    (``hint_off`` floats into ``fbuf``, 0: none) and addresses are read off the tensors on every call: a deep copy / pickle
    copies the buffers, and the hint with them."""
    __slots__ = ("fbuf", "ibuf", "templates", "sr_rows", "M", "hint_off")

    def __init__(self, fbuf, ibuf, M, templates=None, sr_rows=None, hint_off=0):
        self.fbuf, self.ibuf, self.M, self.templates, self.sr_rows, self.hint_off = fbuf, ibuf, M, templates, sr_rows, hint_off

    @staticmethod
    def allocate(M, dev, row_shape=None, hint=False):
        """For M rows; ``row_shape`` (C, rz, rz): with the extraction's outputs; ``hint``: with its order hint (2 .. 256 rows)."""
        n = max(M, 1)
        hint_off = ((10 * n + 7) & ~7) if (hint and 2 <= M <= 256) else 0          # (a 32-byte boundary)
        b = FrameBuffers(torch.empty((hint_off + HINT_FLOATS * M if hint_off else 10 * n,), dtype=_F32, device=dev),
                         torch.empty((4 * n,), dtype=torch.int64, device=dev), M, hint_off=hint_off)
        if row_shape is not None:
            b.templates = torch.empty((M,) + tuple(row_shape), dtype=_F32, device=dev)
            b.sr_rows = torch.empty((M, 4), dtype=_F32, device=dev)
        return b

    def solver_pointers(self):
        """(out_boxes, out_scores, out_ids, out_labels, act_boxes, act_ids, act_labels, act_scores)."""
        fp, ip, M = self.fbuf.data_ptr(), self.ibuf.data_ptr(), self.M
        return fp, fp + 32 * M, ip, ip + 8 * M, fp + 16 * M, ip + 16 * M, ip + 24 * M, fp + 36 * M

    @property
    def hint_ptr(self):
        return self.fbuf.data_ptr() + 4 * self.hint_off if self.hint_off else 0

    def pointers(self):
        """(template boxes, search regions, templates, ids, labels, order hint or 0) of the act rows: the next head's inputs."""
        fp, ip, M = self.fbuf.data_ptr(), self.ibuf.data_ptr(), self.M
        return (fp + 16 * M, self.sr_rows.data_ptr(), self.templates.data_ptr(), ip + 16 * M, ip + 24 * M,
                fp + 4 * self.hint_off if self.hint_off else 0)

    def carry_pointers(self):
        """(templates, boxes, search regions, ids, labels, scores) of the act rows: ``memory_carry``'s order."""
        fp, ip, M = self.fbuf.data_ptr(), self.ibuf.data_ptr(), self.M
        return self.templates.data_ptr(), fp + 16 * M, self.sr_rows.data_ptr(), ip + 16 * M, ip + 24 * M, fp + 36 * M

    def kept(self, K):
        """(boxes [K,4], ids, scores, labels) of the frame's output rows."""
        st, f, i, M = torch.as_strided, self.fbuf, self.ibuf, self.M
        return st(f, (K, 4), (4, 1), 0), st(i, (K,), (1,), 0), st(f, (K,), (1,), 8 * M), st(i, (K,), (1,), M)

    def active(self, A):
        """(boxes [A,4], ids, scores, labels) of the rows the solver leaves active (and what was carried behind them)."""
        st, f, i, M = torch.as_strided, self.fbuf, self.ibuf, self.M
        return st(f, (A, 4), (4, 1), 4 * M), st(i, (A,), (1,), 2 * M), st(f, (A,), (1,), 9 * M), st(i, (A,), (1,), 3 * M)

    def hint_status(self):
        """Status word of the order hint (0 = fine / no hint).  Synchronises: error paths and tests only."""
        return order_hint_status(self.fbuf[self.hint_off:]) if self.hint_off else 0

    def clear_hint_status(self):
        """Zero the hint's status word on the current stream (a head launched on a wrong guess fails its verification)."""
        if self.hint_off:
            w = self.hint_off + HINT_STATUS_WORD
            self.fbuf[w:w + 1].zero_()

    # ---- the record (a numpy array, on the host): its size in words and its slices ---------------------------------------
    record_words = staticmethod(lambda M, capacity: 8 + 4 * M + 3 * capacity)
    kept_rows = staticmethod(lambda rec, M, K: rec[8:8 + K])
    kept_ids = staticmethod(lambda rec, M, K: rec[8 + M:8 + M + K])
    active_ids = staticmethod(lambda rec, M, A: rec[8 + 2 * M:8 + 2 * M + A])
    input_ids = staticmethod(lambda rec, M, capacity: rec[8 + 3 * M + 3 * capacity:8 + 4 * M + 3 * capacity])

    @staticmethod
    def tables(rec, M, capacity):
        """(active ids, dormant ids, the frames they were last active in): the snapshot of the pool's tables."""
        na, nd, base = int(rec[4]), int(rec[5]), 8 + 3 * M
        return rec[base:base + na], rec[base + capacity:base + capacity + nd], rec[base + 2 * capacity:base + 2 * capacity + nd]


def track_solve(det, trk, trk_score_bias, thresholds, nms_thresh, max_dormant_frames, pool_state, pool_capacity,
                host_record=False, carry=None):
    """``smot_track_solve_fwd``: one launch for TrackSolver.forward + the pool transitions + the active-row filter.

    det / trk: ``(boxes [n,4] xyxy, scores [n], ids [n] int64, labels [n] int64 or None)`` device tensors or ``None``
    for an empty segment.  Launch only (no synchronisation).  Returns ``(fbuf, ibuf, rec, M)``: the two output buffers
    and ``rec``, the record on the DEVICE, as ``FrameBuffers`` lays them out; ``track_solve_record(rec)`` brings it to the host.
    ``host_record=ring`` (a ``HostRecordRing``): the kernel writes the record straight into the ring's next pinned
    host buffer (``rec`` is then that host tensor; ``ring.record_event()`` behind this launch, ``ring.wait(rec)`` to
    read it — no copy command; the count of active rows for device-side consumers is ``pool_state[4:5]``).
    ``carry`` = (source addresses (templates, boxes, search regions, ids, labels, scores), first source row, rows, guessed
    first destination row, next_templates address, next_sr address, row_floats): ``smot_track_solve_carry_fwd`` — the
    dormant rows of the track memory go behind the active rows in this launch."""
    lib = _lib or load_library()
    dev = pool_state.device
    segs = [segment_pointers(seg, dev) for seg in (det, trk)]
    M = segs[0][4] + segs[1][4]
    buf = FrameBuffers.allocate(M, dev)
    rec = host_record.next() if host_record else torch.empty((buf.record_words(M, pool_capacity),), dtype=torch.int32, device=dev)
    cur = torch.cuda.current_device()
    if cur != dev.index:
        torch.cuda.set_device(dev.index)
    args = segs[0] + segs[1] + (trk_score_bias, thresholds[0], thresholds[1], thresholds[2], nms_thresh, max_dormant_frames,
                                pool_state.data_ptr(), pool_capacity) + buf.solver_pointers() + (rec.data_ptr(),)
    try:
        if carry is None:
            rc = lib.smot_track_solve_fwd(*args, _stream(dev))
        else:
            src, row0, rows, dst0, nz, nsr, row_floats = carry
            rc = lib.smot_track_solve_carry_fwd(*args, *src, int(row0), int(rows), int(dst0), nz, nsr, int(row_floats), _stream(dev))
    finally:
        if cur != dev.index:
            torch.cuda.set_device(cur)
    if rc:
        _check(rc, "track_solve")
    return buf.fbuf, buf.ibuf, rec, M


def track_solve_record(rec):
    """The solver's record on the host: a copy through a pinned buffer + ONE stream synchronisation (the frame's
    only one).  Everything enqueued on the stream before this call — including launches that consume the
    record's device copy, such as a masked ``emm_extract_cache`` — has completed when it returns."""
    dev, nrec = rec.device, rec.shape[0]
    host = _rec_pinned.get((dev, nrec))
    if host is None:
        if len(_rec_pinned) > 64:
            _rec_pinned.clear()
        host = _rec_pinned[(dev, nrec)] = torch.empty((nrec,), dtype=torch.int32).pin_memory()
    host.copy_(rec, non_blocking=True)
    torch.cuda.current_stream(dev).synchronize()
    return host.numpy().copy()


TRACK_SOLVE_CHUNK = 16               # images per launch of the batched solver (csrc/track_solver.hip: TS_BATCH)


def track_solve_batched(per_image):
    """``smot_track_solve_batched_fwd``: ``track_solve`` for the B images (cameras) of a call, one workgroup per image in
    ONE launch per ``TRACK_SOLVE_CHUNK`` images that have rows.  No synchronisation.

    ``per_image``: B tuples ``(det, trk, trk_score_bias, thresholds, nms_thresh, max_dormant_frames, pool_state,
    pool_capacity)``, each as ``track_solve`` takes them; every image has its own ``pool_state``.  Returns ``(bufs, rec,
    offsets)``: ``bufs[b]`` the image's ``FrameBuffers`` (None for an image without rows: nothing is launched for it and its
    pool state stands), ``rec`` ONE device int32 tensor with the images' records back to back and ``offsets`` (B + 1 words
    into it; an image without rows has an empty segment).  ``track_solve_records(rec, offsets)`` brings them to the host."""
    lib = _lib or load_library()
    B = len(per_image)
    if not 1 <= B <= MAX_IMAGES:
        raise RuntimeError("siammot_amd.track_solve_batched: %d images, need 1..%d per call" % (B, MAX_IMAGES))
    dev = per_image[0][6].device
    # the 27 host arrays of the call, in the entry's order: 18 of pointers, 4 of ints, 5 of floats — three flat arrays, one
    # row of B entries per argument (plain Python lists into array.array: cheaper than element-wise numpy at these sizes)
    ptr = [[] for _ in range(18)]       # det (boxes, scores, ids, labels), trk (the same), pool state, 8 outputs, record
    ints = [[] for _ in range(4)]       # n_det, n_trk, max dormant frames, pool capacity
    flt = [[] for _ in range(5)]        # score bias, track / start / resume thresholds, NMS threshold
    bufs, offsets = [], [0]
    none8 = (0,) * 8
    for b, (det, trk, bias, thresholds, nms_thresh, max_dormant, state, cap) in enumerate(per_image):
        if state.device != dev:
            raise RuntimeError("siammot_amd.track_solve_batched: image %d's pool state lives on %s, image 0's on %s"
                               % (b, state.device, dev))
        s0, s1 = segment_pointers(det, dev), segment_pointers(trk, dev)
        M = s0[4] + s1[4]
        buf = FrameBuffers.allocate(M, dev) if M else None
        bufs.append(buf)
        offsets.append(offsets[-1] + (FrameBuffers.record_words(M, cap) if M else 0))
        for k, v in enumerate(s0[:4] + s1[:4] + (state.data_ptr(),) + (buf.solver_pointers() if M else none8)):
            ptr[k].append(v)
        for k, v in enumerate((s0[4], s1[4], max_dormant, cap)):
            ints[k].append(v)
        for k, v in enumerate((bias, thresholds[0], thresholds[1], thresholds[2], nms_thresh)):
            flt[k].append(v)
    rec = torch.empty((offsets[-1],), dtype=torch.int32, device=dev)
    rp = rec.data_ptr()
    ptr[17] = [rp + 4 * o for o in offsets[:-1]]
    ptr, ints, flt = (_array.array(code, [v for row in rows for v in row])
                      for code, rows in (("Q", ptr), ("i", ints), ("f", flt)))
    P0, I0, F0 = ptr.buffer_info()[0], ints.buffer_info()[0], flt.buffer_info()[0]
    P, I, F = (lambda k: P0 + 8 * B * k), (lambda k: I0 + 4 * B * k), (lambda k: F0 + 4 * B * k)
    cur = torch.cuda.current_device()
    if cur != dev.index:
        torch.cuda.set_device(dev.index)
    try:
        rc = lib.smot_track_solve_batched_fwd(B, P(0), P(1), P(2), P(3), I(0), P(4), P(5), P(6), P(7), I(1), F(0), F(1), F(2),
                                              F(3), F(4), I(2), P(8), I(3), P(9), P(10), P(11), P(12), P(13), P(14), P(15),
                                              P(16), P(17), _stream(dev))
    finally:
        if cur != dev.index:
            torch.cuda.set_device(cur)
    if rc:
        _check(rc, "track_solve_batched")
    return bufs, rec, offsets


_recs_pinned = {}


def track_solve_records(rec, offsets):
    """The records of ``track_solve_batched`` on the host, one numpy array per image (empty for an image without rows): ONE
    copy of the concatenated tensor through a pinned buffer + ONE stream synchronisation, whatever the number of images —
    ``track_solve_record`` for a call's worth of records.  The pinned buffer is kept per device and grown, never per size."""
    dev, n = rec.device, rec.shape[0]
    host = _recs_pinned.get(dev)
    if host is None or host.shape[0] < n:
        host = _recs_pinned[dev] = torch.empty((max(2 * n, 4096),), dtype=torch.int32).pin_memory()
    host[:n].copy_(rec, non_blocking=True)
    torch.cuda.current_stream(dev).synchronize()
    whole = host.numpy()[:n].copy()
    return [whole[offsets[b]:offsets[b + 1]] for b in range(len(offsets) - 1)]


def wait_host_record(flag, fallback, spins=20000):
    """Block until the solver kernel has completed a pinned-memory record (``flag``: its numpy view): poll its completion
    word (stored last, behind a system-scope fence); if it does not show up within ``spins`` reads, call ``fallback`` — a
    synchronisation behind the launch (a kernel fault would otherwise spin for ever) — and raise if even that leaves the
    record incomplete.  Polling sees the record ~10 us earlier than an event wake-up."""
    for _ in range(spins):
        if flag[3] != 0:
            return
    fallback()
    if flag[3] == 0:
        raise RuntimeError("siammot_amd.track_solve: the solver kernel finished without completing its record")


def box_refine_post(head_out, num_classes, reg_classes, boxes, labels, ids, track_conf, weights, xform_clip, clip_wh,
                    tracktor=False):
    """``smot_box_refine_post_fwd``: the box head's post-processing of N propagated tracks + the score average of
    ``_refine_tracks`` in one launch (no synchronisation).  ``head_out`` ``[N, K + 4*KR]`` = class logits | box deltas
    (one GEMM over the concatenated ``cls_score`` / ``bbox_pred`` weights).  Returns ``(boxes [N,4], scores [N], ids [N],
    labels [N])`` in the box head's output order."""
    lib = _lib or load_library()
    head_out = _dev_f32(head_out, "head_out")
    boxes = _dev_f32(boxes, "boxes")
    track_conf = _dev_f32(track_conf, "track_conf")
    N = boxes.shape[0]
    dev = boxes.device
    for name, t in (("labels", labels), ("ids", ids)):
        if not (t.is_cuda and t.dtype is torch.int64 and t.is_contiguous() and t.device == dev and t.shape[0] == N):
            raise RuntimeError("siammot_amd.box_refine_post: %s must be a contiguous int64 [N] tensor on the boxes' device" % name)
    if head_out.dim() != 2 or head_out.shape[0] != N or head_out.shape[1] < num_classes + 4 * reg_classes:
        raise RuntimeError("siammot_amd.box_refine_post: head_out %s does not hold %d logits + %d deltas for %d rows"
                           % (tuple(head_out.shape), num_classes, 4 * reg_classes, N))
    out_boxes = torch.empty((N, 4), dtype=_F32, device=dev)
    out_scores = torch.empty((N,), dtype=_F32, device=dev)
    out_ids = torch.empty((N,), dtype=torch.int64, device=dev)
    out_labels = torch.empty((N,), dtype=torch.int64, device=dev)
    cw, ch = (0.0, 0.0) if clip_wh is None else (float(clip_wh[0]), float(clip_wh[1]))
    with _Launch(head_out, boxes, track_conf, labels, ids) as ln:
        rc = lib.smot_box_refine_post_fwd(_ptr(head_out), head_out.shape[1], int(num_classes), int(reg_classes), _ptr(boxes),
                                          _ptr(labels), _ptr(ids), _ptr(track_conf), N, float(weights[0]),
                                          float(weights[1]), float(weights[2]), float(weights[3]), float(xform_clip), cw, ch,
                                          int(bool(tracktor)), _ptr(out_boxes), _ptr(out_scores), _ptr(out_ids),
                                          _ptr(out_labels), ln.stream)
    _check(rc, "box_refine_post")
    return out_boxes, out_scores, out_ids, out_labels


# capacities of ``box_detect_post`` (include/smot_emm.h): beyond them ``TrackBoxHead.forward`` keeps its torch composition
BOX_DETECT_MAX_ROWS = 2048
BOX_DETECT_MAX_CLASSES = 128
BOX_DETECT_MAX_MASK_BYTES = 64 << 20   # NMS bitmask scratch the box head accepts (box_detect_mask_bytes); beyond: the torch path


def box_detect_mask_bytes(rows, num_classes):
    """Size of the largest part of ``box_detect_post``'s workspace, the NMS bitmasks: 8 bytes per (candidate row, 64-column
    tile) of every foreground class — 12 KB at 300 rows x 2 classes, 67 MB at the capacities 2048 x 128."""
    return (num_classes - 1) * rows * ((rows + 63) // 64) * 8


def box_detect_post(head_out, num_classes, reg_classes, boxes, count, weights, xform_clip, clip_wh, score_thresh,
                    nms_thresh):
    """``smot_box_detect_post_fwd``: the box head's post-processing of M proposals that are all detections (no ids) —
    soft-max, per-class decode, clip, threshold and per-class NMS in four launches, free of host synchronisation.
    ``head_out`` ``[M, >= K + 4*KR]`` = class logits | box deltas; ``count``: a device int32 tensor whose first element is
    the number of rows that exist (rows beyond it are never read).  Returns ``(boxes [cap,4], scores [cap], labels [cap]
    int64, rows [cap] int32, count [K] int32)`` with ``cap = M * (K - 1)``: classes ascending, ascending proposal row
    inside a class, rows beyond ``count[0]`` zero; ``count[1:]`` are the per-class counts.  Nothing is read back."""
    lib = _lib or load_library()
    head_out = _dev_f32(head_out, "head_out")
    boxes = _dev_f32(boxes, "boxes")
    if boxes.dim() != 2 or boxes.shape[1] != 4:
        raise RuntimeError("siammot_amd.box_detect_post: boxes must be [M, 4], got %s" % (tuple(boxes.shape),))
    M, dev = boxes.shape[0], boxes.device
    K, KR = int(num_classes), int(reg_classes)
    if head_out.dim() != 2 or head_out.shape[0] != M or head_out.shape[1] < K + 4 * KR:
        raise RuntimeError("siammot_amd.box_detect_post: head_out %s does not hold %d logits + %d deltas for %d rows"
                           % (tuple(head_out.shape), K, 4 * KR, M))
    if not (isinstance(count, torch.Tensor) and count.is_cuda and count.dtype is torch.int32 and count.device == dev
            and count.numel() >= 1 and count.is_contiguous()):
        raise RuntimeError("siammot_amd.box_detect_post: count must be a contiguous int32 tensor on the boxes' device")
    nbytes = lib.smot_box_detect_post_ws_bytes(M, K)
    if nbytes < 0:
        _check(-1, "box_detect_post")
    stream = _stream(dev)
    work = _workspace(dev, nbytes // 4, ("box_detect", stream.value))
    cap = M * (K - 1)
    out_boxes = torch.empty((cap, 4), dtype=_F32, device=dev)
    out_scores = torch.empty((cap,), dtype=_F32, device=dev)
    out_labels = torch.empty((cap,), dtype=torch.int64, device=dev)
    out_rows = torch.empty((cap,), dtype=torch.int32, device=dev)
    out_count = torch.empty((K,), dtype=torch.int32, device=dev)
    cw, ch = (0.0, 0.0) if clip_wh is None else (float(clip_wh[0]), float(clip_wh[1]))
    with _Launch(head_out, boxes, count) as ln:
        rc = lib.smot_box_detect_post_fwd(_ptr(head_out), head_out.shape[1], K, KR, _ptr(boxes), _ptr(count), M,
                                          float(weights[0]), float(weights[1]), float(weights[2]), float(weights[3]),
                                          float(xform_clip), cw, ch, float(score_thresh), float(nms_thresh), _ptr(work),
                                          _ptr(out_boxes), _ptr(out_scores), _ptr(out_labels), _ptr(out_rows),
                                          _ptr(out_count), ln.stream)
    _check(rc, "box_detect_post")
    return out_boxes, out_scores, out_labels, out_rows, out_count


def box_detect_mask_bytes_batched(rows_per_image, num_classes):
    """``box_detect_mask_bytes`` of a batched call: the sum over its images (one workspace segment per image)."""
    return sum(box_detect_mask_bytes(int(r), num_classes) for r in rows_per_image)


def box_detect_post_batched(head_out, num_classes, reg_classes, boxes, rows_per_image, count, weights, xform_clip, clip_wh,
                            score_thresh, nms_thresh):
    """``smot_box_detect_post_batched_fwd``: ``box_detect_post`` over the B images of a call in the same four launches.
    ``head_out`` ``[M, >= K + 4*KR]`` and ``boxes`` ``[M, 4]`` hold the rows of all images, image b the ``rows_per_image[b]``
    (host ints, each at most ``BOX_DETECT_MAX_ROWS``, zero is fine) consecutive rows after those of images 0..b-1; ``count``:
    a device int32 tensor of B elements, the rows of each image that exist; ``clip_wh``: the one image size.  Returns
    ``(boxes [cap,4], scores [cap], labels [cap] int64, rows [cap] int32, count [B, K] int32)`` with ``cap = M * (K - 1)``:
    the detections of image b start at row ``(K - 1) * sum(rows_per_image[:b])`` and are, with ``count[b]``, bit for bit what
    ``box_detect_post`` returns on that image's rows alone (``rows`` are relative to the image).  Nothing is read back."""
    lib = _lib or load_library()
    head_out = _dev_f32(head_out, "head_out")
    boxes = _dev_f32(boxes, "boxes")
    if boxes.dim() != 2 or boxes.shape[1] != 4:
        raise RuntimeError("siammot_amd.box_detect_post_batched: boxes must be [M, 4], got %s" % (tuple(boxes.shape),))
    M, dev = boxes.shape[0], boxes.device
    K, KR = int(num_classes), int(reg_classes)
    rows = [int(r) for r in rows_per_image]
    B = len(rows)
    if head_out.dim() != 2 or head_out.shape[0] != M or head_out.shape[1] < K + 4 * KR:
        raise RuntimeError("siammot_amd.box_detect_post_batched: head_out %s does not hold %d logits + %d deltas for %d rows"
                           % (tuple(head_out.shape), K, 4 * KR, M))
    if not 1 <= B <= MAX_IMAGES:
        raise RuntimeError("siammot_amd.box_detect_post_batched: %d images, need 1..%d per call" % (B, MAX_IMAGES))
    if not (isinstance(count, torch.Tensor) and count.is_cuda and count.dtype is torch.int32 and count.device == dev
            and count.numel() == B and count.is_contiguous()):
        raise RuntimeError("siammot_amd.box_detect_post_batched: count must be a contiguous int32 tensor of exactly one "
                           "element per image (%d) on the boxes' device" % B)
    starts = _row_starts(rows, B, M)
    nbytes = lib.smot_box_detect_post_batched_ws_bytes(B, _cast(starts), K)
    if nbytes < 0:
        _check(-1, "box_detect_post_batched")
    stream = _stream(dev)
    work = _workspace(dev, nbytes // 4, ("box_detect", stream.value))
    cap = M * (K - 1)
    out_boxes = torch.empty((cap, 4), dtype=_F32, device=dev)
    out_scores = torch.empty((cap,), dtype=_F32, device=dev)
    out_labels = torch.empty((cap,), dtype=torch.int64, device=dev)
    out_rows = torch.empty((cap,), dtype=torch.int32, device=dev)
    out_count = torch.empty((B, K), dtype=torch.int32, device=dev)
    cw, ch = (0.0, 0.0) if clip_wh is None else (float(clip_wh[0]), float(clip_wh[1]))
    with _Launch(head_out, boxes, count) as ln:
        rc = lib.smot_box_detect_post_batched_fwd(_ptr(head_out), head_out.shape[1], K, KR, _ptr(boxes), _ptr(count), M,
                                                  float(weights[0]), float(weights[1]), float(weights[2]), float(weights[3]),
                                                  float(xform_clip), cw, ch, float(score_thresh), float(nms_thresh),
                                                  _ptr(work), _ptr(out_boxes), _ptr(out_scores), _ptr(out_labels),
                                                  _ptr(out_rows), _ptr(out_count), ln.stream, B, _cast(starts))
    _check(rc, "box_detect_post_batched")
    return out_boxes, out_scores, out_labels, out_rows, out_count


def box_refine(features, scales, pooled, sampling_ratio, boxes, labels, ids, track_conf, layers, weights, xform_clip,
               clip_wh, tracktor=False):
    """``smot_box_refine_fwd``: 7x7 pooler -> fc6 -> fc7 -> cls_score | bbox_pred -> post-processing of N <= 128
    propagated tracks in ONE call (six launches, no synchronisation).  ``layers`` = (fc6.weight, fc6.bias, fc7.weight,
    fc7.bias, cls_score.weight, cls_score.bias, bbox_pred.weight, bbox_pred.bias).  Returns ``(boxes, scores, ids,
    labels)`` in the box head's output order."""
    lib = _lib or load_library()
    L = len(scales)
    feats, fp, hs, wsz, sc, ft = _level_arrays(features, scales, what=".box_refine")
    boxes = _dev_f32(boxes, "boxes")
    track_conf = _dev_f32(track_conf, "track_conf")
    w6, b6, w7, b7, wc, bc, wr, br = [_dev_f32(t, "box head parameter") for t in layers]
    N, C, dev = boxes.shape[0], feats[0].shape[1], boxes.device
    K, KR = wc.shape[0], wr.shape[0] // 4
    for name, t in (("labels", labels), ("ids", ids)):
        if not (t.is_cuda and t.dtype is torch.int64 and t.is_contiguous() and t.device == dev and t.shape[0] == N):
            raise RuntimeError("siammot_amd.box_refine: %s must be a contiguous int64 [N] tensor on the boxes' device" % name)
    if w6.shape[1] != C * pooled * pooled or w7.shape[1] != w6.shape[0] or wc.shape[1] != w7.shape[0] or wr.shape[1] != w7.shape[0]:
        raise RuntimeError("siammot_amd.box_refine: layer shapes do not chain")
    need = int(lib.smot_box_refine_ws_floats(N, C, int(pooled), w6.shape[0], w7.shape[0], K, KR))
    ws = _workspace(dev, need, ("box_refine", _stream(dev).value))        # per (device, stream): streams run concurrently
    out_boxes = torch.empty((N, 4), dtype=_F32, device=dev)
    out_scores = torch.empty((N,), dtype=_F32, device=dev)
    out_ids = torch.empty((N,), dtype=torch.int64, device=dev)
    out_labels = torch.empty((N,), dtype=torch.int64, device=dev)
    cw, ch = (0.0, 0.0) if clip_wh is None else (float(clip_wh[0]), float(clip_wh[1]))
    with _Launch(boxes, track_conf, labels, ids, w6, *feats) as ln:
        rc = lib.smot_box_refine_typed_fwd(_cast(fp), ft, _cast(hs), _cast(wsz), _cast(sc), L, C, int(pooled), int(sampling_ratio),
                                           _ptr(boxes), _ptr(labels), _ptr(ids), _ptr(track_conf), N,
                                           _ptr(w6), _ptr(b6), w6.shape[0], _ptr(w7), _ptr(b7), w7.shape[0],
                                           _ptr(wc), _ptr(bc), K, _ptr(wr), _ptr(br), KR,
                                           float(weights[0]), float(weights[1]), float(weights[2]), float(weights[3]),
                                           float(xform_clip), cw, ch, int(bool(tracktor)), _ptr(ws), _ptr(out_boxes),
                                           _ptr(out_scores), _ptr(out_ids), _ptr(out_labels), ln.stream)
    _check(rc, "box_refine")
    return out_boxes, out_scores, out_ids, out_labels


def linear_rows(x, weight, bias=None, relu=False, out=None):
    """``smot_linear_rows_fwd``: ``act(x @ weight.T + bias)`` for x ``[M, K]`` with M <= ``linear_rows_max_rows()`` rows
    (the box head's layers on the propagated tracks: weight streaming on all CUs instead of the library's 128
    workgroups at M = 30).  ``out``: an ``[M, >=N]`` row-major view to write into (column block).  Launch only."""
    lib = _lib or load_library()
    x = _dev_f32(x, "x")
    weight = _dev_f32(weight, "weight")
    M, K = x.shape
    N = weight.shape[0]
    if weight.shape[1] != K:
        raise RuntimeError("siammot_amd.linear_rows: x is [%d,%d], weight [%d,%d]" % (M, K, N, weight.shape[1]))
    if bias is not None:
        bias = _dev_f32(bias, "bias")
    y = out if out is not None else torch.empty((M, N), dtype=_F32, device=x.device)
    if y.stride(1) != 1 or y.shape[0] != M or y.shape[1] < N:
        raise RuntimeError("siammot_amd.linear_rows: out must be a row-major [M, >=N] view")
    need = int(lib.smot_linear_rows_ws_floats(M, K, N))
    ws = _workspace(x.device, need, ("linear_rows", _stream(x.device).value))
    with _Launch(x, weight, y) as ln:
        rc = lib.smot_linear_rows_fwd(_ptr(x), M, K, _ptr(weight), _ptr(bias), N, int(bool(relu)), _ptr(ws), _ptr(y),
                                      y.stride(0), ln.stream)
    _check(rc, "linear_rows")
    return y


def linear_rows_max_rows():
    return (_lib or load_library()).smot_linear_rows_max_rows()


def linear_rows_blocks(x, weight, bias=None, relu=False):
    """Measurement library only (inside ``debug_library()``): ``linear_rows`` on up to ``box_refine_batched_max_rows()`` rows
    in the form the batched refinement runs its layers — row blocks of 128 in the same two launches."""
    lib = _lib or load_library()
    if not hasattr(lib, "smot_debug_linear_rows_blocks_fwd"):
        raise RuntimeError("siammot_amd.linear_rows_blocks: an entry of the measurement library (ops.debug_library())")
    x = _dev_f32(x, "x")
    weight = _dev_f32(weight, "weight")
    M, K = x.shape
    N = weight.shape[0]
    if weight.shape[1] != K:
        raise RuntimeError("siammot_amd.linear_rows_blocks: x is [%d,%d], weight [%d,%d]" % (M, K, N, weight.shape[1]))
    if bias is not None:
        bias = _dev_f32(bias, "bias")
    y = torch.empty((M, N), dtype=_F32, device=x.device)
    need = int(lib.smot_debug_linear_rows_blocks_ws_floats(M, K, N))
    ws = _workspace(x.device, need, ("linear_rows", _stream(x.device).value))
    with _Launch(x, weight, y) as ln:
        rc = lib.smot_debug_linear_rows_blocks_fwd(_ptr(x), M, K, _ptr(weight), _ptr(bias), N, int(bool(relu)), _ptr(ws),
                                                   _ptr(y), N, ln.stream)
    _check(rc, "linear_rows_blocks")
    return y


def box_refine_batched_max_rows():
    return (_lib or load_library()).smot_box_refine_batched_max_rows()


BOX_REFINE_IMAGE_ROWS = 128          # rows of ONE image in a batched refinement call (the one-call path's own limit)


def _refine_outputs(N, dev):
    return (torch.empty((N, 4), dtype=_F32, device=dev), torch.empty((N,), dtype=_F32, device=dev),
            torch.empty((N,), dtype=torch.int64, device=dev), torch.empty((N,), dtype=torch.int64, device=dev))


def box_refine_post_batched(head_out, num_classes, reg_classes, boxes, labels, ids, track_conf, rows_per_image, weights,
                            xform_clip, clip_wh, tracktor=False):
    """``smot_box_refine_post_batched_fwd``: ``box_refine_post`` over the B images of a call in one launch (a workgroup per
    image).  The rows of all images are concatenated, image b the ``rows_per_image[b]`` (host ints, zero is fine) consecutive
    rows after those of images 0..b-1; ``clip_wh``: the one image size.  Returns ``(boxes [N,4], scores [N], ids [N], labels
    [N])`` with image b's rows in its input segment, bit for bit what ``box_refine_post`` returns on them alone."""
    lib = _lib or load_library()
    head_out = _dev_f32(head_out, "head_out")
    boxes = _dev_f32(boxes, "boxes")
    track_conf = _dev_f32(track_conf, "track_conf")
    N, dev = boxes.shape[0], boxes.device
    rows = [int(r) for r in rows_per_image]
    B = len(rows)
    for name, t in (("labels", labels), ("ids", ids)):
        if not (t.is_cuda and t.dtype is torch.int64 and t.is_contiguous() and t.device == dev and t.shape[0] == N):
            raise RuntimeError("siammot_amd.box_refine_post_batched: %s must be a contiguous int64 [N] tensor on the boxes' "
                               "device" % name)
    if head_out.dim() != 2 or head_out.shape[0] != N or head_out.shape[1] < num_classes + 4 * reg_classes:
        raise RuntimeError("siammot_amd.box_refine_post_batched: head_out %s does not hold %d logits + %d deltas for %d rows"
                           % (tuple(head_out.shape), num_classes, 4 * reg_classes, N))
    if not 1 <= B <= MAX_IMAGES:
        raise RuntimeError("siammot_amd.box_refine_post_batched: %d images, need 1..%d per call" % (B, MAX_IMAGES))
    starts = _row_starts(rows, B, N)
    out = _refine_outputs(N, dev)
    cw, ch = (0.0, 0.0) if clip_wh is None else (float(clip_wh[0]), float(clip_wh[1]))
    with _Launch(head_out, boxes, track_conf, labels, ids) as ln:
        rc = lib.smot_box_refine_post_batched_fwd(_ptr(head_out), head_out.shape[1], int(num_classes), int(reg_classes),
                                                  _ptr(boxes), _ptr(labels), _ptr(ids), _ptr(track_conf), N,
                                                  float(weights[0]), float(weights[1]), float(weights[2]), float(weights[3]),
                                                  float(xform_clip), cw, ch, int(bool(tracktor)), _ptr(out[0]), _ptr(out[1]),
                                                  _ptr(out[2]), _ptr(out[3]), ln.stream, B, _cast(starts))
    _check(rc, "box_refine_post_batched")
    return out


def box_refine_batched(features, scales, pooled, sampling_ratio, boxes, labels, ids, track_conf, rows_per_image, layers,
                       weights, xform_clip, clip_wh, tracktor=False):
    """``smot_box_refine_batched_typed_fwd``: ``box_refine`` over the B images of a call — ``features[l]`` = ``[B, C, H_l,
    W_l]``, the rows of all images concatenated, image b the ``rows_per_image[b]`` (host ints, zero is fine, at most
    ``BOX_REFINE_IMAGE_ROWS`` each and ``box_refine_batched_max_rows()`` in all) rows after those of images 0..b-1 — in eight
    launches whatever B is, no synchronisation.  Returns ``(boxes, scores, ids, labels)`` with image b's rows in its input
    segment, bit for bit what ``box_refine`` returns on ``features[l][b:b+1]`` and those rows."""
    lib = _lib or load_library()
    L = len(scales)
    feats, fp, hs, wsz, sc, ft = _level_arrays(features, scales, what=".box_refine_batched", batched=True)
    boxes = _dev_f32(boxes, "boxes")
    track_conf = _dev_f32(track_conf, "track_conf")
    w6, b6, w7, b7, wc, bc, wr, br = [_dev_f32(t, "box head parameter") for t in layers]
    N, dev = boxes.shape[0], boxes.device
    B, C = feats[0].shape[0], feats[0].shape[1]
    K, KR = wc.shape[0], wr.shape[0] // 4
    for name, t in (("labels", labels), ("ids", ids)):
        if not (t.is_cuda and t.dtype is torch.int64 and t.is_contiguous() and t.device == dev and t.shape[0] == N):
            raise RuntimeError("siammot_amd.box_refine_batched: %s must be a contiguous int64 [N] tensor on the boxes' device"
                               % name)
    if w6.shape[1] != C * pooled * pooled or w7.shape[1] != w6.shape[0] or wc.shape[1] != w7.shape[0] or wr.shape[1] != w7.shape[0]:
        raise RuntimeError("siammot_amd.box_refine_batched: layer shapes do not chain")
    if B > MAX_IMAGES:
        raise RuntimeError("siammot_amd.box_refine_batched: %d images, at most %d per call" % (B, MAX_IMAGES))
    starts = _row_starts(rows_per_image, B, N)
    need = int(lib.smot_box_refine_batched_ws_floats(N, C, int(pooled), w6.shape[0], w7.shape[0], K, KR))
    ws = _workspace(dev, need, ("box_refine", _stream(dev).value))
    out = _refine_outputs(N, dev)
    cw, ch = (0.0, 0.0) if clip_wh is None else (float(clip_wh[0]), float(clip_wh[1]))
    with _Launch(boxes, track_conf, labels, ids, w6, *feats) as ln:
        rc = lib.smot_box_refine_batched_typed_fwd(_cast(fp), ft, _cast(hs), _cast(wsz), _cast(sc), L, C, int(pooled),
                                                   int(sampling_ratio), _ptr(boxes), _ptr(labels), _ptr(ids), _ptr(track_conf),
                                                   N, _ptr(w6), _ptr(b6), w6.shape[0], _ptr(w7), _ptr(b7), w7.shape[0],
                                                   _ptr(wc), _ptr(bc), K, _ptr(wr), _ptr(br), KR,
                                                   float(weights[0]), float(weights[1]), float(weights[2]), float(weights[3]),
                                                   float(xform_clip), cw, ch, int(bool(tracktor)), _ptr(ws), _ptr(out[0]),
                                                   _ptr(out[1]), _ptr(out[2]), _ptr(out[3]), ln.stream, B, _cast(starts))
    _check(rc, "box_refine_batched")
    return out


def box_refine_post_max_rows():
    return (_lib or load_library()).smot_box_refine_post_max_rows()


_FRAME_PTRS = ("feats", "heights", "widths", "pad_cells", "scales", "predictor_params", "hann",
               "fc6_w", "fc6_b", "fc7_w", "fc7_b", "cls_w", "cls_b", "reg_w", "reg_b", "pool_state",
               # this frame: the head
               "head_ws", "tpl_boxes", "sr", "templates", "order_hint", "trk_ids", "trk_labels", "trk_boxes", "trk_conf",
               # this frame: refinement, detections, solver, next memory
               "refine_ws", "ref_boxes", "ref_scores", "ref_ids", "ref_labels",
               "det_boxes", "det_scores", "det_ids", "det_labels",
               "out_boxes", "out_scores", "out_ids", "out_labels", "act_boxes", "act_ids", "act_labels", "act_scores",
               "record", "next_templates", "next_sr", "next_order_hint",
               # dormant rows carried by the solver's launch (STAGE_CARRY)
               "carry_templates", "carry_boxes", "carry_sr", "carry_ids", "carry_labels", "carry_scores")
_FRAME_INTS = ("n_trk", "stages", "n_det", "num_levels", "C", "rx", "rz", "sampling_ratio", "gn_groups", "up",
               "use_centerness", "refine", "box_pooled", "box_sampling_ratio", "dim6", "dim7", "num_classes", "reg_classes",
               "tracktor", "max_dormant_frames", "pool_capacity", "carry_src_row0", "carry_rows", "carry_dst_row0")
_FRAME_FLOATS = ("track_thresh", "start_thresh", "resume_thresh", "gn_eps", "pad_pixels", "one_minus_sigma", "sigma",
                 "clip_w", "clip_h", "box_wx", "box_wy", "box_ww", "box_wh", "box_xform_clip",
                 "nms_thresh", "search_expansion", "min_search_wh")
STAGE_HEAD, STAGE_REFINE, STAGE_SOLVE, STAGE_EXTRACT, STAGE_CARRY = 1, 2, 4, 8, 16


class FrameArgs(object):
    """``smot_frame_args`` of include/smot_emm.h as one byte buffer: 52 pointers, 24 ints, 17 floats, in the header's
    order.  Fields are plain Python attributes (``__slots__``); ``pack()`` writes all of them with one ``struct.pack_into``
    (a ctypes.Structure costs ~0.4 us per field assignment).  The fields that change from frame to frame are contiguous
    inside each group: ``poke_head`` / ``poke_rest`` rewrite only those ranges of a block that was packed once."""
    __slots__ = _FRAME_PTRS + _FRAME_INTS + _FRAME_FLOATS + ("_buf", "_addr")
    _FMT = struct.Struct("<%dQ%di%df" % (len(_FRAME_PTRS), len(_FRAME_INTS), len(_FRAME_FLOATS)))
    _HEAD0, _HEAD1 = _FRAME_PTRS.index("head_ws"), _FRAME_PTRS.index("trk_conf") + 1
    _REST1 = len(_FRAME_PTRS)
    _INT0 = 8 * len(_FRAME_PTRS)
    _FLT0 = _INT0 + 4 * len(_FRAME_INTS)
    _HEAD_FMT = struct.Struct("<%dQ" % (_HEAD1 - _HEAD0))
    _REST_FMT = struct.Struct("<%dQ" % (_REST1 - _HEAD1))
    _II = struct.Struct("<ii")
    _III = struct.Struct("<iii")
    _FFF = struct.Struct("<fff")
    _CARRY_INT0 = _INT0 + 4 * _FRAME_INTS.index("carry_src_row0")

    def __init__(self):
        for n in _FRAME_PTRS + _FRAME_INTS:
            setattr(self, n, 0)
        for n in _FRAME_FLOATS:
            setattr(self, n, 0.0)
        self._buf = ctypes.create_string_buffer(self._FMT.size + 8)
        self._addr = ctypes.addressof(self._buf)

    def pack(self):
        g = self.__getattribute__
        self._FMT.pack_into(self._buf, 0, *[g(n) or 0 for n in _FRAME_PTRS], *[int(g(n)) for n in _FRAME_INTS],
                            *[float(g(n)) for n in _FRAME_FLOATS])
        return self._addr

    def poke_head(self, ptrs, n_trk, stages):
        """Rewrite the head's per-frame pointers (``head_ws`` .. ``trk_conf``, in that order; None = NULL) and
        ``n_trk``, ``stages``."""
        self._HEAD_FMT.pack_into(self._buf, 8 * self._HEAD0, *ptrs)
        self._II.pack_into(self._buf, self._INT0, n_trk, stages)
        return self._addr

    _HINT_OFF = 8 * _FRAME_PTRS.index("order_hint")
    _Q = struct.Struct("<Q")

    def fix_head(self, n_trk, hint_ptr):
        """Correct the row count and the order-hint pointer of a head range poked on a guess (stage HEAD stands)."""
        self._II.pack_into(self._buf, self._INT0, n_trk, STAGE_HEAD)
        self._Q.pack_into(self._buf, self._HINT_OFF, hint_ptr)

    def poke_rest(self, ptrs, stages, n_det, thresholds, carry=(0, 0, 0), n_trk=None):
        """Rewrite the per-frame pointers behind the head's (``refine_ws`` .. ``carry_scores``), ``stages``,
        ``n_det``, the three solver thresholds and ``carry`` = (carry_src_row0, carry_rows, carry_dst_row0).
        ``n_trk``: the row count of THIS call's propagated tracks — written here too, because the head range may have been
        poked on a guess for a head that never ran (a frame that leaves no track is followed by a call without
        a head; with the guessed count still in the block the solver read one row too many)."""
        self._REST_FMT.pack_into(self._buf, 8 * self._HEAD1, *ptrs)
        if n_trk is None:
            self._II.pack_into(self._buf, self._INT0 + 4, stages, n_det)
        else:
            self._III.pack_into(self._buf, self._INT0, n_trk, stages, n_det)
        self._III.pack_into(self._buf, self._CARRY_INT0, *carry)
        self._FFF.pack_into(self._buf, self._FLT0, *thresholds)
        return self._addr


def track_frame_addr(lib, addr, dev, stream, feat_type=0):
    """``smot_track_frame_fwd`` on a block the caller keeps packed (``FrameArgs.poke_head`` / ``poke_rest``);
    ``feat_type``: the element type of the maps the block's ``feats`` name (``FEAT_TYPES``; the struct has no field for it)."""
    cur = torch.cuda.current_device()
    if cur != dev.index:
        torch.cuda.set_device(dev.index)
        try:
            rc = (lib.smot_track_frame_fwd(addr, stream) if feat_type == 0
                  else lib.smot_track_frame_typed_fwd(addr, feat_type, stream))
        finally:
            torch.cuda.set_device(cur)
    elif feat_type == 0:
        rc = lib.smot_track_frame_fwd(addr, stream)
    else:
        rc = lib.smot_track_frame_typed_fwd(addr, feat_type, stream)
    if rc:
        _check(rc, "track_frame")


# dormant rows of the track memory copied on the device (TrackingLoop): launches, and frames on which the rows had been
# copied a call early on the guess that nothing changed ("ahead": kept as they were / redone)
MEMORY_CARRY = _collections.Counter()
MEMORY_CARRY_MAX_ROWS = 256
_carry_rows_t = ctypes.c_int * MEMORY_CARRY_MAX_ROWS


def memory_carry(src, src_rows_total, dst, dst_capacity, rows, dst_row0, row_floats, dev, stream, dst_row0_dev=0, lib=None):
    """``smot_memory_carry_fwd`` on bare device addresses: ``src`` / ``dst`` = (templates, boxes, search regions, ids,
    labels, scores) of the memory the frame's head ran on / of the memory being built; ``rows`` the source rows of the
    dormant tracks in the order they are appended (track_head.py:83-86), to rows ``dst_row0`` .. of the destination."""
    lib = lib or _lib or load_library()
    D = len(rows)
    arr = _carry_rows_t(*rows)
    cur = torch.cuda.current_device()
    if cur != dev.index:
        torch.cuda.set_device(dev.index)
    try:
        rc = lib.smot_memory_carry_fwd(src[0], src[1], src[2], src[3], src[4], src[5], int(src_rows_total), dst[0], dst[1], dst[2],
                                       dst[3], dst[4], dst[5], int(dst_capacity), arr, D, int(dst_row0), dst_row0_dev,
                                       int(row_floats), stream)
    finally:
        if cur != dev.index:
            torch.cuda.set_device(cur)
    if rc:
        _check(rc, "memory_carry")
    MEMORY_CARRY["launched"] += 1


def segment_pointers(seg, dev):
    """(boxes, scores, ids, labels or 0, rows) of one checked segment as the solver's entry points take them; None: empty."""
    if seg is None or seg[0].shape[0] == 0:
        return 0, 0, 0, 0, 0
    b, s_, i_, l_ = seg
    _check_segment(b, s_, i_, l_, dev)
    return b.data_ptr(), s_.data_ptr(), i_.data_ptr(), l_.data_ptr() if l_ is not None else 0, b.shape[0]


def _check_segment(b, s_, i_, l_, dev):
    """The solver's input contract for one segment (boxes, scores, ids, labels or None)."""
    if not (b.is_cuda and b.dtype is _F32 and b.is_contiguous() and s_.dtype is _F32 and s_.is_contiguous()
            and i_.dtype is torch.int64 and i_.is_contiguous()):
        raise RuntimeError("siammot_amd.track_solve: boxes/scores must be contiguous fp32 and ids int64 device tensors")
    if b.device != dev:
        raise RuntimeError("siammot_amd.track_solve: boxes live on %s, the pool state on %s" % (b.device, dev))
    if l_ is not None and not (l_.dtype is torch.int64 and l_.is_contiguous() and l_.device == dev):
        raise RuntimeError("siammot_amd.track_solve: labels must be a contiguous int64 tensor on the boxes' device")


def track_solve_max_boxes():
    return (_lib or load_library()).smot_track_solve_max_boxes()


def preprocess_frame(frame, tables, out_hw, mean, std, to_bgr255):
    """uint8 RGB ``[H,W,3]`` device tensor -> fp32 ``[3,OH,OW]`` network input (resize + ToTensor + Normalize in
    one launch).  ``tables`` = (xbounds, xcoeffs, ybounds, ycoeffs, max_tile_rows) from ``siammot_amd.preprocess``."""
    lib = load_library()
    if not isinstance(frame, torch.Tensor) or not frame.is_cuda or frame.dtype != torch.uint8:
        raise RuntimeError("siammot_amd.preprocess_frame: frame must be a uint8 device (ROCm) tensor — no CPU path exists")
    if frame.dim() != 3 or frame.shape[2] != 3:
        raise RuntimeError("siammot_amd.preprocess_frame: frame must be [H, W, 3], got %s" % (tuple(frame.shape),))
    frame = frame.contiguous()
    H, W, _ = frame.shape
    xb, xk, yb, yk, max_rows = tables
    OH, OW = out_hw
    if xb.shape[0] != OW or yb.shape[0] != OH:
        raise RuntimeError("siammot_amd.preprocess_frame: tables are for %dx%d, asked for %dx%d"
                           % (yb.shape[0], xb.shape[0], OH, OW))
    out = torch.empty((3, OH, OW), dtype=torch.float32, device=frame.device)
    m = (ctypes.c_float * 3)(*[float(v) for v in mean])
    s = (ctypes.c_float * 3)(*[float(v) for v in std])
    with _Launch(frame, xb, xk, yb, yk) as ln:
        rc = lib.smot_preprocess_fwd(_ptr(frame), H, W, _ptr(xb), _ptr(xk), xk.shape[1], _ptr(yb), _ptr(yk), yk.shape[1],
                                     OH, OW, int(max_rows), _cast(m), _cast(s), int(bool(to_bgr255)), _ptr(out), ln.stream)
    _check(rc, "preprocess_frame")
    return out


def preprocess_frames(frames, tables, out_hw, mean, std, to_bgr255, dtype=torch.float32, channels_last=False, out=None):
    """The frames of several cameras -> one network input ``[B, 3, OH, OW]`` of ``dtype`` (fp32, fp16 or bf16), contiguous or
    (``channels_last``) in ``torch.channels_last`` memory, in one library call (``smot_preprocess_batch_fwd``: one launch
    per 16 images).  ``frames``: uint8 RGB ``[H_b, W_b, 3]`` device tensors, each of its own size; ``tables``: per frame the
    tuple ``preprocess_frame`` takes (frames of one size share theirs), all made for ``out_hw``.  A half result is bit for
    bit ``fp32_result.to(dtype)``.  ``out``: a tensor of exactly that shape, dtype and layout on the frames' device, written
    in place and returned (anything else raises before the launch)."""
    lib = load_library()
    frames, tables = list(frames), list(tables)
    B = len(frames)
    if not 1 <= B <= MAX_IMAGES:
        raise RuntimeError("siammot_amd.preprocess_frames: %d frames, need 1..%d per call" % (B, MAX_IMAGES))
    if len(tables) != B:
        raise RuntimeError("siammot_amd.preprocess_frames: %d table tuples for %d frames" % (len(tables), B))
    if dtype not in FEAT_TYPES:
        raise RuntimeError("siammot_amd.preprocess_frames: dtype must be float32, float16 or bfloat16, got %s" % (dtype,))
    OH, OW = int(out_hw[0]), int(out_hw[1])
    keep = []
    for b, f in enumerate(frames):
        if not isinstance(f, torch.Tensor) or not f.is_cuda or f.dtype != torch.uint8:
            raise RuntimeError("siammot_amd.preprocess_frames: frames[%d] must be a uint8 device (ROCm) tensor — no CPU path "
                               "exists" % b)
        if f.dim() != 3 or f.shape[2] != 3:
            raise RuntimeError("siammot_amd.preprocess_frames: frames[%d] must be [H, W, 3], got %s" % (b, tuple(f.shape)))
        xb, _, yb, _, _ = tables[b]
        if xb.shape[0] != OW or yb.shape[0] != OH:
            raise RuntimeError("siammot_amd.preprocess_frames: tables[%d] are for %dx%d, asked for %dx%d"
                               % (b, yb.shape[0], xb.shape[0], OH, OW))
        keep.append(f.contiguous())
    dev = keep[0].device
    fmt = _CL if channels_last else torch.contiguous_format
    if out is None:
        out = torch.empty((B, 3, OH, OW), dtype=dtype, device=dev, memory_format=fmt)
    else:
        if not isinstance(out, torch.Tensor) or not out.is_cuda or out.device != dev:
            raise RuntimeError("siammot_amd.preprocess_frames: out must be a tensor on the frames' device (%s)" % dev)
        if tuple(out.shape) != (B, 3, OH, OW) or out.dtype != dtype:
            raise RuntimeError("siammot_amd.preprocess_frames: out must be %s of %s, got %s of %s"
                               % ((B, 3, OH, OW), dtype, tuple(out.shape), out.dtype))
        want = (OH * OW * 3, 1, OW * 3, 3) if channels_last else (3 * OH * OW, OH * OW, OW, 1)
        if tuple(out.stride())[B == 1:] != want[B == 1:]:           # (a dimension of size 1 has no stride to speak of)
            raise RuntimeError("siammot_amd.preprocess_frames: out must be %s with strides %s, got strides %s"
                               % ("channels-last" if channels_last else "contiguous", want, tuple(out.stride())))
    I, P = ctypes.c_int * B, ctypes.c_void_p * B
    tabs = [t for tb in tables for t in tb[:4]]
    m = (ctypes.c_float * 3)(*[float(v) for v in mean])
    s = (ctypes.c_float * 3)(*[float(v) for v in std])
    with _Launch(out, *(keep + tabs)) as ln:
        rc = lib.smot_preprocess_batch_fwd(
            B, _cast(P(*[f.data_ptr() for f in keep])), _cast(I(*[f.shape[0] for f in keep])),
            _cast(I(*[f.shape[1] for f in keep])), _cast(P(*[tb[0].data_ptr() for tb in tables])),
            _cast(P(*[tb[1].data_ptr() for tb in tables])), _cast(I(*[tb[1].shape[1] for tb in tables])),
            _cast(P(*[tb[2].data_ptr() for tb in tables])), _cast(P(*[tb[3].data_ptr() for tb in tables])),
            _cast(I(*[tb[3].shape[1] for tb in tables])), _cast(I(*[int(tb[4]) for tb in tables])), OH, OW, _cast(m), _cast(s),
            int(bool(to_bgr255)), _ptr(out), FEAT_TYPES[dtype] | (FEAT_CHANNELS_LAST if channels_last else 0), ln.stream)
    _check(rc, "preprocess_frames")
    return out
