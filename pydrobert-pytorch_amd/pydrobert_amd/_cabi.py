"""ctypes binding of libpdt_amd.so -- the C ABI declared in include/pdt_amd.h.

This is the only place the host package touches native code.  The library is built
in-tree by ``csrc/Makefile`` (``__graft_entry__.build()``); if it is missing or fails
to load, every operator raises -- there is no fallback path.
"""

import ctypes
import os
import threading
import time

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PDT_AMD_LIB", os.path.join(_HERE, "_lib", "libpdt_amd.so"))

# what pdt_amd_abi_version() must report: the table below is this version's.  A change of the table bumps it
# on both sides.  The one exception so far: the return and combinatorics entry points were added at 12,
# because tests/test_random_walk_cpu.py pinned that number; a library built before them is still refused by
# lib(), with its missing-entry-point message in place of the version one.  13: pdt_pad_variable_backward takes
# the gradient's dtype (a library of version 12 would read the arguments one place off).  14: the attention
# entry points' lse holds two numbers per row, (2, R) (a library of version 13 wrote and read R).  The relaxed-
# sampling entry points were added at 14 in the way of the first exception (the same test file pins 14 now; no
# existing declaration changed), and so were those of the estimators (pdt_mc_reduce*, pdt_imh_chain) and the
# host-only plans of the searches with an n-gram model (pdt_ctc_lm_table_search_plan,
# pdt_ctc_lookup_lm_search_lds_bytes) and the backward of relaxed sampling (pdt_relaxed_backward_parts,
# pdt_relaxed_backward_workspace_bytes, pdt_relaxed_gumbel_backward, pdt_relaxed_bernoulli_backward) and the
# host-only plans of BeamSearch's kernels (pdt_beam_search_step_plan, pdt_beam_search_table_plan) and the fused
# ConcatSoftAttention score (pdt_concat_score, pdt_concat_score_backward, pdt_concat_score_workspace_bytes,
# pdt_concat_score_plan) and the warps' position gradients with the spline evaluation's adjoint
# (pdt_dense_image_warp_flow_backward[_f64], pdt_sparse_image_warp_position_backward[_f64],
# pdt_spline_eval_adjoint, pdt_spline_eval_adjoint_plan) and the entry points that read float16 / bfloat16
# logits as they are (pdt_ctc_prefix_search_elem, pdt_ctc_prefix_search_wide_elem, pdt_ctc_greedy_search_elem,
# pdt_sequence_log_probs_forward_elem, pdt_sequence_log_probs_backward_elem: new names beside the float32 ones,
# which keep their declarations) with the host-only pdt_ctc_prefix_search_wide_plan, and the same for the
# hard-OCD loss (pdt_ocd_loss_forward_elem, pdt_ocd_loss_backward_elem) and the attention entry points
# (pdt_attn_workspace_bytes_elem, pdt_attn_dot_elem, pdt_attn_dot_backward_elem, pdt_attn_pool_elem,
# pdt_attn_pool_backward_elem: the five without the suffix keep refusing every dtype code but 0 and 1) and
# SpecAugment's application (pdt_spec_augment_apply_elem, pdt_spec_augment_apply_warp_elem,
# pdt_spec_augment_apply_backward_elem) with the host-only pdt_spec_augment_apply_form and
# pdt_spec_augment_backward_workspace_bytes.
ABI_VERSION = 14

PDT_OK = 0
PDT_E_ARG = -1
PDT_E_TOO_LONG = -2
PDT_E_UNSUPPORTED = -3
MODE_FINAL, MODE_PREFIX = 0, 1
WARN_REF_NO_EOS, WARN_HYP_NO_EOS, WARN_EMPTY_REF = 1, 2, 4

_c = ctypes
_P = _c.c_void_p
_I64 = _c.c_int64
_INT = _c.c_int
_F = _c.c_float

# name -> (restype, argtypes); mirrors include/pdt_amd.h declaration by declaration
SIGNATURES = {
    "pdt_amd_abi_version": (_INT, []),
    "pdt_amd_set_switch": (_INT, [_c.c_char_p, _INT]),
    "pdt_amd_get_switch": (_INT, [_c.c_char_p, _P]),
    "pdt_lev": (
        _INT,
        [_P, _I64, _I64, _I64, _P, _I64, _I64, _I64, _I64, _INT, _I64, _INT, _F, _F, _F]
        + [_INT, _INT, _INT, _F, _INT, _P, _I64, _I64, _P, _P, _P, _P, _I64, _P],
    ),
    "pdt_lev_keep": (
        _INT,
        [_P, _I64, _I64, _I64, _P, _I64, _I64, _I64, _I64, _INT, _I64, _INT, _F, _F, _F]
        + [_INT, _INT, _INT, _F, _INT, _P, _I64, _I64, _P, _P, _P, _P, _I64, _P],
    ),
    "pdt_lev_classified": (
        _INT,
        [_P, _I64, _I64, _I64, _P, _I64, _I64, _I64, _I64, _INT, _I64, _INT, _F, _F, _F]
        + [_INT, _INT, _INT, _F, _INT, _P, _I64, _I64, _P, _P, _P, _P, _I64, _P],
    ),
    "pdt_lev_workspace_bytes": (_I64, [_I64, _I64, _I64]),
    "pdt_fill_after_eos": (_INT, [_P, _I64, _I64, _I64, _I64, _P, _I64, _I64, _P, _P]),
    "pdt_oc_mask_words": (_I64, [_I64]),
    "pdt_oc_mask": (
        _INT,
        [_P, _I64, _I64, _I64, _P, _I64, _I64, _I64, _I64, _INT, _I64, _INT, _F, _F, _F]
        + [_INT, _P, _P, _P, _P, _P, _I64, _P],
    ),
    "pdt_oc_mask_workspace_bytes": (_I64, [_I64, _I64, _I64]),
    "pdt_oc_expand": (_INT, [_P, _P, _I64, _I64, _I64, _I64, _I64, _P, _I64, _I64, _P]),
    "pdt_ocd_loss_forward": (
        _INT, [_P, _I64, _I64, _I64, _I64, _I64, _I64, _P, _P, _I64, _P, _I64, _P, _P, _P, _P],
    ),
    "pdt_ocd_loss_backward": (
        _INT, [_P, _I64, _I64, _I64, _I64, _I64, _I64, _P, _P, _I64, _P, _I64, _P, _P, _P],
    ),
    "pdt_ocd_loss_forward_elem": (
        _INT, [_P, _I64, _I64, _I64, _I64, _I64, _I64, _P, _P, _I64, _P, _I64, _P, _P, _P, _P, _INT],
    ),
    "pdt_ocd_loss_backward_elem": (
        _INT, [_P, _I64, _I64, _I64, _I64, _I64, _I64, _P, _P, _I64, _P, _I64, _P, _P, _P, _INT],
    ),
    "pdt_ctc_prefix_search_advance": (
        _INT,
        [_P, _I64, _I64, _I64, _P, _I64, _I64, _P, _I64, _I64, _I64, _I64, _I64]
        + [_P, _I64, _I64, _P, _I64, _I64, _P, _I64, _I64, _I64, _I64, _P, _I64, _I64]
        + [_P, _I64, _I64, _P, _I64, _I64, _I64, _P, _P, _P, _P, _P, _P, _P, _P, _P],
    ),
    "pdt_ctc_prefix_search_advance_lm": (
        _INT,
        [_P, _F, _INT, _P, _I64, _I64, _P, _I64, _I64, _I64, _I64, _I64]
        + [_P, _I64, _I64, _P, _I64, _I64, _P, _I64, _I64, _I64, _I64, _P, _I64, _I64]
        + [_P, _I64, _I64, _P, _I64, _I64, _I64, _P, _P, _P, _P, _P, _P, _P, _P, _P],
    ),
    "pdt_beam_search_table": (
        _INT,
        [_P, _I64, _I64, _I64, _P, _I64, _I64, _I64, _I64, _I64, _INT, _I64, _INT, _P, _P, _P, _P, _P, _P],
    ),
    "pdt_beam_search_table_paths": (_INT, [_P, _P, _I64, _I64, _I64, _I64, _I64, _P, _P]),
    "pdt_beam_search_table_plan": (_INT, [_I64, _I64, _I64, _I64]),
    "pdt_beam_search_step_plan": (_INT, [_I64, _I64, _I64, _INT, _I64, _P]),
    "pdt_lens_reach": (_INT, [_P, _I64, _I64, _I64, _I64, _I64, _P, _P]),
    "pdt_beam_search_advance": (
        _INT,
        [_P, _I64, _I64, _I64, _I64, _I64, _I64, _I64, _P, _I64, _I64, _P, _I64, _I64, _I64, _I64]
        + [_P, _I64, _I64, _I64, _P, _P, _P, _P, _P],
    ),
    "pdt_ctc_lookup_lm_search_lds_bytes": (_I64, [_I64, _I64]),
    "pdt_ctc_lookup_lm_search_workspace_bytes": (_I64, [_I64, _I64, _I64, _I64, _I64, _I64]),
    "pdt_ctc_lookup_lm_search": (
        _INT,
        [_P, _I64, _I64, _I64, _P, _I64, _I64, _I64, _I64, _P, _P, _P, _P, _P, _P, _P, _I64, _I64, _I64, _F, _INT]
        + [_P, _P, _P, _P, _P, _I64, _P],
    ),
    "pdt_lm_factor_table": (_INT, [_P, _I64, _I64, _F, _INT, _P, _I64, _P]),
    "pdt_ctc_lm_table_search_workspace_bytes": (_I64, [_I64, _I64, _I64, _I64]),
    "pdt_ctc_lm_table_search_plan": (_INT, [_I64, _I64, _I64, _P]),
    "pdt_ctc_lm_table_search": (
        _INT,
        [_P, _I64, _I64, _I64, _I64, _I64, _I64, _P, _I64, _I64, _P, _P, _I64, _I64, _I64, _I64, _I64, _F, _INT, _P, _P, _P, _P, _P],
    ),
    "pdt_beam_search_step": (
        _INT,
        [_P, _I64, _I64, _I64, _I64, _I64, _I64, _I64, _P, _I64, _I64, _P, _I64, _I64, _I64, _I64]
        + [_P, _I64, _I64, _INT, _I64, _INT, _I64, _P, _P, _P, _P, _P, _P, _P],
    ),
    "pdt_beam_search_step_table": (
        _INT,
        [_P, _I64, _I64, _I64, _P, _P, _I64, _I64, _I64, _I64, _P, _I64, _I64, _P, _I64, _I64, _I64, _I64]
        + [_P, _I64, _I64, _INT, _I64, _INT, _I64, _P, _P, _P, _P, _P, _P, _P],
    ),
    "pdt_row_log_softmax_stats": (_INT, [_P, _I64, _I64, _I64, _I64, _P, _P]),
    "pdt_random_walk_advance": (
        _INT,
        [_P, _I64, _I64, _I64, _I64, _P, _I64, _P, _I64, _P, _I64, _I64, _I64, _P, _I64, _P, _P, _P, _P, _P],
    ),
    "pdt_random_walk_step": (_INT, [_P, _I64, _I64, _I64, _I64, _P, _INT, _I64, _P, _P, _P, _P, _P, _P, _P]),
    "pdt_random_walk_table": (
        _INT,
        [_P, _I64, _I64, _I64, _I64, _P, _P, _I64, _I64, _INT, _I64, _P, _P, _P, _P, _P, _P, _P, _P],
    ),
    "pdt_ctc_greedy_search": (
        _INT, [_P, _I64, _I64, _I64, _I64, _I64, _I64, _P, _I64, _INT, _P, _P, _I64, _I64, _P, _P],
    ),
    "pdt_sequence_log_probs_forward": (_INT, [_P, _P, _I64, _I64, _I64, _I64, _INT, _I64, _P, _P]),
    "pdt_sequence_log_probs_backward": (
        _INT, [_P, _P, _I64, _I64, _I64, _I64, _INT, _I64, _P, _P, _P],
    ),
    "pdt_spline_workspace_bytes": (_I64, [_I64, _I64, _I64, _I64]),
    "pdt_spline_solve": (_INT, [_P, _P, _P, _I64, _I64, _I64, _I64, _INT, _F, _P, _P, _P]),
    "pdt_polyharmonic_spline": (
        _INT, [_P, _P, _P, _I64, _I64, _I64, _I64, _I64, _INT, _F, _P, _P, _P],
    ),
    "pdt_warp_1d_grid": (_INT, [_P, _P, _P, _I64, _I64, _INT, _P, _P]),
    "pdt_spec_augment_draw": (
        _INT,
        [_P, _I64, _I64, _P, _I64, _I64, _F, _F, _I64, _I64, _F, _I64, _F, _I64, _INT, _P, _P, _P, _P, _P, _P, _P, _P, _P],
    ),
    "pdt_spec_augment_apply": (
        _INT,
        [_P, _I64, _I64, _I64, _I64, _I64, _I64, _P, _P, _P, _P, _I64, _P, _P, _I64, _P, _P],
    ),
    "pdt_spec_augment_apply_warp": (
        _INT,
        [_P, _I64, _I64, _I64, _I64, _I64, _I64, _P, _P, _P, _INT, _P, _P, _I64, _P, _P, _I64, _P, _P, _P],
    ),
    "pdt_dense_image_warp": (_INT, [_P, _P, _I64, _I64, _I64, _I64, _INT, _INT, _INT, _P, _P]),
    "pdt_sparse_image_warp": (
        _INT,
        [_P, _P, _P, _I64, _I64, _I64, _I64, _I64, _INT, _F, _INT, _INT, _INT, _P, _P, _INT, _P, _P],
    ),
    "pdt_spec_augment_apply_backward": (
        _INT,
        [_P, _I64, _I64, _I64, _P, _P, _P, _P, _I64, _P, _P, _I64, _P, _P],
    ),
    "pdt_spec_augment_apply_elem": (
        _INT,
        [_P, _I64, _I64, _I64, _I64, _I64, _I64, _P, _P, _P, _P, _I64, _P, _P, _I64, _P, _P, _INT],
    ),
    "pdt_spec_augment_apply_warp_elem": (
        _INT,
        [_P, _I64, _I64, _I64, _I64, _I64, _I64, _P, _P, _P, _INT, _P, _P, _I64, _P, _P, _I64, _P, _P, _P, _INT],
    ),
    "pdt_spec_augment_apply_backward_elem": (
        _INT,
        [_P, _I64, _I64, _I64, _P, _P, _P, _P, _I64, _P, _P, _I64, _P, _P, _INT, _P, _I64],
    ),
    "pdt_spec_augment_backward_workspace_bytes": (_I64, [_I64, _I64, _I64, _INT, _INT]),
    "pdt_spec_augment_apply_form": (
        # (in_addr, out_addr: uint64_t in the header; user-space addresses are below 2^63, the same 8 bytes)
        _INT, [_I64, _I64, _I64, _I64, _I64, _I64, _I64, _I64, _INT, _INT, _INT, _INT],
    ),
    "pdt_dense_image_warp_backward": (
        _INT,
        [_P, _P, _I64, _I64, _I64, _I64, _INT, _INT, _INT, _P, _P],
    ),
    "pdt_sparse_image_warp_backward": (
        _INT,
        [_P, _P, _P, _I64, _I64, _I64, _I64, _I64, _INT, _F, _INT, _INT, _INT, _P, _P, _P],
    ),
    # float64 images: the same argument lists, double pixels
    "pdt_dense_image_warp_f64": (_INT, [_P, _P, _I64, _I64, _I64, _I64, _INT, _INT, _INT, _P, _P]),
    "pdt_dense_image_warp_backward_f64": (_INT, [_P, _P, _I64, _I64, _I64, _I64, _INT, _INT, _INT, _P, _P]),
    "pdt_sparse_image_warp_f64": (
        _INT,
        [_P, _P, _P, _I64, _I64, _I64, _I64, _I64, _INT, _F, _INT, _INT, _INT, _P, _P, _INT, _P, _P],
    ),
    "pdt_sparse_image_warp_backward_f64": (
        _INT,
        [_P, _P, _P, _I64, _I64, _I64, _I64, _I64, _INT, _F, _INT, _INT, _INT, _P, _P, _P],
    ),
    # gradients of the warps with respect to flow / spline values, and the spline evaluation's adjoint
    "pdt_dense_image_warp_flow_backward": (_INT, [_P, _P, _P, _I64, _I64, _I64, _I64, _INT, _INT, _INT, _P, _P]),
    "pdt_dense_image_warp_flow_backward_f64": (_INT, [_P, _P, _P, _I64, _I64, _I64, _I64, _INT, _INT, _INT, _P, _P]),
    "pdt_sparse_image_warp_position_backward": (
        _INT,
        [_P, _P, _P, _P, _I64, _I64, _I64, _I64, _I64, _INT, _INT, _INT, _INT, _P, _INT, _P, _P, _P],
    ),
    "pdt_sparse_image_warp_position_backward_f64": (
        _INT,
        [_P, _P, _P, _P, _I64, _I64, _I64, _I64, _I64, _INT, _INT, _INT, _INT, _P, _INT, _P, _P, _P],
    ),
    "pdt_spline_eval_adjoint_plan": (_INT, [_I64, _I64, _I64, _I64, _I64, _P]),
    "pdt_spline_eval_adjoint": (
        _INT, [_P, _P, _P, _P, _I64, _I64, _I64, _I64, _I64, _I64, _I64, _INT, _P, _P, _P, _P, _P],
    ),
    "pdt_lookup_lm_log_probs": (
        _INT,
        [_P, _I64, _I64, _I64, _I64, _P, _I64, _I64, _P, _P, _P, _P, _P, _P, _P, _I64, _I64, _I64, _I64, _P, _P, _P],
    ),
    "pdt_fusion_ext": (_INT, [_P, _I64, _I64, _I64, _P, _I64, _I64, _P, _I64, _F, _INT, _P, _P]),
    "pdt_pad_variable": (_INT, [_P, _I64, _I64, _I64, _I64, _P, _P, _INT, _P, _I64, _P, _P]),
    "pdt_pad_variable_backward": (_INT, [_P, _INT, _I64, _I64, _I64, _P, _P, _INT, _I64, _P, _P]),
    "pdt_feat_deltas": (
        _INT, [_P, _INT, _I64, _I64, _I64, _I64, _I64, _I64, _I64, _I64, _I64, _I64, _P, _I64, _I64, _INT, _P, _INT, _P, _P],
    ),
    "pdt_feat_deltas_backward": (
        _INT, [_P, _INT, _I64, _I64, _I64, _I64, _I64, _P, _I64, _I64, _INT, _INT, _P, _P],
    ),
    "pdt_mvn_stats_workspace_bytes": (_I64, [_I64, _I64, _I64]),
    "pdt_mvn_stats": (_INT, [_P, _P, _P, _INT, _I64, _I64, _I64, _INT, _P, _P, _P, _P, _I64, _P]),
    "pdt_mvn_apply": (_INT, [_P, _INT, _I64, _I64, _I64, _P, _P, _P, _P]),
    "pdt_mvn_backward": (_INT, [_P, _P, _INT, _I64, _I64, _I64, _P, _P, _P, _P]),
    "pdt_attn_workspace_bytes": (_I64, [_P, _INT, _INT]),
    "pdt_attn_dot": (_INT, [_P, _INT, _P, _P, _P, _P, _P, _P, _P, _P, _I64, _P]),
    "pdt_attn_dot_backward": (
        _INT, [_P, _INT, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I64, _P],
    ),
    "pdt_attn_pool": (_INT, [_P, _INT, _P, _P, _P, _P, _P, _P, _I64, _P]),
    "pdt_attn_pool_backward": (_INT, [_P, _INT, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I64, _P]),
    "pdt_attn_workspace_bytes_elem": (_I64, [_P, _INT, _INT]),
    "pdt_attn_dot_elem": (_INT, [_P, _INT, _P, _P, _P, _P, _P, _P, _P, _P, _I64, _P]),
    "pdt_attn_dot_backward_elem": (
        _INT, [_P, _INT, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I64, _P],
    ),
    "pdt_attn_pool_elem": (_INT, [_P, _INT, _P, _P, _P, _P, _P, _P, _I64, _P]),
    "pdt_attn_pool_backward_elem": (_INT, [_P, _INT, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I64, _P]),
    "pdt_concat_score_workspace_bytes": (_I64, [_P, _INT, _INT]),
    "pdt_concat_score_plan": (_INT, [_P, _INT, _P]),
    "pdt_concat_score": (_INT, [_P, _INT, _P, _P, _P, _P, _P]),
    "pdt_concat_score_backward": (_INT, [_P, _INT, _P, _P, _P, _P, _P, _P, _P, _P, _I64, _P]),
    "pdt_compact_mask": (_INT, [_P, _I64, _I64, _I64, _I64, _P, _P, _I64, _I64, _P, _P]),
    "pdt_gather_steps": (_INT, [_P, _I64, _I64, _I64, _I64, _I64, _I64, _P, _I64, _I64, _I64, _INT, _P, _P, _P]),
    "pdt_chunk_by_slices": (_INT, [_P, _I64, _I64, _I64, _I64, _I64, _I64, _P, _P, _INT, _P, _I64, _P, _P]),
    "pdt_chunk_stats": (_INT, [_P, _P, _I64, _I64, _P, _P, _P]),
    "pdt_chunk_by_slices_backward": (_INT, [_P, _INT, _I64, _I64, _I64, _P, _P, _INT, _I64, _P, _P]),
    "pdt_chunk_tokens": (_INT, [_P, _I64, _I64, _P, _P, _INT, _INT, _P, _P, _P]),
    "pdt_slice_fixed": (_INT, [_I64, _I64, _P, _I64, _I64, _I64, _I64, _P, _INT, _P, _P, _P, _P]),
    "pdt_slice_ref": (_INT, [_P, _I64, _I64, _P, _P, _I64, _I64, _INT, _P, _INT, _P, _P, _P, _P]),
    "pdt_slice_ali_segments": (_INT, [_P, _I64, _I64, _P, _P, _P, _P]),
    "pdt_slice_ali_emit": (_INT, [_P, _I64, _I64, _P, _P, _P, _P, _I64, _I64, _INT, _P, _P, _P]),
    "pdt_time_distributed_return_workspace_bytes": (_I64, [_I64, _I64, _INT, _I64, _I64]),
    "pdt_time_distributed_return": (
        _INT, [_P, _INT, _I64, _I64, _I64, _I64, _P, _INT, _P, _I64, _I64, _P, _I64, _P],
    ),
    "pdt_enumerate_vocab_sequences": (_INT, [_I64, _I64, _INT, _P, _P]),
    "pdt_binomial_coefficient": (_INT, [_P, _P, _I64, _P, _P, _P, _P]),
    "pdt_enumerate_cardinality": (_INT, [_P, _P, _I64, _I64, _I64, _I64, _I64, _P, _INT, _P, _P]),
    "pdt_srswor": (_INT, [_P, _P, _P, _I64, _I64, _P, _P]),
    "pdt_relaxed_group_width": (_INT, [_I64]),
    "pdt_relaxed_rows_per_block": (_INT, [_I64]),
    "pdt_relaxed_gumbel": (_INT, [_INT, _INT, _P, _I64, _I64, _I64, _P, _P, _I64, _I64, _P, _P]),
    "pdt_relaxed_bernoulli": (_INT, [_INT, _INT, _P, _I64, _I64, _I64, _P, _P, _I64, _I64, _P, _P]),
    "pdt_relaxed_backward_parts": (_INT, [_I64, _I64, _I64]),
    "pdt_relaxed_backward_workspace_bytes": (_I64, [_INT, _I64, _I64, _I64]),
    "pdt_relaxed_gumbel_backward": (
        _INT, [_INT, _INT, _P, _P, _I64, _I64, _I64, _P, _P, _I64, _I64, _P, _P, _P, _P],
    ),
    "pdt_relaxed_bernoulli_backward": (
        _INT, [_INT, _INT, _P, _P, _I64, _I64, _I64, _P, _P, _I64, _I64, _P, _P, _P, _P],
    ),
    "pdt_mc_reduce_plan": (_INT, [_I64, _I64, _I64, _I64]),
    "pdt_mc_reduce": (_INT, [_INT, _INT, _INT, _INT, _I64, _I64, _P, _P, _P, _P, _P]),
    "pdt_mc_reduce_backward": (_INT, [_INT, _INT, _INT, _INT, _I64, _I64, _P, _P, _P, _P, _P, _P]),
    "pdt_imh_chain": (_INT, [_INT, _P, _I64, _I64, _P, _I64, _P, _I64, _I64, _I64, _I64, _P, _P, _P, _P]),
    "pdt_ctc_prefix_search_workspace_bytes": (_I64, [_I64, _I64, _I64, _I64]),
    "pdt_ctc_prefix_search_plan": (_INT, [_I64, _I64, _P]),
    "pdt_ctc_prefix_search": (
        _INT,
        [_P, _I64, _I64, _I64, _I64, _I64, _I64, _P, _I64, _I64, _P, _P, _P, _P, _P],
    ),
    "pdt_ctc_prefix_search_wide_workspace_bytes": (_I64, [_I64, _I64, _I64, _I64]),
    "pdt_ctc_prefix_search_wide": (
        _INT,
        [_P, _I64, _I64, _I64, _I64, _I64, _I64, _P, _I64, _I64, _P, _P, _P, _P, _P],
    ),
    # logits of float32 / float16 / bfloat16 read as they are: the siblings' arguments + the element code
    "pdt_ctc_prefix_search_elem": (
        _INT,
        [_P, _I64, _I64, _I64, _I64, _I64, _I64, _P, _I64, _I64, _P, _P, _P, _P, _P, _INT],
    ),
    "pdt_ctc_prefix_search_wide_elem": (
        _INT,
        [_P, _I64, _I64, _I64, _I64, _I64, _I64, _P, _I64, _I64, _P, _P, _P, _P, _P, _INT],
    ),
    "pdt_ctc_prefix_search_wide_plan": (_INT, [_I64, _I64, _P]),
    "pdt_ctc_greedy_search_elem": (
        _INT, [_P, _I64, _I64, _I64, _I64, _I64, _I64, _P, _I64, _INT, _P, _P, _I64, _I64, _P, _P, _INT],
    ),
    "pdt_sequence_log_probs_forward_elem": (_INT, [_P, _P, _I64, _I64, _I64, _I64, _INT, _I64, _P, _P, _INT]),
    "pdt_sequence_log_probs_backward_elem": (
        _INT, [_P, _P, _I64, _I64, _I64, _I64, _INT, _I64, _P, _P, _P, _INT],
    ),
}

_lib = None


def lib():
    """Load (once) and return the native library; raises if it is not built or was built for
    another ABI version (a stale library must not be called through a changed table)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "pydrobert_amd: native library {} not found. Build it with "
                "`python -c 'import __graft_entry__ as g; g.build()'` or "
                "`make -C pydrobert-pytorch_amd/csrc`; there is no fallback "
                "implementation.".format(LIB_PATH)
            )
        L = ctypes.CDLL(LIB_PATH)
        L.pdt_amd_abi_version.restype = _INT
        L.pdt_amd_abi_version.argtypes = []
        version = L.pdt_amd_abi_version()
        if version != ABI_VERSION:
            raise ImportError(
                "pydrobert_amd: native library {} has ABI version {}, this package expects {}. "
                "Rebuild it (`make -C pydrobert-pytorch_amd/csrc`).".format(LIB_PATH, version, ABI_VERSION)
            )
        for name, (res, args) in SIGNATURES.items():
            try:
                fn = getattr(L, name)
            except AttributeError:  # (a library built before this entry point was added)
                raise ImportError(
                    "pydrobert_amd: native library {} lacks {}. Rebuild it "
                    "(`make -C pydrobert-pytorch_amd/csrc`).".format(LIB_PATH, name)
                ) from None
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(rc, what):
    """Map a C-ABI status to the reference's exception type (RuntimeError)."""
    if rc == PDT_OK:
        return
    if rc == PDT_E_ARG:
        raise RuntimeError("{}: invalid argument".format(what))
    if rc == PDT_E_TOO_LONG:
        raise RuntimeError("{}: sequence too long for the MI355X kernel".format(what))
    if rc == PDT_E_UNSUPPORTED:
        raise RuntimeError("{}: no kernel for this layout".format(what))
    raise RuntimeError("{}: HIP error {}".format(what, rc))


def require_hip(*tensors):
    """All tensors must sit on one ROCm device; returns that device."""
    dev = None
    for t in tensors:
        if t is None:
            continue
        if t.device.type != "cuda":
            raise RuntimeError(
                "pydrobert_amd operators run only on ROCm (HIP) device tensors; got a "
                "tensor on '{}'. There is no CPU implementation in this package.".format(t.device)
            )
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise RuntimeError("tensors are on different devices: {} and {}".format(dev, t.device))
    return dev


class HostReport:
    """Four int32 in pinned host memory that a kernel reports a data-dependent verdict to (the reference
    reaches one with a reduction, a copy and a synchronisation in FRONT of the work): ``ptr`` for the kernel,
    ``words`` for the host.  ``armed`` is the device of the launch the words were zeroed for until the host
    reads them: a launch left in flight by an exception between it and its wait may still store to them, so
    arming them again first synchronises that device."""

    def __init__(self):
        self._t = torch.zeros(4, dtype=torch.int32, pin_memory=True)
        self.words = self._t.numpy()  # (a view: reads and writes without torch's indexing machinery)
        self.ptr = self._t.data_ptr()
        self.armed = None

    def disarm(self) -> None:
        """Nothing that was launched stores to the words (an error code, an empty shape, a fallback)."""
        self.armed = None

    def read(self, i: int = 0) -> int:
        """Word ``i``, once the caller has synchronised the stream."""
        self.armed = None
        return int(self.words[i])

    def wait(self, spin_seconds: float = 5e-4) -> int:
        """Word 0, which the kernel RELEASES at system scope (non-zero once written): polled for half a
        millisecond -- pinned host memory is coherent by default, and the interrupt behind hipStreamSynchronize
        costs ~15 us -- then the stream is synchronised (a non-coherent host allocation, a long queue).  The
        words stay armed until then: an exception inside the wait leaves the next arming to synchronise."""
        word = self.words
        t_end = time.perf_counter() + spin_seconds
        while word[0] == 0:
            if time.perf_counter() > t_end:
                stream_synchronize(self.armed)
                break
        self.armed = None  # (the kernel's last store has landed, or its stream has drained)
        return int(word[0])


_HOST_REPORTS = threading.local()


def host_report(device) -> HostReport:
    """This host thread's report words, zeroed and armed for a launch on ``device``."""
    report = getattr(_HOST_REPORTS, "report", None)
    if report is None:
        report = _HOST_REPORTS.report = HostReport()
    elif report.armed is not None:  # (a launch whose report was never read may still store to the words)
        torch.cuda.synchronize(report.armed)
    report.words[:] = 0
    report.armed = device
    return report


def stream_ptr(device):
    try:  # (the raw handle, without a Stream object around it)
        return torch._C._cuda_getCurrentRawStream(device.index)
    except (AttributeError, TypeError):
        return torch.cuda.current_stream(device).cuda_stream


class _NoGuard:
    def __enter__(self):
        return None

    def __exit__(self, *exc):
        return False


_NO_GUARD = _NoGuard()


def stream_synchronize(device):
    """hipStreamSynchronize of the current stream of ``device``."""
    torch.cuda.current_stream(device).synchronize()


def on_device(device):
    """``with on_device(d):`` -- torch.cuda.device(d), or nothing when ``d`` is the current device already
    (the guard's own bookkeeping is several microseconds of a step function's call)."""
    if device.index is None or device.index == torch.cuda.current_device():
        return _NO_GUARD
    return torch.cuda.device(device)


def plain_call(*tensors):
    """True when a call has nothing for the dispatcher to do: no tracing (torch.compile / make_fx / fake
    tensors), no function transform, no dispatch or function mode, and no input autograd would follow.
    The Python wrappers then call the implementation behind their ``custom_op`` directly -- the dispatch of
    a Python custom op costs ~16 us, as much as a step function's kernel.  Same code either way."""
    if torch.compiler.is_compiling():
        return False
    try:
        if (torch._C._len_torch_dispatch_stack() or torch._C._len_torch_function_stack()
                or torch._C._functorch.peek_interpreter_stack() is not None):
            return False
    except AttributeError:  # (another torch: leave it to the dispatcher)
        return False
    grad = torch.is_grad_enabled()
    for t in tensors:
        if t is not None and (type(t) is not torch.Tensor or (grad and t.requires_grad)):
            return False
    return True


def ptr(t):
    return 0 if t is None else t.data_ptr()
