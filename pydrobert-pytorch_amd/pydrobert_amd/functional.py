"""Functional namespace -- mirrors ``pydrobert.torch.functional`` (functional.py:17-95)
for the operators on the MI355X hot path."""

from ._combinatorics import (
    binomial_coefficient,
    enumerate_binary_sequences,
    enumerate_binary_sequences_with_cardinality,
    enumerate_vocab_sequences,
    simple_random_sampling_without_replacement,
)
from ._decoding import ctc_prefix_search
from ._seqops import ctc_greedy_search, sequence_log_probs
from ._step import beam_search_advance, ctc_prefix_search_advance
from ._walk import random_walk_advance
from ._img import (
    dense_image_warp,
    polyharmonic_spline,
    random_shift,
    sparse_image_warp,
    spec_augment,
    spec_augment_apply_parameters,
    spec_augment_draw_parameters,
    warp_1d_grid,
)
from ._feats import chunk_token_sequences_by_slices, feat_deltas, mean_var_norm, slice_spect_data
from ._pad import chunk_by_slices, pad_masked_sequence, pad_variable
from ._rl import time_distributed_return
from ._string import (
    hard_optimal_completion_distillation_loss,
    minimum_error_rate_loss,
    edit_distance,
    error_rate,
    fill_after_eos,
    optimal_completion,
    prefix_edit_distances,
    prefix_error_rates,
)

__all__ = [
    "binomial_coefficient",
    "enumerate_binary_sequences",
    "enumerate_binary_sequences_with_cardinality",
    "enumerate_vocab_sequences",
    "simple_random_sampling_without_replacement",
    "time_distributed_return",
    "chunk_by_slices",
    "chunk_token_sequences_by_slices",
    "pad_masked_sequence",
    "slice_spect_data",
    "feat_deltas",
    "mean_var_norm",
    "pad_variable",
    "random_shift",
    "ctc_greedy_search",
    "random_walk_advance",
    "sequence_log_probs",
    "hard_optimal_completion_distillation_loss",
    "minimum_error_rate_loss",
    "beam_search_advance",
    "ctc_prefix_search",
    "ctc_prefix_search_advance",
    "dense_image_warp",
    "polyharmonic_spline",
    "sparse_image_warp",
    "spec_augment",
    "spec_augment_apply_parameters",
    "spec_augment_draw_parameters",
    "warp_1d_grid",
    "edit_distance",
    "error_rate",
    "fill_after_eos",
    "optimal_completion",
    "prefix_edit_distances",
    "prefix_error_rates",
]
