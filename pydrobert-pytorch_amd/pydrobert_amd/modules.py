"""Module namespace -- mirrors ``pydrobert.torch.modules`` (modules.py:28-124) for the
operators on the MI355X hot path."""

from ._attn import (
    ConcatSoftAttention,
    DotProductSoftAttention,
    GeneralizedDotProductSoftAttention,
    GlobalSoftAttention,
    MultiHeadedAttention,
)
from ._decoding import BeamSearch, CTCPrefixSearch
from ._img import (
    DenseImageWarp,
    PolyharmonicSpline,
    RandomShift,
    SparseImageWarp,
    SpecAugment,
    Warp1DGrid,
)
from ._feats import ChunkTokenSequencesBySlices, FeatureDeltas, MeanVarianceNormalization, SliceSpectData
from ._pad import ChunkBySlices, PadMaskedSequence, PadVariable
from ._seqops import CTCGreedySearch, SequenceLogProbabilities
from ._walk import RandomWalk
from ._rl import TimeDistributedReturn
from ._relaxed import GumbelOneHotCategoricalRebarControlVariate, LogisticBernoulliRebarControlVariate
from ._lm import (
    ExtractableSequentialLanguageModel,
    ExtractableShallowFusionLanguageModel,
    LookupLanguageModel,
    MixableSequentialLanguageModel,
    MixableShallowFusionLanguageModel,
    SequentialLanguageModel,
    ShallowFusionLanguageModel,
)
from ._string import (
    HardOptimalCompletionDistillationLoss,
    MinimumErrorRateLoss,
    EditDistance,
    ErrorRate,
    FillAfterEndOfSequence,
    OptimalCompletion,
    PrefixEditDistances,
    PrefixErrorRates,
)

__all__ = [
    "ChunkBySlices",
    "ChunkTokenSequencesBySlices",
    "PadMaskedSequence",
    "SliceSpectData",
    "ConcatSoftAttention",
    "DotProductSoftAttention",
    "GeneralizedDotProductSoftAttention",
    "GlobalSoftAttention",
    "MultiHeadedAttention",
    "FeatureDeltas",
    "MeanVarianceNormalization",
    "PadVariable",
    "RandomShift",
    "DenseImageWarp",
    "PolyharmonicSpline",
    "SparseImageWarp",
    "SpecAugment",
    "Warp1DGrid",
    "CTCGreedySearch",
    "RandomWalk",
    "SequenceLogProbabilities",
    "TimeDistributedReturn",
    "GumbelOneHotCategoricalRebarControlVariate",
    "LogisticBernoulliRebarControlVariate",
    "HardOptimalCompletionDistillationLoss",
    "MinimumErrorRateLoss",
    "BeamSearch",
    "CTCPrefixSearch",
    "ExtractableSequentialLanguageModel",
    "ExtractableShallowFusionLanguageModel",
    "LookupLanguageModel",
    "MixableShallowFusionLanguageModel",
    "ShallowFusionLanguageModel",
    "MixableSequentialLanguageModel",
    "SequentialLanguageModel",
    "EditDistance",
    "ErrorRate",
    "FillAfterEndOfSequence",
    "OptimalCompletion",
    "PrefixEditDistances",
    "PrefixErrorRates",
]
