"""Distribution namespace -- mirrors ``pydrobert.torch.distributions`` (distributions.py:22-45): the relaxed
distributions and their interfaces, the sequence distribution, and the SRSWOR distribution, on this package's
MI355X kernels.  Like the reference's, distributions can be neither scripted nor traced."""

from ._combinatorics import BinaryCardinalityConstraint, SimpleRandomSamplingWithoutReplacement
from ._relaxed import (
    ConditionalStraightThrough,
    Density,
    GumbelOneHotCategorical,
    LogisticBernoulli,
    StraightThrough,
)
from ._walk import SequentialLanguageModelDistribution, TokenSequenceConstraint

__all__ = [
    "BinaryCardinalityConstraint",
    "ConditionalStraightThrough",
    "Density",
    "GumbelOneHotCategorical",
    "LogisticBernoulli",
    "SequentialLanguageModelDistribution",
    "SimpleRandomSamplingWithoutReplacement",
    "StraightThrough",
    "TokenSequenceConstraint",
]
