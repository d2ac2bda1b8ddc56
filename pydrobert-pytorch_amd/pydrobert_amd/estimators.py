"""Estimator namespace -- mirrors ``pydrobert.torch.estimators`` (estimators.py:29-50): estimators of expectations
whose reductions over the sample axis, and whose Metropolis-Hastings chain, run on this package's MI355X kernels.
The reference's deprecated functional interface (``to_z``, ``reinforce``, ``relax``, ``REBARControlVariate``) is not
carried over.  Like the reference's, estimators can be neither scripted nor traced."""

from ._estimators import (
    DirectEstimator,
    EnumerateEstimator,
    Estimator,
    FunctionOnSample,
    ImportanceSamplingEstimator,
    IndependentMetropolisHastingsEstimator,
    MonteCarloEstimator,
    RelaxEstimator,
    ReparameterizationEstimator,
    StraightThroughEstimator,
)

__all__ = [
    "Estimator",
    "EnumerateEstimator",
    "FunctionOnSample",
    "ImportanceSamplingEstimator",
    "IndependentMetropolisHastingsEstimator",
    "MonteCarloEstimator",
    "DirectEstimator",
    "RelaxEstimator",
    "ReparameterizationEstimator",
    "StraightThroughEstimator",
]
