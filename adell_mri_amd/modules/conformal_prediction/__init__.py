from .conformal import AdaptivePredictionSets  # noqa: F401
