from .batch_ensemble import BatchEnsemble, BatchEnsembleWrapper  # noqa: F401
