from .callbacks import MultiPhaseTraining
from .optim import EarlyStopper, create_param_groups
from .regularization import ElasticWeightConsolidation

__all__ = [
    "MultiPhaseTraining",
    "EarlyStopper",
    "create_param_groups",
    "ElasticWeightConsolidation",
]
