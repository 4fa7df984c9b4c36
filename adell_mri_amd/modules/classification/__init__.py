from .classification import (CatNet, GlobalPooling, OrdNet, ViTClassifier,  # noqa: F401
                             label_to_ordinal, ordinal_prediction_to_class)
from .ensemble import AveragingEnsemble, EnsembleNet, GenericEnsemble  # noqa: F401
from .losses import (BCEWithLogitsLoss, CrossEntropyLoss, OrdinalSigmoidalLoss,  # noqa: F401
                     configure_loss_fn, ordinal_sigmoidal_loss, relative_order_consistency)
from .multiple_instance_learning import (MILAttention, MultipleInstanceClassifier,  # noqa: F401
                                         TransformableTransformer)
from .pl import (AveragingEnsemblePL, GenericEnsemblePL,  # noqa: F401,E402
                 MultipleInstanceClassifierPL, TransformableTransformerPL)
