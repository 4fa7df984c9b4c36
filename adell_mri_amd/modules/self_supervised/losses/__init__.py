from .functional import byol_loss, simsiam_loss  # noqa: F401
from .ntxent import NTXentLoss  # noqa: F401
from .vicreg import VICRegLocalLoss, VICRegLoss  # noqa: F401
from .dino import DinoLoss  # noqa: F401
