from .losses import complete_iou_loss  # noqa: F401
from .map import mAP, average_precision  # noqa: F401
from .nets import CoarseDetector3d, YOLONet3d  # noqa: F401
from .pl import CoarseDetector3dPL, YOLONet3dPL, real_boxes_from_centres_sizes  # noqa: F401
from .utils import (bb_volume, calculate_iou, check_overlap, maxpool_default, nms_nd,  # noqa: F401
                    pyramid_default, resnet_default)
