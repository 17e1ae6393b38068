"""image-segmentation-project_amd — MI355X-native U-Net segmentation training path.

Drop-in for the hot path of SwagMag1213/image-segmentation-project
(``advanced_models.UNetWithBackbone`` resnet34/no-attention, ``losses``
bce/dice/combo, ``utils.calculate_metrics``, ``train.train_epoch/evaluate``),
plus softmax losses and argmax metrics for mutually exclusive classes
(``CrossEntropyLoss``, ``SoftmaxDiceLoss``, ``SoftmaxComboLoss``, ``confusion_matrix``)
and tiled whole-frame inference on frames of any size (``predict``) with
instance labelling of the predicted masks (``label_instances``), exact distance
maps and growth of the instances (``distance_transform``, ``grow_instances``),
growth along allowed pixels, watershed and splitting of touching cells
(``geodesic_grow``, ``watershed``, ``split_instances``) and
their scores against a ground truth (``match_instances``, ``instance_metrics``),
per-instance shape, contact and intensity tables of any label map
(``measure_instances``, ``region_properties``) with filtering and renumbering on
the device (``select_instances``),
linking of the instances of consecutive frames into tracks or 3-D objects
(``link_instances``, ``track_properties``),
and the training targets of that scheme from a ground-truth instance map
(``boundary_targets``, ``border_weight_map``, ``nearest_two_instances``; per-pixel
weights in ``CrossEntropyLoss`` / ``SoftmaxComboLoss``),
computed by hand-written gfx950 HIP kernels in ``libunet_hip.so`` (C ABI:
``include/unet_hip.h``).  The directory name carries hyphens, so import it with
``importlib.import_module("image-segmentation-project_amd")``.
"""
from .advanced_models import UNetWithBackbone  # noqa: F401
from .losses import (BCELoss, ComboLoss, CrossEntropyLoss, DiceLoss, SoftmaxComboLoss,  # noqa: F401
                     SoftmaxDiceLoss, get_loss_function)
from .utils import (EarlyStopping, calculate_metrics, calculate_metrics_from_logits,  # noqa: F401
                    calculate_metrics_per_class, calculate_metrics_per_class_from_logits,
                    calculate_multiclass_metrics, confusion_matrix, get_device, metrics_from_confusion)
from .train import (evaluate, quick_train, train_epoch, train_model, TensorLoader,  # noqa: F401
                    GraphedTrainStep)
from .synthetic import random_batch, synthetic_cells  # noqa: F401
from . import dataset  # noqa: F401
from .dataset import CellAugmenter, CellSegmentationDataset, prepare_data, preprocess  # noqa: F401
from .predict import predict, tile_origins  # noqa: F401
from .instances import instance_properties, label_instances  # noqa: F401
from .distance import distance_transform, grow_instances  # noqa: F401
from .geodesic import geodesic_grow, split_instances, watershed  # noqa: F401
from .weights import border_weight_map, boundary_targets, nearest_two_instances  # noqa: F401
from .match import InstanceMatch, instance_metrics, match_instances  # noqa: F401
from .measure import (MEASURE_COLUMNS, InstanceMeasure, measure_instances, region_properties,  # noqa: F401
                      select_instances)
from .track import TRACK_COLUMNS, TRACK_STATUS, InstanceLinks, link_instances, track_properties  # noqa: F401
from . import ddp  # noqa: F401
from . import optim  # noqa: F401
from .optim import Adam  # noqa: F401
from .ddp import enable_data_parallel  # noqa: F401
from ._lib import LIB_PATH  # noqa: F401

__version__ = "0.1.0"
