"""Network factories of the hot path: ``get_classification_network``
(adell_mri/utils/network_factories.py:136-305), ``get_deconfounded_classification_network``
(:309-402), ``get_segmentation_network`` (:493-701) and
``get_ssl_network`` (:705-1028) on this
package's HIP-backed modules. Same argument lists, same keyword plumbing into the ``*PL``
constructors, same ``ValueError`` for an unknown ``net_type``. ``ssl_method="dino"`` builds
``DINOPL``, ``ssl_method="ibot"`` ``iBOTPL`` and ``ssl_method="ijepa"`` ``IJEPAPL`` on a ViT encoder
(:799-956; ``TypeError`` for any other ``net_type``) and ``ssl_method="mae"``
``ViTMaskedAutoEncoderPL`` (:851-867). Members outside the built path (the MONAI wrappers, Barlow
Twins)
raise ``NotImplementedError`` -- there is no eager-torch fallback.
"""
from typing import Any, Callable

import numpy as np
import torch
import torch.nn.functional as F

from ..modules.classification.pl import ClassNetPL, OrdNetPL, ViTClassifierPL
from ..modules.layers.adn_fn import get_adn_fn
from ..modules.object_detection.losses import complete_iou_loss
from ..modules.object_detection.pl import YOLONet3dPL
from ..modules.segmentation.pl import (BrUNetPL, SWINUNetPL, UNETRPL, UNetPL,
                                       UNetPlusPlusPL)
from ..modules.self_supervised.pl import (DINOPL, IJEPAPL, SelfSLConvNeXtPL, SelfSLResNetPL,
                                          SelfSLUNetPL, ViTMaskedAutoEncoderPL, iBOTPL)

OPTIMIZER_EPS_DEFAULT = 1e-8
_MAE_STACK_KEYS = ("number_of_blocks", "hidden_dim", "n_heads", "mlp_structure")
ALLOWED_NET_TYPES = {
    "classification": ["unet", "vit", "factorized_vit", "cat", "ord", "vgg"],
    "segmentation": ["unet", "brunet", "unetpp", "unetr", "monai_unetr", "swin", "monai_swin"],
}


def _first_given(*sizes):
    for size in sizes:
        if size is not None:
            return size
    return None


def get_classification_network(
        net_type: str, network_config: dict[str, Any], dropout_param: float, seed: int,
        n_classes: int, keys: list[str], clinical_feature_keys: list[str],
        train_loader_call: Callable, max_epochs: int, warmup_steps: int, start_decay: int,
        crop_size: int, clinical_feature_means: torch.Tensor = None,
        clinical_feature_stds: torch.Tensor = None, label_smoothing: float | None = None,
        mixup_alpha: float | None = None, partial_mixup: float | None = None,
        optimizer_eps: float = OPTIMIZER_EPS_DEFAULT):
    """network_factories.py:136-305: ``"cat"`` builds ``ClassNetPL``, ``"ord"`` ``OrdNetPL`` and
    ``"vit"`` ``ViTClassifierPL``, with the reference's keyword plumbing (``act_fn`` / ``norm_fn``
    popped from ``network_config`` into the 3-D ``adn_fn``, the ``BatchPreprocessing`` of the three
    mixup arguments as ``training_batch_preproc``). An unknown ``net_type`` is the reference's
    ``ValueError``; ``"unet"``, ``"factorized_vit"`` and ``"vgg"``, and a non-empty
    ``clinical_feature_keys`` (the hybrid / tabular classifier), raise ``NotImplementedError``."""
    from .batch_preprocessing import BatchPreprocessing

    if net_type not in ALLOWED_NET_TYPES["classification"]:
        raise ValueError(f"net_type '{net_type}' not valid, has to be one of "
                         f"{ALLOWED_NET_TYPES['classification']}")
    if net_type in ("unet", "factorized_vit", "vgg"):
        raise NotImplementedError(f"net_type '{net_type}' is not built for classification "
                                  "(built: 'cat', 'ord', 'vit')")
    if len(clinical_feature_keys) > 0:
        raise NotImplementedError("clinical_feature_keys: the hybrid (image + tabular) classifier is "
                                  "not built")
    network_config = dict(network_config)
    act_fn = network_config.pop("act_fn", "swish")
    norm_fn = network_config.pop("norm_fn", "batch")
    adn_fn = get_adn_fn(3, norm_fn, act_fn=act_fn, dropout_param=dropout_param)
    batch_preprocessing = BatchPreprocessing(label_smoothing, mixup_alpha, partial_mixup, seed)
    boilerplate_args = {
        "in_channels": len(keys), "n_classes": n_classes,
        "training_dataloader_call": train_loader_call, "image_key": "image", "label_key": "label",
        "n_epochs": max_epochs, "warmup_steps": warmup_steps,
        "training_batch_preproc": batch_preprocessing, "start_decay": start_decay,
        "optimizer_eps": optimizer_eps,
    }
    if net_type == "vit":
        network_config["image_size"] = tuple(int(x) for x in crop_size)
        return ViTClassifierPL(
            adn_fn=get_adn_fn(1, "identity", act_fn="gelu", dropout_param=dropout_param),
            **boilerplate_args, **network_config)
    if net_type == "ord":
        for k in ["net_type", "in_channels", "n_classes", "adn_fn"]:
            network_config.pop(k, None)
        return OrdNetPL(adn_fn=adn_fn, **boilerplate_args, **network_config)
    for k in ["in_channels", "n_classes", "adn_fn"]:
        network_config.pop(k, None)
    return ClassNetPL(net_type=net_type, adn_fn=adn_fn, **boilerplate_args, **network_config)


def get_deconfounded_classification_network(
        network_config: dict[str, Any], dropout_param: float, seed: int, n_classes: int,
        keys: list[str], cat_confounder_key: list[str], cont_confounder_key: list[str],
        cat_vars: list[list[str]], cont_vars: int, train_loader_call: Callable, max_epochs: int,
        warmup_steps: int, start_decay: int, n_features_deconfounder: int = 64,
        exclude_surrogate_variables: bool = False, label_smoothing: float | None = None,
        mixup_alpha: float | None = None, partial_mixup: float | None = None,
        optimizer_eps: float = OPTIMIZER_EPS_DEFAULT):
    """network_factories.py:309-402: ``DeconfoundedNetPL`` with the reference's keyword plumbing
    (``act_fn``, default "relu", and ``norm_fn`` popped from a copy of ``network_config`` into the
    3-D ``adn_fn``, the ``BatchPreprocessing`` of the three mixup arguments, a
    ``CategoricalConversion`` of ``cat_vars`` as the embedder and its level counts as
    ``n_cat_deconfounder``). ``network_config`` names the feature extractor
    (``feature_extraction_module="cat"``); without it the reference's default "vgg" raises
    ``NotImplementedError``."""
    from ..modules.classification.deconfounded_classification import CategoricalConversion
    from ..modules.classification.pl import DeconfoundedNetPL
    from .batch_preprocessing import BatchPreprocessing

    network_config = dict(network_config)
    act_fn = network_config.pop("act_fn", "relu")
    norm_fn = network_config.pop("norm_fn", "batch")
    adn_fn = get_adn_fn(3, norm_fn, act_fn=act_fn, dropout_param=dropout_param)
    batch_preprocessing = BatchPreprocessing(label_smoothing, mixup_alpha, partial_mixup, seed)
    cat_conv = CategoricalConversion(cat_vars) if cat_vars is not None else None
    boilerplate_args = {
        "in_channels": len(keys), "n_classes": n_classes,
        "training_dataloader_call": train_loader_call, "image_key": "image", "label_key": "label",
        "n_epochs": max_epochs, "warmup_steps": warmup_steps,
        "training_batch_preproc": batch_preprocessing, "start_decay": start_decay,
        "optimizer_eps": optimizer_eps,
    }
    n_cat_deconfounder = [len(x) for x in cat_vars] if cat_vars is not None else None
    return DeconfoundedNetPL(
        adn_fn=adn_fn, embedder=cat_conv, n_features_deconfounder=n_features_deconfounder,
        n_cat_deconfounder=n_cat_deconfounder, n_cont_deconfounder=cont_vars,
        cat_confounder_key=cat_confounder_key, cont_confounder_key=cont_confounder_key,
        exclude_surrogate_variables=exclude_surrogate_variables, **boilerplate_args,
        **network_config)


def get_detection_network(
        network_config: dict[str, Any], dropout_param: float, loss_gamma: float, loss_comb: float,
        class_weights: torch.Tensor, train_loader_call: Callable, iou_threshold: float, n_classes: int,
        anchor_array: np.ndarray, n_epochs: int, warmup_steps: int, boxes_key: str, box_class_key: str,
        dev: str, optimizer_eps: float = OPTIMIZER_EPS_DEFAULT):
    """network_factories.py:406-489: ``YOLONet3dPL`` with ``complete_iou_loss`` as the box loss, the
    batch-norm ``adn_fn`` of ``activation_fn`` (default "swish"), ``label_key="bb_map"``, the
    classification loss ``F.binary_cross_entropy`` / ``F.cross_entropy`` by ``n_classes`` and the
    objectness loss ``F.binary_cross_entropy``; ``"classification_loss_fn"`` / ``"object_loss_fn"``
    keys pick from ``loss_factory`` instead, ``batch_size`` defaults to 1, every other key goes to the
    constructor. As in the reference ``dev`` is not handed on (the network is built on "cuda" unless
    ``network_config`` carries ``dev``), and with an ``object_loss_fn`` key and all three of
    ``loss_gamma`` / ``loss_comb`` / ``class_weights`` given it reads ``get_loss_param_dict``, which
    this package does not have: ``NotImplementedError``."""
    from .utils import loss_factory

    act_fn = network_config["activation_fn"] if "activation_fn" in network_config else "swish"
    if "classification_loss_fn" in network_config:
        k = "binary" if n_classes == 2 else "categorical"
        classification_loss_fn = loss_factory[k][network_config["classification_loss_fn"]]
    else:
        classification_loss_fn = F.binary_cross_entropy if n_classes == 2 else F.cross_entropy
    if "object_loss_fn" in network_config:
        object_loss_fn = loss_factory["binary"][network_config["object_loss_fn"]]
    else:
        object_loss_fn = F.binary_cross_entropy
    net_cfg = {k: network_config[k] for k in network_config
               if k not in ["activation_fn", "classification_loss_fn", "object_loss_fn"]}
    if "batch_size" not in net_cfg:
        net_cfg["batch_size"] = 1
    classification_loss_params = {}
    if (loss_gamma is None) or (loss_comb is None) or (class_weights is None):
        object_loss_params = {}
    elif "object_loss_fn" not in network_config:
        # the reference reads an unbound ``object_loss_key`` here: UnboundLocalError
        raise UnboundLocalError("get_detection_network: loss parameters need an 'object_loss_fn' key "
                                "(the reference fails here too)")
    else:
        raise NotImplementedError("get_detection_network: object loss parameters "
                                  "(get_loss_param_dict) are not built")
    adn_fn = get_adn_fn(3, norm_fn="batch", act_fn=act_fn, dropout_param=dropout_param)
    return YOLONet3dPL(
        training_dataloader_call=train_loader_call, image_key="image", label_key="bb_map",
        boxes_key=boxes_key, box_label_key=box_class_key, anchor_sizes=anchor_array, adn_fn=adn_fn,
        iou_threshold=iou_threshold, classification_loss_fn=classification_loss_fn,
        object_loss_fn=object_loss_fn, reg_loss_fn=complete_iou_loss,
        object_loss_params=object_loss_params,
        classification_loss_params=classification_loss_params, n_epochs=n_epochs,
        warmup_steps=warmup_steps, n_classes=n_classes, optimizer_eps=optimizer_eps, **net_cfg)


def get_segmentation_network(
        net_type: str, network_config: dict[str, Any], bottleneck_classification: bool,
        clinical_feature_keys: list[str], all_aux_keys: list[str],
        clinical_feature_params: dict[str, torch.Tensor], clinical_feature_key_net: str,
        aux_key_net: str, max_epochs: int, encoding_operations: list[torch.nn.Module],
        picai_eval: bool, lr_encoder: float, encoder_checkpoint: str,
        res_config_file: str | None, deep_supervision: bool, n_classes: int, keys: list[str],
        optimizer_str: str = "sgd", optimizer_eps: float = OPTIMIZER_EPS_DEFAULT,
        start_decay: float | int = 1.0, warmup_steps: float | int = 0.0,
        train_loader_call: Callable = None, random_crop_size: list[int] = None,
        crop_size: list[int] = None, pad_size: list[int] = None, resize_size: list[int] = None,
        semi_supervised: bool = False, max_steps_optim: int = None, seed: int = 42):
    """``network_config`` is what ``parse_config_unet`` returned; ``encoding_operations`` is the
    list the entrypoint prepares (``[None]`` without an SSL backbone, train.py:672-734)."""
    if net_type not in ALLOWED_NET_TYPES["segmentation"]:
        raise ValueError(f"net_type '{net_type}' not valid, has to be one of "
                         f"{ALLOWED_NET_TYPES['segmentation']}")
    # image size for the transformer members: the first of random crop / crop / pad / resize
    size = _first_given(random_crop_size, crop_size, pad_size, resize_size)
    common = dict(
        training_dataloader_call=train_loader_call, label_key="mask", n_classes=n_classes,
        bottleneck_classification=bottleneck_classification,
        skip_conditioning=len(all_aux_keys), skip_conditioning_key=aux_key_net,
        feature_conditioning=len(clinical_feature_keys),
        feature_conditioning_params=clinical_feature_params,
        feature_conditioning_key=clinical_feature_key_net, n_epochs=max_epochs,
        picai_eval=picai_eval, lr_encoder=lr_encoder, start_decay=start_decay,
        warmup_steps=warmup_steps, optimizer_str=optimizer_str, optimizer_eps=optimizer_eps)

    if net_type == "unet" and semi_supervised is True:   # network_factories.py:602-620
        from ..modules.semi_supervised_segmentation import (LocalContrastiveLoss,
                                                            UNetContrastiveSemiSL)
        from .utils import ExponentialMovingAverage

        ema = ExponentialMovingAverage(decay=0.99, final_decay=1.0, n_steps=max_steps_optim)
        return UNetContrastiveSemiSL(
            encoding_operations=encoding_operations[0], image_key="image",
            semi_sl_image_key_1="semi_sl_image_1", semi_sl_image_key_2="semi_sl_image_2",
            deep_supervision=deep_supervision, ema=ema,
            loss_fn_semi_sl=LocalContrastiveLoss(seed=seed), **common, **network_config)
    if net_type in ("monai_unetr", "monai_swin"):
        raise NotImplementedError(f"{net_type}: the MONAI wrappers are outside the HIP path "
                                  "(SURVEY.md section 2: out of scope)")
    if net_type == "brunet":
        network_config["in_channels"] = network_config["in_channels"] // len(keys)
        net = BrUNetPL(encoders=encoding_operations, image_keys=keys,
                       n_input_branches=len(keys), deep_supervision=deep_supervision,
                       **common, **network_config)
        if encoder_checkpoint is not None and res_config_file is None:
            for encoder, ckpt in zip(net.encoders, encoder_checkpoint):
                encoder.load_state_dict(torch.load(ckpt, weights_only=False)["state_dict"])
        return net
    if net_type == "unetpp":
        return UNetPlusPlusPL(encoding_operations=encoding_operations[0], image_key="image",
                              **common, **network_config)
    if net_type == "unet":
        return UNetPL(encoding_operations=encoding_operations[0], image_key="image",
                      deep_supervision=deep_supervision, **common, **network_config)
    sd = network_config["spatial_dimensions"]
    network_config["image_size"] = size[:sd]
    if net_type == "unetr":
        network_config["patch_size"] = network_config["patch_size"][:sd]
        return UNETRPL(image_key="image", deep_supervision=deep_supervision, **common,
                       **network_config)
    return SWINUNetPL(image_key="image", deep_supervision=deep_supervision, **common,
                      **network_config)


_RESNET_DEFAULTS = dict(
    backbone_args={"spatial_dim": 2, "in_channels": 1,
                   "structure": [(64, 64, 3, 2), (128, 128, 3, 2), (256, 256, 3, 2),
                                 (512, 512, 3, 2)],
                   "maxpool_structure": [2, 2, 2, 2], "adn_fn": torch.nn.Identity,
                   "res_type": "resnet"},
    projection_head_args={"in_channels": 512, "structure": [512, 128],
                          "adn_fn": torch.nn.Identity},
    prediction_head_args={"in_channels": 128, "structure": [512, 128],
                          "adn_fn": torch.nn.Identity})


_DINO_BACKBONE_DEFAULTS = {"image_size": [224, 224], "patch_size": [16, 16], "in_channels": 1,
                           "number_of_blocks": 4, "attention_dim": 96, "embedding_size": 96,
                           "n_heads": 3}


def get_ssl_network(train_loader_call: Callable, max_epochs: int, max_steps_optim: int,
                    warmup_steps: int, ssl_method: str, ema: torch.nn.Module, net_type: str,
                    network_config: dict[str, Any], stop_gradient: bool,
                    optimizer_eps: float = OPTIMIZER_EPS_DEFAULT):
    """``network_config`` is ``parse_config_ssl``'s second return value. As in the reference,
    simclr / byol / vicreg / vicregl always build the ResNet wrapper from the three ``*_args``
    dictionaries (defaults :754-790) -- for vicregl with ``VICRegLocalLoss(**vic_reg_loss_params)``
    on the "representation" feature maps and the boxes of the batch; every other method name with ``net_type="convnext"``
    builds ``SelfSLConvNeXtPL`` from the whole configuration (:998-1026). ``"dino"`` builds
    ``DINOPL`` (ViT backbone + MLP projection head, defaults :875-901) and needs ``ema``.
    ``"ibot"`` builds ``iBOTPL`` (:907-956) in the reference's order: ``TypeError`` unless
    ``net_type == "vit"``, ``feature_map_dimensions`` (image size // patch size) and
    ``n_encoder_features`` (``embedding_size``, else ``attention_dim``) derived from
    ``backbone_args``, the masker's patch sizes [4, 4] ... [8, 8] by default, ``ValueError`` without
    ``ema`` (raised by ``iBOTPL``). One difference on purpose: the reference's built-in 224 x 224
    default backbone is not mirrored for iBOT -- a configuration without ``"backbone_args"`` raises
    ``NotImplementedError``; every real configuration names its backbone.
    ``"ijepa"`` builds ``IJEPAPL`` (:799-849) the same way: ``TypeError`` unless ``net_type ==
    "vit"``, the predictor's ``projection_head_args`` two blocks of ``n_encoder_features`` with 3
    heads by default, patch sizes [4, 4] ... [8, 8], one context and four target blocks,
    ``predictor_dim`` None, ``image_key="image"``, ``ValueError`` without ``ema`` (raised by
    ``IJEPAPL``) -- and, as for iBOT, ``NotImplementedError`` without ``"backbone_args"``.
    ``"mae"`` builds ``ViTMaskedAutoEncoderPL`` (:851-867): ``encoder_args`` and ``decoder_args`` from
    the network configuration, ``image_size``, ``patch_size`` and ``in_channels`` (default 1) read
    from ``encoder_args``, ``input_dim_size = encoder_args.get("embed_dim", 96)``, ``mask_fraction``
    0.75 by default, ``image_key="image"``, ``ema`` removed from the common parameters and no
    ``net_type`` check. One difference on purpose: the reference's 224 x 224 / 16 x 16 default is
    not mirrored and a stack without its size dies there with ``KeyError`` -- here a configuration
    whose ``encoder_args`` or ``decoder_args`` is missing or lacks ``number_of_blocks``,
    ``hidden_dim``, ``n_heads`` or ``mlp_structure``, or whose ``encoder_args`` lacks ``image_size``
    or ``patch_size``, raises ``NotImplementedError`` naming the key. MAE has no collective of its
    own and has run at world size 1 only."""
    common = {"training_dataloader_call": train_loader_call, "n_epochs": max_epochs,
              "n_steps": max_steps_optim, "warmup_steps": warmup_steps, "ema": ema,
              "batch_size": network_config.get("batch_size", 32),
              "optimizer_eps": optimizer_eps}
    for key in ("learning_rate", "weight_decay"):
        if key in network_config:
            common[key] = network_config[key]
    if ssl_method in ("simclr", "byol", "vicreg", "vicregl"):
        config = {k: network_config.get(k, v) for k, v in _RESNET_DEFAULTS.items()}
        if ssl_method == "simclr":
            config["prediction_head_args"] = None
        config.update(ssl_method=ssl_method, stop_gradient=stop_gradient,
                      temperature=network_config.get("temperature", 0.1),
                      vic_reg_loss_params=network_config.get("vic_reg_loss_params", {}))
        return SelfSLResNetPL(**{**common, **config})
    if ssl_method == "dino":
        if net_type != "vit":
            raise TypeError("DINO only supports net_type='vit', got %s" % net_type)
        config = {"aug_image_key_1": "augmented_image_1", "aug_image_key_2": "augmented_image_2",
                  "backbone_args": network_config.get("backbone_args", dict(_DINO_BACKBONE_DEFAULTS)),
                  "projection_head_args": network_config.get("projection_head_args",
                                                             {"structure": [512, 256, 128]}),
                  "out_dim": network_config.get("out_dim", 65536),
                  "temperature": network_config.get("temperature", 0.1),
                  "centers_m": network_config.get("centers_m", 0.9),
                  "teacher_score_method": network_config.get("teacher_score_method", "center"),
                  "stop_gradient": stop_gradient, "optimizer_eps": optimizer_eps}
        return DINOPL(**{**common, **config})
    if ssl_method == "ibot":
        if net_type != "vit":
            raise TypeError("iBOT only supports net_type='vit', got %s" % net_type)
        if "backbone_args" not in network_config:
            raise NotImplementedError(
                "ssl_method 'ibot': the reference's built-in 224 x 224 default backbone is not "
                "mirrored for iBOT; `backbone_args` must be given in the network configuration")
        backbone_args = network_config["backbone_args"]
        config = {"aug_image_key_1": "augmented_image_1", "aug_image_key_2": "augmented_image_2",
                  "backbone_args": backbone_args,
                  "projection_head_args": network_config.get("projection_head_args",
                                                             {"structure": [512, 256, 128]}),
                  "out_dim": network_config.get("out_dim", 65536),
                  "feature_map_dimensions": [s // p for s, p in zip(backbone_args["image_size"],
                                                                    backbone_args["patch_size"])],
                  "n_encoder_features": backbone_args.get("embedding_size",
                                                          backbone_args["attention_dim"]),
                  "min_patch_size": network_config.get("min_patch_size", [4, 4]),
                  "max_patch_size": network_config.get("max_patch_size", [8, 8]),
                  "temperature": network_config.get("temperature", 0.1),
                  "centers_m": network_config.get("centers_m", 0.9),
                  "teacher_score_method": network_config.get("teacher_score_method", "center"),
                  "stop_gradient": stop_gradient, "optimizer_eps": optimizer_eps}
        return iBOTPL(**{**common, **config})
    if ssl_method == "ijepa":
        if net_type != "vit":
            raise TypeError("IJEPA only supports net_type='vit', got %s" % net_type)
        if "backbone_args" not in network_config:
            raise NotImplementedError(
                "ssl_method 'ijepa': the reference's built-in 224 x 224 default backbone is not "
                "mirrored for I-JEPA; `backbone_args` must be given in the network configuration")
        backbone_args = network_config["backbone_args"]
        n_encoder_features = backbone_args.get("embedding_size", backbone_args["attention_dim"])
        config = {"image_key": "image", "backbone_args": backbone_args,
                  "projection_head_args": network_config.get(
                      "projection_head_args",
                      {"number_of_blocks": 2, "attention_dim": n_encoder_features,
                       "hidden_dim": n_encoder_features, "n_heads": 3}),
                  "feature_map_dimensions": [s // p for s, p in zip(backbone_args["image_size"],
                                                                    backbone_args["patch_size"])],
                  "n_encoder_features": n_encoder_features,
                  "min_patch_size": network_config.get("min_patch_size", [4, 4]),
                  "max_patch_size": network_config.get("max_patch_size", [8, 8]),
                  "n_patches": network_config.get("n_patches", 1),
                  "n_masked_patches": network_config.get("n_masked_patches", 4),
                  "predictor_dim": network_config.get("predictor_dim", None),
                  "stop_gradient": stop_gradient, "optimizer_eps": optimizer_eps}
        return IJEPAPL(**{**common, **config})
    if ssl_method == "mae":
        for args_key, needed in (("encoder_args", _MAE_STACK_KEYS + ("image_size", "patch_size")),
                                 ("decoder_args", _MAE_STACK_KEYS)):
            if args_key not in network_config:
                raise NotImplementedError(
                    f"ssl_method 'mae': `{args_key}` must be given in the network configuration "
                    "(the reference's built-in 224 x 224 default is not mirrored)")
            for key in needed:
                if key not in network_config[args_key]:
                    raise NotImplementedError(
                        f"ssl_method 'mae': `{args_key}` lacks `{key}` (the reference's defaults "
                        "are not mirrored; its transformer stacks have none)")
        encoder_args, decoder_args = network_config["encoder_args"], network_config["decoder_args"]
        config = {"image_key": "image", "image_size": encoder_args["image_size"],
                  "patch_size": encoder_args["patch_size"],
                  "in_channels": encoder_args.get("in_channels", 1),
                  "input_dim_size": encoder_args.get("embed_dim", 96),
                  "encoder_args": encoder_args, "decoder_args": decoder_args,
                  "mask_fraction": network_config.get("mask_fraction", 0.75),
                  "optimizer_eps": optimizer_eps}
        del common["ema"]
        return ViTMaskedAutoEncoderPL(**{**common, **config})
    if ssl_method == "barlow":
        raise NotImplementedError(f"ssl_method {ssl_method!r} (Barlow-Twins wrapper) is "
                                  "outside the HIP path (SURVEY.md section 2: out of scope)")
    boilerplate = {"training_dataloader_call": train_loader_call,
                   "aug_image_key_1": "augmented_image_1",
                   "aug_image_key_2": "augmented_image_2", "box_key_1": "box_1",
                   "box_key_2": "box_2", "n_epochs": max_epochs, "n_steps": max_steps_optim,
                   "warmup_steps": warmup_steps, "ssl_method": ssl_method, "ema": ema,
                   "stop_gradient": stop_gradient, "temperature": 0.1,
                   "optimizer_eps": optimizer_eps}
    if net_type == "unet_encoder":
        return SelfSLUNetPL(**boilerplate, **network_config)
    if net_type == "convnext":
        network_config["backbone_args"] = {k: v for k, v in network_config["backbone_args"].items()
                                           if k != "res_type"}
        return SelfSLConvNeXtPL(**boilerplate, **network_config)
    return SelfSLResNetPL(**boilerplate, **network_config)
