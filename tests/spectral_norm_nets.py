"""The two applied networks of the spectral-norm tests on this package's classes, with the weights
the fixtures of tools/make_spectral_norm_golden.py start from."""
import copy

import numpy as np
import torch

import spectral_norm_cases as C
from classification_cases import fill


# the classification wrapper holds its network as ``network``; the fixture was recorded on the network
PREFIX = {"unet": "", "cat": "network."}


def strip(tag, key):
    assert key.startswith(PREFIX[tag]), key
    return key[len(PREFIX[tag]):]


def net_gold(tag):
    return np.load(C.NET_GOLD[tag], allow_pickle=False)


def build(tag):
    """The ``*PL`` wrapper of a fixture network with the fill of the fixture, every dropout at 0."""
    if tag == "unet":
        from adell_mri_amd.modules.activations import activation_factory
        from adell_mri_amd.modules.segmentation.losses import CompoundLoss, binary_focal_loss
        from adell_mri_amd.modules.segmentation.pl import UNetPL

        net = UNetPL(image_key="image", label_key="mask", learning_rate=C.UNET_LR,
                     weight_decay=C.UNET_WD, loss_fn=CompoundLoss([(binary_focal_loss, dict(C.FOCAL))]),
                     activation_fn=activation_factory["swish"], **copy.deepcopy(C.UNET_KW))
        gain = C.UNET_GAIN
    else:
        from test_classification import build_pl

        net, _ = build_pl(C.CAT_NAME)
        gain = C.CAT_GAIN
    inner = getattr(net, "network", net)
    inner.load_state_dict(fill(inner.state_dict(), gain))
    return net


def batch(tag, device):
    if tag == "unet":
        x, y = C.unet_batch()
        return {"image": torch.from_numpy(x).to(device), "mask": torch.from_numpy(y).to(device)}
    from classification_cases import CONFIGS

    return {"image": torch.from_numpy(C.cat_input()).to(device),
            "label": torch.tensor(CONFIGS[C.CAT_NAME][3]).to(device)}


def initial_state(net, g, tag):
    """The fixture's initial ``state_dict`` for a parametrised ``net``: its own (filled) weights and the
    fixture's ``_u`` / ``_v`` draws."""
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    for k in sd:
        if k.endswith(("._u", "._v")):
            sd[k] = torch.from_numpy(g["init:" + strip(tag, k)]).to(sd[k].device)
    return sd
