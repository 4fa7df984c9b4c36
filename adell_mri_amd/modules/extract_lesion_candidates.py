"""The reference's ``adell_mri/modules/extract_lesion_candidates.py`` (Report-Guided-Annotation
post-processing) with its three function names, keyword names and defaults, computed on the device
by ``ops.lesion_candidates`` (csrc/components.hip). scipy is not a dependency.

One 3-D probability map in, ``(hard_blobs, [(index, confidence), ...], indexed)`` out: a device
tensor gives device tensors (``indexed`` int32), a numpy array is copied to the current device and
gives numpy arrays of the reference's dtypes (``indexed`` int32 in the static modes, what
``scipy.ndimage.label`` returns, and int64 in the dynamic mode, ``np.zeros_like(..., dtype=int)``).
Building the list is one host synchronisation (the table length) on top of those of the device
call: none in the static modes, rounds + 1 in the dynamic mode.

The confidences of the list are Python floats with the reference's values: in the static modes
``np.round(float64(peak), d)`` (the reference takes the maximum of an int32 x float32 product, which
numpy makes float64, so the list keeps more digits than the float32 map painted with it); in the
dynamic mode the float32 value of the painted map (``np.max(all_hard_blobs)``, :101).

Input must be float32; float16 and bfloat16 are converted to float32 (the reference converts
float16, :178-179). float64, integer and complex maps raise TypeError: the device path is fp32 and
cannot keep float64 maxima. Values are assumed finite and non-negative (probabilities).
"""
from typing import List, Optional, Tuple, Union

import numpy as np
import torch

from .. import ops

_FAILSAFE = 0.01


def _run(softmax, threshold, dynamic, **kw):
    as_numpy = isinstance(softmax, np.ndarray)
    x = softmax
    if as_numpy:
        if x.dtype not in (np.float32, np.float16):
            raise TypeError(f"extract_lesion_candidates: {x.dtype} input: the device path is fp32 "
                            "(float16 is converted); float64 maxima cannot be kept, and integer or "
                            "complex maps are not probabilities")
        x = torch.from_numpy(np.ascontiguousarray(x)).to(torch.device("cuda", torch.cuda.current_device()))
    elif not torch.is_tensor(x):
        raise TypeError(f"extract_lesion_candidates: expected a numpy array or a tensor, got "
                        f"{type(softmax).__name__}")
    if x.dim() != 3:
        raise ValueError(f"extract_lesion_candidates: one 3-D volume per call, got shape "
                         f"{tuple(x.shape)} (the reference labels with a 3x3x3 structure; "
                         "ops.lesion_candidates takes batches)")
    hard, indexed, n, ids, conf, peak, _ = ops._lesion_candidates(x, threshold, **kw)
    k = int(n)                                   # the host synchronisation of the list
    ids = ids[:k].cpu().numpy()
    d = kw["max_prob_round_decimals"]
    if dynamic:
        values = conf[:k].cpu().numpy().astype(np.float64)
    else:
        values = peak[:k].cpu().numpy().astype(np.float64)
        if d is not None:
            values = np.round(values, d)
    confidences = [(int(i), float(c)) for i, c in zip(ids, values)]
    if as_numpy:
        hard = hard.cpu().numpy()
        indexed = indexed.cpu().numpy()
        if dynamic:
            indexed = indexed.astype(np.int64)
    return hard, confidences, indexed


def extract_lesion_candidates_static(
    softmax,
    threshold: float = 0.10,
    min_voxels_detection: int = 10,
    max_prob_round_decimals: Optional[int] = 4,
) -> Tuple[object, List[Tuple[int, float]], object]:
    """Extract lesion candidates from a softmax volume using a static threshold (:19-55)."""
    return _run(softmax, float(threshold), False, min_voxels_detection=min_voxels_detection,
                num_lesions_to_extract=0, dynamic_threshold_factor=1.0,
                max_prob_round_decimals=max_prob_round_decimals,
                remove_adjacent_lesion_candidates=True)


def extract_lesion_candidates_dynamic(
    softmax,
    min_voxels_detection: int = 10,
    num_lesions_to_extract: int = 5,
    dynamic_threshold_factor: float = 2.5,
    max_prob_round_decimals: Optional[int] = None,
    remove_adjacent_lesion_candidates: bool = True,
    max_prob_failsafe_stopping_threshold: float = 0.01,
) -> Tuple[object, List[Tuple[int, float]], object]:
    """Generate detection proposals using a dynamic threshold to determine the location and size of
    lesions (:58-134). The stopping threshold is the reference's 0.01 on the device."""
    if float(max_prob_failsafe_stopping_threshold) != _FAILSAFE:
        raise NotImplementedError("extract_lesion_candidates_dynamic: the device loop stops at the "
                                  f"reference's default of {_FAILSAFE}, got "
                                  f"{max_prob_failsafe_stopping_threshold}")
    return _run(softmax, "dynamic", True, min_voxels_detection=min_voxels_detection,
                num_lesions_to_extract=num_lesions_to_extract,
                dynamic_threshold_factor=dynamic_threshold_factor,
                max_prob_round_decimals=max_prob_round_decimals,
                remove_adjacent_lesion_candidates=remove_adjacent_lesion_candidates)


def extract_lesion_candidates(
    softmax,
    threshold: Union[str, float] = "dynamic-fast",
    min_voxels_detection: int = 10,
    num_lesions_to_extract: int = 5,
    dynamic_threshold_factor: float = 2.5,
    max_prob_round_decimals: Optional[int] = None,
    remove_adjacent_lesion_candidates: bool = True,
) -> Tuple[object, List[Tuple[int, float]], object]:
    """Generate detection proposals using a dynamic or static threshold to determine the size of
    lesions (:137-227): ``threshold`` is ``"dynamic"``, ``"dynamic-fast"`` or a number."""
    if isinstance(threshold, str) and threshold == "dynamic":
        return extract_lesion_candidates_dynamic(
            softmax, min_voxels_detection=min_voxels_detection,
            num_lesions_to_extract=num_lesions_to_extract,
            dynamic_threshold_factor=dynamic_threshold_factor,
            max_prob_round_decimals=max_prob_round_decimals,
            remove_adjacent_lesion_candidates=remove_adjacent_lesion_candidates)
    if not (isinstance(threshold, str) and threshold == "dynamic-fast"):
        threshold = float(threshold)
    return _run(softmax, threshold, False, min_voxels_detection=min_voxels_detection,
                num_lesions_to_extract=num_lesions_to_extract,
                dynamic_threshold_factor=dynamic_threshold_factor,
                max_prob_round_decimals=max_prob_round_decimals,
                remove_adjacent_lesion_candidates=remove_adjacent_lesion_candidates)
