"""numpy restatement of the reference's lesion-candidate extraction
(adell_mri/modules/extract_lesion_candidates.py) for the tests, on tests/picai_ref.py's labelling.
Same values and dtypes as the reference under numpy 2 promotion: thresholds and the 0.01 stopping
value compare in float32, a component's maximum is rounded in float64 (the reference takes it from
an int32 x float32 product) and painted as float32. Checked against the fixture (generated from the
real reference) and, where scipy imports, against scipy directly."""
import numpy as np

from picai_ref import label


def _label_stats(clipped):
    lab, n = label(clipped != 0)
    flat = lab.ravel()
    counts = np.bincount(flat, minlength=n + 1)
    peaks = np.zeros(n + 1, np.float32)
    np.maximum.at(peaks, flat, clipped.ravel())
    return lab, n, counts, peaks


def static(softmax, threshold=0.10, min_voxels_detection=10, max_prob_round_decimals=4):
    """(hard_blobs float32, [(index, confidence float)], indexed int32) (:19-55)."""
    x = np.asarray(softmax, dtype=np.float32)
    clipped = x.copy()
    clipped[x < np.float32(threshold)] = 0
    lab, n, counts, peaks = _label_stats(clipped)
    keep = counts > min_voxels_detection
    keep[0] = False
    values = peaks.astype(np.float64)
    if max_prob_round_decimals is not None:
        values = np.round(values, max_prob_round_decimals)
    paint = np.where(keep, values, 0.0).astype(np.float32)
    hard = np.where(clipped > 0, paint[lab], np.float32(0)).astype(np.float32)
    indexed = np.where(keep[lab], lab, 0).astype(np.int32)
    confidences = [(int(i), float(values[i])) for i in range(1, n + 1) if keep[i]]
    return hard, confidences, indexed


def _dilate(mask):
    D, H, W = mask.shape
    p = np.zeros((D + 2, H + 2, W + 2), bool)
    p[1:-1, 1:-1, 1:-1] = mask
    out = np.zeros_like(mask)
    for dz in range(3):
        for dy in range(3):
            for dx in range(3):
                out |= p[dz:dz + D, dy:dy + H, dx:dx + W]
    return out


def dynamic(softmax, min_voxels_detection=10, num_lesions_to_extract=5, dynamic_threshold_factor=2.5,
            max_prob_round_decimals=None, remove_adjacent_lesion_candidates=True):
    """(hard_blobs float32, [(index, confidence float)], indexed int64) (:58-134); ``rounds`` is
    kept as a function attribute of the last call for the tests of the synchronisation count."""
    working = np.asarray(softmax, dtype=np.float32).copy()
    hard = np.zeros_like(working)
    indexed = np.zeros(working.shape, np.int64)
    confidences = []
    factor = np.float32(dynamic_threshold_factor)
    dynamic.rounds = 0
    while len(confidences) < num_lesions_to_extract:
        index = 1 + len(confidences)
        m = working.max()
        if m < np.float32(0.01):
            break
        dynamic.rounds += 1
        blobs, _, _ = static(working, m / factor, min_voxels_detection, max_prob_round_decimals)
        best = blobs.max()
        mask = blobs == best
        # label(mask) == 1: the component of the mask that comes first in raster order
        mask_lab, _ = label(mask)
        mask = mask_lab == 1
        blob = blobs * mask
        overlap = bool((mask & _dilate(hard > 0)).any())
        if not (remove_adjacent_lesion_candidates and overlap):
            hard += blob
            confidences.append((index, float(best)))
            indexed += mask * index
        working = working * (~mask)
    return hard, confidences, indexed


def extract(softmax, threshold="dynamic-fast", min_voxels_detection=10, num_lesions_to_extract=5,
            dynamic_threshold_factor=2.5, max_prob_round_decimals=None,
            remove_adjacent_lesion_candidates=True):
    """The reference's ``extract_lesion_candidates`` (:137-227) on a float32 volume."""
    x = np.asarray(softmax, dtype=np.float32)
    if isinstance(threshold, str) and threshold == "dynamic":
        return dynamic(x, min_voxels_detection, num_lesions_to_extract, dynamic_threshold_factor,
                       max_prob_round_decimals, remove_adjacent_lesion_candidates)
    if isinstance(threshold, str) and threshold == "dynamic-fast":
        threshold = float(x.max() / np.float32(dynamic_threshold_factor))
    return static(x, float(threshold), min_voxels_detection, max_prob_round_decimals)
