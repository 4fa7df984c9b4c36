"""``mAP`` (mirror of adell_mri/modules/object_detection/map.py:11-133): predictions and targets are
kept per image (``update``); ``compute`` matches them image by image -- predictions above
``score_threshold`` in ascending score order, per target box the prediction with the highest IoU among
those that ``check_overlap`` it (lowest index on a tie, as ``argmax``), a hit when that IoU is >
``iou_threshold`` -- and feeds (class probabilities of the matched prediction, class of the target) of
the hits to an average precision. An image counts only when at least one box overlaps; with no hit in
any image the result is NaN.

On the GPU the matching of ALL images is one launch (csrc/detect.hip, a wavefront per target box); the
small tables then go to the host, where numpy computes the average precision. torchmetrics is not
installed where this package is built, so the average precision is the package's own definition
(``average_precision``): binary, the step-wise sum over the distinct score thresholds of
(R_n - R_{n-1}) P_n (NaN without a positive); multi-class, one-vs-rest averaged over the classes that
have a positive. The surface is the one ``trainer.validate_steps`` reads (``compute_async``)."""
import numpy as np
import torch

from .utils import calculate_iou, check_overlap


def _binary_ap(scores, labels):
    scores, labels = np.asarray(scores, np.float64), np.asarray(labels) > 0
    P = int(labels.sum())
    if P == 0 or scores.size == 0:
        return float("nan")
    order = np.argsort(-scores, kind="stable")
    scores, labels = scores[order], labels[order]
    last = np.r_[np.nonzero(np.diff(scores))[0], scores.size - 1]     # end of each run of equal scores
    tp = np.cumsum(labels)[last].astype(np.float64)
    precision = tp / (last + 1.0)
    recall = tp / P
    return float(np.sum(np.diff(np.r_[0.0, recall]) * precision))


def average_precision(scores, labels, num_classes=None):
    """Binary (``num_classes`` None: scores [n], labels in {0, 1}) or one-vs-rest multi-class
    (scores [n, C], labels in [0, C)) average precision as the module text defines it."""
    scores = np.asarray(scores, np.float64)
    labels = np.asarray(labels).astype(np.int64).reshape(-1)
    if num_classes is None:
        return _binary_ap(scores.reshape(-1), labels)
    scores = scores.reshape(labels.shape[0], num_classes)
    per_class = [_binary_ap(scores[:, c], labels == c) for c in range(num_classes)
                 if (labels == c).any()]
    return float(np.mean(per_class)) if per_class else float("nan")


class mAP(torch.nn.Module):
    def __init__(self, ndim=3, score_threshold=0.5, iou_threshold=0.5, n_classes=2):
        super().__init__()
        self.ndim = ndim
        self.iou_threshold = iou_threshold
        self.score_threshold = score_threshold
        self.n_classes = n_classes
        self.num_classes = n_classes
        self.pred_list = []
        self.target_list = []
        self.pred_keys = ["boxes", "scores", "labels"]
        self.target_keys = ["boxes", "labels"]
        self.hits = 0
        self._ap_scores, self._ap_labels = [], []

    def check_input(self, x, what):
        if what == "pred":
            K = self.pred_keys
        elif what == "target":
            K = self.target_keys
        for y in x:
            keys = y.keys()
            if not all([k in keys for k in K]):
                raise ValueError("{} should have the keys {}".format(what, K))
            for k in K:
                if len(y[k].shape) == 0:
                    y[k] = y[k].unsqueeze(0)
            if len(np.unique([y[k].shape[0] for k in K])) > 1:
                raise ValueError("Inputs in {} should have the same number of elements".format(what))

    def update(self, pred, target):
        self.check_input(pred, "pred")
        self.check_input(target, "target")
        self.pred_list.extend(pred)
        self.target_list.extend(target)

    def forward(self, pred, target):
        self.update(pred, target)

    def _sorted(self, pred):
        pbb, ps, pcp = [pred[k] for k in self.pred_keys]
        ps_v = ps > self.score_threshold
        pbb, ps, pcp = pbb[ps_v], ps[ps_v], pcp[ps_v]
        score_order = torch.argsort(ps, stable=True)
        return pbb[score_order], ps[score_order], pcp[score_order]

    def match_image(self, pred, target):
        """(best prediction per target box, its IoU, whether any box overlaps, the sorted class
        probabilities) of one image: steps 1-3 of ``compute_image`` in torch ops."""
        pbb, ps, pcp = self._sorted(pred)
        tbb = target["boxes"]
        n_pred, n_target = pbb.shape[0], tbb.shape[0]
        iou_array = torch.zeros([n_target, n_pred], device=pcp.device)
        any_hit = False
        for i in range(n_target):
            cur_bb = torch.unsqueeze(tbb[i], 0)
            overlap = check_overlap(cur_bb, pbb, self.ndim)
            if overlap.sum() > 0:
                iou_array[i, overlap] = calculate_iou(cur_bb, pbb[overlap], self.ndim).float()
                any_hit = True
        if not any_hit:
            return None, None, False, pcp
        best_pred = torch.argmax(iou_array, 1)
        return best_pred, iou_array[torch.arange(0, n_target), best_pred], True, pcp

    def _feed(self, best_pred, true_ious, pcp, tc):
        hit = true_ious > self.iou_threshold
        if hit.sum() > 0:
            self._ap_scores.append(pcp[best_pred][hit].detach().double().cpu().numpy())
            self._ap_labels.append(tc[hit].int().cpu().numpy())
            self.hits += 1

    def compute_image(self, pred, target):
        best_pred, true_ious, any_hit, pcp = self.match_image(pred, target)
        if any_hit:
            self._feed(best_pred, true_ious, pcp, target["labels"].to(pcp.device))

    def _compute_device(self):
        """Every image's matching in one launch; an image where nothing overlaps has best IoU 0
        everywhere and so feeds nothing, as in ``compute_image``."""
        from ... import ops

        dev = self.pred_list[0]["boxes"].device
        sorted_preds = [self._sorted(p) for p in self.pred_list]
        starts = np.cumsum([0] + [s[0].shape[0] for s in sorted_preds])
        tcount = [int(t["boxes"].shape[0]) for t in self.target_list]
        if sum(tcount) == 0:
            return
        preds = torch.cat([s[0] for s in sorted_preds]).float().reshape(-1, 6).contiguous()
        targets = torch.cat([t["boxes"].to(dev).float().reshape(-1, 6) for t in self.target_list]).contiguous()
        image = torch.from_numpy(np.repeat(np.arange(len(tcount)), tcount).astype(np.int32)).to(dev)
        best, iou = ops.det_match(targets, image, preds,
                                  torch.from_numpy(starts.astype(np.int32)).to(dev))
        t0 = np.cumsum([0] + tcount)
        for i, (s, t) in enumerate(zip(sorted_preds, self.target_list)):
            if tcount[i] == 0 or s[0].shape[0] == 0:
                continue
            b, v = best[t0[i]:t0[i + 1]].long(), iou[t0[i]:t0[i + 1]]
            self._feed(b, v, s[2], t["labels"].to(dev))

    def compute(self):
        on_gpu = (len(self.pred_list) > 0 and self.ndim == 3
                  and all(p["boxes"].is_cuda for p in self.pred_list))
        if on_gpu:
            self._compute_device()
        else:
            for pred, target in zip(self.pred_list, self.target_list):
                self.compute_image(pred, target)
        if self.hits > 0:
            scores = np.concatenate([s.reshape(s.shape[0], -1) for s in self._ap_scores])
            labels = np.concatenate([l.reshape(-1) for l in self._ap_labels])
            nc = None if self.n_classes == 2 else self.n_classes
            return torch.Tensor([average_precision(scores, labels, nc)])
        return torch.Tensor([torch.nan])

    def compute_async(self):
        """(value, bad-target count) for ``trainer.validate_steps``; the matching's tables are read
        on the host here."""
        dev = self.pred_list[0]["boxes"].device if self.pred_list else "cpu"
        return self.compute().reshape(()).to(dev), torch.zeros((), device=dev)

    def reset(self):
        self.pred_list = []
        self.target_list = []
        self.hits = 0
        self._ap_scores, self._ap_labels = [], []
