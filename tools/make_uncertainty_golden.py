#!/usr/bin/env python3
"""Fixtures of the bootstrap AUC interval and of adaptive prediction sets from the REAL reference
(needs a checkout of the reference, ADELL_REFERENCE; no test reads it, the tests read the fixtures):

    python tools/make_uncertainty_golden.py -> tests/golden/uncertainty.npz,
                                               tests/golden/uncertainty_surface.json

The reference is imported through the stub recipe of tools/make_deconfounded_golden.py.
``AdaptivePredictionSets`` and ``bootstrap_metric`` are the real ones; ``torchmetrics`` and ``tqdm``,
which are not installed, are stubbed (a ``Metric`` name for the annotation, a ``trange`` that is a
plain range with ``set_description``). Lightning is not installed either, so the signatures of
``ClassPLABC.calibrate`` / ``predict_calibrated_step`` are read from their source text.

* aps_<n>_<C>_*: inputs (tests/uncertainty_cases.py), the reference's ``qhat``, the whole output of its
  ``forward`` on the calibration rows, and the cumulative probabilities and scores by the expressions of
  its ``calculate`` (the module keeps neither).
* boot_<name>_*: inputs, every index row the real ``bootstrap_metric`` drew (``torch.randperm`` is
  recorded while it runs), the value of every resample, the mean and the quantiles. The metric it
  drives is the fp64 Mann-Whitney object below (``preds`` / ``target`` / ``reset`` / ``update`` /
  ``compute``), binary or one-vs-rest macro with the conventions of ``classification_metrics``.
"""
import ast
import json
import os
import sys
import types

import numpy as np

os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("ADELL_REFERENCE") or os.path.join(os.path.dirname(ROOT), "reference")
sys.path.insert(0, ROOT)
for name, path in [
    ("adell_mri", "adell_mri"), ("adell_mri.modules", "adell_mri/modules"),
    ("adell_mri.utils", "adell_mri/utils"),
    ("adell_mri.modules.conformal_prediction", "adell_mri/modules/conformal_prediction"),
]:
    m = types.ModuleType(name)
    m.__path__ = [os.path.join(REF, path)]
    sys.modules[name] = m


class _Range:
    def __init__(self, n):
        self.n = n

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False

    def set_description(self, text):
        pass

    def __iter__(self):
        return iter(range(self.n))


sys.modules["torchmetrics"] = types.ModuleType("torchmetrics")
sys.modules["torchmetrics"].Metric = object
sys.modules["tqdm"] = types.ModuleType("tqdm")
sys.modules["tqdm"].trange = _Range
import torch  # noqa: E402

from adell_mri.modules.conformal_prediction.conformal import AdaptivePredictionSets  # noqa: E402
from adell_mri.utils import bootstrap_metrics as RB  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tests"))
import uncertainty_cases as C  # noqa: E402
import uncertainty_ref as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")


class MannWhitneyAUROC:
    """fp64 AUC by the rank-sum statistic with average ranks; one-vs-rest macro beyond two classes."""

    def __init__(self, n_classes):
        self.n_classes = n_classes
        self.preds, self.target, self.values = [], [], []

    def reset(self):
        self.preds, self.target = [], []

    def update(self, preds, target):
        self.preds.append(preds)
        self.target.append(target)

    @staticmethod
    def _auc(s, y):
        s = s.double()
        pos, neg = s[y == 1], s[y == 0]
        if pos.numel() == 0 or neg.numel() == 0:
            return None
        gt = (pos[:, None] > neg[None, :]).double().sum()
        eq = (pos[:, None] == neg[None, :]).double().sum()
        return (gt + 0.5 * eq) / (pos.numel() * neg.numel())

    def compute(self):
        s, y = torch.cat(self.preds), torch.cat(self.target)
        if self.n_classes == 2:
            v = self._auc(s, y)
            v = torch.tensor(float("nan"), dtype=torch.float64) if v is None else v
        else:
            vs = [self._auc(s[:, c], (y == c).long()) for c in range(self.n_classes)]
            vs = [u for u in vs if u is not None]
            v = torch.stack(vs).mean() if vs else torch.tensor(float("nan"), dtype=torch.float64)
        self.values.append(float(v))
        return v


def gen_aps(out):
    for n, K in C.APS_CPU_CASES:
        p, y = C.aps_inputs(n, K)
        pt, yt = torch.from_numpy(p), torch.from_numpy(y)
        aps = AdaptivePredictionSets(C.ALPHA)
        aps.update(yt, pt)
        aps.calculate()
        # the expressions of calculate(), whose intermediate results the module does not keep
        pi = pt.argsort(1, descending=True)
        srt = torch.take_along_dim(pt, pi, axis=1).cumsum(axis=1)
        cum = torch.take_along_dim(srt, pi.argsort(axis=1), axis=1)
        key = C.aps_key(n, K)
        out[key + "_p"], out[key + "_y"] = p, y
        out[key + "_qhat"] = aps.qhat.detach().numpy()
        out[key + "_out"] = aps(pt).detach().numpy()
        out[key + "_cum"] = cum.numpy()
        out[key + "_scores"] = cum[range(n), yt].numpy()
        # the restatement agrees with the reference on this case, bit for bit
        assert np.array_equal(R.aps_cumulative(p), out[key + "_cum"]), key
        assert np.float32(R.aps_qhat(p, y, C.ALPHA)) == out[key + "_qhat"], key
        assert np.array_equal(R.aps_sets(p, out[key + "_qhat"]), out[key + "_out"][:, :K] > 0), key


def gen_boot(out):
    for name, (n, K, samples, size, seed) in C.BOOT_CASES.items():
        s, y = C.boot_inputs(name)
        metric = MannWhitneyAUROC(K)
        metric.update(torch.from_numpy(s), torch.from_numpy(y))
        rows, randperm = [], torch.randperm

        def recording(*args, **kwargs):
            rows.append(randperm(*args, **kwargs))
            return rows[-1]

        torch.randperm = recording
        try:
            mean, quantiles = RB.bootstrap_metric(metric, samples=samples, sample_size=size, seed=seed)
        finally:
            torch.randperm = randperm
        m = int(size * n)
        idx = torch.stack([r[:m] for r in rows]).numpy().astype(np.int32)
        assert idx.shape == (samples, m) and mean.dtype == torch.float64
        key = "boot_" + name
        out[key + "_scores"], out[key + "_labels"], out[key + "_idx"] = s, y, idx
        out[key + "_values"] = np.array(metric.values, dtype=np.float64)
        out[key + "_mean"], out[key + "_quantiles"] = mean.numpy(), quantiles.numpy()
        assert out[key + "_mean"].shape == (1,) and out[key + "_quantiles"].shape == (2, 1)
        vals, mu, qs = R.bootstrap(s, y, K, idx.astype(np.int64))
        assert np.abs(vals - out[key + "_values"]).max() < 1e-14, key
        assert abs(mu - out[key + "_mean"][0]) < 1e-14, key
        assert np.abs(qs - out[key + "_quantiles"][:, 0]).max() < 1e-14, key


def source_signature(path, cls, fn):
    """[name, default source text | None] per parameter of a function read from source text."""
    with open(os.path.join(REF, path)) as fh:
        tree = ast.parse(fh.read())
    body = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == cls).body
    node = next(n for n in body if isinstance(n, ast.FunctionDef) and n.name == fn)
    a = node.args
    pos = a.posonlyargs + a.args
    defaults = [None] * (len(pos) - len(a.defaults)) + [ast.unparse(d) for d in a.defaults]
    out = [[p.arg, d] for p, d in zip(pos, defaults)]
    if a.vararg:
        out.append(["*" + a.vararg.arg, None])
    if a.kwarg:
        out.append(["**" + a.kwarg.arg, None])
    return out


def gen_surface():
    surface = {
        "signatures": {
            **{f"AdaptivePredictionSets.{fn}": C.signature_of(getattr(AdaptivePredictionSets, fn))
               for fn in ("__init__", "update", "calculate", "reset", "forward")},
            "bootstrap_metric": C.signature_of(RB.bootstrap_metric),
            "cat_if_necessary": C.signature_of(RB.cat_if_necessary),
        },
        "source_signatures": {
            f"ClassPLABC.{fn}": source_signature("adell_mri/modules/classification/pl.py",
                                                 "ClassPLABC", fn)
            for fn in ("calibrate", "predict_calibrated_step")},
        "not_implemented_message": _message(),
    }
    path = os.path.join(OUT, "uncertainty_surface.json")
    with open(path, "w") as fh:
        json.dump(surface, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(f"{path}: {os.path.getsize(path)} bytes")


def _message():
    try:
        RB.bootstrap_metric(object())
    except NotImplementedError as e:
        return str(e)
    raise AssertionError("the reference took an object without preds and target")


def main():
    out = {}
    gen_aps(out)
    gen_boot(out)
    path = os.path.join(OUT, "uncertainty.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes, {len(out)} arrays")
    gen_surface()


if __name__ == "__main__":
    main()
