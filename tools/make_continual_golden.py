#!/usr/bin/env python3
"""Fixture of the continual-learning package from the REAL reference (needs a checkout of the
reference, ADELL_REFERENCE; no test reads it, the tests read the fixture):

    python tools/make_continual_golden.py   -> tests/golden/continual.npz

The reference's continuous_learning/regularization.py and optim.py are loaded by file path (they
import torch, numpy and the standard library only). Inputs come from tests/continual_cases.py.

Per p of ``PS`` and parameter state of ``STATES`` over the named tensors of ``SHAPES``:
  pen32 / g32   the reference's fp32 penalty (its __call__) and the gradients autograd gives each live
                parameter;
  pen64 / g64   the same sum of p-norms evaluated by torch in fp64 from the same fp32 inputs (the
                reference's own call cannot: it accumulates into an fp32 ``torch.zeros([1])``);
  err_pen, err_g  ``ref_err``: the reference's relative deviation from fp64 (gradients: per tensor, as
                a fraction of the largest |g64|; 0 where both are 0).
Then the name lists ``create_param_groups`` yields for ``GROUP_CASES`` (leftovers on and off) as JSON,
and ``EarlyStopper``'s decisions over ``LOSSES`` for ``STOPPERS``.
"""
import importlib.util
import json
import os
import sys

import numpy as np

os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("ADELL_REFERENCE") or os.path.join(os.path.dirname(ROOT), "reference")
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import continual_cases as C  # noqa: E402


def load(name):
    path = os.path.join(REF, "adell_mri", "modules", "continuous_learning", name + ".py")
    spec = importlib.util.spec_from_file_location("reference_" + name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


REG, OPT = load("regularization"), load("optim")


def rel(a, r):
    a, r = np.asarray(a, dtype=np.float64), np.asarray(r, dtype=np.float64)
    top = np.abs(r).max()
    return float(np.abs(a - r).max() / top) if top > 0 else float(np.abs(a - r).max())


def gen_penalty(out):
    for p in C.PS:
        for st in C.STATES:
            key = f"{p}:{st}"
            ewc = REG.ElasticWeightConsolidation(C.Named(C.anchors()), p=p)
            live = C.Named(C.state(st))
            pen = ewc(live)
            assert pen.shape == (1,) and pen.dtype == torch.float32
            pen.sum().backward()
            g32 = {k: q.grad.numpy() for k, q in live.named_parameters()}
            live64, anchor64 = C.Named(C.state(st), torch.float64), C.Named(C.anchors(), torch.float64)
            a64 = dict(anchor64.named_parameters())
            pen64 = sum(torch.norm(q - a64[k].detach(), p=p) for k, q in live64.named_parameters())
            pen64.backward()
            out["pen32:" + key] = pen.detach().numpy()
            out["pen64:" + key] = np.float64(pen64.detach())
            out["err_pen:" + key] = np.float64(rel(pen.detach().numpy(), float(pen64.detach())))
            worst = 0.0
            for k, q in live64.named_parameters():
                assert np.isfinite(g32[k]).all() and torch.isfinite(q.grad).all(), (key, k)
                out[f"g32:{key}:{k}"] = g32[k]
                out[f"g64:{key}:{k}"] = q.grad.numpy()
                e = rel(g32[k], q.grad.numpy())
                out[f"err_g:{key}:{k}"] = np.float64(e)
                worst = max(worst, e)
            print(f"p={p} {st:10s}: penalty {float(pen.detach()):.7f} (fp64 {float(pen64.detach()):.10f}), reference fp32 "
                  f"vs fp64: penalty {out['err_pen:' + key]:.2e}, gradients {worst:.2e}")


def gen_groups(out):
    for case, var_groups in C.GROUP_CASES.items():
        for leftovers in (True, False):
            model = C.group_model()
            names = {id(q): k for k, q in model.named_parameters()}
            groups = OPT.create_param_groups(model, var_groups, include_leftovers=leftovers)
            lists = [[names[id(q)] for q in g["params"]] for g in groups]
            out[f"groups:{case}:{int(leftovers)}"] = np.array(json.dumps(lists))
            print(f"groups {case} leftovers={leftovers}: {lists}")


def gen_stoppers(out):
    for tag, (patience, min_delta) in C.STOPPERS.items():
        stopper = OPT.EarlyStopper(patience, min_delta)
        out["stop:" + tag] = np.array([bool(stopper(torch.tensor(v))) for v in C.LOSSES])
        print(f"stopper {tag}: {out['stop:' + tag].astype(int).tolist()}")


def main():
    out = {}
    gen_penalty(out)
    gen_groups(out)
    gen_stoppers(out)
    np.savez_compressed(C.GOLD, **out)
    print(f"wrote {C.GOLD}: {os.path.getsize(C.GOLD)} bytes")
    assert os.path.getsize(C.GOLD) < (1 << 20)


if __name__ == "__main__":
    main()
