"""The f16x3 conv planner over a dense grid of descriptors (tools/conv_plan_sweep.py): every host-only
query entry -- plan, split-K workspace, statistics rows with and without workspace, rows_ok, fused-
epilogue rows, transposed-conv plan -- still answers what tests/golden/conv_f16x3_plan_sweep.npz
records. tests/test_conv_plans.py pins one named case per branch; this pins the thresholds between
them, so a change of the planner's code that was not meant to change a plan shows here, with the
descriptors it moved. No GPU: the planner reads no device property. A deliberate retune regenerates
the file with the tool."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location(
        "conv_plan_sweep", os.path.join(ROOT, "tools", "conv_plan_sweep.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _report(tool, desc, got, want, columns, switches):
    bad = np.nonzero((got != want).any(axis=1))[0]
    lines = [f"{len(bad)} of {len(desc)} descriptors answer differently; the first:"]
    for i in bad[:10]:
        cols = np.nonzero(got[i] != want[i])[0]
        lines.append("  {} {}: {}".format(
            switches[desc[i, 0]] or "", desc[i, 1:].tolist(),
            ", ".join(f"{columns[c]} {got[i, c]} (recorded {want[i, c]})" for c in cols)))
    return "\n".join(lines)


def test_every_query_answers_as_recorded():
    tool = _tool()
    gold = np.load(tool.GOLDEN)
    conv, convt = tool.grid()
    # the grid follows the case tables of three test files: a new case there needs a new file
    assert np.array_equal(conv, gold["conv"]) and np.array_equal(convt, gold["convt"]), (
        "the descriptor grid changed: regenerate the file (tools/conv_plan_sweep.py)")
    a, t = tool.answers(conv, convt)
    tool.check_coverage(a, t)
    assert np.array_equal(a, gold["conv_answers"]), _report(
        tool, conv, a, gold["conv_answers"], tool.ANSWER_COLUMNS, tool.SWITCHES)
    assert np.array_equal(t, gold["convt_answers"]), _report(
        tool, convt, t, gold["convt_answers"], tool.CONVT_COLUMNS, tool.SWITCHES)
