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


def test_every_weight_gradient_query_answers_as_recorded():
    """The weight-gradient host path (csrc/conv_wgrad_f16.hip adell_wgrad_route, csrc/conv_wgrad.hip)
    the same way, from tests/golden/conv_wgrad_plan_sweep.npz: both workspace queries, rows_ok, the
    z-ring plan, every entry of adell_conv3d_bwd_weight_f16x3_plan (route, regions, per-plane and fp32
    instance) under no switch, wgrad_nozring and wgrad_no16, and the transposed-conv workspace. The
    stride-2 route reads the CU count, which is 256 without a device and on the MI355X."""
    tool = _tool()
    gold = np.load(tool.WGRAD_GOLDEN)
    _, convt = tool.grid()
    wg = tool.wgrad_grid()
    want = gold["wgrad_answers"].T       # (stored column by column)
    assert np.array_equal(wg, gold["wgrad"].T) and np.array_equal(convt, gold["convt"]), (
        "the descriptor grid changed: regenerate the file (tools/conv_plan_sweep.py wgrad)")
    a, t = tool.wgrad_answers(wg, convt)
    tool.check_wgrad_coverage(wg, a, t)
    assert np.array_equal(a, want), _report(tool, wg, a, want, tool.WGRAD_COLUMNS,
                                            tool.WGRAD_SWITCHES)
    bad = np.nonzero(t != gold["convt_workspace"])[0]
    assert len(bad) == 0, [(convt[i, 1:].tolist(), int(t[i]), int(gold["convt_workspace"][i]))
                          for i in bad[:10]]
