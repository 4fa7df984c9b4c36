"""adell_attention_desc and the three attention entries that take it (csrc/tokens.hip adell_att_fill):
every refusal comes before the first HIP call, so all of it runs without a GPU. The pointers are
addresses inside a small host buffer that no case gets far enough to read (tests/test_abi.py does the
same); each case names the entry, what it changes in a call that would otherwise launch, and a piece
of the error text it expects after the entry's name."""
import ctypes

import pytest

from adell_mri_amd import _lib, ops

ENTRIES = ("fwd", "bwd", "bias_grad")
NOPS = dict(fwd=4, bwd=8, bias_grad=5)
OPERANDS = ("q", "k", "v", "out", "dout", "dq", "dk", "dv")

_BUF = (ctypes.c_float * 64)()
BASE = (ctypes.addressof(_BUF) + 15) & ~15          # 16-byte aligned, 4-byte aligned at BASE + 4


def _desc(entry, strided, **over):
    """A call that passes every check: 4 sequences (2 items of 2 heads) of 64 tokens, 64-wide heads."""
    f = dict(BH=4, H=2, T=64, A=64, Dv=64, scale=0.125, drop_p=0.0, rng_offset=0, seed=1, bias=None,
             labels=None, nbias=2 if entry == "bias_grad" else 0, nlab=0)
    row = over.pop("row", {})         # operand name -> row stride
    f.update(over)
    d = _lib.AttentionDesc(**f)
    d.strided = int(strided)
    for i, name in enumerate(OPERANDS):
        C = f["A"] if name in ("q", "k", "dq", "dk") else f["Dv"]
        d.stride[i][0], d.stride[i][1], d.stride[i][2] = 2 * 64 * C, 64 * C, row.get(name, C)
    return d


def _call(entry, d, ptr=None, ws_floats=None):
    """The entry with BASE for every pointer but those in `ptr` (name -> address or None)."""
    ptr = ptr or {}
    h = _lib.lib()
    g = lambda name: ptr.get(name, BASE)                                     # noqa: E731
    ops_ = [g(n) for n in OPERANDS]
    if entry == "fwd":
        return h.adell_attention_fwd(ctypes.byref(d), *ops_[:4], g("lse"), None)
    if entry == "bwd":
        return h.adell_attention_bwd(ctypes.byref(d), *ops_[:5], g("lse"), *ops_[5:], None)
    nws = h.adell_attention_bias_grad_workspace_floats(d.nbias, d.T) if ws_floats is None else ws_floats
    return h.adell_attention_bias_grad(ctypes.byref(d), *ops_[:5], g("lse"), g("dbias"), g("workspace"), nws,
                                       None)


# (id, entries, strided, descriptor fields, pointers, expected piece of the error text)
CASES = [
    ("T=0", ENTRIES, 0, dict(T=0), {}, "bad dims"),
    ("A=257", ENTRIES, 0, dict(A=257), {}, "head dims up to 256"),
    ("bias with nbias=0", ENTRIES, 0, dict(bias=BASE, nbias=0), {}, "bias needs nbias > 0"),
    ("labels with nlab=0", ENTRIES, 0, dict(labels=BASE, nlab=0), {}, "labels need nlab > 0"),
    ("drop_p=1", ENTRIES, 0, dict(drop_p=1.0), {}, "bad dropout probability"),
    ("null out", ("fwd",), 0, {}, dict(out=None), "null pointer"),
    ("null lse", ENTRIES, 0, {}, dict(lse=None), "null pointer"),
    ("null dq", ("bwd",), 0, {}, dict(dq=None), "null pointer"),
    ("null dbias", ("bias_grad",), 0, {}, dict(dbias=None), "null pointer"),
    ("strided A=Dv=48 at T=64", ("fwd", "bwd"), 1, dict(A=48, Dv=48), {}, "no MFMA instance"),
    ("strided q off by 4 bytes", ("fwd", "bwd"), 1, {}, dict(q=BASE + 4), "q must be 16-byte aligned"),
    ("strided dv off by 4 bytes", ("bwd",), 1, {}, dict(dv=BASE + 4), "dv must be 16-byte aligned"),
    ("strided row stride A+2", ("fwd", "bwd"), 1, dict(row=dict(k=66)), {}, "multiples of 4"),
    ("strided row stride below the width", ENTRIES, 1, dict(row=dict(v=60)), {}, "rows at least 64 apart"),
    ("strided BH % H != 0", ENTRIES, 1, dict(BH=5), {}, "are not items of"),
    ("bias_grad nbias=0", ("bias_grad",), 0, dict(nbias=0), {}, "nbias must be in [1, BH]"),
    ("bias_grad nbias > BH", ("bias_grad",), 0, dict(nbias=5), {}, "nbias must be in [1, BH]"),
    ("bias_grad nbias=65536", ("bias_grad",), 0, dict(BH=131072, nbias=65536), {}, "at most 65535"),
    ("bwd A=300", ("bwd",), 0, dict(A=300), {}, "head dims up to 256"),
]
PARAMS = [pytest.param(e, s, f, p, text, id=f"{e}: {name}") for name, es, s, f, p, text in CASES for e in es]


@pytest.mark.parametrize("entry,strided,fields,ptr,text", PARAMS)
def test_refused_before_any_launch(entry, strided, fields, ptr, text):
    rc = _call(entry, _desc(entry, strided, **fields), ptr)
    err = _lib.lib().adell_last_error().decode()
    assert rc == _lib.E_BADARG, (rc, err)
    assert err.startswith("attention_" + entry) and text in err, err


def test_null_descriptor_is_refused():
    h = _lib.lib()
    assert h.adell_attention_fwd(None, BASE, BASE, BASE, BASE, BASE, None) == _lib.E_BADARG
    assert h.adell_last_error().startswith(b"attention_fwd")


def test_bias_grad_refuses_a_workspace_one_float_short():
    """32 sequences on 2 slices of one 128 x 128 tile each: 16 chunks, the most there are, so the call
    needs all of what adell_attention_bias_grad_workspace_floats answers."""
    d = _desc("bias_grad", 0, BH=32, nbias=2)
    need = _lib.lib().adell_attention_bias_grad_workspace_floats(2, 64)
    assert need == 16 * 2 * 64 * 64
    rc = _call("bias_grad", d, ws_floats=need - 1)
    err = _lib.lib().adell_last_error().decode()
    assert rc == _lib.E_BADARG and err.startswith("attention_bias_grad") and "workspace too small" in err, err
    rc = _call("bias_grad", d, dict(workspace=None))
    assert rc == _lib.E_BADARG and b"workspace too small" in _lib.lib().adell_last_error()


def test_descriptor_mirrors_the_header():
    """Field order and types of include/adell_hip.h, and its size: 72 bytes before the strides."""
    assert [n for n, _ in _lib.AttentionDesc._fields_] == [
        "BH", "H", "T", "A", "Dv", "scale", "drop_p", "rng_offset", "seed", "bias", "labels", "nbias",
        "nlab", "strided", "stride"]
    assert _lib.AttentionDesc.stride.offset == 72 and ctypes.sizeof(_lib.AttentionDesc) == 72 + 8 * 3 * 8


def test_strided_ok_is_the_forward_plan_and_follows_the_switch():
    assert ops.attention_strided_ok(50, 64, 64)
    assert not ops.attention_strided_ok(15, 64, 64) and not ops.attention_strided_ok(50, 64, 48)
    with _lib.tuning(attn_nomfma=1):
        assert not ops.attention_strided_ok(50, 64, 64)
    assert ops.attention_strided_ok(50, 64, 64)
