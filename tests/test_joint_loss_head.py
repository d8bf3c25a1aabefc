"""Host side of the joint model's loss head (csrc/loss_head.h loss_joint_*; diffsbdd_amd/loss_head.py joint_forward):
the C ABI exists with the binding's signatures, the output row count matches what the binding unbinds, and bad arguments
are refused before anything is launched.  No GPU needed."""
import ctypes as C
import inspect
import re

from diffsbdd_amd import _lib, loss_head

NEW = ("dsbdd_loss_joint_out_rows", "dsbdd_loss_joint_pre", "dsbdd_loss_joint_post", "dsbdd_loss_joint_post_backward")


def _cfg(**kw):
    base = dict(batch=2, n_lig=5, n_pocket=9, atom_nf=10, residue_nf=10, timesteps=20, remove_com=0, vnode_idx=-1,
                norm_value_x=5.0, norm_value_h=5.0, norm_bias_h=0.0, n1_tab=0, n2_tab=0)
    base.update(kw)
    return _lib.LossCfg(**base)


def test_joint_entry_points_exist_with_the_binding_signatures():
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.SIGNATURES, name
        fn = getattr(lib, name)
        res, args = _lib.SIGNATURES[name]
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    # stream, cfg, then the pointer arguments of include/diffsbdd_hip.h
    assert len(_lib.SIGNATURES["dsbdd_loss_joint_pre"][1]) == 2 + 20
    assert len(_lib.SIGNATURES["dsbdd_loss_joint_post"][1]) == 2 + 10
    assert len(_lib.SIGNATURES["dsbdd_loss_joint_post_backward"][1]) == 2 + 14


def test_out_rows_equal_what_joint_forward_unbinds():
    lib = _lib.load()
    rows = lib.dsbdd_loss_joint_out_rows()
    src = inspect.getsource(loss_head._JointPost.forward)
    m = re.search(r"^\s*(.+?) = out\.unbind\(0\)", src, re.M)
    assert m, "the Function unbinds the kernel's output rows"
    assert rows == len(m.group(1).split(",")) == 8
    # the per-sample rows before the network call are the conditional head's layout
    src = inspect.getsource(loss_head.joint_forward)
    m = re.search(r"^\s*\((.+?)\) = ps\.unbind\(0\)", src, re.M)
    assert m and lib.dsbdd_loss_rows() == len(m.group(1).split(","))


def test_null_and_bad_arguments_are_refused_before_any_launch():
    lib = _lib.load()
    ok = _cfg()
    one = C.c_void_p(1).value           # never dereferenced: the argument checks come first
    # null config, batch < 1
    assert lib.dsbdd_loss_joint_pre(None, None, *([None] * 20)) == _lib.ERR_ARG
    assert lib.dsbdd_loss_joint_post(None, None, *([None] * 10)) == _lib.ERR_ARG
    assert lib.dsbdd_loss_joint_post_backward(None, None, *([None] * 14)) == _lib.ERR_ARG
    bad = _cfg(batch=0)
    assert lib.dsbdd_loss_joint_pre(None, C.byref(bad), *([one] * 20)) == _lib.ERR_ARG
    assert lib.dsbdd_loss_joint_post(None, C.byref(bad), *([one] * 10)) == _lib.ERR_ARG
    assert lib.dsbdd_loss_joint_post_backward(None, C.byref(bad), *([one] * 14)) == _lib.ERR_ARG
    # every required pointer, one at a time (pre: the table [10] and the normalised batch [16:20] are optional)
    for i in range(20):
        if i == 10 or i >= 16:
            continue
        args = [one] * 20
        args[10] = None
        args[i] = None
        assert lib.dsbdd_loss_joint_pre(None, C.byref(ok), *args) == _lib.ERR_ARG, i
    for i in range(10):
        args = [one] * 10
        args[i] = None
        assert lib.dsbdd_loss_joint_post(None, C.byref(ok), *args) == _lib.ERR_ARG, i
    for i in range(14):
        if 7 <= i <= 11:                  # the five incoming gradients may each be absent
            continue
        args = [one] * 14
        args[i] = None
        assert lib.dsbdd_loss_joint_post_backward(None, C.byref(ok), *args) == _lib.ERR_ARG, i
    # a table without its shape
    args = [one] * 20
    assert lib.dsbdd_loss_joint_pre(None, C.byref(ok), *args) == _lib.ERR_ARG
    assert b"argument" in lib.dsbdd_last_error()
