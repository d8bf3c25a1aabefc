"""CPU: the host side of gradient accumulation -- the config key, the window partition of an epoch, and the argument
checks of the two C-ABI entry points (`dsbdd_train_net_backward_acc`, `dsbdd_train_net_forward_held`)."""
import ctypes

import pytest

from diffsbdd_amd import _lib
from diffsbdd_amd import train as T
from diffsbdd_amd.engine import make_config
from oracle import weights as W

BASE_CFG = dict(dataset="crossdock", datadir="d", mode="pocket_conditioning", batch_size=4, lr=1e-3, n_epochs=1,
                egnn_params={"hidden_nf": 64}, diffusion_params={"diffusion_steps": 20, "diffusion_loss_type": "l2"})


def test_config_accepts_accumulate_grad_batches():
    cfg = T.check_config({**BASE_CFG, "accumulate_grad_batches": 4})
    assert cfg["accumulate_grad_batches"] == 4
    assert T.check_config({**BASE_CFG, "accumulate_grad_batches": 1})["accumulate_grad_batches"] == 1
    assert "accumulate_grad_batches" not in T.check_config(BASE_CFG)          # absent stays absent: today's hyper-parameters


@pytest.mark.parametrize("k", [0, -1, 2.5])
def test_config_refuses_a_window_below_one_or_not_an_integer(k):
    with pytest.raises(ValueError, match="accumulate_grad_batches"):
        T.check_config({**BASE_CFG, "accumulate_grad_batches": k})


def test_more_than_one_gpu_is_refused_and_the_message_names_the_way_out():
    with pytest.raises(NotImplementedError, match="accumulate_grad_batches"):
        T.check_config({**BASE_CFG, "gpus": 4})
    with pytest.raises(NotImplementedError, match="accumulate_grad_batches"):
        T.check_config({**BASE_CFG, "gpus": 2, "accumulate_grad_batches": 2})


@pytest.mark.parametrize("n,k,want", [(7, 3, [3, 3, 1]), (6, 2, [2, 2, 2]), (3, 1, [1, 1, 1]), (2, 5, [2]), (0, 4, [])])
def test_accumulation_windows(n, k, want):
    assert T.accumulation_windows(n, k) == want


def test_accumulation_windows_refuses_an_empty_window():
    with pytest.raises(ValueError):
        T.accumulation_windows(3, 0)


def _hp(cfg):
    keys = ("atom_nf", "residue_nf", "joint_nf", "hidden_nf", "n_layers", "inv_sublayers", "attention", "tanh",
            "update_pocket_coords", "reflection_equivariant", "edge_embedding_dim", "edge_cutoff_ligand", "edge_cutoff_pocket",
            "edge_cutoff_interaction", "norm_constant", "normalization_factor")
    return {k: cfg[k] for k in keys}


def test_c_abi_argument_errors_of_the_accumulating_entry_points():
    """A null handle or a null `accumulate` table returns DSBDD_ERR_ARG with a message; nothing is launched (no GPU here)."""
    lib = _lib.load()
    cfg = make_config(**_hp(W.arch_cfg("small_cond")[0]))
    h = ctypes.c_void_p()
    assert lib.dsbdd_train_net_create(ctypes.byref(cfg), ctypes.byref(h)) == 0
    n = lib.dsbdd_train_net_param_count(h)
    one = ctypes.c_void_p(4096)          # any non-null, never dereferenced on these paths
    ptrs = (ctypes.c_void_p * n)(*([4096] * n))
    flags = (ctypes.c_uint8 * n)()
    graph = _lib.TrainGraph()
    back = (ctypes.byref(graph), ptrs, ptrs, flags, one, 1 << 20, one, 1 << 20, 0, one, one, None, None)
    assert lib.dsbdd_train_net_backward_acc(None, None, *back) == _lib.ERR_ARG
    assert b"handle" in lib.dsbdd_last_error()
    assert lib.dsbdd_train_net_backward_acc(h, None, *back[:3], None, *back[4:]) == _lib.ERR_ARG
    assert b"accumulate" in lib.dsbdd_last_error()
    assert lib.dsbdd_train_net_backward_acc(h, None, *back) == _lib.ERR_ARG       # (the zeroed graph: refused before any launch)
    fwd = (ctypes.byref(graph), ptrs, one, 1 << 20, one, 1 << 20, one, one, one, 1, 1, one, one, one)
    for held in (0, 1):
        assert lib.dsbdd_train_net_forward_held(None, None, *fwd, held) == _lib.ERR_ARG
        assert b"handle" in lib.dsbdd_last_error()
        assert lib.dsbdd_train_net_forward_held(h, None, *fwd, held) == _lib.ERR_ARG
    lib.dsbdd_train_net_destroy(h)
