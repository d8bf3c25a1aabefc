"""CPU: the host side of data-parallel training -- how a window of world * k micro-batches is split over the ranks, what
`check_config` accepts for a given world size, the validation assignment with its ordered float64 sum, the weight
checksum, and the argument checks of `dsbdd_optim_step_ranks` (nothing is launched: no GPU here)."""
import ctypes

import numpy as np
import pytest
import torch

from diffsbdd_amd import _lib
from diffsbdd_amd import train as T

BASE_CFG = dict(dataset="crossdock", datadir="d", mode="pocket_conditioning", batch_size=4, lr=1e-3, n_epochs=1,
                egnn_params={"hidden_nf": 64}, diffusion_params={"diffusion_steps": 20, "diffusion_loss_type": "l2"})


@pytest.mark.parametrize("n,world,k", [(4, 2, 2), (3, 2, 2), (1, 4, 1), (5, 4, 1), (0, 2, 1)])
def test_block_split_of_a_window(n, world, k):
    """n batches are walked in windows of world * k (the last may be shorter); every window is split into blocks of k."""
    batches = list(range(100, 100 + n))
    sizes = T.accumulation_windows(n, world * k)
    assert sum(sizes) == n and all(1 <= s <= world * k for s in sizes)
    if n > world * k:                                   # more than one window holds: refused, not truncated
        with pytest.raises(ValueError):
            T.rank_block(n, world, k, 0)
    seen, start = [], 0
    for m in sizes + [0]:                               # (and the empty window: nobody holds anything)
        window = batches[start:start + m]
        blocks = [T.rank_block(m, world, k, r) for r in range(world)]
        assert all(0 <= lo <= hi <= m and hi - lo <= k for lo, hi in blocks)
        assert [lo for lo, _ in blocks] == [min(r * k, m) for r in range(world)]
        assert sum((window[lo:hi] for lo, hi in blocks), []) == window        # the union, in order, is the window
        holds = [hi > lo for lo, hi in blocks]
        n_ranks = T.contributing_ranks(m, k)
        assert holds == [r < n_ranks for r in range(world)]                  # the ranks that hold a micro-batch are a prefix
        assert n_ranks == sum(holds) and (n_ranks >= 1) == (m >= 1)
        seen += window
        start += m
    assert seen == batches


def test_an_epoch_is_walked_in_windows_of_world_times_k():
    assert T.accumulation_windows(3, 2 * 1) == [2, 1]                         # 3 batches, 2 ranks: rank 1 is empty in the last
    assert [T.rank_block(1, 2, 1, r) for r in range(2)] == [(0, 1), (1, 1)]
    with pytest.raises(ValueError):
        T.rank_block(2, 2, 1, 2)                                              # no such rank


def test_check_config_takes_the_world_size_as_an_argument(monkeypatch):
    monkeypatch.setenv("WORLD_SIZE", "2")                                     # never read from the environment
    assert T.check_config({**BASE_CFG, "gpus": 2}, world=2)["gpus"] == 2
    assert T.check_config({**BASE_CFG, "gpus": 2, "accumulate_grad_batches": 3}, 2)["accumulate_grad_batches"] == 3
    with pytest.raises(NotImplementedError, match="accumulate_grad_batches") as e:
        T.check_config({**BASE_CFG, "gpus": 2}, world=1)
    assert "python -m torch.distributed.run --nproc-per-node 2 -m diffsbdd_amd.train --config" in str(e.value)
    with pytest.raises(NotImplementedError, match="accumulate_grad_batches"):
        T.check_config({**BASE_CFG, "gpus": 2})
    with pytest.raises(ValueError, match="gpus"):
        T.check_config({**BASE_CFG, "gpus": 1}, world=2)
    with pytest.raises(ValueError, match="gpus"):
        T.check_config(BASE_CFG, world=2)                                     # an absent key is gpus: 1
    with pytest.raises(ValueError, match="gpus"):
        T.check_config({**BASE_CFG, "gpus": 4}, world=2)
    with pytest.raises(ValueError):
        T.check_config(BASE_CFG, world=0)
    assert "gpus" not in T.check_config(BASE_CFG)


def test_sample_eval_is_refused_under_ranks_and_the_message_names_the_checkpoint():
    se = {"every_n_epochs": 1, "n_samples": 4}
    assert T.check_config({**BASE_CFG, "sample_eval": se})["sample_eval"] == se
    with pytest.raises(NotImplementedError, match="checkpoint"):
        T.check_config({**BASE_CFG, "gpus": 2, "sample_eval": se}, world=2)


@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_validation_sum_over_the_ranks_is_the_sequential_sum_bit_for_bit(world):
    g = torch.Generator().manual_seed(7)
    per_batch = (torch.randn(11, generator=g, dtype=torch.float64) * 10.0 ** torch.randint(-3, 6, (11,), generator=g)).tolist()
    sequential = torch.zeros((), dtype=torch.float64)
    for v in per_batch:                                                       # `validate` on one GPU
        sequential += torch.tensor(v, dtype=torch.float64)
    vectors = torch.zeros(world, len(per_batch), dtype=torch.float64)
    for b, v in enumerate(per_batch):
        vectors[T.validation_rank(b, world), b] = v
    assert sorted(T.validation_rank(b, world) for b in range(world)) == list(range(world))
    assert int((vectors != 0).sum(0).max()) == 1                              # one owner per batch: the others add +0
    combined = vectors[0].clone()
    for r in range(1, world):                                                 # all_reduce(SUM), in any order: x + 0 is exact
        combined = combined + vectors[r]
    assert combined.tolist() == per_batch
    total = T.ordered_sum(combined.tolist())
    assert np.float64(total).tobytes() == np.float64(float(sequential)).tobytes()
    assert np.float64(T.ordered_sum(sorted(per_batch))).tobytes() != np.float64(total).tobytes()      # (the order matters)


def test_weights_checksum_sees_one_flipped_bit_and_a_swap():
    g = torch.Generator().manual_seed(1)
    a = [torch.randn(5, 3, generator=g), torch.randn(17, generator=g)]
    base = int(T.weights_checksum(a))
    assert int(T.weights_checksum([t.clone() for t in a])) == base
    b = [t.clone() for t in a]
    b[1].view(torch.int32)[4] ^= 1
    assert int(T.weights_checksum(b)) != base
    c = [t.clone() for t in a]
    c[0].view(-1)[[0, 1]] = c[0].view(-1)[[1, 0]]
    assert int(T.weights_checksum(c)) != base
    assert int(T.weights_checksum([torch.zeros(3), -torch.zeros(3)])) != int(T.weights_checksum([torch.zeros(3), torch.zeros(3)]))


def test_c_abi_argument_errors_of_the_rank_step():
    lib = _lib.load()
    cfg = _lib.OptimCfg(1e-3, 0.9, 0.999, 1e-8, 1e-12, 1)
    numel = (ctypes.c_int64 * 2)(5, 8197)
    h = ctypes.c_void_p()
    assert lib.dsbdd_optim_create(ctypes.byref(cfg), 2, numel, ctypes.byref(h)) == 0
    elems = lib.dsbdd_optim_state_elems(h)
    assert elems == 8 + 8200 and lib.dsbdd_optim_state_offset(h, 1) == 8
    base = 1 << 20                                        # never dereferenced on these paths
    grads = (ctypes.c_void_p * 2)(base, base + 4 * 8)
    steps = (ctypes.c_int32 * 2)(1, 1)
    call = lib.dsbdd_optim_step_ranks
    assert call(None, None, base, elems, 2, base, grads, steps, 1e-3) == _lib.ERR_ARG
    assert call(h, None, None, elems, 2, base, grads, steps, 1e-3) == _lib.ERR_ARG
    for n_ranks in (0, -1):
        assert call(h, None, base, elems, n_ranks, base, grads, steps, 1e-3) == _lib.ERR_ARG
        assert b"n_ranks" in lib.dsbdd_last_error()
    assert call(h, None, base, elems - 1, 2, base, grads, steps, 1e-3) == _lib.ERR_ARG
    assert b"rank_stride" in lib.dsbdd_last_error()
    wrong = (ctypes.c_void_p * 2)(base, base + 4 * 5)     # not the region of out_flat
    assert call(h, None, base, elems, 2, base, wrong, steps, 1e-3) == _lib.ERR_ARG
    assert b"out_flat" in lib.dsbdd_last_error()
    assert call(h, None, base, elems, 2, base, grads, steps, 1e-3) == _lib.ERR_STATE      # well-formed, but nothing is bound
    lib.dsbdd_optim_destroy(h)
