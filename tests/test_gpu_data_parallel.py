"""GPU: data-parallel ranks over the ordered gradient-bucket reduce.

1. `ClippedAdamW.step_ranks` (dsbdd_optim_step_ranks: optim_reduce_norm_kernel + the unchanged update launch) against
   torch's ordered in-place adds into a bucket followed by `step()`: bit for bit, no tolerance anywhere.
2. Two Trainers as the two ranks of one window in ONE process (local_window on each, apply_window on both) against one
   Trainer with accumulate_grad_batches = 2: bit for bit.
3. k = 2 on two ranks: bit for bit "each rank's sequential sum, then rank order"; against accumulate_grad_batches = 4 it
   is another association of the same float32 sum and is held to the rule of tests/test_gpu_trainer.py (error <= 2 x
   the float32 reference's own error against float64, floor 4 ulp, never above 1e-4).
4. Ranks as processes: two on the one GPU over gloo against one process with accumulate_grad_batches = 2, and one rank on
   nccl (the device-side all_gather) against the plain run: the files they leave are equal, tensor by tensor."""
import json
import os
import shutil
import socket
import subprocess
import sys
from argparse import Namespace

import numpy as np
import pytest
import torch

from tests._golden import GOLDEN_DIR
from tests.test_gpu_accumulate import acc_config, epoch_batches, trainer, window_by_hand
from tests.test_gpu_trainer import HIST, ULP4, _same, _state, complexes, dev, ref_step, small_config

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SIZES = [1, 3, 255, 8192, 8197, 20_000, 7]       # a chunk is 8192 elements; the last tensor has no gradient
MANY = [5] * 205                                 # a launch takes 200 tensors


# ---- 1. the kernel ---------------------------------------------------------------------------------------------------------
def _optimizer(sizes, seed, clip):
    from diffsbdd_amd.optim import ClippedAdamW
    g = torch.Generator().manual_seed(seed)
    params = [torch.nn.Parameter(torch.randn(n, generator=g).to(dev())) for n in sizes]
    opt = ClippedAdamW(params, lr=1e-2, clip_grad=clip)
    if clip:
        opt.set_queue([2.0, 2.5])                 # far below the norms: every step clips, the norm's bits reach the weights
    return params, opt


def _nan_equal(a, b):
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))


@pytest.mark.parametrize("variant", ["plain", "no_clip", "alias", "odd_stride"])
@pytest.mark.parametrize("n_ranks", [1, 2, 3, 8])
def test_step_ranks_is_the_ordered_torch_sum_then_step_bit_for_bit(n_ranks, variant):
    """`alias`: out_flat IS rank 0's slot of the gathered buffer.  `odd_stride`: the ranks' slots are not 16 bytes apart
    (the kernel's scalar loads, same element order)."""
    clip = variant != "no_clip"
    for sizes, no_grad in ((SIZES, {len(SIZES) - 1}), (MANY, set())):
        pa, a = _optimizer(sizes, 11, clip)
        pb, b = _optimizer(sizes, 11, clip)
        elems = int(a.lib.dsbdd_optim_state_elems(a._h))
        stride = elems + (5 if variant == "odd_stride" else 8)
        gathered = torch.empty(n_ranks, stride, device=dev())
        bucket_a = a.gradient_bucket(flat=gathered[0, :elems]) if variant == "alias" else a.gradient_bucket()
        bucket_b = b.gradient_bucket()
        assert (bucket_a.flat.data_ptr() == gathered.data_ptr()) == (variant == "alias")
        gen = torch.Generator().manual_seed(100 + n_ranks)
        reversed_differs = False
        for step in range(3):
            gathered.fill_(float("nan"))          # padding, the tail and the tensor without a gradient: NaN in every rank
            for r in range(n_ranks):
                for i, p in enumerate(pa):
                    if i not in no_grad:
                        o = a._offsets[i]
                        gathered[r, o:o + p.numel()] = (torch.randn(p.numel(), generator=gen) * 10.0 ** (r % 3)).to(dev())
            before = gathered.clone()
            # expected: torch's ordered in-place adds into the other optimiser's bucket, then the existing step()
            bucket_b.flat.fill_(float("nan"))
            for i, p in enumerate(pb):
                if i in no_grad:
                    p.grad = None
                    continue
                o, view = b._offsets[i], bucket_b.view(p)
                view.copy_(before[0, o:o + p.numel()])
                for r in range(1, n_ranks):
                    view.add_(before[r, o:o + p.numel()])
                p.grad = view
                back = before[n_ranks - 1, o:o + p.numel()].clone()
                for r in range(n_ranks - 2, -1, -1):
                    back.add_(before[r, o:o + p.numel()])
                reversed_differs |= not torch.equal(back, view)
            b.step()
            # the fused launch
            if variant != "alias":
                bucket_a.flat.fill_(float("nan"))
            for i, p in enumerate(pa):
                p.grad = None if i in no_grad else bucket_a.view(p)
            a.step_ranks(gathered, n_ranks)
            torch.cuda.synchronize()
            assert _nan_equal(bucket_a.flat, bucket_b.flat)                      # the reduced bucket; NaN where nothing is written
            if variant == "alias":
                assert _nan_equal(gathered[1:], before[1:]) and _nan_equal(gathered[0, elems:], before[0, elems:])
            else:
                assert _nan_equal(gathered, before)                              # the inputs are only read
            for i, (p, q) in enumerate(zip(pa, pb)):
                assert torch.equal(p, q), (step, i)
                if i in no_grad:
                    assert p not in a.state and q not in b.state
                    continue
                for key in ("exp_avg", "exp_avg_sq", "max_exp_avg_sq"):
                    assert torch.equal(a.state[p][key], b.state[q][key]), (step, i, key)
            assert a.clip_report() == b.clip_report()
            assert a.state_dict()["state"].keys() == b.state_dict()["state"].keys()
        # not vacuous: the order of the sum is visible in the bits (a + b == b + a, so only from three ranks on)
        assert reversed_differs == (n_ranks >= 3)
        if clip:
            rep = a.clip_report()
            assert rep["steps"] == 3 and np.isfinite(rep["last_norm"]) and rep["last_norm"] > 0
        for i in no_grad:
            assert torch.equal(pa[i].detach().cpu(), _optimizer(sizes, 11, clip)[0][i].detach().cpu())     # untouched


def test_step_ranks_refuses_a_gradient_outside_the_bucket():
    params, opt = _optimizer([5, 9], 3, True)
    elems = int(opt.lib.dsbdd_optim_state_elems(opt._h))
    gathered = torch.zeros(2, elems, device=dev())
    params[0].grad = torch.zeros(5, device=dev())
    with pytest.raises(ValueError, match="bucket"):
        opt.step_ranks(gathered, 2)
    params[0].grad = None
    with pytest.raises(ValueError, match="n_ranks"):
        opt.step_ranks(gathered, 3)
    with pytest.raises(TypeError):
        opt.step_ranks(gathered[:, :elems - 1], 2)


# ---- 2 / 3. the two halves of a window, ranks in one process -----------------------------------------------------------------
def rank_trainer(arch, tmp, rank, world, k):
    from diffsbdd_amd import train as T
    cfg = acc_config(arch, tmp, k)
    cfg["gpus"] = world
    return T.Trainer(cfg, HIST, complexes(), None, device=dev(), world=world, rank=rank)


def window_on_ranks(ranks, window, first_micro_step, k):
    """One window through the public halves, the exchange replaced by a stack of the ranks' buckets."""
    from diffsbdd_amd import train as T
    world, n = len(ranks), len(window)
    halves = []
    for tr in ranks:
        lo, hi = T.rank_block(n, world, k, tr.rank)
        halves.append(tr.local_window(window[lo:hi], first_micro_step + lo))
    n_ranks = T.contributing_ranks(n, k)
    assert all(flags == halves[0][1] for _, flags in halves[:n_ranks])            # contributing ranks agree
    assert all(not any(flags) for _, flags in halves[n_ranks:])
    gathered = torch.stack([tr.optimizer.gradient_bucket().flat for tr in ranks])
    losses = [loss for loss, _ in halves]
    out = [tr.apply_window(gathered, n_ranks, losses, flags=None if tr.rank < n_ranks else halves[0][1]) for tr in ranks]
    for tr in ranks:
        tr.micro_step = first_micro_step + n
    return out


@pytest.mark.parametrize("arch", ["small_cond", "small_joint"])
def test_two_ranks_in_one_process_are_one_gpu_accumulating_two(arch, tmp_path):
    ranks = [rank_trainer(arch, tmp_path / f"r{r}", r, 2, 1) for r in range(2)]
    single = trainer(arch, tmp_path / "s", 2)
    micro = 0
    for epoch in range(2):                                  # 3 batches per epoch: windows [2, 1], rank 1 empty in the second
        batches = epoch_batches(single, epoch)
        assert len(batches) == 3
        for window in (batches[0:2], batches[2:3]):
            got = window_on_ranks(ranks, window, micro, 1)
            want = single.training_window(window)
            micro += len(window)
            assert torch.equal(got[0], want) and torch.equal(got[1], want) and bool(torch.isfinite(want))
    assert single.global_step == 4 and single.micro_step == micro == 6
    _same(_state(ranks[0]), _state(ranks[1]))
    _same(_state(ranks[0]), _state(single))
    logged = [torch.stack([v for _, v in tr._pending]) for tr in (*ranks, single)]
    assert torch.equal(logged[0], logged[2]) and torch.equal(logged[1], logged[2]) and logged[2].numel() == 4
    assert ranks[0].optimizer.clip_report() == single.optimizer.clip_report()
    if arch == "small_cond":                                # the residue decoder has no gradient on any rank
        assert any(p not in ranks[1].optimizer.state for p in ranks[1].params)


def test_two_ranks_accumulating_two_are_the_rank_sums_in_rank_order(tmp_path):
    arch = "small_cond"
    ranks = [rank_trainer(arch, tmp_path / f"r{r}", r, 2, 2) for r in range(2)]
    hand, four = trainer(arch, tmp_path / "h", 4), trainer(arch, tmp_path / "f", 4)
    batches = epoch_batches(hand, 0) + epoch_batches(hand, 1)[:1]
    p0 = [p.detach().clone() for p in hand.params]
    queue0 = hand.optimizer.clip_report()["queue"]
    got = window_on_ranks(ranks, batches, 0, 2)
    # by hand: each rank's sequential sum (micro-steps 0, 1 and 2, 3; every loss / 4), then rank order
    g0, l0 = window_by_hand(hand, batches[0:2], 4, step=False)
    g1, l1 = window_by_hand(hand, batches[2:4], 4, step=False)
    assert hand.micro_step == 4
    for p, a, b in zip(hand.params, g0, g1):
        assert (a is None) == (b is None)
        p.grad = None if a is None else a + b
    hand.optimizer.step()
    hand.optimizer.zero_grad(set_to_none=True)
    hand.global_step += 1
    _same(_state(ranks[0]), _state(hand))
    _same(_state(ranks[1]), _state(hand))
    assert torch.equal(got[0], l0 + l1) and torch.equal(got[1], l0 + l1)
    # against accumulate_grad_batches = 4, ((g0 + g1) + g2) + g3: the rule of test_one_window_is_the_pieces_written_out...
    grads4, _ = window_by_hand(four, batches, 4, step=False)
    r32 = ref_step(p0, grads4, None, queue0, torch.float32)
    r64 = ref_step(p0, grads4, None, queue0, torch.float64)
    worst = (0.0, 0.0)
    for i, p in enumerate(ranks[0].params):
        if grads4[i] is None:
            assert torch.equal(p.detach(), p0[i])
            continue
        hip, a64, a32 = (v.detach().double().cpu() for v in (p, r64[0][i], r32[0][i]))
        mag = float(a64.abs().max())
        e_ref, e = float((a32 - a64).abs().max()) / mag, float((hip - a64).abs().max()) / mag
        worst = (max(worst[0], e_ref), max(worst[1], e))
        assert e <= max(2 * e_ref, ULP4) and e <= 1e-4, (i, e, e_ref)
    print(f"  two ranks x 2 against one window of 4: worst err_ref {worst[0]:.3e}  ranks {worst[1]:.3e}")


def test_resume_under_another_window_size_only_at_an_epoch_boundary(tmp_path):
    from diffsbdd_amd import train as T
    ds = complexes()
    tr = trainer("small_cond", tmp_path, 2)
    tr.fit(max_steps=1)
    assert (tr.epoch, tr.batch_in_epoch) == (0, 2)
    inside = shutil.copy(tr.save_checkpoint(), str(tmp_path / "inside.ckpt"))
    tr.fit(max_steps=2)
    assert (tr.epoch, tr.batch_in_epoch) == (1, 0)
    boundary = tr.save_checkpoint()
    with torch.serialization.safe_globals([Namespace]):
        assert torch.load(boundary, map_location="cpu", weights_only=True)["world"] == 1
    with pytest.raises(ValueError, match="epoch"):
        T.Trainer.resume(inside, ds, None, device=dev(), overrides={"accumulate_grad_batches": 3})
    with pytest.raises(ValueError, match="epoch"):                        # two ranks x 2 are windows of 4, not of 2
        T.Trainer.resume(inside, ds, None, device=dev(), world=2, rank=1)
    same = T.Trainer.resume(inside, ds, None, device=dev(), overrides={"accumulate_grad_batches": 1}, world=2, rank=0)
    assert (same.world, same.accumulate, same.batch_in_epoch, same.cfg["gpus"]) == (2, 1, 2, 2)      # 2 x 1 = 1 x 2
    other = T.Trainer.resume(boundary, ds, None, device=dev(), overrides={"accumulate_grad_batches": 3})
    assert (other.accumulate, other.epoch, other.batch_in_epoch, other.global_step) == (3, 1, 0, 2)
    _same(_state(other), _state(tr))


# ---- 4. ranks as processes ---------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def _write_run(tmp, name, **keys):
    import yaml
    data = tmp / "data"
    if not data.is_dir():
        data.mkdir()
        for split in ("train", "val"):
            shutil.copy(os.path.join(GOLDEN_DIR, "trainer_complexes.npz"), data / (split + ".npz"))
        np.save(data / "size_distribution.npy", HIST)
    cfg = small_config(tmp=tmp)
    cfg.update(datadir=str(data), logdir=str(tmp / name), log_every=1, **keys)
    path = tmp / (name + ".yml")
    path.write_text(yaml.safe_dump(cfg))
    return path, tmp / name / "run"


def _train(config, ranks=None, backend=None):
    """`python -m diffsbdd_amd.train --max-steps 3` as one plain process, or as `ranks` ranks under torch.distributed.run."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env.update(HSA_ENABLE_IPC_MODE_LEGACY="0", MASTER_ADDR="127.0.0.1")
    tail = ["-m", "diffsbdd_amd.train", "--config", str(config), "--device", "cuda:0", "--max-steps", "3"]
    if ranks is None:
        cmd = [sys.executable] + tail
    else:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(ranks), "--master-addr",
               "127.0.0.1", "--master-port", str(_free_port())] + tail + ["--backend", backend]
    run = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-3000:]          # (a failed run ends the test: nothing is started after it)
    return run


def _same_files(run_a, run_b):
    with torch.serialization.safe_globals([Namespace]):
        a, b = (torch.load(d / "checkpoints" / "last.ckpt", map_location="cpu", weights_only=True) for d in (run_a, run_b))
    assert a["global_step"] == b["global_step"] == 3 and a["micro_step"] == b["micro_step"] and a["epoch"] == b["epoch"] == 1
    assert a["clip_queue"] == b["clip_queue"] and a["batch_in_epoch"] == b["batch_in_epoch"]
    assert a["state_dict"].keys() == b["state_dict"].keys()
    for k, v in a["state_dict"].items():
        assert torch.equal(v, b["state_dict"][k]), k
    sa, sb = a["optimizer_states"][0]["state"], b["optimizer_states"][0]["state"]
    assert sa.keys() == sb.keys() and len(sa) > 0
    for i in sa:
        assert all(torch.equal(torch.as_tensor(sa[i][k]), torch.as_tensor(sb[i][k])) for k in sa[i]), i
    rows_a, rows_b = ([json.loads(line) for line in open(d / "metrics.jsonl")] for d in (run_a, run_b))
    train_a, train_b = ([(r["step"], r["loss/train"]) for r in rows if "loss/train" in r] for rows in (rows_a, rows_b))
    assert train_a == train_b and [s for s, _ in train_a] == [1, 2, 3]          # one row per step: rank 0 alone wrote them
    val_a, val_b = ([r["loss/val"] for r in rows if "loss/val" in r] for rows in (rows_a, rows_b))
    assert val_a == val_b and len(val_a) == 1 and np.isfinite(val_a[0])
    return a, b


def test_two_ranks_on_one_gpu_over_gloo_leave_the_files_of_one_gpu_accumulating_two(tmp_path):
    one_cfg, one_dir = _write_run(tmp_path, "one", gpus=1, accumulate_grad_batches=2)
    two_cfg, two_dir = _write_run(tmp_path, "two", gpus=2)
    _train(one_cfg)
    run = _train(two_cfg, ranks=2, backend="gloo")
    a, b = _same_files(two_dir, one_dir)
    assert a["world"] == 2 and b["world"] == 1 and a["micro_step"] == 5
    assert sorted(f.name for f in two_dir.iterdir()) == ["checkpoints", "metrics.jsonl"]
    assert sorted(f.name for f in (two_dir / "checkpoints").iterdir()) == sorted(f.name for f in (one_dir / "checkpoints").iterdir())
    summaries = [line for line in run.stdout.splitlines() if line.startswith("{")]
    assert len(summaries) == 1 and json.loads(summaries[0])["global_step"] == 3   # rank 0 alone reports


def test_one_rank_on_nccl_is_the_plain_run(tmp_path):
    """The device-side all_gather (RCCL) with a one-rank communicator: `--backend nccl` makes a single rank run the
    exchange, the bucket window and step_ranks."""
    plain_cfg, plain_dir = _write_run(tmp_path, "plain", gpus=1)
    rank_cfg, rank_dir = _write_run(tmp_path, "rank", gpus=1)
    _train(plain_cfg)
    _train(rank_cfg, ranks=1, backend="nccl")
    a, b = _same_files(rank_dir, plain_dir)
    assert a["world"] == b["world"] == 1 and a["micro_step"] == 3
