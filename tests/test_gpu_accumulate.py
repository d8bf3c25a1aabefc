"""GPU: gradient accumulation into the optimiser's flat gradient bucket.

The accumulating stores of `dsbdd_train_net_backward_acc` must give `(g1 + g2) + g3` BIT FOR BIT, where g_i is what the
overwriting backward writes for micro-batch i and the sums are torch's float32 adds: the kernels form the complete new
gradient first and add the old value last with one rounding, so there is no tolerance in cases 1 - 4 and 6 - 9.  Case 5
holds the optimiser step on the accumulated gradient to the rule of tests/test_gpu_trainer.py: error <= 2 x the float32
reference's own error against float64, floor 4 ulp, never above 1e-4."""
import contextlib
import copy
import ctypes as C
import functools
import json
import os
import shutil

import numpy as np
import pytest
import torch

from oracle import weights as W
from tests.test_gpu_train import dev, make_dynamics, problem
from tests.test_gpu_trainer import HIST, ULP4, _same, _state, complexes, ref_step, small_config, within

pytestmark = pytest.mark.gpu

SMALL = ([5, 7, 6], [40, 35, 38])
WIDE = ([23] * 2, [286] * 2)            # H = 256: split-K weight gradients with many chunks
SHAPES = {"small_cond": SMALL, "small_joint": SMALL, "small_variant": SMALL, "crossdock_fullatom_cond": WIDE}
SEEDS = (41, 42, 43)


@contextlib.contextmanager
def env(name, value):
    old = os.environ.get(name)
    os.environ[name] = value
    try:
        yield
    finally:
        if old is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = old


def module(arch):
    cfg, _ = W.arch_cfg(arch)
    m = make_dynamics(cfg, copy.deepcopy(W.random_state_dict(cfg, seed=1)))
    m.train(True)
    return cfg, m


@functools.lru_cache(maxsize=None)
def micro_batches(arch):
    cfg, _ = W.arch_cfg(arch)
    out = []
    for seed in SEEDS:
        xl, xp, t, ml, mp = problem(cfg, *SHAPES[arch], seed=seed)
        gen = torch.Generator().manual_seed(seed + 100)
        wl, wp = torch.randn(xl.shape, generator=gen), torch.randn(xp.shape, generator=gen)
        out.append(tuple(v.to(dev()) for v in (xl, xp, t, ml, mp, wl, wp)))
    return out


def backward(m, mb, loss):
    xl, xp, t, ml, mp, wl, wp = mb
    o_l, o_p = m(xl, xp, t, ml, mp)
    total = (o_l * wl).sum()
    if loss == "both":
        total = total + (o_p * wp).sum()
    total.backward()


@functools.lru_cache(maxsize=None)
def expected(arch, loss):
    """(g1 + g2) + g3 per parameter name through the EXISTING path (fresh gradient tensors, one micro-batch at a time);
    None where the loss reaches no gradient.  Computed once per case and only read afterwards."""
    _, m = module(arch)
    per = []
    for mb in micro_batches(arch):
        m.zero_grad(set_to_none=True)
        backward(m, mb, loss)
        per.append({n: None if p.grad is None else p.grad.detach().clone() for n, p in m.named_parameters()})
    out = {}
    for n in per[0]:
        gs = [g[n] for g in per]
        assert all(g is None for g in gs) or all(g is not None for g in gs), n
        out[n] = None if gs[0] is None else (gs[0] + gs[1]) + gs[2]
    return out


def bucket_of(m):
    from diffsbdd_amd.optim import ClippedAdamW
    opt = ClippedAdamW(list(m.parameters()))
    bucket = opt.gradient_bucket()
    assert opt.gradient_bucket() is bucket                       # created once
    assert bucket.flat.dtype == torch.float32 and bucket.flat.dim() == 1
    assert bucket.flat.numel() == int(opt.lib.dsbdd_optim_state_elems(opt._h))
    for i, p in enumerate(opt._params):
        off = int(opt.lib.dsbdd_optim_state_offset(opt._h, i))
        assert bucket.view(p).data_ptr() == bucket.flat.data_ptr() + 4 * off and bucket.view(p).shape == p.shape
    return opt, bucket


def window(m, bucket, arch, loss):
    from diffsbdd_amd.train_net import accumulating
    m.zero_grad(set_to_none=True)
    with accumulating(m, bucket) as win:
        for mb in micro_batches(arch):
            backward(m, mb, loss)
    return win


def check_window(m, bucket, arch, loss):
    want = expected(arch, loss)
    for n, p in m.named_parameters():
        if want[n] is None:
            assert p.grad is None, n
            assert bool(torch.isnan(bucket.view(p)).all()), n
        else:
            got = bucket.view(p)
            assert bool(torch.isfinite(got).all()), n                  # the window's first write overwrote the NaNs
            assert torch.equal(got, want[n]), (n, (got - want[n]).abs().max().item())
            assert p.grad is not None and p.grad.data_ptr() == got.data_ptr() and p.grad.shape == p.shape, n


# ---- 1. the accumulating stores ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch,loss", [("small_cond", "both"), ("small_joint", "both"), ("small_variant", "both"),
                                       ("crossdock_fullatom_cond", "both"), ("small_cond", "ligand_only")])
def test_accumulating_stores_are_the_torch_sum_bit_for_bit(arch, loss):
    """`ligand_only`: the loss ignores eps_pocket as the pocket-conditioned training loss does -- residue_decoder.* has no
    gradient, keeps `p.grad is None` and its bucket region is never written."""
    _, m = module(arch)
    opt, bucket = bucket_of(m)
    bucket.flat.fill_(float("nan"))
    win = window(m, bucket, arch, loss)
    assert (win.forwards, win.held, win.backwards) == (3, 2, 3)
    check_window(m, bucket, arch, loss)
    n_none = sum(v is None for v in expected(arch, loss).values())
    assert (n_none > 0) == (loss == "ligand_only")
    window(m, bucket, arch, loss)                                        # a second window, the bucket NOT cleared
    check_window(m, bucket, arch, loss)


# ---- 2. side streams -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch", ["small_joint", "crossdock_fullatom_cond"])
def test_accumulating_stores_keep_the_bits_on_the_side_streams(arch):
    flats = []
    for mask in ("0", "7", "15"):
        with env("DSBDD_TRAIN_STREAMS", mask):
            _, m = module(arch)                                          # a new module: a new handle, created under this mask
            opt, bucket = bucket_of(m)
            for rep in range(3):
                bucket.flat.fill_(float("nan"))
                window(m, bucket, arch, "both")
                check_window(m, bucket, arch, "both")
                flats.append(bucket.flat.clone())
    for f in flats[1:]:
        assert torch.equal(torch.nan_to_num(f, nan=-1.0), torch.nan_to_num(flats[0], nan=-1.0))     # (padding stays NaN)


# ---- 3. the held pack ----------------------------------------------------------------------------------------------------
def test_held_pack_is_the_fresh_pack_and_does_not_outlive_the_window():
    from diffsbdd_amd import _lib
    from diffsbdd_amd.train_hip import TrainGraph, _stream
    from diffsbdd_amd.train_net import _net_of, _ptr_table, accumulating
    arch = "small_cond"
    _, m = module(arch)
    opt, bucket = bucket_of(m)
    mbs = micro_batches(arch)
    xl, xp, t, ml, mp = mbs[1][:5]
    plain = [o.detach().clone() for o in m(xl, xp, t, ml, mp)]
    with accumulating(m, bucket) as win:
        m(*mbs[0][:5])
        second = [o.detach().clone() for o in m(xl, xp, t, ml, mp)]
    assert (win.forwards, win.held) == (2, 1)
    assert torch.equal(second[0], plain[0]) and torch.equal(second[1], plain[1])
    with torch.no_grad():
        m.egnn.embedding.weight.mul_(1.5)
    after = m(xl, xp, t, ml, mp)
    assert not torch.equal(after[0].detach(), plain[0])                  # outside a window every forward re-packs
    with accumulating(m, bucket) as win:                                 # and so does the first forward of the next window
        again = m(xl, xp, t, ml, mp)
    assert win.held == 0 and torch.equal(again[0].detach(), after[0].detach())
    # the C-ABI refuses to reuse the pack for other tensors
    net = _net_of(m)
    named = dict(m.named_parameters())
    ps = [named[n].detach() for n in net.names]
    x = torch.cat((xl[:, :3], xp[:, :3]), 0).contiguous()
    g = TrainGraph(m, ml, mp, x, batch=int(t.numel()))
    ws = torch.empty(int(net.lib.dsbdd_train_net_workspace_bytes(net.handle, C.byref(g.c))), dtype=torch.uint8, device=dev())
    pack = net.pack_for(dev())
    eps_l, eps_p = torch.empty_like(xl), torch.empty_like(xp)
    status = torch.zeros(1, dtype=torch.int32, device=dev())
    tt = t.reshape(-1).contiguous()

    def call(params, held):
        return net.lib.dsbdd_train_net_forward_held(
            net.handle, _stream(dev()), C.byref(g.c), _ptr_table(params), pack.data_ptr(), pack.numel(), ws.data_ptr(), ws.numel(),
            xl.data_ptr(), xp.data_ptr(), tt.data_ptr(), tt.numel(), 1, eps_l.data_ptr(), eps_p.data_ptr(), status.data_ptr(), held)
    assert call(ps, 1) == 0
    assert torch.equal(eps_l, after[0].detach())
    other = list(ps)
    other[3] = ps[3].clone()
    assert call(other, 1) == _lib.ERR_STATE
    assert b"pack" in net.lib.dsbdd_last_error()
    torch.cuda.synchronize()


# ---- 4 - 9. the trainer --------------------------------------------------------------------------------------------------
def acc_config(arch, tmp, k):
    cfg = small_config(arch, tmp)
    if k is not None:
        cfg["accumulate_grad_batches"] = k
    return cfg


def trainer(arch, tmp, k, optimizer="hip"):
    from diffsbdd_amd import train as T
    return T.Trainer(acc_config(arch, tmp, k), HIST, complexes(), None, device=dev(), optimizer=optimizer)


def epoch_batches(tr, epoch):
    from diffsbdd_amd.dataset import epoch_permutation
    order = epoch_permutation(len(tr.train_set), tr.seed, epoch).tolist()
    bs = int(tr.cfg["batch_size"])
    return [tr.train_set.collate(order[i:i + bs]) for i in range(0, len(order), bs)]


def window_by_hand(tr, batches, k, step=True):
    """One window from the pieces: every micro-batch keyed by the micro-step counter, nll.mean(0) / k through the EXISTING
    backward (fresh gradient tensors), the gradients summed by torch in micro-batch order, one optimiser step.
    -> (the accumulated gradients, the sum of the scaled losses)"""
    tr.ddpm.train()
    total, losses = None, None
    for data in batches:
        tr.optimizer.zero_grad(set_to_none=True)
        tr._key_step(tr.micro_step)
        nll, _ = tr.forward(data)
        loss = nll.mean(0) / k
        loss.backward()
        tr.micro_step += 1
        gs = [None if p.grad is None else p.grad.detach().clone() for p in tr.params]
        total = gs if total is None else [a if b is None else a + b for a, b in zip(total, gs)]
        losses = loss.detach() if losses is None else losses + loss.detach()
    if step:
        for p, g in zip(tr.params, total):
            p.grad = g
        tr.optimizer.step()
        tr.optimizer.zero_grad(set_to_none=True)
        tr.global_step += 1
    return total, losses


@pytest.mark.parametrize("arch", ["small_cond", "small_joint"])
def test_one_window_is_the_pieces_written_out_and_agrees_with_float64(arch, tmp_path):
    tr, other = trainer(arch, tmp_path / "a", 3), trainer(arch, tmp_path / "b", 3)
    batches = epoch_batches(tr, 0)
    assert len(batches) == 3
    p0 = [p.detach().clone() for p in tr.params]
    queue0 = tr.optimizer.clip_report()["queue"]
    loss = tr.training_window(batches)
    grads, loss_hand = window_by_hand(other, batches, 3)
    assert tr.global_step == 1 and tr.micro_step == 3 and other.micro_step == 3
    _same(_state(tr), _state(other))
    assert torch.equal(loss, loss_hand) and bool(torch.isfinite(loss))
    assert tr.optimizer.clip_report() == other.optimizer.clip_report()
    no_grad = [n for (n, p), g in zip(((n, p) for n, p in tr.ddpm.named_parameters() if p.requires_grad), grads) if g is None]
    if arch == "small_cond":
        assert no_grad and all("residue_decoder" in n for n in no_grad)
        assert all(p not in tr.optimizer.state for p, g in zip(tr.params, grads) if g is None)
    else:
        assert not no_grad
    # 5: the step on the accumulated float32 gradient against torch's AdamW + the restated clipping in float32 / float64
    r32 = ref_step(p0, grads, None, queue0, torch.float32)
    r64 = ref_step(p0, grads, None, queue0, torch.float64)
    worst = (0.0, 0.0)
    for i, p in enumerate(tr.params):
        if grads[i] is None:
            assert torch.equal(p.detach(), p0[i])
            continue
        hip, a64, a32 = (v.detach().double().cpu() for v in (p, r64[0][i], r32[0][i]))
        mag = float(a64.abs().max())
        e_ref, e = float((a32 - a64).abs().max()) / mag, float((hip - a64).abs().max()) / mag
        worst = (max(worst[0], e_ref), max(worst[1], e))
        assert e <= max(2 * e_ref, ULP4) and e <= 1e-4, (i, e, e_ref)
    print(f"  {arch} window of 3: worst err_ref {worst[0]:.3e}  hip {worst[1]:.3e}")
    within("queue", np.array(tr.optimizer.clip_report()["queue"]), np.array(r64[2].items), np.array(r32[2].items))


def test_fit_steps_on_a_short_last_window(tmp_path):
    tr, other = trainer("small_cond", tmp_path / "a", 2), trainer("small_cond", tmp_path / "b", 2)
    tr.fit(max_steps=4)
    assert (tr.global_step, tr.micro_step, tr.epoch, tr.batch_in_epoch) == (4, 6, 2, 0)
    rows = [json.loads(line) for line in open(tr.metrics_path)]
    assert [r["step"] for r in rows] == [2, 4]                 # log_every = 2; the epoch's end has nothing left to flush
    assert all(np.isfinite(r["loss/train"]) and np.isfinite(r["loss/train_mean"]) for r in rows)
    last = []
    for epoch in range(2):
        batches = epoch_batches(other, epoch)
        assert len(batches) == 3
        last = [window_by_hand(other, batches[0:2], 2)[1], window_by_hand(other, batches[2:3], 2)[1]]     # windows [2, 1]
    assert other.global_step == 4 and other.micro_step == 6
    _same(_state(tr), _state(other))
    assert rows[-1]["loss/train"] == float(last[-1])           # the short window's loss is divided by 2 as well


def test_a_window_of_one_is_the_trainer_without_the_key(tmp_path):
    a, b = trainer("small_cond", tmp_path / "a", 1), trainer("small_cond", tmp_path / "b", None)
    a.fit(max_steps=4)
    b.fit(max_steps=4)
    assert a.micro_step == a.global_step == b.micro_step == b.global_step == 4
    _same(_state(a), _state(b))
    assert open(a.metrics_path).read() == open(b.metrics_path).read()


def test_resume_inside_an_epoch_of_windows_is_the_uninterrupted_run(tmp_path):
    from argparse import Namespace
    from diffsbdd_amd import train as T
    ds = complexes()
    a = trainer("small_cond", tmp_path / "a", 2)
    a.fit(max_steps=6)
    b = trainer("small_cond", tmp_path / "b", 2)
    b.fit(max_steps=3)
    assert (b.global_step, b.micro_step, b.epoch, b.batch_in_epoch) == (3, 5, 1, 2)
    path = shutil.copy(b.save_checkpoint(), str(tmp_path / "step3.ckpt"))
    del b
    with torch.serialization.safe_globals([Namespace]):
        ck = torch.load(path, map_location="cpu", weights_only=True)
    assert ck["micro_step"] == 5 and ck["global_step"] == 3 and ck["batch_in_epoch"] == 2
    c = T.Trainer.resume(path, ds, None, device=dev())
    assert (c.global_step, c.micro_step, c.epoch, c.batch_in_epoch, c.accumulate) == (3, 5, 1, 2, 2)
    c.fit(max_steps=6)
    assert c.micro_step == a.micro_step == 9
    _same(_state(a), _state(c))
    ck.pop("micro_step")                                       # a checkpoint written before accumulation existed
    old = str(tmp_path / "old.ckpt")
    torch.save(ck, old)
    d = T.Trainer.resume(old, ds, None, device=dev())
    assert d.micro_step == d.global_step == 3


def test_bucket_switch_reproducibility_and_no_read_backs(tmp_path):
    runs = {}
    for name, value in (("bucket", "1"), ("again", "1"), ("torch", "0")):
        with env("DSBDD_GRAD_BUCKET", value):
            tr = trainer("small_cond", tmp_path / name, 3)
            copies = tr.optimizer.host_copies
            tr.training_window(epoch_batches(tr, 0))
            tr.training_window(epoch_batches(tr, 1))
            assert tr.optimizer.host_copies == copies          # the steady state reads nothing back
            runs[name] = _state(tr)
    _same(runs["bucket"], runs["again"])
    _same(runs["bucket"], runs["torch"])                       # both legs are the same ordered float32 sums
    # fit: the only device-to-host copies are those of flush_metrics
    tr = trainer("small_cond", tmp_path / "fit", 2)
    inside = [0]
    flush = tr.flush_metrics

    def counted():
        before = tr.optimizer.host_copies
        flush()
        inside[0] += tr.optimizer.host_copies - before
    tr.flush_metrics = counted
    before = tr.optimizer.host_copies
    tr.fit(max_steps=1)                                        # (stops inside the epoch: no checkpoint, which reads the queue)
    assert tr.global_step == 1 and tr.micro_step == 2
    assert tr.optimizer.host_copies - before == inside[0] == 1


def test_torch_optimizer_accumulates_through_torch(tmp_path):
    tr = trainer("small_cond", tmp_path, 2, optimizer="torch")
    tr.fit(max_steps=2)
    assert (tr.global_step, tr.micro_step, tr.epoch) == (2, 3, 1)
    assert len(tr.clipper.items) == 3                          # the first large value + one norm per WINDOW
    rows = [json.loads(line) for line in open(tr.metrics_path)]
    assert rows and all(np.isfinite(r["loss/train"]) for r in rows)
