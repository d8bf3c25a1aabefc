"""The training loop around the HIP training step: `python -m diffsbdd_amd.train --config cfg.yml [--resume ckpt]`.

Counterpart of the reference's train.py + the training half of lightning_modules.py without pytorch_lightning, wandb or
torch_scatter: the processed-complex reader (dataset.py), `nll_from_terms` (lightning_modules.py:246-302), the optional
Lennard-Jones term (aux_loss.py), `ClippedAdamW` (optim.py) and checkpoints in the Lightning layout that
`LigandGenerator.from_checkpoint` reads.

Determinism: the shuffling is a function of (seed, epoch), the diffusion times of (seed, micro_step) and the noise of
(seed, sample, row, column, draw) with the draw counter set from micro_step (the number of micro-batches seen so far;
equal to global_step without accumulation), so a resumed run IS the uninterrupted run, bit for bit.

Gradient accumulation (`accumulate_grad_batches: k`, Lightning's semantics): the epoch's batches are walked in windows
of k (the last one may be shorter and still steps), every micro-batch's loss is `nll.mean(0) / k`, clipping and AdamW
run once per window and `global_step` counts optimiser steps.  With the HIP optimiser the window's gradients are summed
by the backward kernels in the optimiser's flat gradient bucket (train_net.accumulating).  `gpus: N` with
`accumulate_grad_batches: k` of the reference is reached on one GPU with `accumulate_grad_batches: N * k`.

Data-parallel ranks (`gpus: N`): `python -m torch.distributed.run --nproc-per-node N -m diffsbdd_amd.train --config
cfg.yml [--backend nccl|gloo]`.  Every rank walks the same batch list; a window holds N * k micro-batches, rank r runs
the contiguous block r of k (`rank_block`; the ranks that hold anything are a prefix) keyed by the global micro-step,
every loss is `nll.mean(0) / (N * k)`; ONE all_gather per window moves [bucket | has-gradient flags | loss] (on the
device with RCCL, through the host with gloo, where the ranks may share a GPU), and every rank folds the gathered buckets
in RANK ORDER inside the optimiser's first launch (`ClippedAdamW.step_ranks`).  No all_reduce, whose order is the
library's: with k = 1 the run on N ranks is the one-GPU run with `accumulate_grad_batches: N` bit for bit (weights,
optimiser state, clip queue, loss/train, loss/val); with k > 1 the gradient is the sum over ranks of each rank's
sequential sum, another association of the same float32 sum.  No parameter broadcast: the ranks hold identical weights
by construction and compare a 64-bit checksum of them at every epoch's end.  Validation batch b runs on rank b % N and
the per-batch float64 sums are added in batch order.  Rank 0 alone writes checkpoints and metrics; every rank loads on
resume; a checkpoint records `world`, and another N * k is accepted only at an epoch's boundary.  Memory: N gathered
buckets (4 bytes per parameter each) on every rank.  No run on more than one GPU has been made; the all_gather over
xGMI and scaling are not measured (profiles/data_parallel.md).

Out of scope (refused with a message): `virtual_nodes` (AppendVirtualNodes draws random virtual atoms per item),
`augment_noise > 0` / `augment_rotation` (the reference raises NotImplementedError for them), `gpus > 1` in a process
that is not one of that many ranks (the message names `accumulate_grad_batches` and the launch line), and with ranks
`optimizer="torch"` and `sample_eval` (evaluate from the checkpoint).
Accepted and ignored with one warning: `wandb_params`, `visualize_*`, the RDKit-based `eval_params` / `eval_epochs`.

Sampled-molecule evaluation (the reference's `validation_epoch_end`, lightning_modules.py:382-398) is asked for with a key
of its own, `sample_eval: {every_n_epochs, n_samples, batch_size, timesteps}`: on the due epochs `evaluate_samples()`
samples ligands for the validation pockets and logs `sample/*` records of `metrics.MoleculeSetMetrics` (see
`metrics.METRICS_COVERAGE` for what they are).  It draws from keys of its own, (seed, epoch, batch), and touches neither
the weights nor the training randomness: a run with the block and one without it end with the same weights, bit for bit.
"""
from __future__ import annotations

import argparse
import contextlib
import json
import os
import warnings
from argparse import Namespace

import numpy as np
import torch

from .aux_loss import LennardJones, WeightSchedule
from .dataset import ProcessedDataset, epoch_permutation
from .optim import ClippedAdamW, ReferenceClipper, QUEUE_KEY

DRAWS_PER_STEP = 16          # noise draws reserved per micro-batch (a training forward makes one or two)
_EVAL_DRAW_BASE = 1 << 40    # validation draws live apart from the training ones
_SAMPLE_EVAL_KEYS = ("every_n_epochs", "n_samples", "batch_size", "timesteps")
_IGNORED = ("wandb_params", "visualize_sample_epoch", "visualize_chain_epoch", "eval_params", "eval_epochs",
            "enable_progress_bar", "num_sanity_val_steps", "num_workers")


def nll_from_terms(terms, ligand, pocket, *, loss_type, training, T, x_dims, atom_nf, residue_nf, aux=None):
    """lightning_modules.py:246-302 on the 12-tuple of `ddpm.forward` (a 13th `info` entry is taken along).
    `aux` = (weight_schedule, lj) adds the Lennard-Jones term (l2 training only).  Element-wise float32 arithmetic in
    the reference's order; no host synchronisation.  -> (nll [batch], info)"""
    (delta_log_px, error_t_lig, error_t_pocket, SNR_weight, loss_0_x_ligand, loss_0_x_pocket, loss_0_h,
     neg_log_const_0, kl_prior, log_pN, t_int, xh_lig_hat) = terms[:12]
    info = dict(terms[12]) if len(terms) > 12 and terms[12] is not None else {}
    l2_train = loss_type == "l2" and training
    if l2_train:
        lig_size = ligand["size"]
        denom_lig = x_dims * lig_size + atom_nf * lig_size
        error_t_lig = error_t_lig / denom_lig
        denom_pocket = (x_dims + residue_nf) * pocket["size"]
        error_t_pocket = error_t_pocket / denom_pocket
        loss_t = 0.5 * (error_t_lig + error_t_pocket)
        loss_0_x_ligand = loss_0_x_ligand / (x_dims * lig_size)
        loss_0_x_pocket = loss_0_x_pocket / (x_dims * pocket["size"])
        loss_0 = loss_0_x_ligand + loss_0_x_pocket + loss_0_h
    else:
        loss_t = -T * 0.5 * SNR_weight * (error_t_lig + error_t_pocket)
        loss_0 = loss_0_x_ligand + loss_0_x_pocket + loss_0_h
        loss_0 = loss_0 + neg_log_const_0
    nll = loss_t + loss_0 + kl_prior
    if not l2_train:
        nll = nll - delta_log_px
        nll = nll - log_pN
    if aux is not None and l2_train:
        schedule, lj = aux
        weighted = schedule(t_int.long()) * lj(xh_lig_hat, ligand["mask"], ligand["size"].shape[0])
        nll = nll + weighted
        info["weighted_lj"] = weighted.mean(0)
    info["error_t_lig"] = error_t_lig.mean(0)
    info["error_t_pocket"] = error_t_pocket.mean(0)
    info["SNR_weight"] = SNR_weight.mean(0)
    info["loss_0"] = loss_0.mean(0)
    info["kl_prior"] = kl_prior.mean(0)
    info["delta_log_px"] = delta_log_px.mean(0)
    info["neg_log_const_0"] = neg_log_const_0.mean(0)
    info["log_pN"] = log_pN.mean(0)
    return nll, info


# ---- configuration ----------------------------------------------------------------------------------------------------
def _plain(v):
    if isinstance(v, Namespace):
        return {k: _plain(x) for k, x in vars(v).items()}
    if isinstance(v, dict):
        return {k: _plain(x) for k, x in v.items()}
    return v


def check_config(cfg, world=1):
    """Validates a training configuration with the reference's YAML keys; -> plain dict.  Refuses what is out of scope,
    warns once about what is accepted and ignored.  `world`: the number of data-parallel ranks this process is one of
    (the caller's knowledge, never read from the environment); `gpus` must equal it."""
    cfg = {k: _plain(v) for k, v in dict(cfg).items()}
    world = int(world)
    if world < 1:
        raise ValueError(f"world must be >= 1, got {world}")
    for key in ("dataset", "datadir", "mode", "batch_size", "lr", "n_epochs", "egnn_params", "diffusion_params"):
        if key not in cfg:
            raise ValueError(f"training config: '{key}' is missing")
    if cfg.get("virtual_nodes", False):
        raise NotImplementedError("virtual_nodes: True is out of scope of this trainer (AppendVirtualNodes draws random "
                                  "virtual atoms per item)")
    if cfg.get("augment_noise", 0) and cfg["augment_noise"] > 0:
        raise NotImplementedError("augment_noise > 0 is not supported (the reference raises NotImplementedError too)")
    if cfg.get("augment_rotation", False):
        raise NotImplementedError("augment_rotation is not supported (the reference raises NotImplementedError too)")
    gpus = int(cfg.get("gpus", 1))
    if gpus > 1 and world == 1:
        raise NotImplementedError("gpus > 1: multi-GPU training is out of scope of this trainer; set gpus: 1 and multiply "
                                  "accumulate_grad_batches by the number of GPUs for the same effective batch, or start "
                                  f"one rank per GPU: python -m torch.distributed.run --nproc-per-node {gpus} "
                                  "-m diffsbdd_amd.train --config cfg.yml")
    if gpus != world:
        raise ValueError(f"gpus: {gpus} does not match the {world} rank(s) this run was started with (gpus must equal the "
                         "world size)")
    if gpus > 1 and cfg.get("sample_eval") is not None:
        raise NotImplementedError("sample_eval with gpus > 1 is out of scope (sampled-molecule evaluation is not split over "
                                  "ranks): drop the block and evaluate from the checkpoint on one GPU")
    k = cfg.get("accumulate_grad_batches", 1)
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1:
        raise ValueError(f"accumulate_grad_batches must be an integer >= 1, got {k!r}")
    if cfg.get("sample_eval") is not None:
        se = cfg["sample_eval"]
        if not isinstance(se, dict) or set(se) - set(_SAMPLE_EVAL_KEYS):
            raise ValueError(f"sample_eval takes the keys {_SAMPLE_EVAL_KEYS}, got {se!r}")
        for key, v in se.items():
            if v is not None and (isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1):
                raise ValueError(f"sample_eval.{key} must be an integer >= 1, got {v!r}")
    ignored = [k for k in cfg if k in _IGNORED or k.startswith("visualize_")]
    if ignored:
        warnings.warn("training config: accepted and ignored: " + ", ".join(sorted(ignored)) +
                      " (no wandb, visualisation or RDKit-based evaluation in this trainer)")
    cfg.setdefault("pocket_representation", "CA")
    cfg.setdefault("clip_grad", True)
    cfg.setdefault("auxiliary_loss", False)
    cfg.setdefault("seed", 0)
    cfg.setdefault("log_every", 50)
    cfg.setdefault("logdir", ".")
    cfg.setdefault("run_name", "run")
    return cfg


def accumulation_windows(n_batches, k):
    """The sizes of the accumulation windows over an epoch of `n_batches` batches: full windows of `k`, then the rest."""
    n_batches, k = int(n_batches), int(k)
    if n_batches < 0 or k < 1:
        raise ValueError("accumulation_windows needs n_batches >= 0 and k >= 1")
    return [min(k, n_batches - lo) for lo in range(0, n_batches, k)]


def rank_block(n, world, k, rank):
    """The micro-batches [lo, hi) of a window of `n` (at most world * k) that rank `rank` runs: contiguous blocks of k in
    rank order, so the ranks that hold at least one micro-batch are the prefix 0 .. contributing_ranks(n, k) - 1."""
    n, world, k, rank = int(n), int(world), int(k), int(rank)
    if world < 1 or k < 1 or not 0 <= rank < world or not 0 <= n <= world * k:
        raise ValueError(f"rank_block: no window of {n} micro-batches for rank {rank} of {world} with k = {k}")
    return min(rank * k, n), min((rank + 1) * k, n)


def contributing_ranks(n, k):
    """How many ranks hold a micro-batch of a window of n."""
    return (int(n) + int(k) - 1) // int(k)


def validation_rank(batch, world):
    """The rank that evaluates validation batch `batch`."""
    return int(batch) % int(world)


def ordered_sum(values):
    """The float64 sum of per-batch values in batch order, started from +0 as `validate` does on one GPU."""
    total = 0.0
    for v in values:
        total += float(v)
    return total


def weights_checksum(tensors):
    """A 64-bit checksum of the float32 tensors' bit patterns (position-weighted, wrapping int64 arithmetic on the
    tensors' device): equal weights give equal checksums on every rank.  -> int64 device scalar"""
    acc = None
    for t in tensors:
        bits = t.detach().reshape(-1).view(torch.int32).to(torch.int64) & 0xFFFFFFFF
        s = (bits * torch.arange(1, bits.numel() + 1, dtype=torch.int64, device=bits.device)).sum()
        acc = s if acc is None else acc * 1000003 + s
    return acc


def load_config(path, resume_hparams=None, world=1):
    import yaml
    with open(path) as f:
        cfg = yaml.safe_load(f)
    if "resume" in cfg:
        raise ValueError("'resume' is a command line option, not a config key")
    if resume_hparams is not None:                          # train.py:29-38: the checkpoint's values win
        for k, v in resume_hparams.items():
            v = _plain(v)
            if k in cfg and cfg[k] != v and k != "node_histogram":
                warnings.warn(f"Config parameter '{k}' (value: {cfg[k]}) will be overwritten with value {v} from the checkpoint.")
            cfg[k] = v
    return check_config(cfg, world)


# ---- the loop -----------------------------------------------------------------------------------------------------------
class Trainer:
    """fit() / training_step() / training_window() / validate() / save_checkpoint() / resume() around `ddpm.forward` and
    the HIP optimiser.  `optimizer="torch"` selects torch.optim.AdamW plus the host-side restatement of the reference's
    clipping (A/B); it accumulates through torch.

    Data-parallel ranks: `world` processes build the same Trainer with their `rank`; a window is then
    local_window() on the rank's block of micro-batches, one all_gather of the buckets (torch.distributed's default
    group, which the caller has initialised) and apply_window() on every rank.  `collective=True` takes that route at
    world 1 as well (a one-rank process group)."""

    def __init__(self, config, node_histogram, train_set=None, val_set=None, device="cuda", optimizer="hip", world=1, rank=0,
                 collective=None):
        from .generate import LigandGenerator
        self.world, self.rank = int(world), int(rank)
        self.cfg = cfg = check_config(config, self.world)
        if not 0 <= self.rank < self.world:
            raise ValueError(f"rank {rank} is outside the world of {world}")
        self.collective = self.world > 1 if collective is None else bool(collective)
        if self.world > 1 and not self.collective:
            raise ValueError("more than one rank needs the exchange (collective=True)")
        self.device = torch.device(device)
        self.node_histogram = np.asarray(node_histogram).tolist()
        if optimizer not in ("hip", "torch"):
            raise ValueError("optimizer must be 'hip' or 'torch'")
        if self.collective and optimizer != "hip":
            raise NotImplementedError("data-parallel ranks run on the HIP optimiser only (the ordered bucket reduce is its "
                                      "first launch); optimizer='torch' is for gpus: 1")
        self.optimizer_kind = optimizer
        self.seed = int(cfg["seed"])
        self.accumulate = int(cfg.get("accumulate_grad_batches", 1))
        with torch.random.fork_rng(devices=[self.device] if self.device.type == "cuda" else []):
            torch.manual_seed(self.seed)                   # the initial weights are a function of the seed as well
            gen = LigandGenerator(dataset=cfg["dataset"], egnn_params=cfg["egnn_params"],
                                  diffusion_params=cfg["diffusion_params"], mode=cfg["mode"],
                                  node_histogram=self.node_histogram, pocket_representation=cfg["pocket_representation"],
                                  virtual_nodes=False, device=self.device)
        self.gen = gen
        self.ddpm = gen.ddpm
        self.loss_type = cfg["diffusion_params"]["diffusion_loss_type"]
        self.T = cfg["diffusion_params"]["diffusion_steps"]
        self.x_dims, self.atom_nf, self.residue_nf = 3, gen.atom_nf, gen.aa_nf
        self.aux = None
        if cfg["auxiliary_loss"]:
            lp = cfg["loss_params"]
            self.aux = (WeightSchedule(self.T, lp["max_weight"], lp["schedule"], device=self.device),
                        LennardJones(gen.lig_type_decoder, self.ddpm.norm_values[0], lp.get("clamp_lj"), device=self.device))
        self.params = [p for p in self.ddpm.parameters() if p.requires_grad]
        hyper = dict(lr=cfg["lr"], betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-12)       # lightning_modules.py:175-177
        if optimizer == "hip":
            self.optimizer = ClippedAdamW(self.params, clip_grad=bool(cfg["clip_grad"]), **hyper)
            self.clipper = None
        else:
            self.optimizer = torch.optim.AdamW(self.params, amsgrad=True, **hyper)
            self.clipper = ReferenceClipper() if cfg["clip_grad"] else None
        self.train_set, self.val_set = train_set, val_set
        self.epoch, self.global_step, self.batch_in_epoch = 0, 0, 0
        self.micro_step = 0                # micro-batches seen so far: the key of the noise and the diffusion times
        self.best_val, self.best_path = float("inf"), None
        self.run_dir = os.path.join(cfg["logdir"], cfg["run_name"])
        self.ckpt_dir = os.path.join(self.run_dir, "checkpoints")
        self.metrics_path = os.path.join(self.run_dir, "metrics.jsonl")
        self._pending = []                 # (global_step, device scalars) since the last fetch
        self._t_gen = torch.Generator()
        self.ddpm.t_int_source = self._draw_t
        self._t_key = 0
        self.sample_eval = cfg.get("sample_eval")
        self._set_metrics = None           # MoleculeSetMetrics with the training split's keys and type counts, built once
        self._row = self._gathered = None  # the exchange: this rank's [bucket | flags | loss] and every rank's (_exchange_buffers)
        self._flag_rows = {}               # flags -> their float32 device image (they rarely change: no copy per window)
        self._mismatch = None              # device flag: contributing ranks disagreed on the flags (nccl; read at a flush)

    # -- randomness: everything derives from (seed, epoch, micro_step) -----------------------------------------------------
    def _draw_t(self, batch):
        lowest = 0 if self.ddpm.training else 1
        self._t_gen.manual_seed((self.seed * 7919 + self._t_key) % (2 ** 63))
        return torch.randint(lowest, self.T + 1, (batch, 1), generator=self._t_gen).float()

    def _key_step(self, key):
        self.ddpm.seed(self.seed)
        self.ddpm._draw = int(key) * DRAWS_PER_STEP
        self._t_key = int(key)

    # -- one batch ---------------------------------------------------------------------------------------------------------
    def ligand_and_pocket(self, data):
        dev = self.device
        ligand = {"x": data["lig_coords"].to(dev, torch.float32), "one_hot": data["lig_one_hot"].to(dev, torch.float32),
                  "size": data["num_lig_atoms"].to(dev, torch.int64), "mask": data["lig_mask"].to(dev, torch.int64)}
        pocket = {"x": data["pocket_coords"].to(dev, torch.float32), "one_hot": data["pocket_one_hot"].to(dev, torch.float32),
                  "size": data["num_pocket_nodes"].to(dev, torch.int64), "mask": data["pocket_mask"].to(dev, torch.int64)}
        return ligand, pocket

    def forward(self, data):
        ligand, pocket = self.ligand_and_pocket(data)
        terms = self.ddpm(ligand, pocket, return_info=True)
        return nll_from_terms(terms, ligand, pocket, loss_type=self.loss_type, training=self.ddpm.training, T=self.T,
                              x_dims=self.x_dims, atom_nf=self.atom_nf, residue_nf=self.residue_nf, aux=self.aux)

    def training_step(self, data):
        """A window of one batch (see training_window)."""
        return self.training_window([data])

    def _window(self):
        """Where the window's gradients are summed: the optimiser's bucket (HIP optimiser, k > 1), else torch's p.grad."""
        if self.accumulate > 1 and isinstance(self.optimizer, ClippedAdamW):
            from .train_net import accumulating
            return accumulating(self.ddpm.dynamics, self.optimizer.gradient_bucket())
        return contextlib.nullcontext()

    def training_window(self, batches):
        """forward -> backward for every micro-batch of one accumulation window (at most `accumulate_grad_batches`; every
        loss is nll.mean(0) / accumulate_grad_batches, in a short window too), then clip -> AdamW once; -> the sum of the
        scaled losses as a device scalar (no read-back)."""
        if self.collective:
            return self.ranks_window(batches)
        if not 1 <= len(batches) <= self.accumulate:
            raise ValueError("a window holds 1 to accumulate_grad_batches (%d) batches, got %d" % (self.accumulate, len(batches)))
        self.ddpm.train()
        total = None
        with self._window():
            for data in batches:
                self._key_step(self.micro_step)
                nll, info = self.forward(data)
                loss = nll.mean(0)
                if self.accumulate > 1:
                    loss = loss / self.accumulate
                loss.backward()
                self.micro_step += 1
                total = loss.detach() if total is None else total + loss.detach()
        if self.clipper is not None:
            self.clipper.clip(self.params)
        self.optimizer.step()
        self.optimizer.zero_grad(set_to_none=True)
        self.global_step += 1
        self._pending.append((self.global_step, total))
        return total

    # -- data-parallel ranks: a window in two halves around one all_gather ---------------------------------------------------
    def _exchange_buffers(self):
        """This rank's row [bucket | per-tensor has-gradient flags | loss | padding to 4] -- the optimiser's bucket IS its
        head, so nothing is packed -- and the [world, row] gather buffer."""
        if self._row is None:
            elems = int(self.optimizer.lib.dsbdd_optim_state_elems(self.optimizer._h))
            stride = (elems + len(self.params) + 1 + 3) & ~3
            self._row = torch.zeros(stride, dtype=torch.float32, device=self.device)
            self._gathered = torch.zeros(self.world, stride, dtype=torch.float32, device=self.device)
            if self.optimizer._bucket is None:
                self.optimizer.gradient_bucket(flat=self._row[:elems])
        return self._row, self._gathered

    def local_window(self, batches, first_micro_step):
        """This rank's half of a window: forward -> backward of `batches` (none, for a rank past the window's end) into the
        optimiser's gradient bucket, micro-batch j keyed by first_micro_step + j, every loss nll.mean(0) / (world *
        accumulate_grad_batches).  A gradient that arrived outside the bucket is copied into it, so that afterwards every
        `p.grad` is the bucket's view or None.  `micro_step` is the caller's to advance (by the WINDOW's micro-batches).
        -> (the sum of the scaled losses as a device scalar, the per-parameter has-gradient flags)"""
        from .train_net import accumulating
        if not isinstance(self.optimizer, ClippedAdamW):
            raise NotImplementedError("local_window needs the HIP optimiser's gradient bucket")
        if len(batches) > self.accumulate:
            raise ValueError("a rank runs at most accumulate_grad_batches (%d) micro-batches of a window, got %d"
                             % (self.accumulate, len(batches)))
        self._exchange_buffers()
        bucket = self.optimizer.gradient_bucket()
        scale = self.world * self.accumulate
        self.ddpm.train()
        total = None
        with accumulating(self.ddpm.dynamics, bucket):
            for j, data in enumerate(batches):
                self._key_step(int(first_micro_step) + j)
                nll, info = self.forward(data)
                loss = nll.mean(0)
                if scale > 1:
                    loss = loss / scale
                loss.backward()
                total = loss.detach() if total is None else total + loss.detach()
        flags = []
        for p in self.params:
            flags.append(p.grad is not None)
            if p.grad is not None and p.grad.data_ptr() != bucket.view(p).data_ptr():
                bucket.view(p).copy_(p.grad)
                p.grad = bucket.view(p)
        if total is None:
            total = torch.zeros((), dtype=torch.float32, device=self.device)
        return total, flags

    def apply_window(self, gathered, n_ranks, losses, flags=None):
        """The other half, the same on every rank: `ClippedAdamW.step_ranks` on the first `n_ranks` rows of `gathered`
        (the contributing ranks' buckets, folded in rank order inside the optimiser's first launch), zero_grad, one more
        `global_step`, and the logged loss = the ranks' losses summed in rank order (queued, no read-back).  `flags`: the
        contributing ranks' has-gradient flags for a rank that ran no micro-batch of this window (its own `p.grad` are
        all None); None keeps this rank's `p.grad`.  -> the logged loss as a device scalar"""
        n_ranks = int(n_ranks)
        if flags is not None:
            bucket = self.optimizer.gradient_bucket()
            for p, f in zip(self.params, flags):
                p.grad = bucket.view(p) if f else None
        self.optimizer.step_ranks(gathered, n_ranks)
        self.optimizer.zero_grad(set_to_none=True)
        self.global_step += 1
        total = losses[0].clone()                  # (a view of the gather buffer would change under the queue)
        for r in range(1, n_ranks):
            total = total + losses[r]
        self._pending.append((self.global_step, total))
        return total

    def _exchange(self, loss, flags, n_ranks):
        """The window's ONE collective: all_gather of the rows.  nccl keeps them on the device (the flags' agreement is
        accumulated in a device flag and read with the next flush); gloo goes through the host, where the flags are
        compared at once.  -> (gathered [world, row] on the device, the contributing ranks' flags on the host)"""
        import torch.distributed as dist
        row, gathered = self._exchange_buffers()
        n, elems = len(self.params), self.optimizer.gradient_bucket().flat.numel()
        bucket = self.optimizer.gradient_bucket()
        if bucket.flat.data_ptr() != row.data_ptr():       # (the bucket existed before the first exchange)
            row[:elems] = bucket.flat
        key = tuple(flags)
        if key not in self._flag_rows:
            self._flag_rows[key] = torch.tensor([float(f) for f in flags], dtype=torch.float32).to(self.device)
        row[elems:elems + n] = self._flag_rows[key]
        row[elems + n] = loss
        mine = self.rank < n_ranks
        if dist.get_backend() == "nccl":
            dist.all_gather_into_tensor(gathered.view(-1), row)
            theirs = gathered[:n_ranks, elems:elems + n]
            bad = (theirs != theirs[0]).any()
            self._mismatch = bad if self._mismatch is None else self._mismatch | bad
            if not mine:
                flags = (theirs[0] != 0).tolist()
        else:
            host = torch.empty(gathered.shape, dtype=torch.float32)
            dist.all_gather(list(host.unbind(0)), row.cpu())
            theirs = host[:n_ranks, elems:elems + n]
            if bool((theirs != theirs[0]).any()):
                raise RuntimeError("data-parallel ranks disagree on which parameters have a gradient in this window")
            if not mine:
                flags = (theirs[0] != 0).tolist()
            gathered.copy_(host)
        return gathered, flags

    def _check_flags_agreed(self):
        if self._mismatch is not None:
            bad, self._mismatch = bool(self._mismatch), None
            if bad:
                raise RuntimeError("data-parallel ranks disagree on which parameters have a gradient in a window")

    def ranks_window(self, window, collate=None):
        """One window of at most world * accumulate_grad_batches micro-batches, the same list on every rank: this rank's
        block (rank_block) through local_window, the exchange, apply_window.  `collate`: applied to this rank's items only."""
        n, k = len(window), self.accumulate
        if not 1 <= n <= self.world * k:
            raise ValueError("a window holds 1 to world * accumulate_grad_batches (%d) batches, got %d" % (self.world * k, n))
        lo, hi = rank_block(n, self.world, k, self.rank)
        block = window[lo:hi] if collate is None else [collate(b) for b in window[lo:hi]]
        n_ranks = contributing_ranks(n, k)
        loss, flags = self.local_window(block, self.micro_step + lo)
        gathered, flags = self._exchange(loss, flags, n_ranks)
        self.micro_step += n
        elems = self.optimizer.gradient_bucket().flat.numel()
        return self.apply_window(gathered, n_ranks, gathered[:, elems + len(self.params)], None if lo < hi else flags)

    @torch.no_grad()
    def validate(self):
        """Mean `loss/val` over the validation split (eval mode, no_grad), weighted by batch size as Lightning's log."""
        self.ddpm.eval()
        n = len(self.val_set)
        bs = int(self.cfg.get("eval_batch_size", self.cfg["batch_size"]))
        if self.collective:
            return self._validate_ranks(n, bs)
        total = torch.zeros((), dtype=torch.float64, device=self.device)
        for b, lo in enumerate(range(0, n, bs)):
            idx = list(range(lo, min(lo + bs, n)))
            self._key_step(_EVAL_DRAW_BASE // DRAWS_PER_STEP + self.epoch * 100003 + b)
            nll, _ = self.forward(self.val_set.collate(idx))
            total += nll.double().sum()
        self.ddpm.train()
        return float(total / n)

    def _validate_ranks(self, n, bs):
        """Batch b on rank b % world; the per-batch float64 sums meet in one vector by all_reduce(SUM) -- exact: every
        other rank adds +0 -- which is then summed in batch order on the host: the one-GPU value, bit for bit."""
        import torch.distributed as dist
        starts = list(range(0, n, bs))
        sums = torch.zeros(len(starts), dtype=torch.float64, device=self.device)
        for b, lo in enumerate(starts):
            if validation_rank(b, self.world) != self.rank:
                continue
            self._key_step(_EVAL_DRAW_BASE // DRAWS_PER_STEP + self.epoch * 100003 + b)
            nll, _ = self.forward(self.val_set.collate(list(range(lo, min(lo + bs, n)))))
            sums[b] = nll.double().sum()
        self.ddpm.train()
        if dist.get_backend() != "nccl":
            sums = sums.cpu()
        dist.all_reduce(sums, op=dist.ReduceOp.SUM)
        total = torch.tensor(ordered_sum(sums.tolist()), dtype=torch.float64, device=self.device)
        return float(total / n)            # the division of `validate`, on the same device (torch multiplies by 1 / n there)

    # -- sampled molecules (lightning_modules.py:412-549) ------------------------------------------------------------------------
    def _sample_key(self, batch):
        """The key of one evaluation batch's draws: a function of (seed, epoch, batch), apart from the training keys."""
        return ((self.seed * 1000003 + self.epoch) * 100003 + int(batch) + _EVAL_DRAW_BASE) % (2 ** 63)

    @torch.no_grad()
    def evaluate_samples(self):
        """Samples `sample_eval.n_samples` ligands -- for the validation pockets, item (i * batch_size + j) % len(val) as
        `sample_and_analyze_given_pocket`, with sizes from `size_distribution.sample_conditional`; the joint model draws
        whole complexes with `ddpm.sample` -- and evaluates them with one group per pocket against the training split.
        -> the `sample/*` record.  Leaves the model in training mode and the training keys untouched."""
        from .metrics import MoleculeSetMetrics, reference_from_dataset
        se = self.sample_eval or {}
        val, dev = self.val_set, self.device
        n_samples = int(se.get("n_samples") or len(val))
        bs = min(int(se.get("batch_size") or self.cfg["batch_size"]), n_samples)
        timesteps = se.get("timesteps")
        if self._set_metrics is None:
            keys = counts = None
            if self.train_set is not None and len(self.train_set):
                keys, counts = reference_from_dataset(self.train_set, self.gen.dataset_info, device=dev)
            self._set_metrics = MoleculeSetMetrics(self.gen.dataset_info, keys, counts)
        joint = self.cfg["mode"] == "joint"
        self.ddpm.eval()
        xs, types, masks, groups, done = [], [], [], [], 0
        try:
            for i in range((n_samples + bs - 1) // bs):
                n = min(bs, n_samples - done)
                key = self._sample_key(i)
                with torch.random.fork_rng(devices=[dev] if dev.type == "cuda" else []):
                    torch.manual_seed(key)
                    self.ddpm.seed(key)
                    if joint:
                        n_lig, n_pocket = self.ddpm.size_distribution.sample(n)
                        xh_lig, _, lig_mask, _ = self.ddpm.sample(n, n_lig, n_pocket, timesteps=timesteps, device=dev)
                        groups += [0] * n
                    else:
                        idx = [(i * bs + j) % len(val) for j in range(n)]
                        _, pocket = self.ligand_and_pocket(val.collate(idx))
                        n_lig = self.ddpm.size_distribution.sample_conditional(n1=None, n2=pocket["size"])
                        xh_lig, _, lig_mask, _ = self.ddpm.sample_given_pocket(pocket, n_lig, timesteps=timesteps)
                        groups += idx
                xs.append(xh_lig[:, :self.x_dims])
                types.append(xh_lig[:, self.x_dims:].argmax(1))
                masks.append(lig_mask + done)
                done += n
        finally:
            self.ddpm.train()
        res = self._set_metrics.evaluate(torch.cat(xs), torch.cat(types), torch.cat(masks), groups=groups, batch=done)
        record = {"epoch": self.epoch, "step": self.global_step}
        for k in ("validity", "connectivity", "uniqueness", "novelty", "diversity", "kl_div_atom_types", "n", "n_valid",
                  "n_connected", "n_unique"):
            record["sample/" + k] = res[k]
        return record

    # -- metrics -----------------------------------------------------------------------------------------------------------
    def _log(self, record):
        if self.rank != 0:                 # rank 0 alone writes files
            return
        os.makedirs(self.run_dir, exist_ok=True)
        with open(self.metrics_path, "a") as f:
            f.write(json.dumps(record) + "\n")

    def flush_metrics(self):
        """One synchronisation: the pending device scalars and the clip record."""
        self._check_flags_agreed()
        if not self._pending:
            return
        if self.rank != 0:
            self._pending = []
            return
        steps = [s for s, _ in self._pending]
        values = torch.stack([v for _, v in self._pending]).tolist()
        self._pending = []
        record = {"epoch": self.epoch, "step": steps[-1], "loss/train": values[-1],
                  "loss/train_mean": float(np.mean(values))}
        if isinstance(self.optimizer, ClippedAdamW) and self.optimizer.clip_grad:
            rep = self.optimizer.clip_report()
            record.update({"grad_norm": rep["last_norm"], "max_grad_norm": rep["last_max_norm"], "n_clips": rep["n_clips"]})
        elif self.clipper is not None:
            record.update({"grad_norm": self.clipper.last_norm, "max_grad_norm": self.clipper.last_max,
                           "n_clips": self.clipper.n_clips})
        self._log(record)

    # -- the loop ----------------------------------------------------------------------------------------------------------
    def fit(self, max_steps=None):
        cfg = self.cfg
        bs, n = int(cfg["batch_size"]), len(self.train_set)
        while self.epoch < int(cfg["n_epochs"]):
            order = epoch_permutation(n, self.seed, self.epoch).tolist()
            batches = [order[i:i + bs] for i in range(0, n, bs)]
            # batch_in_epoch only ever stops at a window boundary: a checkpoint never holds a half-filled bucket
            # (with ranks a window holds world * k micro-batches and every rank collates its own block only)
            starts = np.cumsum([0] + accumulation_windows(len(batches), self.world * self.accumulate)).tolist()
            while self.batch_in_epoch < len(batches):
                if max_steps is not None and self.global_step >= max_steps:
                    self.flush_metrics()
                    return
                hi = min(b for b in starts if b > self.batch_in_epoch)
                if self.collective:
                    self.ranks_window(batches[self.batch_in_epoch:hi], collate=self.train_set.collate)
                else:
                    self.training_window([self.train_set.collate(b) for b in batches[self.batch_in_epoch:hi]])
                self.batch_in_epoch = hi
                if self.global_step % int(cfg["log_every"]) == 0:
                    self.flush_metrics()
            self.flush_metrics()
            val = None
            if self.val_set is not None and len(self.val_set):
                val = self.validate()
                self._log({"epoch": self.epoch, "step": self.global_step, "loss/val": val})
                if self.sample_eval is not None and (self.epoch + 1) % int(self.sample_eval.get("every_n_epochs") or 1) == 0:
                    self._log(self.evaluate_samples())
            self.epoch += 1
            self.batch_in_epoch = 0
            if self.collective:
                self.check_ranks_in_step()
            self.save_checkpoint(val)

    def check_ranks_in_step(self):
        """Every rank must hold the same weights without ever broadcasting them: the ranks compare a 64-bit checksum of
        their weights' bit patterns (one small all_gather, one read-back per epoch)."""
        import torch.distributed as dist
        mine = weights_checksum(self.params).reshape(1)
        if dist.get_backend() != "nccl":
            mine = mine.cpu()
        sums = [torch.zeros_like(mine) for _ in range(self.world)]
        dist.all_gather(sums, mine)
        sums = [int(s) for s in sums]
        if any(s != sums[0] for s in sums):
            raise RuntimeError("data-parallel ranks hold different weights after epoch %d (checksums %s)" % (self.epoch - 1, sums))

    # -- checkpoints (Lightning layout, generate.load_checkpoint) ------------------------------------------------------------
    def hyper_parameters(self):
        cfg = self.cfg
        hp = {k: v for k, v in cfg.items()}
        for k in ("egnn_params", "diffusion_params", "loss_params", "eval_params", "wandb_params"):
            if isinstance(hp.get(k), dict):
                hp[k] = Namespace(**hp[k])
        hp["node_histogram"] = self.node_histogram
        hp["virtual_nodes"] = False
        hp["outdir"] = self.run_dir
        return hp

    def checkpoint(self):
        opt = self.optimizer.state_dict()
        if self.clipper is not None:
            opt[QUEUE_KEY] = {"items": list(self.clipper.items), "n_clips": self.clipper.n_clips}
        sd = {"ddpm." + k: v.detach().cpu() for k, v in self.ddpm.state_dict().items()}
        return {"state_dict": sd, "hyper_parameters": self.hyper_parameters(), "optimizer_states": [opt],
                "epoch": self.epoch, "global_step": self.global_step, "batch_in_epoch": self.batch_in_epoch,
                "micro_step": self.micro_step, "world": self.world,
                "optimizer_kind": self.optimizer_kind, QUEUE_KEY: opt.get(QUEUE_KEY), "best_val": self.best_val}

    def save_checkpoint(self, val_loss=None):
        """`last.ckpt` always, `best-model-epoch=NN.ckpt` when `loss/val` improved (train.py:103-110)."""
        last = os.path.join(self.ckpt_dir, "last.ckpt")
        if self.rank != 0:                 # rank 0 alone writes files; `loss/val` is the same number on every rank
            if val_loss is not None and val_loss < self.best_val:
                self.best_val = float(val_loss)
            return last
        os.makedirs(self.ckpt_dir, exist_ok=True)
        ck = self.checkpoint()
        if val_loss is not None and val_loss < self.best_val:
            self.best_val = ck["best_val"] = float(val_loss)
            best = os.path.join(self.ckpt_dir, "best-model-epoch=%02d.ckpt" % max(self.epoch - 1, 0))
            torch.save(ck, best)
            if self.best_path and self.best_path != best and os.path.isfile(self.best_path):
                os.remove(self.best_path)
            self.best_path = best
        torch.save(ck, last + ".tmp")
        os.replace(last + ".tmp", last)
        return last

    def load_checkpoint(self, path):
        with torch.serialization.safe_globals([Namespace]):
            ck = torch.load(path, map_location="cpu", weights_only=True)
        own = {k[len("ddpm."):]: v for k, v in ck["state_dict"].items() if k.startswith("ddpm.")}
        self.ddpm.load_state_dict(own, strict=False)
        self.ddpm.dynamics.invalidate_engine()
        opt = dict(ck["optimizer_states"][0])
        queue = opt.get(QUEUE_KEY)
        if self.clipper is not None:
            opt.pop(QUEUE_KEY, None)
            if queue is not None:
                self.clipper = ReferenceClipper(queue["items"])
                self.clipper.n_clips = int(queue.get("n_clips", 0))
        self.optimizer.load_state_dict(opt)
        self.epoch, self.global_step = int(ck.get("epoch", 0)), int(ck.get("global_step", 0))
        self.batch_in_epoch = int(ck.get("batch_in_epoch", 0))
        # a position inside an epoch is a window boundary of the run that wrote it: another world * k has other windows
        then = int(ck.get("world", 1)) * int(_plain(ck["hyper_parameters"]).get("accumulate_grad_batches", 1))
        if then != self.world * self.accumulate and self.batch_in_epoch != 0:
            raise ValueError("the checkpoint stands inside an epoch (batch %d) of windows of %d micro-batches; this run has "
                             "windows of %d: resume it with the same world * accumulate_grad_batches, or from a checkpoint "
                             "at an epoch's end" % (self.batch_in_epoch, then, self.world * self.accumulate))
        self.micro_step = int(ck.get("micro_step", self.global_step))      # (checkpoints written before accumulation)
        self.best_val = float(ck.get("best_val", float("inf")))

    @classmethod
    def resume(cls, path, train_set=None, val_set=None, device="cuda", optimizer=None, overrides=None, world=1, rank=0,
               collective=None):
        """A Trainer continued from a checkpoint written by `save_checkpoint` (every rank loads it; `gpus` follows the
        world this run has)."""
        with torch.serialization.safe_globals([Namespace]):
            ck = torch.load(path, map_location="cpu", weights_only=True)
        hp = {k: _plain(v) for k, v in ck["hyper_parameters"].items()}
        hp.update(overrides or {})
        hist = hp.pop("node_histogram")
        hp.pop("outdir", None)
        hp["gpus"] = int(world)
        tr = cls(hp, hist, train_set, val_set, device=device, optimizer=optimizer or ck.get("optimizer_kind", "hip"),
                 world=world, rank=rank, collective=collective)
        tr.load_checkpoint(path)
        return tr


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--config", type=str, required=True)
    p.add_argument("--resume", type=str, default=None)
    p.add_argument("--optimizer", choices=("hip", "torch"), default="hip")
    p.add_argument("--max-steps", type=int, default=None)
    p.add_argument("--device", type=str, default="cuda")
    p.add_argument("--backend", choices=("nccl", "gloo"), default=None,
                   help="torch.distributed backend of data-parallel ranks started by torch.distributed.run (default: nccl = "
                        "RCCL, one GPU per rank); gloo exchanges through the host and lets every rank use the same "
                        "--device; given explicitly, a single rank runs the exchange as well")
    args = p.parse_args(argv)
    from . import sharding
    rank, local_rank, world = sharding.init_distributed(backend=args.backend, one_gpu_per_rank=args.backend != "gloo",
                                                        force=args.backend is not None)
    collective = world > 1 or args.backend is not None
    if collective and args.backend != "gloo" and args.device == "cuda":
        args.device = "cuda:%d" % local_rank
    resume_hp = None
    if args.resume is not None:
        with torch.serialization.safe_globals([Namespace]):
            resume_hp = torch.load(args.resume, map_location="cpu", weights_only=True)["hyper_parameters"]
        # (`gpus` is this launch's to say: a checkpoint at an epoch's end resumes under another number of ranks)
        resume_hp = {k: v for k, v in resume_hp.items() if k not in ("node_histogram", "outdir", "gpus")}
    cfg = load_config(args.config, resume_hp, world)
    hist = np.load(os.path.join(cfg["datadir"], "size_distribution.npy")).tolist()
    train_set = ProcessedDataset(os.path.join(cfg["datadir"], "train.npz"), device=args.device)
    val_path = os.path.join(cfg["datadir"], "val.npz")
    val_set = ProcessedDataset(val_path, device=args.device) if os.path.isfile(val_path) else None
    trainer = Trainer(cfg, hist, train_set, val_set, device=args.device, optimizer=args.optimizer, world=world, rank=rank,
                      collective=collective)
    if args.resume is not None:
        trainer.load_checkpoint(args.resume)
    trainer.fit(max_steps=args.max_steps)
    if args.max_steps is not None:
        trainer.save_checkpoint()
    if rank == 0:
        print(json.dumps({"epoch": trainer.epoch, "global_step": trainer.global_step,
                          "checkpoint": os.path.join(trainer.ckpt_dir, "last.ckpt"), "metrics": trainer.metrics_path}))
    if collective:
        import torch.distributed as dist
        dist.barrier(device_ids=[torch.device(args.device).index or 0] if dist.get_backend() == "nccl" else None)
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
