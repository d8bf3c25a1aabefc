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

Out of scope (refused with a message): `virtual_nodes` (AppendVirtualNodes draws random virtual atoms per item),
`augment_noise > 0` / `augment_rotation` (the reference raises NotImplementedError for them), `gpus > 1` (data-parallel
ranks; the same effective batch is reached with `accumulate_grad_batches`).
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


def check_config(cfg):
    """Validates a training configuration with the reference's YAML keys; -> plain dict.  Refuses what is out of scope,
    warns once about what is accepted and ignored."""
    cfg = {k: _plain(v) for k, v in dict(cfg).items()}
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
    if int(cfg.get("gpus", 1)) > 1:
        raise NotImplementedError("gpus > 1: multi-GPU training is out of scope of this trainer; set gpus: 1 and multiply "
                                  "accumulate_grad_batches by the number of GPUs for the same effective batch")
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


def load_config(path, resume_hparams=None):
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
    return check_config(cfg)


# ---- the loop -----------------------------------------------------------------------------------------------------------
class Trainer:
    """fit() / training_step() / training_window() / validate() / save_checkpoint() / resume() around `ddpm.forward` and
    the HIP optimiser.  `optimizer="torch"` selects torch.optim.AdamW plus the host-side restatement of the reference's
    clipping (A/B); it accumulates through torch."""

    def __init__(self, config, node_histogram, train_set=None, val_set=None, device="cuda", optimizer="hip"):
        from .generate import LigandGenerator
        self.cfg = cfg = check_config(config)
        self.device = torch.device(device)
        self.node_histogram = np.asarray(node_histogram).tolist()
        if optimizer not in ("hip", "torch"):
            raise ValueError("optimizer must be 'hip' or 'torch'")
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

    @torch.no_grad()
    def validate(self):
        """Mean `loss/val` over the validation split (eval mode, no_grad), weighted by batch size as Lightning's log."""
        self.ddpm.eval()
        n = len(self.val_set)
        bs = int(self.cfg.get("eval_batch_size", self.cfg["batch_size"]))
        total = torch.zeros((), dtype=torch.float64, device=self.device)
        for b, lo in enumerate(range(0, n, bs)):
            idx = list(range(lo, min(lo + bs, n)))
            self._key_step(_EVAL_DRAW_BASE // DRAWS_PER_STEP + self.epoch * 100003 + b)
            nll, _ = self.forward(self.val_set.collate(idx))
            total += nll.double().sum()
        self.ddpm.train()
        return float(total / n)

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
        os.makedirs(self.run_dir, exist_ok=True)
        with open(self.metrics_path, "a") as f:
            f.write(json.dumps(record) + "\n")

    def flush_metrics(self):
        """One synchronisation: the pending device scalars and the clip record."""
        if not self._pending:
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
            starts = np.cumsum([0] + accumulation_windows(len(batches), self.accumulate)).tolist()
            while self.batch_in_epoch < len(batches):
                if max_steps is not None and self.global_step >= max_steps:
                    self.flush_metrics()
                    return
                hi = min(b for b in starts if b > self.batch_in_epoch)
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
            self.save_checkpoint(val)

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
                "micro_step": self.micro_step,
                "optimizer_kind": self.optimizer_kind, QUEUE_KEY: opt.get(QUEUE_KEY), "best_val": self.best_val}

    def save_checkpoint(self, val_loss=None):
        """`last.ckpt` always, `best-model-epoch=NN.ckpt` when `loss/val` improved (train.py:103-110)."""
        os.makedirs(self.ckpt_dir, exist_ok=True)
        ck = self.checkpoint()
        last = os.path.join(self.ckpt_dir, "last.ckpt")
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
        self.micro_step = int(ck.get("micro_step", self.global_step))      # (checkpoints written before accumulation)
        self.best_val = float(ck.get("best_val", float("inf")))

    @classmethod
    def resume(cls, path, train_set=None, val_set=None, device="cuda", optimizer=None, overrides=None):
        """A Trainer continued from a checkpoint written by `save_checkpoint`."""
        with torch.serialization.safe_globals([Namespace]):
            ck = torch.load(path, map_location="cpu", weights_only=True)
        hp = {k: _plain(v) for k, v in ck["hyper_parameters"].items()}
        hp.update(overrides or {})
        hist = hp.pop("node_histogram")
        hp.pop("outdir", None)
        tr = cls(hp, hist, train_set, val_set, device=device, optimizer=optimizer or ck.get("optimizer_kind", "hip"))
        tr.load_checkpoint(path)
        return tr


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--config", type=str, required=True)
    p.add_argument("--resume", type=str, default=None)
    p.add_argument("--optimizer", choices=("hip", "torch"), default="hip")
    p.add_argument("--max-steps", type=int, default=None)
    p.add_argument("--device", type=str, default="cuda")
    args = p.parse_args(argv)
    resume_hp = None
    if args.resume is not None:
        with torch.serialization.safe_globals([Namespace]):
            resume_hp = torch.load(args.resume, map_location="cpu", weights_only=True)["hyper_parameters"]
        resume_hp = {k: v for k, v in resume_hp.items() if k not in ("node_histogram", "outdir")}
    cfg = load_config(args.config, resume_hp)
    hist = np.load(os.path.join(cfg["datadir"], "size_distribution.npy")).tolist()
    train_set = ProcessedDataset(os.path.join(cfg["datadir"], "train.npz"), device=args.device)
    val_path = os.path.join(cfg["datadir"], "val.npz")
    val_set = ProcessedDataset(val_path, device=args.device) if os.path.isfile(val_path) else None
    trainer = Trainer(cfg, hist, train_set, val_set, device=args.device, optimizer=args.optimizer)
    if args.resume is not None:
        trainer.load_checkpoint(args.resume)
    trainer.fit(max_steps=args.max_steps)
    if args.max_steps is not None:
        trainer.save_checkpoint()
    print(json.dumps({"epoch": trainer.epoch, "global_step": trainer.global_step,
                      "checkpoint": os.path.join(trainer.ckpt_dir, "last.ckpt"), "metrics": trainer.metrics_path}))


if __name__ == "__main__":
    main()
