"""`ClippedAdamW`: the reference's adaptive gradient clipping and AdamW(amsgrad) as two HIP launches (csrc/optim.h).

One `step()` does what `LigandPocketDDPM.configure_gradient_clipping` (lightning_modules.py:874-899: queue of the last
50 gradient norms, threshold 1.5 mean + 2 std, `clip_grad_norm_`) followed by
`torch.optim.AdamW(lr, betas, eps, weight_decay, amsgrad=True).step()` do in the reference, without a device-to-host
copy: the queue, the norm and the clip decision stay on the device; `clip_report()` reads them on demand.

Differences to the reference, on purpose:
  * `p.grad` is left UNSCALED (the clip coefficient is applied to the gradient as the update kernel reads it);
    `clip_grad_norm_` scales `p.grad` in place.  Nothing in the loop reads `p.grad` after the step.
  * "Clipped gradient with value ..." is not printed per step; the record is kept on the device (`clip_report()`).

The state is torch's: `state[p]` holds `step`, `exp_avg`, `exp_avg_sq`, `max_exp_avg_sq` (views into three flat
buffers the kernels stream over), created when `p` first has a gradient, so `state_dict()` / `load_state_dict()`
exchange with `torch.optim.AdamW(amsgrad=True)`; the queue travels as the extra key `clip_queue`.

Data-parallel ranks: `step_ranks(gathered, n_ranks)` is `step()` on the sum of the ranks' gradient buckets, folded per
element in rank order (float32, one rounding per add) by the first launch itself (`optim_reduce_norm_kernel` takes the
place of the norm launch: no extra launch, no extra pass over the gradient), bit for bit what torch's ordered adds into
the bucket followed by `step()` give.  It needs `n_ranks` gathered buckets on the device beside the optimiser's own.

`ReferenceClipper` is the host-side restatement of the reference's clipping (with its three host read-backs per
step): the `optimizer="torch"` leg of the trainer, parity tests and tools/train_step_bench.py use it.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib

QUEUE_LEN = 50
QUEUE_FIRST = 3000.0          # lightning_modules.py:85-88, "Add large value that will be flushed."
QUEUE_KEY = "clip_queue"
# torch.optim.AdamW's own param-group keys beside the hyper-parameters, so that a state dict written here loads there
TORCH_GROUP_DEFAULTS = dict(maximize=False, foreach=None, capturable=False, differentiable=False, fused=None,
                            decoupled_weight_decay=True)


def queue_max_norm(items):
    """1.5 mean + 2 std (population, np.std) of the recent norms: lightning_modules.py:880-882."""
    return 1.5 * np.mean(items) + 2 * np.std(items)


class ReferenceClipper:
    """configure_gradient_clipping + utils.Queue of the reference, on the host, read-backs included."""

    def __init__(self, items=None):
        self.items = [QUEUE_FIRST] if items is None else [float(v) for v in items]     # newest first (utils.py:20-23)
        self.n_clips = 0
        self.last_norm = self.last_max = float("nan")

    def add(self, item):
        self.items.insert(0, float(item))
        if len(self.items) > QUEUE_LEN:
            self.items.pop()

    def decide(self, grad_norm):
        """The queue arithmetic for one step, given the norm as a Python float: -> (max_norm, clipped)."""
        max_norm = float(queue_max_norm(self.items))
        clipped = grad_norm > max_norm
        self.add(max_norm if clipped else grad_norm)
        self.n_clips += int(clipped)
        self.last_norm, self.last_max = grad_norm, max_norm
        return max_norm, clipped

    def clip(self, params):
        """Scales `p.grad` in place as the reference does; -> (grad_norm, max_norm) as Python floats."""
        params = [p for p in params if p.grad is not None]
        max_norm = float(queue_max_norm(self.items))
        if not params:
            grad_norm = torch.tensor(0.)
        else:                                                                       # utils.get_grad_norm
            grad_norm = torch.norm(torch.stack([torch.norm(p.grad.detach(), 2.0) for p in params]), 2.0)
        torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type=2.0)             # what Lightning's clip_gradients calls
        gn = float(grad_norm)                                                       # host read-back
        self.decide(gn)
        return gn, max_norm


def attach_queue(state_dict, items, n_clips=0):
    """Adds the clip queue (newest first) to an optimiser state dict in torch.optim.AdamW's layout."""
    state_dict[QUEUE_KEY] = {"items": [float(v) for v in items], "n_clips": int(n_clips)}
    return state_dict


class GradientBucket:
    """ONE flat float32 device tensor that holds every parameter's gradient at the offsets of the optimiser's state
    (`dsbdd_optim_state_offset`): the destination of the accumulating backward (train_net.accumulating), and the unit a
    data-parallel exchange works on (`ClippedAdamW.step_ranks`).  `view(p)` is the region of parameter `p`, shaped like
    `p`.  `flat`: the caller's storage for it (e.g. this rank's slot of a gather buffer) instead of a new tensor."""

    def __init__(self, params, offsets, elems, device, flat=None):
        if flat is None:
            flat = torch.zeros(elems, dtype=torch.float32, device=device)
        elif (flat.dtype != torch.float32 or flat.device != torch.device(device) or flat.dim() != 1 or flat.numel() != elems or
              not flat.is_contiguous() or flat.data_ptr() % 16):
            raise ValueError("a gradient bucket is a contiguous, 16-byte aligned float32 tensor of %d elements on %s" % (elems, device))
        self.flat = flat
        self._views = {id(p): self.flat[o:o + p.numel()].view(p.shape) for p, o in zip(params, offsets)}
        self._params = list(params)          # (keeps the ids above alive)

    def __contains__(self, p):
        return id(p) in self._views

    def view(self, p):
        return self._views[id(p)]


class ClippedAdamW(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-12, clip_grad=True):
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=True, **TORCH_GROUP_DEFAULTS)
        super().__init__(params, defaults)
        hyper = [tuple(g[k] for k in ("lr", "betas", "eps", "weight_decay", "amsgrad")) for g in self.param_groups]
        if any(h != hyper[0] for h in hyper):
            raise ValueError("ClippedAdamW takes one set of hyper-parameters: the param groups differ (%r)" % (hyper,))
        if not hyper[0][4]:
            raise ValueError("ClippedAdamW implements amsgrad=True only")
        self._params = [p for g in self.param_groups for p in g["params"]]
        for p in self._params:
            if p.dtype != torch.float32:
                raise TypeError("ClippedAdamW needs float32 parameters, got %s" % p.dtype)
            if p.device.type != "cuda":
                raise _lib.HipLibraryError("ClippedAdamW runs on the GPU only (a parameter is on %s); there is no CPU "
                                           "fallback" % p.device)
            if p.device != self._params[0].device:
                raise ValueError("ClippedAdamW needs every parameter on one device")
            if not p.is_contiguous() or p.numel() == 0:
                raise ValueError("ClippedAdamW needs contiguous, non-empty parameters")
        self.clip_grad = bool(clip_grad)
        self.device = self._params[0].device
        self.lib = _lib.load()
        n = len(self._params)
        lr, betas, eps, weight_decay = hyper[0][:4]
        cfg = _lib.OptimCfg(lr, betas[0], betas[1], eps, weight_decay, int(self.clip_grad))
        numel = (C.c_int64 * n)(*[p.numel() for p in self._params])
        h = C.c_void_p()
        _lib.check(self.lib.dsbdd_optim_create(C.byref(cfg), n, numel, C.byref(h)), "dsbdd_optim_create")
        self._h = h
        elems = int(self.lib.dsbdd_optim_state_elems(h))
        self._offsets = [int(self.lib.dsbdd_optim_state_offset(h, i)) for i in range(n)]
        self._flat = torch.zeros(3, elems, dtype=torch.float32, device=self.device)        # exp_avg | exp_avg_sq | max_exp_avg_sq
        self._ws = torch.empty(int(self.lib.dsbdd_optim_workspace_bytes(h)), dtype=torch.uint8, device=self.device)
        _lib.check(self.lib.dsbdd_optim_bind(h, self._stream(), self._flat[0].data_ptr(), self._flat[1].data_ptr(),
                                             self._flat[2].data_ptr(), self._ws.data_ptr(), self._ws.numel()),
                   "dsbdd_optim_bind")
        self._steps = [0] * n
        self._ptrs = None
        self._grad_arr = (C.c_void_p * n)()
        self._step_arr = (C.c_int32 * n)()
        self.host_copies = 0           # device-to-host copies this object has made (clip_report / state_dict only)
        self._bucket = None

    def __del__(self):
        try:
            self.lib.dsbdd_optim_destroy(self._h)
        except Exception:
            pass

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def _views(self, i):
        p, o = self._params[i], self._offsets[i]
        return [self._flat[k, o:o + p.numel()].view(p.shape) for k in range(3)]

    def _make_state(self, i):
        m, v, vmax = self._views(i)
        self.state[self._params[i]] = {"step": torch.tensor(float(self._steps[i])), "exp_avg": m, "exp_avg_sq": v,
                                       "max_exp_avg_sq": vmax}

    def gradient_bucket(self, flat=None):
        """The optimiser's `GradientBucket`, created on first use and then kept: `step()` reads `p.grad` pointers as ever,
        which are views of it after an accumulating backward.  `flat`: storage for a bucket that does not exist yet."""
        if self._bucket is None:
            self._bucket = GradientBucket(self._params, self._offsets, int(self.lib.dsbdd_optim_state_elems(self._h)),
                                          self.device, flat=flat)
        elif flat is not None:
            raise ValueError("the gradient bucket exists already: its storage is chosen at its first use")
        return self._bucket

    def zero_grad(self, set_to_none=True):
        """`None` gradients are what "this tensor is skipped" hangs on; zeros would decay and count a step."""
        super().zero_grad(set_to_none=set_to_none)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        keep = []
        ptrs = []
        for i, p in enumerate(self._params):
            g = p.grad
            ptrs.append(p.data_ptr())
            if g is None:
                self._grad_arr[i] = None
                continue
            if g.is_sparse or g.dtype != torch.float32 or g.device != self.device:
                raise TypeError("ClippedAdamW needs dense float32 gradients on the parameters' device")
            if not g.is_contiguous():
                g = g.contiguous()
                keep.append(g)
            self._grad_arr[i] = g.data_ptr()
            self._steps[i] += 1
            self._step_arr[i] = self._steps[i]
            if self._steps[i] == 1 and p not in self.state:
                self._make_state(i)
        stream = self._stream()
        self._follow_params(ptrs, stream)
        _lib.check(self.lib.dsbdd_optim_step(self._h, stream, self._grad_arr, self._step_arr,
                                             float(self.param_groups[0]["lr"])), "dsbdd_optim_step")
        return loss

    def _follow_params(self, ptrs, stream):
        if ptrs != self._ptrs:                                      # the device table follows the parameters' storage
            arr = (C.c_void_p * len(ptrs))(*ptrs)
            _lib.check(self.lib.dsbdd_optim_set_params(self._h, stream, arr), "dsbdd_optim_set_params")
            self._ptrs = ptrs

    @torch.no_grad()
    def step_ranks(self, gathered, n_ranks):
        """One step of data-parallel ranks (`dsbdd_optim_step_ranks`): row r of `gathered` (float32, on the device, unit
        stride within a row; columns past the bucket's length are ignored) starts with rank r's gradient bucket.  The
        first `n_ranks` rows are summed per element in rank order, ((g0 + g1) + g2) + ..., into this optimiser's bucket
        by the first launch -- which may BE one of the rows (`gradient_bucket(flat=gathered[r, :elems])`) -- and the step
        is `step()` on that sum, bit for bit.  `p.grad` is the bucket's view of `p`, or None: the tensor is skipped and
        its region of every row is neither read nor written.  Step counts and state creation as in `step()`."""
        bucket = self.gradient_bucket()
        elems, n_ranks = bucket.flat.numel(), int(n_ranks)
        if (not torch.is_tensor(gathered) or gathered.dtype != torch.float32 or gathered.device != self.device or
                gathered.dim() != 2 or gathered.stride(1) != 1 or gathered.shape[1] < elems):
            raise TypeError("step_ranks needs a 2-d float32 tensor on the parameters' device with rows of at least %d "
                            "contiguous elements" % elems)
        if not 1 <= n_ranks <= gathered.shape[0]:
            raise ValueError("n_ranks must be 1 to the number of rows (%d), got %d" % (gathered.shape[0], n_ranks))
        ptrs = []
        for i, p in enumerate(self._params):
            g = p.grad
            ptrs.append(p.data_ptr())
            if g is None:
                self._grad_arr[i] = None
                continue
            view = bucket.view(p)
            if g.data_ptr() != view.data_ptr() or g.shape != view.shape or g.dtype != torch.float32 or not g.is_contiguous():
                raise ValueError("step_ranks: p.grad must be the gradient bucket's view of the parameter, or None")
            self._grad_arr[i] = g.data_ptr()
            self._steps[i] += 1
            self._step_arr[i] = self._steps[i]
            if self._steps[i] == 1 and p not in self.state:
                self._make_state(i)
        stream = self._stream()
        self._follow_params(ptrs, stream)
        _lib.check(self.lib.dsbdd_optim_step_ranks(self._h, stream, gathered.data_ptr(), gathered.stride(0), n_ranks,
                                                   bucket.flat.data_ptr(), self._grad_arr, self._step_arr,
                                                   float(self.param_groups[0]["lr"])), "dsbdd_optim_step_ranks")

    # ---- the device-side record ---------------------------------------------------------------------------------------
    def clip_report(self):
        """Reads the queue and the clip record from the device (one synchronisation): dict with `queue` (newest first),
        `n_clips`, `last_norm`, `last_max_norm`, `last_coef`, `steps`."""
        out = (C.c_double * 64)()
        _lib.check(self.lib.dsbdd_optim_state_read(self._h, self._stream(), out, 64), "dsbdd_optim_state_read")
        self.host_copies += 1
        n = int(out[0])
        return {"queue": [out[1 + i] for i in range(n)], "n_clips": int(out[51]), "last_norm": out[52],
                "last_max_norm": out[53], "steps": int(out[54]), "last_coef": out[55]}

    def set_queue(self, items, n_clips=0, steps=0):
        arr = (C.c_double * len(items))(*[float(v) for v in items])
        _lib.check(self.lib.dsbdd_optim_state_write(self._h, self._stream(), arr, len(items), float(n_clips), float(steps)),
                   "dsbdd_optim_state_write")

    # ---- torch.optim.AdamW's layout -------------------------------------------------------------------------------------
    def state_dict(self):
        for i, p in enumerate(self._params):
            if p in self.state:
                self.state[p]["step"] = torch.tensor(float(self._steps[i]))
        sd = super().state_dict()
        if self.clip_grad:
            rep = self.clip_report()
            attach_queue(sd, rep["queue"], rep["n_clips"])
        return sd

    def load_state_dict(self, state_dict):
        state_dict = dict(state_dict)
        queue = state_dict.pop(QUEUE_KEY, None)
        super().load_state_dict(state_dict)
        for g in self.param_groups:
            if not g.get("amsgrad", False):
                raise ValueError("ClippedAdamW resumes amsgrad=True states only")
        loaded = dict(self.state)
        self.state.clear()
        self._flat.zero_()
        for i, p in enumerate(self._params):
            st = loaded.get(p)
            if st is None:                      # never had a gradient: no entry, as in torch
                self._steps[i] = 0
                continue
            self._steps[i] = int(round(float(st["step"])))
            self._make_state(i)
            for k in ("exp_avg", "exp_avg_sq", "max_exp_avg_sq"):
                self.state[p][k].copy_(st[k])
        if queue is not None and self.clip_grad:
            self.set_queue(queue["items"], queue.get("n_clips", 0), 0)
