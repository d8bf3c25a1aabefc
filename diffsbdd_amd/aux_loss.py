"""The auxiliary Lennard-Jones term of the training loss (lightning_modules.py:284-292, :304-331, :902-914) on one HIP
launch (csrc/lj_loss.h): potential per sample and its derivative with respect to the coordinates in the same pass.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from .chem_tables import lennard_jones_rm


def lj_sigma(rm_pm, norm_value_x):
    """sigma = 2^(-1/6) rm / 100 (pm -> A) / norm_values[0], float64 [A][A]."""
    return 2.0 ** (-1.0 / 6.0) * (np.asarray(rm_pm, dtype=np.float64) / 100.0 / float(norm_value_x))


class _LJ(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xh, mask, batch, sigma, clamp):
        lib = _lib.load()
        dev = xh.device
        if dev.type != "cuda":
            raise _lib.HipLibraryError("the Lennard-Jones term runs on the GPU only; there is no CPU fallback")
        x = xh.detach().to(torch.float32).contiguous()
        n, ld = x.shape
        nt = sigma.shape[0]
        if ld != 3 + nt:
            raise ValueError(f"xh has {ld - 3} feature columns, the radii table {nt} atom types")
        mask = mask.to(device=dev, dtype=torch.int64).contiguous()
        u = torch.empty(batch, dtype=torch.float32, device=dev)
        dx = torch.zeros(n, 3, dtype=torch.float32, device=dev)
        types = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        _lib.check(lib.dsbdd_lj_potential(torch.cuda.current_stream(dev).cuda_stream, x.data_ptr(), ld, nt, mask.data_ptr(),
                                          n, batch, sigma.data_ptr(), float(clamp) if clamp is not None else 0.0,
                                          int(clamp is not None), types.data_ptr(), u.data_ptr(), dx.data_ptr()),
                   "dsbdd_lj_potential")
        ctx.save_for_backward(dx, mask)
        ctx.ld = ld
        ctx.dtype = xh.dtype
        return u

    @staticmethod
    def backward(ctx, g_u):
        dx, mask = ctx.saved_tensors
        g = torch.zeros(dx.shape[0], ctx.ld, dtype=torch.float32, device=dx.device)
        g[:, :3] = dx * g_u.to(torch.float32)[mask].unsqueeze(1)          # the type argmax carries no gradient
        return g.to(ctx.dtype), None, None, None, None


class LennardJones:
    """`lj_potential(x_lig_hat, h_lig_hat, mask)` of the reference on `xh_lig_hat` [n][3 + atom_nf]."""

    def __init__(self, atom_decoder, norm_value_x, clamp_lj=None, device="cuda"):
        self.rm = lennard_jones_rm(atom_decoder)
        self.sigma = torch.from_numpy(lj_sigma(self.rm, norm_value_x)).to(device).contiguous()
        self.clamp = None if clamp_lj is None else float(clamp_lj)

    def __call__(self, xh_lig_hat, mask, batch):
        return _LJ.apply(xh_lig_hat, mask, int(batch), self.sigma, self.clamp)


class WeightSchedule:
    """lightning_modules.py:902-914 as a device table indexed by t_int."""

    def __init__(self, T, max_weight, mode="linear", device="cpu"):
        if mode == "linear":
            w = torch.linspace(max_weight, 0, T + 1)
        elif mode == "constant":
            w = max_weight * torch.ones(T + 1)
        else:
            raise NotImplementedError(f"{mode} weight schedule is not available.")
        self.weights = w.to(device)

    def __call__(self, t_array):
        return self.weights[t_array.to(self.weights.device)]
