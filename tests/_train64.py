"""Ragged and degenerate training batches of `EGNNDynamics` and their float64 reference, for
tests/test_train_reference.py (CPU: the conditions the GPU test relies on) and tests/test_gpu_train_degenerate.py.

Nothing here touches the GPU or the HIP library: the reference is `oracle.egnn_oracle.dynamics_forward` under autograd on
the CPU, on the exact edge list (`get_edges(..., exact=True)` of the float64 coordinates, teacher-forced), in float64 (the
reference) or float32 (the yardstick: `err_ref` of the tolerance rule `within_case`).
"""
from __future__ import annotations

import functools
import statistics

import torch

from oracle import egnn_oracle as eo
from oracle import weights as W

from tests._steps64 import ULP4

JOINT = ("small_joint", "moad_fullatom_joint")          # cutoffs 0.8 / 1.4, every row moves: spread 0.6
SMALL2 = ("small_cond", "small_joint")


def problem(cfg, n_lig, n_poc, seed, spread=3.0):
    """Seeded inputs of a training call (also those of tests/test_gpu_train.py and tests/test_gpu_accumulate.py):
    -> xh_atoms, xh_residues, t [B][1], mask_atoms, mask_residues on the CPU; ligand positions at half the pocket's spread."""
    g = torch.Generator().manual_seed(seed)
    B = len(n_lig)
    ml = torch.repeat_interleave(torch.arange(B), torch.tensor(n_lig))
    mp = torch.repeat_interleave(torch.arange(B), torch.tensor(n_poc))
    a, r = cfg["atom_nf"], cfg["residue_nf"]
    xl = torch.cat([torch.randn(len(ml), 3, generator=g) * spread * 0.5, torch.randn(len(ml), a, generator=g)], 1)
    xp = torch.cat([torch.randn(len(mp), 3, generator=g) * spread, torch.randn(len(mp), r, generator=g)], 1)
    t = torch.rand(B, 1, generator=g)
    return xl, xp, t, ml, mp


# name -> n_lig, n_poc, seed (seeds: per-architecture exceptions), shared_t (t of one element), moved = (sample, shift of
# its ligand on every axis) or None, archs.  The smallest shapes that reach the branches named in
# profiles/train_net_error.md; the full-width kernels (H = 256, H = 192, six blocks) run on `ragged` only.
CASES = {
    # a sample without ligand atoms, a one-atom ligand, a sample without pocket atoms; one t per sample
    "ragged": dict(n_lig=[5, 0, 1, 7], n_poc=[40, 35, 38, 0], seed=21, seeds={"small_variant": 26}, shared_t=False,
                   moved=None, archs=("small_cond", "small_joint", "small_variant", "crossdock_ca_cond",
                                      "crossdock_fullatom_cond", "moad_fullatom_joint")),
    # sample id 1 has no node at all
    "hole": dict(n_lig=[5, 0, 3], n_poc=[40, 0, 38], seed=21, seeds={}, shared_t=False, moved=None, archs=SMALL2),
    # n_lig == 0: the pocket-conditioned architectures have n_upd == 0 and e_upd == 0 (the identity branch of both
    # coordinate stages); the joint one moves every row (seed 23: at 21 and 22 two pocket pairs lie within 1e-4 of 0.8)
    "no_ligand": dict(n_lig=[0, 0], n_poc=[40, 35], seed=21, seeds={"small_joint": 23}, shared_t=False, moved=None,
                      archs=("small_cond", "small_joint", "small_variant")),
    # n_pocket == 0, N == n_lig
    "no_pocket": dict(n_lig=[6, 9], n_poc=[0, 0], seed=21, seeds={}, shared_t=False, moved=None, archs=SMALL2),
    # a ligand with no ligand-pocket edge.  20, not 100: at 100 the cross product about the sample mean cancels and the
    # float32 oracle itself is off by 6e-5 to 8e-5
    "far": dict(n_lig=[5, 7, 6], n_poc=[40, 35, 38], seed=21, seeds={}, shared_t=False, moved=(1, 20.0), archs=SMALL2),
    # E = 2, self loops only.  Not on the architectures with a cross-product MLP: two nodes are collinear with their
    # mean, the cross product is exactly 0 in float64 and rounding noise in float32
    "single": dict(n_lig=[1], n_poc=[1], seed=21, seeds={}, shared_t=False, moved=None, archs=("small_variant",)),
    # `ragged` with t of one element: the t_count == 1 arm
    "shared_t": dict(n_lig=[5, 0, 1, 7], n_poc=[40, 35, 38, 0], seed=21, seeds={}, shared_t=True, moved=None, archs=SMALL2),
}

PAIRS = [(c, a) for c, spec in CASES.items() for a in spec["archs"]]
# `TrainGraph` cannot be built for a batch with an empty node set: an empty tensor has no data pointer and
# dsbdd_build_edges answers DSBDD_ERR_ARG to a NULL mask whatever its length (profiles/train_net_error.md).  These two
# cases have their reference checked on the CPU and wait for that to be lifted; the GPU tests run the others.
NEEDS_EMPTY_NODE_SET = ("no_ligand", "no_pocket")
GPU_PAIRS = [(c, a) for c, a in PAIRS if c not in NEEDS_EMPTY_NODE_SET]


def spread_of(arch):
    return 0.6 if arch in JOINT else 3.0


def seed_of(case, arch):
    spec = CASES[case]
    return spec["seeds"].get(arch, spec["seed"])


@functools.lru_cache(maxsize=None)
def inputs(case, arch):
    """-> dict(cfg, xl, xp, t, ml, mp, wl, wp), float32 on the CPU; wl / wp weight the two outputs in the loss."""
    spec = CASES[case]
    cfg, _ = W.arch_cfg(arch)
    xl, xp, t, ml, mp = problem(cfg, spec["n_lig"], spec["n_poc"], seed_of(case, arch), spread=spread_of(arch))
    if spec["moved"] is not None:
        b, shift = spec["moved"]
        xl[ml == b, :3] += shift
    if spec["shared_t"]:
        t = t[:1].clone()
    gen = torch.Generator().manual_seed(99)
    wl, wp = torch.randn(xl.shape, generator=gen), torch.randn(xp.shape, generator=gen)
    return dict(cfg=cfg, xl=xl, xp=xp, t=t, ml=ml, mp=mp, wl=wl, wp=wp)


def cutoffs(cfg):
    return cfg["edge_cutoff_ligand"], cfg["edge_cutoff_pocket"], cfg["edge_cutoff_interaction"]


@functools.lru_cache(maxsize=None)
def exact_edges(case, arch):
    """The edge list of the case's float32 coordinates with distances evaluated in float64, int64 [2][E], (row, col) order."""
    p = inputs(case, arch)
    return eo.get_edges(p["ml"], p["mp"], p["xl"][:, :3].double(), p["xp"][:, :3].double(), *cutoffs(p["cfg"]), exact=True)


def ambiguous_pairs(case, arch, tol=1e-4):
    """Number of same-sample pairs whose float64 distance lies within `tol` of the cutoff that applies to them."""
    p = inputs(case, arch)
    return int(eo.edge_ambiguity_band(p["ml"], p["mp"], p["xl"][:, :3], p["xp"][:, :3], *cutoffs(p["cfg"]), tol).sum())


def param_names(cfg):
    """The names of `EGNNDynamics.named_parameters()`: coord_mlp.4.weight and cross_product_mlp.4.weight are one tensor."""
    return [n for n in W.dynamics_param_shapes(cfg) if not n.endswith("cross_product_mlp.4.weight")]


@functools.lru_cache(maxsize=None)
def reference(case, arch, dtype, loss_on=("l", "p")):
    """-> {eps_l, eps_p, d_xh_atoms, d_xh_residues, <parameter name>: gradient ...} in `dtype`, detached.
    loss = (eps_l * wl).sum() + (eps_p * wp).sum() (`loss_on`: which of the two terms).  A parameter the loss does not
    depend on has a zero gradient here."""
    p = inputs(case, arch)
    cfg = p["cfg"]
    sd32 = W.random_state_dict(cfg, seed=1)
    leaves = {}
    sd = {}
    for k, v in sd32.items():               # the twin names of random_state_dict share ONE tensor: keep that
        if id(v) not in leaves:
            leaves[id(v)] = v.to(dtype).clone().requires_grad_(True)
        sd[k] = leaves[id(v)]
    xl, xp = (p[k].to(dtype).clone().requires_grad_(True) for k in ("xl", "xp"))
    eps_l, eps_p, _ = eo.dynamics_forward(sd, cfg, xl, xp, p["t"].to(dtype), p["ml"], p["mp"], edges=exact_edges(case, arch))
    loss = 0
    if "l" in loss_on:
        loss = loss + (eps_l * p["wl"].to(dtype)).sum()
    if "p" in loss_on:
        loss = loss + (eps_p * p["wp"].to(dtype)).sum()
    loss.backward()
    zero = lambda v: v.grad.detach() if v.grad is not None else torch.zeros_like(v)
    out = dict(eps_l=eps_l.detach(), eps_p=eps_p.detach(), d_xh_atoms=zero(xl), d_xh_residues=zero(xp))
    for n in param_names(cfg):
        out[n] = zero(sd[n])
    return out


def magnitude(v):
    return float(v.detach().double().abs().max()) if v.numel() else 0.0


@functools.lru_cache(maxsize=None)
def err_refs(case, arch, loss_on=("l", "p")):
    """-> ({quantity: err_ref}, median).  err_ref = max |float32 oracle - float64 oracle| / the quantity's largest float64
    magnitude; a quantity that is identically 0 in float64 counts with the absolute float32 value (0 when the zero is
    structural); empty quantities are left out."""
    r64, r32 = reference(case, arch, torch.float64, loss_on), reference(case, arch, torch.float32, loss_on)
    errs = {}
    for k, v in r64.items():
        if v.numel() == 0:
            continue
        mag = magnitude(v)
        errs[k] = float((r32[k].double() - v).abs().max()) / (mag if mag > 0 else 1.0)
    return errs, statistics.median(errs.values())


def structural_zeros(case, arch):
    """Names of the quantities that are 0 by the structure of the case (no row, or a masked update), not by value."""
    cfg = inputs(case, arch)["cfg"]
    names = param_names(cfg)
    if case == "no_ligand":
        z = [n for n in names if n.startswith(("atom_encoder.", "atom_decoder."))]
        if not cfg["update_pocket_coords"]:
            z += [n for n in names if ".gcl_equiv." in n]
        return z
    if case == "no_pocket":
        return [n for n in names if n.startswith("residue_")]
    if case == "single":
        return [n for n in names if ".gcl_equiv." in n]
    return []


def group_of(name):
    """The quantity groups of profiles/train_net_error.md."""
    if name in ("eps_l", "eps_p"):
        return "outputs"
    if name.startswith("d_xh_"):
        return "input gradients"
    if name.startswith(("atom_", "residue_")):
        return "encoders/decoders"
    if name.startswith(("egnn.embedding", "edge_embedding")):
        return "embeddings"
    if ".edge_mlp." in name:
        return "edge MLPs"
    if ".node_mlp." in name:
        return "node MLPs"
    if ".att_mlp." in name:
        return "attention"
    if ".gcl_equiv." in name:
        return "coordinate MLPs"
    raise KeyError(name)


# The factor over err_ref per quantity group.  The project's standing factor is 2.  Measured on one MI355X over GPU_PAIRS
# and the three float32 evaluations the GPU offers (network walk, per-stage Functions, DSBDD_TRAIN=torch), 1 037 non-zero
# quantities each: every path sits at the distance of the float32 oracle itself (median err / err_ref 0.54 .. 1.24 per
# group and path), and the tails pass 2 on all three alike -- largest err / err_ref of walk / Functions / torch: input
# gradients 2.08 / 2.16 / 1.34, encoders and decoders 2.29 / 2.07 / 1.77, node MLPs 2.33 / 2.64 / 2.33, attention 4.75 /
# 6.75 / 8.54, coordinate MLPs 2.63 / 3.09 / 4.41 (edge MLPs 1.67 / 1.48 / 4.88, embeddings 1.37 / 0.97 / 1.18, outputs
# 1.00 / 1.00 / 1.40 stay at 2).  That is summation order: an attention bias is ONE number summed over every edge, and a
# few ulp of it are 1e-6.  Where a HIP path passed 2, the group's factor is 1.5 times the largest ratio a HIP path showed
# (profiles/train_net_error.md has the quantities).
FACTOR = {"input gradients": 1.5 * 2.16, "encoders/decoders": 1.5 * 2.29, "node MLPs": 1.5 * 2.64, "attention": 1.5 * 6.75,
          "coordinate MLPs": 1.5 * 3.09}


def factor_of(name):
    return FACTOR.get(group_of(name), 2.0)


def within_case(name, hip, ref64, ref32, floor, label=""):
    """The project's rule (tests/_steps64.py: `within`): |hip - f64| <= max(F err_ref, 4 ulp) of the quantity's largest
    float64 magnitude, and 1e-4 at most -- with err_ref = the larger of the quantity's own float32-vs-float64 oracle error
    and `floor`, the median of that error over all quantities of the same (case, architecture): one bias vector's float32
    error can be near zero by accident, and the HIP path sums in another order.  F = 2, or the group's entry of FACTOR.
    Prints its figures, then asserts.  -> dict(err_ref, hip, bound, mag)."""
    hip, ref64, ref32 = (torch.as_tensor(v).detach().cpu().double().reshape(-1) for v in (hip, ref64, ref32))
    assert hip.numel() == ref64.numel(), (label, name, hip.numel(), ref64.numel())
    if ref64.numel() == 0:
        return dict(err_ref=0.0, hip=0.0, bound=ULP4, mag=0.0)
    mag = max(float(ref64.abs().max()), 1e-30)
    own = float((ref32 - ref64).abs().max()) / mag
    err_ref = max(own, floor)
    err = float((hip - ref64).abs().max()) / mag
    bound = min(max(factor_of(name) * err_ref, ULP4), 1e-4)
    print(f"  {label} {name}: err_ref {err_ref:.3e} (own {own:.3e})  hip {err:.3e}  bound {bound:.3e}  (magnitude {mag:.3e})")
    assert torch.isfinite(hip).all(), (label, name)
    assert err <= bound, (label, name, err, bound)
    return dict(err_ref=err_ref, hip=err, bound=bound, mag=mag)
