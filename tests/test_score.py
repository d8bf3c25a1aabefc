"""Scoring given ligands, host side (no GPU): the time grid, the combination of the terms against
`train.nll_from_terms` on the reference's recorded evaluation-mode terms, and every refusal of
`ConditionalDDPM.nll_given_pocket` (all raised before any launch)."""
import os

import numpy as np
import pytest
import torch

from diffsbdd_amd import _lib, score
from diffsbdd_amd.train import nll_from_terms
from tests._golden import Case
from tests.test_ligand_design import make_generator
from tests.test_oracle_golden import LOSS_NAMES, loss_inputs


# --------------------------------------------------------------------------- time grid
@pytest.mark.parametrize("T,K", [(20, 1), (20, 3), (20, 7), (20, 20), (500, 10), (7, 6)])
def test_time_grid_strata_partition_the_times(T, K):
    times, weights = score.time_grid(T, K, seed=4)
    assert times.dtype == torch.int64 and weights.dtype == torch.float32 and times.shape == weights.shape == (K,)
    lo = [j * T // K + 1 for j in range(K)]
    hi = [(j + 1) * T // K for j in range(K)]
    assert lo[0] == 1 and hi[-1] == T and all(hi[j] + 1 == lo[j + 1] for j in range(K - 1))       # a partition of 1..T
    assert all(lo[j] <= int(times[j]) <= hi[j] for j in range(K))
    assert weights.tolist() == [float(hi[j] - lo[j] + 1) for j in range(K)] and float(weights.sum()) == T


def test_time_grid_ends_and_determinism():
    t, w = score.time_grid(20, 20, seed=9)
    assert t.tolist() == list(range(1, 21)) and w.tolist() == [1.0] * 20
    t, w = score.time_grid(20, 1, seed=9)
    assert w.tolist() == [20.0] and 1 <= int(t[0]) <= 20
    a, b = score.time_grid(500, 10, seed=3), score.time_grid(500, 10, seed=3)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert any(not torch.equal(score.time_grid(500, 10, seed=s)[0], a[0]) for s in (4, 5, 6))
    for K in (0, 21):
        with pytest.raises(ValueError, match="n_times"):
            score.time_grid(20, K, seed=0)


# --------------------------------------------------------------------------- host combination
def test_combine_terms_is_nll_from_terms_on_the_reference_golden():
    c = Case("loss_small_cond_eval")
    terms = tuple(c.t("out_" + n) for n in LOSS_NAMES)
    ligand, pocket = loss_inputs(c)
    T = c.ddpm["timesteps"]
    want, _ = nll_from_terms(terms, ligand, pocket, loss_type="l2", training=False, T=T, x_dims=3,
                             atom_nf=c.cfg["atom_nf"], residue_nf=c.cfg["residue_nf"])
    g = dict(zip(LOSS_NAMES, terms))
    nll, loss_t = score.combine_terms(float(T), g["SNR_weight"], g["error_t_lig"], g["loss_0_x_ligand"], g["loss_0_h"],
                                      g["neg_log_constants"], g["kl_prior"], g["delta_log_px"], g["log_pN"])
    assert nll.dtype == torch.float32 and nll.shape == want.shape == (3,)
    rel = ((nll - want).abs() / want.abs().clamp(min=1.0)).max().item()
    print(f"[combine] nll {nll.tolist()}, max relative difference {rel:.2e}")
    assert rel <= 1e-6
    # [B, K] inputs with K = 2: a slot of weight zero changes nothing
    two = lambda v: torch.stack([v, v], 1)
    nll2, _ = score.combine_terms(torch.tensor([float(T), 0.0]), two(g["SNR_weight"]), two(g["error_t_lig"]),
                                  g["loss_0_x_ligand"], g["loss_0_h"], g["neg_log_constants"], g["kl_prior"],
                                  g["delta_log_px"], g["log_pN"])
    assert torch.equal(nll2, nll)


# --------------------------------------------------------------------------- refusals, all before any launch
def _batch(sizes=(5, 8, 6), n_pocket=40, atom_nf=10, residue_nf=10):
    g = torch.Generator().manual_seed(0)
    n, B = sum(sizes), len(sizes)
    oh = lambda rows, nf: torch.nn.functional.one_hot(torch.randint(0, nf, (rows,), generator=g), nf).float()
    ligand = {"x": torch.randn(n, 3, generator=g), "one_hot": oh(n, atom_nf), "size": torch.tensor(sizes),
              "mask": torch.repeat_interleave(torch.arange(B), torch.tensor(sizes))}
    pocket = {"x": torch.randn(B * n_pocket, 3, generator=g) * 5, "one_hot": oh(B * n_pocket, residue_nf),
              "size": torch.full((B,), n_pocket), "mask": torch.repeat_interleave(torch.arange(B), n_pocket)}
    return ligand, pocket


def test_refusals_without_a_gpu():
    gen = make_generator("small_cond", "pocket_conditioning")           # histogram [40][400], CPU
    ddpm = gen.ddpm
    ligand, pocket = _batch()
    # joint model, learned schedule, virtual atoms
    joint = make_generator("small_joint", "joint").ddpm
    with pytest.raises(NotImplementedError, match="pocket-conditioned"):
        joint.nll_given_pocket(ligand, pocket)
    from diffsbdd_amd.conditional_model import ConditionalDDPM
    learned = ConditionalDDPM(dynamics=ddpm.dynamics, atom_nf=10, residue_nf=10, n_dims=3, size_histogram=np.ones((40, 400)),
                              timesteps=20, noise_schedule="learned", loss_type="vlb", norm_values=(1.0, 4.0))
    with pytest.raises(NotImplementedError, match="schedule"):
        learned.nll_given_pocket(ligand, pocket)
    ddpm.vnode_idx = 3
    try:
        with pytest.raises(NotImplementedError, match="virtual"):
            ddpm.nll_given_pocket(ligand, pocket)
    finally:
        ddpm.vnode_idx = None
    # sizes outside the histogram, or of probability zero: named by ligand index, no clamp
    big_l, big_p = _batch(sizes=(5, 41, 6))
    with pytest.raises(ValueError, match="ligand 1.*histogram"):
        ddpm.nll_given_pocket(big_l, big_p)
    wide_l, wide_p = _batch(n_pocket=400)
    with pytest.raises(ValueError, match="ligand 0.*histogram"):
        ddpm.nll_given_pocket(wide_l, wide_p)
    table = ddpm.size_distribution._table(0, torch.device("cpu"))
    saved = table[6, 40].item()
    table[6, 40] = float("-inf")
    try:
        with pytest.raises(ValueError, match="ligand 2.*probability zero"):
            ddpm.nll_given_pocket(ligand, pocket)
    finally:
        table[6, 40] = saved
    # unsorted masks
    bad = dict(ligand, mask=ligand["mask"].flip(0))
    with pytest.raises(ValueError, match="sorted"):
        ddpm.nll_given_pocket(bad, pocket)
    bad_p = dict(pocket, mask=pocket["mask"].flip(0))
    with pytest.raises(ValueError, match="sorted"):
        ddpm.nll_given_pocket(ligand, bad_p)
    # the time slots
    for kw in (dict(n_times=0), dict(n_times=21), dict(times=[0, 3]), dict(times=[21]), dict(times=[2.5]),
               dict(times=torch.ones(2, 3)), dict(times=[3, 4], weights=[1.0, 2.0, 3.0]), dict(max_states=0),
               dict(ligand_ids=[0, 1])):
        with pytest.raises(ValueError):
            ddpm.nll_given_pocket(ligand, pocket, **kw)
    # injected noise needs a single chunk
    ddpm.set_noise_source(lambda shape: torch.zeros(shape))
    try:
        with pytest.raises(ValueError, match="single chunk"):
            ddpm.nll_given_pocket(ligand, pocket, n_times=4, max_states=7)
    finally:
        ddpm.set_noise_source(None)
    # a CPU module / CPU tensors: no fallback
    keep = {k: v.clone() for k, v in ligand.items()}
    with pytest.raises(_lib.HipLibraryError):
        ddpm.nll_given_pocket(ligand, pocket, n_times=2)
    assert all(torch.equal(ligand[k], keep[k]) for k in keep)          # the dicts are not modified
    assert not ddpm.training


def test_score_abi_is_declared_on_both_sides():
    with open(os.path.join(os.path.dirname(_lib._HERE), "include", "diffsbdd_hip.h")) as f:
        header = f.read()
    for name in ("dsbdd_score_rows", "dsbdd_score_cond_pre", "dsbdd_score_cond_post", "dsbdd_score_reduce"):
        assert name in _lib.SIGNATURES and f"int {name}(" in header
    assert _lib.ABI_VERSION == 6


def test_score_entry_points_refuse_bad_arguments_without_a_launch():
    import ctypes as C
    lib = _lib.load()
    assert [lib.dsbdd_score_rows(w) for w in (0, 1, 2, 3)] == [8, 4, 8, 0]
    mk = lambda **kw: _lib.LossCfg(**{**dict(batch=3, n_lig=19, n_pocket=120, atom_nf=10, residue_nf=10, timesteps=20,
                                             remove_com=1, vnode_idx=-1, norm_value_x=1.0, norm_value_h=4.0, norm_bias_h=0.0,
                                             n1_tab=12, n2_tab=60), **kw})
    err = lambda: lib.dsbdd_last_error().decode()
    pre = lambda cfg, n_slots, first, n: lib.dsbdd_score_cond_pre(None, C.byref(cfg), n_slots, first, n, 64, 512, *[None] * 17)
    post = lambda cfg, n_slots, first, n: lib.dsbdd_score_cond_post(None, C.byref(cfg), n_slots, first, n, 64, 512, *[None] * 7)
    for fn in (pre, post):
        assert fn(mk(), 2, 0, 6) == _lib.ERR_ARG and "null argument" in err()          # a valid chunk, no arrays
        for cfg, n_slots, first, n in ((mk(vnode_idx=3), 2, 0, 6),                   # virtual atoms
                                       (mk(), 1, 0, 3),                               # no time slot
                                       (mk(), 2, 5, 2), (mk(), 2, -1, 2), (mk(), 2, 0, 0),      # chunk outside the 6 states
                                       (mk(batch=0), 2, 0, 1), (mk(norm_value_h=0.0), 2, 0, 1)):
            assert fn(cfg, n_slots, first, n) == _lib.ERR_ARG and "chunk" in err(), (n_slots, first, n)
    assert lib.dsbdd_score_reduce(None, 3, 2, None, None, None, None) == _lib.ERR_ARG
    assert lib.dsbdd_score_reduce(None, 0, 2, None, None, None, None) == _lib.ERR_ARG
